"""PCA over resident CLS rows on the GPU (csrc/rows_pca.hip through cbas_rows_pca_fit / _project, then cbas_amd.framemap).

  bounds       mean, covariance (read from the front of the workspace) and total_variance against the float64 restatement of the very
               fp16 rows handed to the device, each within its a-priori bound
  exact        small-integer rows with an integer column mean: every product and partial sum is exact, so the mean and C equal
               float64's bit for bit, across chunk and part boundaries
  solver       orthonormal components, descending eigenvalues, the sign rule, the Ritz residual against the device's own C, the
               subspace against float64's on a planted spectrum
  projection   scores and residual against float64 with the device's own mean and components
  invariance   bit for bit: two fits, another ld, a slice, with and without the residual, C symmetric
The bounds are derived in rows_pca_ref.py.  Cases print their largest error / bound (run with -s)."""
import csv
import os

import numpy as np
import pytest
import torch

import rows_pca_ref as R
from cbas_amd import _lib, framemap as F, search as S, synth

pytestmark = pytest.mark.gpu

PAD = np.float16(60000.0)                  # in the columns past D: read into any sum, it shows
ITERS = F.DEFAULT_ITERS


def store(x, pad=8):
    """The fp16 rows as a device tensor with `pad` columns of PAD after the D."""
    img = np.full((x.shape[0], x.shape[1] + pad), PAD, np.float16)
    img[:, :x.shape[1]] = x
    return torch.from_numpy(img).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fit(rows, D, k, normalize, iters=ITERS):
    """cbas_rows_pca_fit on a (N, ld) fp16 device tensor; numpy outputs, `cov` from the front of the workspace."""
    lib = _lib.load()
    N = rows.shape[0]
    need = int(lib.cbas_rows_pca_workspace_bytes(N, D, k))
    assert need > 0, lib.cbas_last_error()
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    mean, comp = torch.full((D,), 7.0, device="cuda"), torch.full((k, D), 7.0, device="cuda")
    eig, tv = torch.full((k,), 7.0, device="cuda"), torch.full((1,), 7.0, device="cuda")
    _lib.check(lib.cbas_rows_pca_fit(rows.data_ptr(), N, D, rows.shape[1], k, iters, int(normalize), mean.data_ptr(), comp.data_ptr(),
                                     eig.data_ptr(), tv.data_ptr(), ws.data_ptr(), need, None), "cbas_rows_pca_fit")
    torch.cuda.synchronize()
    return {"mean": mean.cpu().numpy(), "comp": comp.cpu().numpy(), "eig": eig.cpu().numpy(), "tv": tv.cpu().numpy(),
            "cov": ws[:D * D * 4].cpu().numpy().view(np.float32).reshape(D, D).copy(), "dev": (mean, comp)}


def project(rows, D, normalize, mean, comp, scale=None, want_resid=True, first=0, n=None):
    lib = _lib.load()
    n = rows.shape[0] - first if n is None else n
    k = comp.shape[0]
    scores = torch.full((n, k), 7.0, device="cuda")
    resid = torch.full((n,), 7.0, device="cuda") if want_resid else None
    _lib.check(lib.cbas_rows_pca_project(rows.data_ptr() + first * rows.shape[1] * 2, n, D, rows.shape[1], k, int(normalize), mean.data_ptr(),
                                         comp.data_ptr(), None if scale is None else scale.data_ptr(), scores.data_ptr(),
                                         None if resid is None else resid.data_ptr(), None), "cbas_rows_pca_project")
    torch.cuda.synchronize()
    return scores.cpu().numpy(), (resid.cpu().numpy() if want_resid else None)


def rows_for(D, N, normalize):
    x = R.planted(7 * D + N, N, D)
    if normalize and N > 4:
        x[N // 2] = 0                                                          # a zero row: rn = 0, u = 0
    return x


# ---- a. mean, covariance and total variance against float64 ----------------------------------------------------------------------------
# D = 160: two column tiles, the second partial - the tile pairs (0,0), (0,1), (1,1); N = 65537: 65 chunks, two a part, the last part short
SHAPES = [(D, N) for D in (32, 160, 768) for N in (2, 63, 1024, 1025)] + [(32, 65537), (160, 65537)]


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("D,N", SHAPES)
def test_bounds(D, N, normalize):
    x = rows_for(D, N, normalize)
    got = fit(store(x), D, 1, normalize, iters=1)
    mu, C = R.mean_cov(x, normalize)
    cb, d = R.cov_bound(x, normalize)
    rm = float((np.abs(got["mean"] - mu) / d).max())
    rc = float((np.abs(got["cov"] - C) / cb).max())
    rt = abs(float(got["tv"][0]) - np.trace(C)) / R.trace_bound(x, normalize)
    print(f"D={D} N={N} normalize={normalize}: error / bound: mean {rm:.3f}, covariance {rc:.3f}, total variance {rt:.3f}")
    assert np.array_equal(bits(got["cov"]), bits(got["cov"].T.copy())), "C is not symmetric bit for bit"
    assert rm < 1 and rc < 1 and rt < 1


# ---- b. exact: integer rows with an integer mean ----------------------------------------------------------------------------------------
def test_exact():
    D, N = 32, 65537
    assert R.partition(N) == (65, 2, 33)
    x, centre = R.exact_rows(5, N, D)
    got = fit(store(x), D, 1, 0, iters=1)
    x64 = x.astype(np.float64)
    assert np.array_equal(got["mean"].astype(np.float64), x64.mean(axis=0)) and np.array_equal(got["mean"], centre.astype(np.float32))
    xc = x64 - centre
    want = (xc.T @ xc / (N - 1)).astype(np.float32)                             # integers below 2^24 over 2^16: exact
    assert np.array_equal(bits(got["cov"]), bits(want))


# ---- c. the solver on that C -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("D,N,k", [(160, 1025, 1), (160, 1025, 3), (160, 1025, 8), (32, 63, 8), (768, 1025, 3)])
def test_solver(D, N, k, normalize):
    x = rows_for(D, N, normalize)
    got = fit(store(x), D, k, normalize)
    ref = R.fit(x, k, normalize)
    spectrum = ref["spectrum"]
    assert spectrum[k] / spectrum[k - 1] < 0.6                                  # the fixture: 64 rounds converge far below rounding
    Cd, Q, lam = got["cov"].astype(np.float64), got["comp"].astype(np.float64), got["eig"].astype(np.float64)
    gram = Q @ Q.T
    norms = np.abs(np.sqrt(np.diag(gram)) - 1).max()
    off = np.abs(gram - np.diag(np.diag(gram))).max()
    assert norms <= (D / 256 + 2 * k + 16) * R.E and off <= 8 * R.E * np.sqrt(D)
    assert (np.diff(got["eig"]) <= 0).all() and all(got["comp"][j][np.argmax(np.abs(got["comp"][j]))] > 0 for j in range(k))
    tol = R.ritz_tolerance(Cd, k)
    ritz = np.linalg.norm(Q @ Cd - lam[:, None] * Q, axis=1)
    # the subspace against float64's (Davis-Kahan's sin-theta theorem on the residual of Q against C_64)
    num = np.linalg.norm(Cd - ref["cov"]) + np.sqrt(k) * tol
    gap = spectrum[k - 1] - spectrum[k]
    V = ref["components"]
    sine = np.linalg.norm(Q.T - V.T @ (V @ Q.T), 2)
    print(f"D={D} N={N} k={k} normalize={normalize}: Ritz residual / tolerance {(ritz / tol).max():.3f}, sine / bound {sine / (num / (gap - num)):.3f}, "
          f"| |q| - 1 | {norms:.1e}, largest q_i . q_j {off:.1e}")
    assert (ritz < tol).all() and num < gap and sine < num / (gap - num)
    assert np.abs(lam - ref["eigenvalues"]).max() <= num
    assert abs(float(got["tv"][0]) - ref["total_variance"]) < R.trace_bound(x, normalize)


# ---- d. the projection, with the device's own mean and components ------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("D,N,k", [(32, 2, 1), (32, 1025, 8), (160, 63, 3), (160, 1024, 1), (768, 63, 8), (768, 1025, 3)])
def test_projection(D, N, k, normalize):
    x = rows_for(D, N, normalize)
    rows = store(x)
    got = fit(rows, D, k, normalize)
    mean, comp = got["dev"]
    scores, resid = project(rows, D, normalize, mean, comp)
    s64, r64, _, _ = R.project(x, normalize, got["mean"], got["comp"])
    rs = float((np.abs(scores - s64) / R.score_bound(x, normalize, got["mean"], got["comp"])).max())
    rr = float((np.abs(resid - r64) / R.residual_bound(x, normalize, got["mean"], got["comp"])).max())
    print(f"D={D} N={N} k={k} normalize={normalize}: error / bound: scores {rs:.3f}, residual {rr:.3f}")
    assert rs < 1 and rr < 1 and (resid >= 0).all()
    if normalize and N > 4:                                                    # the zero row: u = 0, so c = -mean
        assert np.abs(scores[N // 2] - (-got["mean"].astype(np.float64)) @ got["comp"].astype(np.float64).T).max() <= \
            R.score_bound(x, normalize, got["mean"], got["comp"])[N // 2].max()
    # scale multiplies exactly once; the residual stays that of the unscaled scores
    scale = (1.0 / np.sqrt(np.maximum(got["eig"].astype(np.float64), 1e-30))).astype(np.float32)
    white, r2 = project(rows, D, normalize, mean, comp, scale=torch.from_numpy(scale).cuda())
    assert np.array_equal(bits(white), bits(scores * scale[None, :])) and np.array_equal(bits(r2), bits(resid))
    # with and without the residual; a slice that starts off the 128-row tile
    assert np.array_equal(bits(project(rows, D, normalize, mean, comp, want_resid=False)[0]), bits(scores))
    for first, n in ((0, 1), (5, min(N - 5, R.TILE)), (N - 1, 1), (R.TILE - 3, N - R.TILE + 3)):
        if first < 0 or n < 1 or first + n > N:
            continue
        part = project(rows, D, normalize, mean, comp, first=first, n=n)
        assert np.array_equal(bits(part[0]), bits(scores[first:first + n])) and np.array_equal(bits(part[1]), bits(resid[first:first + n]))


# ---- e. invariance of the fit, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [0, 1])
def test_invariance(normalize):
    D, N, k = 160, 2 * R.CHUNK + 77, 3
    x = rows_for(D, N, normalize)
    a, b, wide, tight = fit(store(x), D, k, normalize), fit(store(x), D, k, normalize), fit(store(x, pad=40), D, k, normalize), fit(store(x, pad=0), D, k, normalize)
    for key in ("mean", "comp", "eig", "tv", "cov"):
        for other in (b, wide, tight):
            assert a[key].tobytes() == other[key].tobytes(), key
    assert np.array_equal(bits(a["cov"]), bits(a["cov"].T.copy()))


# ---- f. refusals: by return code and a word of the message; none of these calls writes an output ---------------------------------------------
def test_refusals():
    lib = _lib.load()
    names = ("rows", "mean", "comp", "eig", "tv", "ws", "scale", "scores", "resid")
    bufs = {name: torch.full((1 << 18,), 3.0, device="cuda") for name in names}

    def ptrs(null, shift):
        p = {name: bufs[name].data_ptr() for name in names}
        for name in null:
            p[name] = None
        if shift:
            p[shift] += 4
        return p

    def rc_fit(n=100, D=64, ld=64, k=3, iters=2, normalize=1, ws_bytes=4 << 18, null=(), shift=None):
        p = ptrs(null, shift)
        return lib.cbas_rows_pca_fit(p["rows"], n, D, ld, k, iters, normalize, p["mean"], p["comp"], p["eig"], p["tv"], p["ws"], ws_bytes, None)

    def rc_project(n=100, D=64, ld=64, k=3, normalize=1, null=(), shift=None, **_):
        p = ptrs(null, shift)
        return lib.cbas_rows_pca_project(p["rows"], n, D, ld, k, normalize, p["mean"], p["comp"], p["scale"], p["scores"], p["resid"], None)

    def refused(code, word):
        msg = lib.cbas_last_error().decode()
        assert code == -1 and word in msg, (code, word, msg)           # CBAS_EINVAL
    for rc in (rc_fit, rc_project):
        refused(rc(k=0), "k =")
        refused(rc(k=9), "k =")
        refused(rc(D=48), "multiple of 32")
        refused(rc(D=0), "multiple of 32")
        refused(rc(D=1568, ld=1568), "multiple of 32")
        refused(rc(ld=32), "ld =")
        refused(rc(ld=68), "multiple of 8")
        refused(rc(n=-1), "n_rows")
        refused(rc(normalize=2), "normalize")
        refused(rc(normalize=-1), "normalize")
        for name in ("rows", "mean", "comp"):
            refused(rc(shift=name), "16-byte aligned")
            refused(rc(null=(name,)), "NULL")
    refused(rc_fit(n=1), "n_rows")
    refused(rc_fit(n=0), "n_rows")
    refused(rc_fit(n=16_777_217), "n_rows")
    refused(rc_fit(iters=0), "iters")
    refused(rc_fit(shift="ws"), "16-byte aligned")
    for name in ("eig", "tv", "ws"):
        refused(rc_fit(null=(name,)), "NULL")
    refused(rc_project(null=("scores",)), "NULL")
    need = int(lib.cbas_rows_pca_workspace_bytes(100, 64, 3))
    assert need == 4 * 64 * 64 + 4 * 3 * 64 + 4 * 64 + 400 and need <= 4 << 18
    refused(rc_fit(ws_bytes=need - 1), "workspace")
    for args in ((1, 64, 3), (100, 48, 3), (100, 1568, 3), (100, 64, 0), (100, 64, 9), (16_777_217, 64, 3)):
        assert lib.cbas_rows_pca_workspace_bytes(*args) == -1
    # at most 64 D x D blocks whatever n_rows: 151 MB of them at D = 768
    big = int(lib.cbas_rows_pca_workspace_bytes(2_000_000, 768, 8))
    assert big == 64 * 4 * 768 * 768 + 4 * 8 * 768 + 4 * 768 * 1954 + 4 * 2_000_000
    assert int(lib.cbas_rows_pca_workspace_bytes(16_777_216, 768, 8)) - 4 * 768 * 16384 - 4 * 16_777_216 == big - 4 * 768 * 1954 - 4 * 2_000_000
    torch.cuda.synchronize()
    for name in names:                                                 # every buffer is as it was
        assert bool((bufs[name] == 3.0).all()), name
    # the neighbours that must be served: an exact workspace, both optional pointers NULL, no rows at all
    bufs["rows"].copy_(torch.from_numpy(np.resize(np.random.default_rng(1).standard_normal(1 << 15).astype(np.float16).view(np.float32), 1 << 18)).cuda())
    assert rc_fit(ws_bytes=need) == 0
    assert rc_project(null=("scale", "resid")) == 0 and rc_project(n=0, null=("rows", "scores")) == 0
    torch.cuda.synchronize()
    assert bool((bufs["resid"] == 3.0).all()) and not bool((bufs["scores"][:300] == 3.0).any()) and bool((bufs["scores"][300:] == 3.0).all())


# ---- g. through the Python layer ------------------------------------------------------------------------------------------------------
def test_python_layer(tmp_path):
    C, D = 4, 64
    sizes = (300, 420)
    paths, truth = synth.cls_project(str(tmp_path), sizes, D, C, seed=3)
    index = S.FrameIndex(paths, "cuda:0")
    N = index.n_rows
    scores, basis = index.pca()
    assert scores.shape == (N, 3) and scores.dtype == torch.float32 and scores.is_cuda and basis.n_components == 3 and basis.normalize
    assert (basis.dim, basis.n_rows, basis.iters) == (D, N, F.DEFAULT_ITERS) and (np.diff(basis.eigenvalues) <= 0).all()
    ratio = basis.explained_variance_ratio
    assert (ratio > 0).all() and ratio.sum() <= 1 + 1e-5
    again, resid = F.project(index, basis, return_residual=True)
    assert np.array_equal(bits(again.cpu().numpy()), bits(scores.cpu().numpy())) and resid.shape == (N,) and bool((resid >= 0).all())
    direct = fit(index.rows, D, 3, 1)
    assert direct["comp"].tobytes() == basis.components.tobytes() and direct["mean"].tobytes() == basis.mean.tobytes()
    # against float64: the scores' sample variances are the eigenvalues
    host = scores.cpu().numpy().astype(np.float64)
    ref = R.fit(index.rows.cpu().numpy(), 3, 1)
    assert np.allclose(host.var(axis=0, ddof=1), ref["eigenvalues"], rtol=1e-3)
    white = F.project(index, basis, whiten=True).cpu().numpy().astype(np.float64)
    assert np.allclose(white.var(axis=0, ddof=1), 1.0, rtol=1e-3)
    # later recordings land on the earlier map: the same bits as inside the first index
    basis.save(str(tmp_path / "map.npz"))
    loaded = F.FramePCA.load(str(tmp_path / "map.npz"))
    second = S.FrameIndex(paths[1:], "cuda:0")
    s2, same = second.pca(basis=loaded)
    assert same is loaded and np.array_equal(bits(s2.cpu().numpy()), bits(scores.cpu().numpy()[300:]))
    with pytest.raises(ValueError, match="width"):
        index.pca(basis=F.FramePCA(np.zeros(32), np.zeros((3, 32)), np.zeros(3), 1.0, 32, True, 10, 64))
    with pytest.raises(ValueError, match="normalize"):
        index.pca(normalize=False, basis=loaded)
    plain = index.pca(n_components=2, normalize=False, iters=32)[1]
    assert plain.n_components == 2 and not plain.normalize and plain.iters == 32
    # the files
    frames = str(tmp_path / "frames.csv")
    F.write_frames_csv(frames, index, scores, resid)
    with open(frames, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["file", "frame", "pc1", "pc2", "pc3", "residual"] and len(rows) == N + 1 and rows[301][:2] == [paths[1], "0"]
    hits = F.outliers(index, resid, top=7, min_gap=15)
    rh = resid.cpu().numpy()
    first = {p: int(f) for p, (f, _) in zip(index.files, index._table)}
    assert len(hits) == 7 and hits[0]["residual"] == float(rh.max()) and all(a["residual"] >= b["residual"] for a, b in zip(hits, hits[1:]))
    assert all(rh[first[h["file"]] + h["frame"]] == np.float32(h["residual"]) for h in hits)
    assert all(abs(a["frame"] - b["frame"]) > 15 for i, a in enumerate(hits) for b in hits[i + 1:] if a["file"] == b["file"])
    # the command line, end to end
    clusters = index.cluster(n_clusters=4, iters=5)[2]
    clusters.save(str(tmp_path / "clusters.npz"))
    png, out_csv, cli_map = str(tmp_path / "map.png"), str(tmp_path / "outliers.csv"), str(tmp_path / "cli.npz")
    assert F.main(["--files", *paths, "--out", frames, "--png", png, "--bins", "64", "--color-by-motifs", str(tmp_path / "clusters.npz"),
                   "--outliers", out_csv, "--top", "7", "--save", cli_map]) == 0
    from PIL import Image
    with Image.open(png) as pic:
        assert pic.format == "PNG" and pic.size == (64, 64) and pic.mode == "RGB" and np.asarray(pic).max() == 255
    with open(frames, newline="") as f:
        rows = list(csv.reader(f))
    assert len(rows) == N + 1 and [float(v) for v in rows[1][2:5]] == [float(f"{v:.6g}") for v in scores.cpu().numpy()[0]]
    with open(out_csv, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == F.OUTLIER_COLUMNS and [(r[1], int(r[2])) for r in rows[1:]] == [(h["file"], h["frame"]) for h in hits]
    assert F.FramePCA.load(cli_map).components.tobytes() == basis.components.tobytes()
    assert F.main(["--files", *paths[1:], "--load", cli_map, "--out", frames, "--whiten"]) == 0
    with open(frames, newline="") as f:
        rows = list(csv.reader(f))
    assert len(rows) == 421 and os.path.exists(png)
