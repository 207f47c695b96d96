"""The host side of the PCA over resident CLS rows: the library surface, the float64 restatement against numpy.cov + eigh, the partition
of the covariance pass, and the parts of cbas_amd.framemap that need no GPU."""
import os
import re
import types

import numpy as np
import pytest
import torch

import rows_pca_ref as R
from cbas_amd import _lib, framemap as F, search as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cbas_rows_pca_workspace_bytes", "cbas_rows_pca_fit", "cbas_rows_pca_project")


# ---- the library surface -----------------------------------------------------------------------------------------------------------
def test_signatures_header_and_readme():
    from ctypes import c_int, c_int32, c_int64, c_void_p
    for name in NAMES:
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES[NAMES[0]] == (c_int64, [c_int64, c_int32, c_int32])
    res, args = _lib.SIGNATURES[NAMES[1]]
    assert res is c_int and args == [c_void_p, c_int64, c_int32, c_int64, c_int32, c_int32, c_int32] + [c_void_p] * 5 + [c_int64, c_void_p]
    res, args = _lib.SIGNATURES[NAMES[2]]
    assert res is c_int and args == [c_void_p, c_int64, c_int32, c_int64, c_int32, c_int32] + [c_void_p] * 6
    with open(os.path.join(ROOT, "include", "cbas_mi355x.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\(", header), name
    assert re.search(r"#define CBAS_ROWS_PCA_CHUNK\s+(\d+)", header).group(1) == str(F.CHUNK) == str(R.CHUNK)
    assert re.search(r"#define CBAS_ROWS_PCA_MAX_PARTS\s+(\d+)", header).group(1) == str(F.MAX_PARTS) == str(R.MAX_PARTS)
    assert re.search(r"#define CBAS_ABI_VERSION\s+11\b", header)                  # additive entry points: the version stays
    with open(os.path.join(ROOT, "cbas_amd", "csrc", "exports.map")) as f:
        assert "cbas_*" in f.read()
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert f"{len(_lib.SIGNATURES)} entry points" in readme and len(_lib.SIGNATURES) == 88 and "cbas_amd.framemap" in readme
    from cbas_amd import build, encoder
    assert "rows_pca.hip" in build.SOURCES and build.EXTRA_FLAGS["rows_pca.hip"] == build.NO_PACKED
    assert os.path.exists(os.path.join(build.CSRC, "rows_pca.hip")) and R.TILE == F.TILE
    assert F.DEFAULT_ITERS == encoder.PCA_DEFAULT_ITERS and (F.MAX_COMPONENTS, F.MAX_DIM) == (R.MAX_K, R.MAX_D)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [0, 1])
def test_restatement_against_numpy(normalize):
    N, D, k = 700, 64, 3
    x = R.planted(3, N, D)
    x[11] = 0                                                                   # a zero row: u = 0 under normalize
    u = R.working_rows(x, normalize)
    if normalize:
        norms = np.linalg.norm(u, axis=1)
        assert np.abs(np.delete(norms, 11) - 1).max() < 1e-4 and (u[11] == 0).all()
        exact = x.astype(np.float64) / np.maximum(np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True), 1e-300)
        assert np.abs(u - exact).max() <= (R.g(D / 4 + 2) / 2 + 2 * R.E) * np.abs(exact).max()        # rn: the sum's roundings halved, one more
    else:
        assert np.array_equal(u, x.astype(np.float64))
    out = R.fit(x, k, normalize)
    assert np.allclose(out["mean"], u.mean(axis=0), rtol=0, atol=1e-13) and np.allclose(out["cov"], np.cov(u, rowvar=False), rtol=0, atol=1e-12)
    w, V = np.linalg.eigh(np.cov(u, rowvar=False))
    assert np.allclose(out["eigenvalues"], w[::-1][:k], rtol=1e-12) and abs(out["total_variance"] - w.sum()) < 1e-10
    for j in range(k):
        q = out["components"][j]
        assert abs(abs(q @ V[:, -1 - j]) - 1) < 1e-9 and q[np.argmax(np.abs(q))] > 0                 # the sign rule
    spectrum = out["spectrum"]
    if not normalize:
        assert (spectrum[:R.PLANTED - 1] >= 2 * spectrum[1:R.PLANTED]).all()                        # well separated: each twice the next
    scores, resid, c, _ = R.project(x, normalize, out["mean"], out["components"])
    assert np.allclose(scores.var(axis=0, ddof=1), out["eigenvalues"], rtol=1e-9) and np.abs(scores.mean(axis=0)).max() < 1e-12
    assert np.allclose(resid.sum() / (N - 1), spectrum[k:].sum(), rtol=1e-9) and (resid >= 0).all()
    white = R.project(x, normalize, out["mean"], out["components"], 1 / np.sqrt(out["eigenvalues"]))[0]
    assert np.allclose(white.var(axis=0, ddof=1), 1.0, rtol=1e-9)


def test_bounds_are_small_and_positive():
    for N, D in ((2, 32), (1025, 160), (3000, 768)):
        for normalize in (0, 1):
            x = R.planted(N + D, N, D)
            out = R.fit(x, min(3, N - 1), normalize)
            cb, d = R.cov_bound(x, normalize)
            assert (d > 0).all() and (cb > 0).all() and np.array_equal(d, R.mean_bound(x, normalize))
            assert cb.max() < 1e-3 * max(np.abs(out["cov"]).max(), 1e-6) * 50 and R.trace_bound(x, normalize) > np.trace(cb)
            sb = R.score_bound(x, normalize, out["mean"], out["components"])
            rb = R.residual_bound(x, normalize, out["mean"], out["components"])
            assert sb.shape == (N, min(3, N - 1)) and (sb > 0).all() and sb.max() < 1e-3 and (rb > 0).all() and rb.max() < 1e-2
            assert 0 < R.ritz_tolerance(out["cov"], 3) < 1e-3 * max(out["total_variance"], 1e-3)
    x, c = R.exact_rows(1, 2049, 32)
    assert np.array_equal(x.astype(np.float64).mean(axis=0), c) and np.abs(x.astype(np.float64) - c).max() <= 3


# ---- the partition -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [2, 1024, 1025, 65536, 65537, 2_000_000, 16_777_216])
def test_partition(n_rows):
    chunks, per, parts = R.partition(n_rows)
    assert (chunks, per, parts) == F.partition(n_rows)
    assert chunks == -(-n_rows // R.CHUNK) and 1 <= parts <= R.MAX_PARTS and per == -(-chunks // R.MAX_PARTS)
    spans = R.part_spans(n_rows)
    assert len(spans) == parts and spans[0][0] == 0 and all(n >= 1 for _, n in spans)
    assert all(a + n == b for (a, n), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] == n_rows      # every row once
    assert all(a % R.CHUNK == 0 and n <= per * R.CHUNK for a, n in spans)
    if n_rows == 65537:
        assert (chunks, per, parts) == (65, 2, 33) and spans[-1][1] == 1            # two chunks a part, the last part short
    if n_rows == 2_000_000:
        assert (chunks, per, parts) == (1954, 31, 64)


# ---- cbas_amd.framemap without a GPU -------------------------------------------------------------------------------------------------
def some_basis(D=32, k=3, normalize=True):
    rng = np.random.default_rng(4)
    return F.FramePCA(rng.standard_normal(D), rng.standard_normal((k, D)), [3.0, 2.0, 0.5][:k], 6.5, D, normalize, 1234, 64)


def test_basis_round_trip(tmp_path):
    a = some_basis()
    path = str(tmp_path / "map.npz")
    a.save(path)
    b = F.FramePCA.load(path)
    for key in ("mean", "components", "eigenvalues"):
        assert getattr(b, key).tobytes() == getattr(a, key).tobytes() and getattr(b, key).dtype == np.float32
    assert (b.total_variance, b.dim, b.normalize, b.n_rows, b.iters, b.n_components) == (6.5, 32, True, 1234, 64, 3)
    assert np.allclose(b.explained_variance_ratio, [3 / 6.5, 2 / 6.5, 0.5 / 6.5]) and b.explained_variance_ratio.dtype == np.float32
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == {"mean", "components", "eigenvalues", "total_variance", "dim", "normalize", "n_rows", "iters"}
    with pytest.raises(ValueError, match="width"):
        F.FramePCA(np.zeros(16), np.zeros((3, 32)), np.zeros(3), 1.0, 32, True, 10, 64)
    with pytest.raises(ValueError, match="width"):
        F.FramePCA(np.zeros(32), np.zeros((9, 32)), np.zeros(9), 1.0, 32, True, 10, 64)


def test_density_map_by_hand():
    scores = np.array([[0.0, 0.0, 9.0], [1.0, 1.0, 9.0], [0.1, 0.2, 9.0], [0.9, 0.1, 9.0], [0.49, 0.99, 9.0]], np.float32)
    counts, extent = F.density_map(scores, bins=2)
    assert extent == (0.0, 1.0, 0.0, 1.0) and counts.dtype == np.int64
    assert counts.tolist() == [[2, 1], [1, 1]]                                  # counts[iy, ix]; the point on the upper edge in the last bin
    labels = np.array([0, 2, 0, 1, 2])
    per, _ = F.density_map(torch.from_numpy(scores), bins=2, labels=labels, n_labels=3)
    assert per.shape == (2, 2, 3) and np.array_equal(per.sum(axis=2), counts)
    assert per[0, 0].tolist() == [2, 0, 0] and per[0, 1].tolist() == [0, 1, 0] and per[1, 0].tolist() == [0, 0, 1] and per[1, 1].tolist() == [0, 0, 1]
    clipped, _ = F.density_map(scores, bins=2, extent=(0.0, 0.5, 0.0, 0.5))
    assert clipped.tolist() == [[2, 0], [0, 0]]                                 # frames outside the extent are not counted
    other, _ = F.density_map(scores, bins=1, components=(0, 2))
    assert other.tolist() == [[5]]
    for bad in (dict(bins=0), dict(components=(0, 3)), dict(labels=np.zeros(4, int)), dict(labels=labels, n_labels=2), dict(extent=(1, 0, 0, 1))):
        with pytest.raises(ValueError):
            F.density_map(scores, **{"bins": 2, **bad})
    img = F.render_map(counts)
    assert img.shape == (2, 2, 3) and img.dtype == np.uint8 and img[1, 0].tolist() == [255, 255, 255]        # y upwards: the fullest bin, white
    assert img[0, 0, 0] == img[0, 1, 0] == img[1, 1, 0] == int(255 * np.log(2) / np.log(3))
    col = F.render_map(per)
    pal = F.label_palette(3)
    assert col[1, 0].tolist() == (pal[0] * 255).astype(np.uint8).tolist() and col[0, 0].tolist() == (np.log(2) / np.log(3) * pal[2] * 255).astype(np.uint8).tolist()
    with pytest.raises(ValueError, match="counts"):
        F.render_map(np.zeros((2, 3)))


def test_render_map_writes_a_png(tmp_path):
    from PIL import Image
    counts, _ = F.density_map(np.random.default_rng(0).standard_normal((500, 2)), bins=16, labels=np.arange(500) % 4, n_labels=4)
    path = str(tmp_path / "map.png")
    img = F.render_map(counts, path, size=64)
    with Image.open(path) as pic:
        assert pic.format == "PNG" and pic.size == (64, 64) and pic.mode == "RGB"
    assert img.shape == (16, 16, 3)


def fake_index(device="cpu", dim=32, sizes=(6, 4)):
    table = np.array([[sum(sizes[:i]), n] for i, n in enumerate(sizes)], np.int64)
    idx = types.SimpleNamespace(device=torch.device(device), dim=dim, n_rows=int(sum(sizes)), files=[f"clip{i}_cls.h5" for i in range(len(sizes))],
                                _table=table, rows=torch.zeros((int(sum(sizes)), dim), dtype=torch.float16))

    def locate(m):
        i = int(np.searchsorted(table[:, 0], m, side="right")) - 1
        return idx.files[i], int(m - table[i, 0])
    idx.locate = locate
    return idx


def test_outliers_and_csv_on_the_host(tmp_path):
    import csv
    index = fake_index()
    resid = np.array([0.1, 5.0, 4.0, 0.2, 4.5, 0.3, 9.0, 9.0, 0.1, 3.0], np.float32)
    hits = F.outliers(index, resid, top=10, min_gap=1)
    # file 0: peaks at 1 and 4 (2 is beside a larger one); file 1: frames 0 and 1 are equal, the earlier is the peak; frame 3
    assert [(h["file"], h["frame"]) for h in hits] == [("clip1_cls.h5", 0), ("clip0_cls.h5", 1), ("clip0_cls.h5", 4), ("clip1_cls.h5", 3)]
    assert [h["residual"] for h in hits] == [9.0, 5.0, 4.5, 3.0]
    assert [(h["file"], h["frame"]) for h in F.outliers(index, resid, top=2, min_gap=5)] == [("clip1_cls.h5", 0), ("clip0_cls.h5", 1)]
    assert len(F.outliers(index, resid, top=50, min_gap=0)) == 10                  # no gap: every frame is its own peak
    with pytest.raises(ValueError, match="residual"):
        F.outliers(index, resid[:5])
    with pytest.raises(ValueError, match="top"):
        F.outliers(index, resid, top=0)
    scores = np.arange(20, dtype=np.float32).reshape(10, 2) / 4
    path = str(tmp_path / "frames.csv")
    F.write_frames_csv(path, index, scores, resid)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["file", "frame", "pc1", "pc2", "residual"] and len(rows) == 11
    assert rows[1] == ["clip0_cls.h5", "0", "0", "0.25", "0.1"] and rows[7][:2] == ["clip1_cls.h5", "0"] and rows[10][:2] == ["clip1_cls.h5", "3"]
    F.write_frames_csv(path, index, torch.from_numpy(scores))
    with open(path, newline="") as f:
        assert next(csv.reader(f)) == ["file", "frame", "pc1", "pc2"]
    with pytest.raises(ValueError, match="scores"):
        F.write_frames_csv(path, index, scores[:3])
    F.write_outliers_csv(path, hits)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == F.OUTLIER_COLUMNS and rows[1] == ["0", "clip1_cls.h5", "0", "9"]


def test_refusals_without_a_gpu():
    index, basis = fake_index(), some_basis()
    with pytest.raises(RuntimeError, match="GPU"):
        F.fit_pca(index)
    with pytest.raises(RuntimeError, match="GPU"):
        F.project(index, basis)
    with pytest.raises(RuntimeError, match="GPU"):
        F.pca_frames(index, basis=basis)
    with pytest.raises(ValueError, match="GPU"):
        F.project_rows(index.rows, basis)
    assert "basis" in S.FrameIndex.pca.__code__.co_varnames
    gpu_like = fake_index()
    gpu_like.device = types.SimpleNamespace(type="cuda")                          # past the device check: the basis is looked at next
    with pytest.raises(ValueError, match="width 64"):
        F.project(gpu_like, some_basis(D=64))
    with pytest.raises(ValueError, match="normalize"):
        F.project(gpu_like, some_basis(normalize=False), normalize=True)
    with pytest.raises(ValueError, match="normalize"):
        F.pca_frames(gpu_like, normalize=False, basis=basis)
    for bad in (dict(n_components=0), dict(n_components=9), dict(iters=0)):
        with pytest.raises(ValueError):
            F.fit_pca(gpu_like, **bad)
    gpu_like.n_rows = 1
    with pytest.raises(ValueError, match="rows"):
        F.fit_pca(gpu_like)


def test_cli_parser():
    _, a = F.parse_cli(["--dir", "rec", "--out", "f.csv"])
    assert (a.dir, a.components, a.no_normalize, a.whiten, a.load, a.save, a.out, a.png, a.color_by_motifs, a.color_by_outputs, a.outliers) == \
        ("rec", 3, False, False, None, None, "f.csv", None, None, None, None)
    _, a = F.parse_cli(["--files", "a_cls.h5", "b_cls.h5", "--components", "8", "--no-normalize", "--whiten", "--save", "m.npz", "--out", "f.csv",
                        "--png", "m.png", "--color-by-motifs", "c.npz", "--outliers", "o.csv"])
    assert a.files == ["a_cls.h5", "b_cls.h5"] and (a.components, a.no_normalize, a.whiten, a.save, a.png, a.color_by_motifs, a.outliers) == \
        (8, True, True, "m.npz", "m.png", "c.npz", "o.csv")
    _, a = F.parse_cli(["--dir", "rec", "--load", "m.npz", "--out", "f.csv", "--png", "m.png", "--color-by-outputs", "probe"])
    assert a.load == "m.npz" and a.color_by_outputs == "probe"
    for bad in (["--dir", "rec"],                                                                    # no --out
                ["--out", "f.csv"],                                                                  # no rows
                ["--dir", "rec", "--files", "a_cls.h5", "--out", "f.csv"],
                ["--dir", "rec", "--out", "f.csv", "--components", "0"],
                ["--dir", "rec", "--out", "f.csv", "--components", "9"],
                ["--dir", "rec", "--out", "f.csv", "--iters", "0"],
                ["--dir", "rec", "--out", "f.csv", "--png", "m.png", "--bins", "0"],
                ["--dir", "rec", "--out", "f.csv", "--outliers", "o.csv", "--top", "0"],
                ["--dir", "rec", "--out", "f.csv", "--outliers", "o.csv", "--min-gap", "-1"],
                ["--dir", "rec", "--out", "f.csv", "--load", "m.npz", "--save", "n.npz"],
                ["--dir", "rec", "--out", "f.csv", "--load", "m.npz", "--no-normalize"],
                ["--dir", "rec", "--out", "f.csv", "--load", "m.npz", "--iters", "8"],
                ["--dir", "rec", "--out", "f.csv", "--color-by-motifs", "c.npz"],                    # a colour without a picture
                ["--dir", "rec", "--out", "f.csv", "--color-by-outputs", "probe"],
                ["--dir", "rec", "--out", "f.csv", "--png", "m.png", "--color-by-motifs", "c.npz", "--color-by-outputs", "probe"],
                ["--dir", "rec", "--out", "f.csv", "--png", "m.png", "--components", "1"]):
        with pytest.raises(SystemExit):
            F.parse_cli(bad)
