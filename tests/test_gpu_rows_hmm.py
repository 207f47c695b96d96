"""The motif HMM's two passes on the GPU (csrc/rows_hmm.hip through cbasx_rows_emissions / cbasx_rows_weighted_sums) and the fit
through ``FrameIndex.motif_hmm``.

  bounds       emissions (probs, lognorm) and weighted sums (sums, mass) against float64 of the very fp16 rows handed to the device,
               within the bounds rows_hmm_ref.py derives from the sum orders; cases print their largest error / bound (run with -s)
  invariance   bit for bit: two calls, a row alone against the same row inside 129, another ld
  edges        a zero row, kappa 0 (exactly the softmax of logw), kappa 1e4 (nothing non-finite), rows of zero weight
  refusals     CBAS_EINVAL with a word of the message, every output as it was
  end to end   planted states that the float64 reference alone recovers: the device's labels are the reference's, two fits and a
               saved model agree bit for bit
"""
import numpy as np
import pytest
import torch

import rows_hmm_ref as H
from cbas_amd import _lib, bouts, h5io, motif_hmm as M, search as S

pytestmark = pytest.mark.gpu

PAD = np.float16(60000.0)                  # in the columns past D: read into any sum, it shows


def store(x, pad=8):
    img = np.full((x.shape[0], x.shape[1] + pad), PAD, np.float16)
    img[:, :x.shape[1]] = x
    return torch.from_numpy(img).cuda()


def make_rows(seed, N, D):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, D)) * rng.uniform(0.3, 4.0, size=(N, 1))).astype(np.float16)
    tiny = np.float16(6.2e-5)              # no fp16 subnormals: what the MFMA does with them is not part of the contract
    x[(np.abs(x) < tiny) & (x != 0)] = tiny
    return x


def make_means(seed, C, D):
    m = np.random.default_rng(seed).standard_normal((C, D))
    return (m / np.linalg.norm(m, axis=1, keepdims=True)).astype(np.float32)


def emit(rows, D, means, kappa, logw=None, normalize=1, first=0, n=None, want_lognorm=True):
    lib = _lib.load()
    n = rows.shape[0] - first if n is None else n
    C = means.shape[0]
    mu = torch.from_numpy(np.ascontiguousarray(means, np.float32)).cuda()
    lw = None if logw is None else torch.from_numpy(np.ascontiguousarray(logw, np.float32)).cuda()
    probs = torch.full((max(n, 1), C), -7.0, device="cuda")
    lognorm = torch.full((max(n, 1),), -7.0, device="cuda") if want_lognorm else None
    _lib.check(lib.cbasx_rows_emissions(rows.data_ptr() + first * rows.shape[1] * 2, n, D, rows.shape[1], C, int(normalize), mu.data_ptr(), float(kappa),
                                        None if lw is None else lw.data_ptr(), probs.data_ptr(), None if lognorm is None else lognorm.data_ptr(), None),
               "cbasx_rows_emissions")
    torch.cuda.synchronize()
    return probs[:n].cpu().numpy(), (lognorm[:n].cpu().numpy() if want_lognorm else None)


def wsums(rows, D, w, normalize=1):
    lib = _lib.load()
    N, C = w.shape
    need = int(lib.cbasx_rows_weighted_sums_workspace_bytes(N, D, C))
    assert need == H.workspace_bytes(N, D, C), lib.cbas_last_error()
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    wd = torch.from_numpy(np.ascontiguousarray(w, np.float32)).cuda() if N else torch.zeros((1, C), device="cuda")
    sums = torch.full((C, D), -7.0, dtype=torch.float64, device="cuda")
    mass = torch.full((C,), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(lib.cbasx_rows_weighted_sums(rows.data_ptr(), N, D, rows.shape[1], C, int(normalize), wd.data_ptr(), sums.data_ptr(), mass.data_ptr(),
                                            ws.data_ptr(), need, None), "cbasx_rows_weighted_sums")
    torch.cuda.synchronize()
    return sums.cpu().numpy(), mass.cpu().numpy()


# D: one block, one chunk, a chunk tail, the product.  C: the NG boundaries.  N: the tile of the pass and one or two parts of the sums
SHAPES = [(129, 32, 1, 1), (129, 64, 2, 0), (127, 96, 15, 1), (128, 96, 16, 1), (129, 96, 17, 0), (193, 64, 33, 1), (129, 768, 64, 1),
          (1, 64, 16, 1), (63, 32, 48, 1), (64, 64, 4, 0), (65, 768, 9, 1)]


@pytest.mark.parametrize("N,D,C,normalize", SHAPES)
def test_emissions_within_bounds(N, D, C, normalize):
    x, means = make_rows(N + D, N, D), make_means(C, C, D)
    if N > 5:
        x[5] = 0                                                               # a zero row
    logw = np.random.default_rng(3).standard_normal(C).astype(np.float32)
    rows = store(x)
    for kappa, lw in ((8.0, logw), (60.0, None)):
        probs, lognorm = emit(rows, D, means, kappa, lw, normalize)
        want_p, want_l = H.emissions(x, means, kappa, lw, normalize)
        pb, lb = H.emissions_bound(x, means, kappa, lw, normalize)
        rp, rl = (np.abs(probs - want_p) / pb).max(), (np.abs(lognorm - want_l) / lb).max()
        print(f"N={N} D={D} C={C} norm={normalize} kappa={kappa}: probs error/bound {rp:.3f}, lognorm error/bound {rl:.3f}")
        assert np.isfinite(probs).all() and rp <= 1.0 and rl <= 1.0
        assert np.abs(probs.astype(np.float64).sum(axis=1) - 1).max() <= H.E + H.g(7)      # the division's rounding and the device's own sum
        if N > 5 and lw is not None:
            soft = np.exp(lw.astype(np.float64) - lw.max())
            assert np.abs(probs[5] - soft / soft.sum()).max() <= 16 * H.E      # expf to 2 ulp, the sum's g(7), the division


def test_emissions_edges_and_invariance():
    N, D, C = 129, 96, 17
    x, means = make_rows(1, N, D), make_means(2, C, D)
    x[40] = 0
    logw = np.random.default_rng(4).standard_normal(C).astype(np.float32)
    rows = store(x)
    a, la = emit(rows, D, means, 20.0, logw)
    b, lb = emit(rows, D, means, 20.0, logw)
    assert a.tobytes() == b.tobytes() and la.tobytes() == lb.tobytes()                   # two calls
    wide = store(x, pad=40)
    c, lc = emit(wide, D, means, 20.0, logw)
    assert a.tobytes() == c.tobytes() and la.tobytes() == lc.tobytes()                   # another ld
    for r in (0, 40, 77, 128):                                                           # a row alone, wherever it lay
        one, lone = emit(rows, D, means, 20.0, logw, first=r, n=1)
        assert one[0].tobytes() == a[r].tobytes() and lone[0].tobytes() == la[r].tobytes(), r
    quiet, none = emit(rows, D, means, 20.0, logw, want_lognorm=False)
    assert none is None and quiet.tobytes() == a.tobytes()
    # kappa 0 and a zero row: exactly the softmax of logw, the same bits in every row
    zero, lz = emit(rows, D, means, 0.0, logw)
    assert all(zero[r].tobytes() == zero[0].tobytes() for r in range(N)) and zero[0].tobytes() == a[40].tobytes()
    soft = np.exp(logw.astype(np.float64) - logw.max())
    assert np.abs(zero[0] - soft / soft.sum()).max() <= 16 * H.E and np.abs(lz - np.log2(np.exp(logw.astype(np.float64)).sum())).max() <= 1e-5
    flat, lf = emit(rows, D, means, 0.0, None)
    assert (flat == np.float32(1.0) / np.float32(C)).all() and np.abs(lf - np.log2(C)).max() <= 2e-6
    # kappa 1e4: near one-hot, nothing non-finite, still within the bound
    hot, lh = emit(rows, D, means, 1e4, None)
    assert np.isfinite(hot).all() and np.isfinite(lh).all() and np.abs(hot.sum(axis=1) - 1).max() <= 1e-6
    want_p, want_l = H.emissions(x, means, 1e4)
    pb, lbnd = H.emissions_bound(x, means, 1e4)
    assert (np.abs(hot - want_p) <= pb).all() and (np.abs(lh - want_l) <= lbnd).all()
    assert (np.delete(hot, 40, axis=0).max(axis=1) > 0.5).mean() > 0.9
    assert emit(rows, D, means, 1.0, n=0)[0].shape == (0, C)


# N: one row either side of one part (64 rows) and of two, a ragged block, several parts; C and D as above
SUM_SHAPES = [(1, 32, 1, 1), (63, 64, 2, 0), (64, 64, 15, 1), (65, 96, 16, 1), (127, 96, 17, 0), (128, 32, 33, 1), (129, 768, 64, 1),
              (129, 768, 9, 1), (300, 640, 20, 1), (1000, 1536, 5, 0), (16449, 32, 3, 1)]      # the last: parts of 128 rows


@pytest.mark.parametrize("N,D,C,normalize", SUM_SHAPES)
def test_weighted_sums_within_bounds(N, D, C, normalize):
    rng = np.random.default_rng(N + C)
    x = make_rows(N + D + 1, N, D)
    w = rng.dirichlet(np.ones(C) * 0.3, size=N).astype(np.float32)
    w[rng.random(N) < 0.2] = 0                                                 # frames outside every clip: rows of zero weight
    if N > 3:
        x[3] = 0
    rows = store(x)
    sums, mass = wsums(rows, D, w, normalize)
    want_s, want_m = H.weighted_sums(x, w, normalize)
    sb, mb = H.sums_bound(x, w, normalize)
    rs = (np.abs(sums - want_s) / np.maximum(sb, 1e-300)).max()
    rm = (np.abs(mass - want_m) / np.maximum(mb, 1e-300)).max()
    print(f"N={N} D={D} C={C} norm={normalize}: sums error/bound {rs:.3f}, mass error/bound {rm:.3f}")
    assert (np.abs(sums - want_s) <= sb).all() and (np.abs(mass - want_m) <= mb).all()
    again = wsums(rows, D, w, normalize)
    assert again[0].tobytes() == sums.tobytes() and again[1].tobytes() == mass.tobytes()
    wide = wsums(store(x, pad=24), D, w, normalize)
    assert wide[0].tobytes() == sums.tobytes() and wide[1].tobytes() == mass.tobytes()


def test_weighted_sums_edges():
    N, D, C = 129, 64, 4
    x = make_rows(9, N, D)
    rows = store(x)
    sums, mass = wsums(rows, D, np.zeros((N, C), np.float32))
    assert (sums == 0).all() and (mass == 0).all()
    w = np.zeros((N, C), np.float32)
    w[70, 2] = 1.0                                                             # one row, one state: that row's u, whatever the part
    sums, mass = wsums(rows, D, w)
    u = H.R.working_rows(x[70:71], 1)[0]
    assert (np.delete(sums, 2, axis=0) == 0).all() and mass.tolist() == [0, 0, 1, 0] and (np.abs(sums[2] - u) <= H.sums_bound(x, w)[0][2]).all()
    w[100, 1] = np.nan                                                         # a NaN weight propagates into its state alone
    sums, mass = wsums(rows, D, w)
    assert np.isnan(sums[1]).all() and np.isnan(mass[1]) and np.isfinite(sums[[0, 2, 3]]).all() and np.isfinite(mass[[0, 2, 3]]).all()
    empty = wsums(rows, D, np.zeros((0, C), np.float32))                       # no rows: zeros
    assert (empty[0] == 0).all() and (empty[1] == 0).all()


def test_refusals():
    lib = _lib.load()
    names = ("rows", "means", "logw", "probs", "lognorm", "w", "sums", "mass", "ws")
    bufs = {name: torch.full((1 << 18,), 3.0, device="cuda") for name in names}

    def ptrs(null, shift):
        p = {name: bufs[name].data_ptr() for name in names}
        for name in null:
            p[name] = None
        if shift:
            p[shift] += 4
        return p

    def rc_emit(n=100, D=64, ld=64, C=5, normalize=1, kappa=2.0, null=(), shift=None):
        p = ptrs(null, shift)
        return lib.cbasx_rows_emissions(p["rows"], n, D, ld, C, normalize, p["means"], kappa, p["logw"], p["probs"], p["lognorm"], None)

    def rc_sums(n=100, D=64, ld=64, C=5, normalize=1, ws_bytes=4 << 18, null=(), shift=None, kappa=None):
        p = ptrs(null, shift)
        return lib.cbasx_rows_weighted_sums(p["rows"], n, D, ld, C, normalize, p["w"], p["sums"], p["mass"], p["ws"], ws_bytes, None)

    def refused(code, word):
        msg = lib.cbas_last_error().decode()
        assert code == -1 and word in msg, (code, word, msg)                   # CBAS_EINVAL
    for rc in (rc_emit, rc_sums):
        refused(rc(C=0), "C =")
        refused(rc(C=65), "C =")
        refused(rc(D=48), "multiple of 32")
        refused(rc(D=0), "multiple of 32")
        refused(rc(D=1568, ld=1568), "multiple of 32")
        refused(rc(ld=32), "ld =")
        refused(rc(ld=68), "multiple of 8")
        refused(rc(n=-1), "n_rows")
        refused(rc(normalize=2), "normalize")
        refused(rc(shift="rows"), "16-byte aligned")
        refused(rc(null=("rows",)), "NULL")
    for kappa in (-1.0, float("nan"), float("inf")):
        refused(rc_emit(kappa=kappa), "kappa")
    for name in ("means", "probs"):
        refused(rc_emit(null=(name,)), "NULL")
    refused(rc_emit(shift="means"), "16-byte aligned")
    for name in ("w", "sums", "mass", "ws"):
        refused(rc_sums(null=(name,)), "NULL")
    refused(rc_sums(shift="ws"), "16-byte aligned")
    refused(rc_sums(shift="sums"), "8-byte aligned")
    need = int(lib.cbasx_rows_weighted_sums_workspace_bytes(100, 64, 5))
    assert need == H.workspace_bytes(100, 64, 5) <= 4 << 18
    refused(rc_sums(ws_bytes=need - 1), "workspace")
    for args in ((-1, 64, 5), (100, 48, 5), (100, 1568, 5), (100, 64, 0), (100, 64, 65)):
        assert lib.cbasx_rows_weighted_sums_workspace_bytes(*args) == -1
    assert int(lib.cbasx_rows_weighted_sums_workspace_bytes(2_000_000, 768, 64)) == H.workspace_bytes(2_000_000, 768, 64) <= 256 * (4 * 64 * 768 + 256)
    torch.cuda.synchronize()
    for name in names:                                                         # every buffer is as it was
        assert bool((bufs[name] == 3.0).all()), name
    # the neighbours that must be served: an exact workspace, every optional pointer NULL
    assert rc_emit(null=("logw", "lognorm")) == 0 and rc_sums(ws_bytes=need) == 0
    torch.cuda.synchronize()
    assert bool((bufs["lognorm"] == 3.0).all()) and not bool((bufs["probs"][:500] == 3.0).any()) and not bool((bufs["sums"][:640] == 3.0).any())


def test_planted_states_end_to_end(tmp_path):
    x, table, states, dirs = H.planted(seed=5, lengths=(300, 1500, 40), D=64, C=4)
    C, D = dirs.shape
    start = dirs + 0.25 * np.random.default_rng(1).standard_normal(dirs.shape)
    start = (start / np.linalg.norm(start, axis=1, keepdims=True)).astype(np.float32)
    A0 = bouts.sticky_transitions(C, mean_duration=40, as_probs=True).astype(np.float64)
    want = H.fit(x, table, start, A0, kappa=10.0, iters=5)
    ref_labels = want["gamma"].argmax(axis=1)
    top = np.sort(want["gamma"], axis=1)
    match = (want["means"] @ dirs.T).argmax(axis=1)
    assert np.array_equal(match[ref_labels], states) and (top[:, -1] - top[:, -2]).min() > 0.5       # the reference alone reaches them
    paths = []
    for i, (first, n) in enumerate(table):
        paths.append(str(tmp_path / f"clip{i}_cls.h5"))
        with h5io.ClsWriter(paths[-1], D) as w:
            w.append(x[first:first + n])
    index = S.FrameIndex(paths, "cuda:0")
    gamma, model = index.motif_hmm(iters=5, temperature=0.1, init=start)
    assert gamma.is_cuda and gamma.dtype == torch.float32 and gamma.shape == (x.shape[0], C)
    assert np.array_equal(gamma.argmax(dim=1).cpu().numpy(), ref_labels) and np.array_equal(model.labels(index).cpu().numpy(), ref_labels)
    print("gamma error", np.abs(gamma.cpu().numpy() - want["gamma"]).max(), "means error", np.abs(model.means - want["means"]).max(),
          "loglik", model.loglik, want["loglik"])
    assert np.abs(gamma.cpu().numpy() - want["gamma"]).max() < 1e-3 and np.abs(model.means - want["means"]).max() < 1e-4
    assert np.abs(model.loglik - want["loglik"]).max() <= 1e-5 * np.abs(want["loglik"]).max()
    g2, m2 = index.motif_hmm(iters=5, temperature=0.1, init=start)
    assert torch.equal(g2, gamma)
    for key in ("means", "transitions", "prior", "occupancy", "loglik"):
        assert getattr(m2, key).tobytes() == getattr(model, key).tobytes(), key
    model.save(str(tmp_path / "hmm.npz"))
    assert torch.equal(M.MotifHMM.load(str(tmp_path / "hmm.npz")).posteriors(index), gamma)
    # the default start and the calibrated temperature find the same states
    g3, auto = index.motif_hmm(n_states=C, iters=5)
    m3 = (auto.means @ dirs.T).argmax(axis=1)
    assert 0.005 < auto.temperature < 1.0 and np.array_equal(m3[g3.argmax(dim=1).cpu().numpy()], states)
