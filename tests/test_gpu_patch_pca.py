"""Patch-feature PCA on the GPU (csrc/patch_pca.hip through cbas_patch_pca_fit / cbas_patch_pca_project), against float64 computed
from the very fp32 rows handed to the device, then through DinoEncoder.patch_pca and attention_maps.  Every bound was fixed before
the first run (u = 2^-24):

  mean         two-stage sum, 64 rows per partial, partials in order, one division:
               |mu^ - mu| <= (ceil(M / 64) + min(M, 64) + 1) u mean_m |x_m|
  covariance   patch_pca_ref.cov_bound: per element, M products as ceil(M / 1024) fmaf chains of at most 1024 terms (the fp32 MFMA
               is an fmaf chain), the chains added in order, one division, each factor fl(x - mu^):
               |C^_ij - C_ij| <= gamma sum_m a_mi a_mj / (M - 1) + M d_i d_j / (M - 1),  gamma = (ceil(M / 1024) + min(M, 1024) + 4) u,
               a_mi = |x~_mi| + d_i, d_i the mean's bound above (the rounded mean's term: the centred rows sum to zero, so a shift d of
               the mean adds exactly M d_i d_j to the sum of products).  C^ is symmetric bit for bit.
  eigenpairs   Davis-Kahan with the margin 4 the issue fixes: sin(q^_j, v_j) <= 4 E / gap_j and |lambda^_j - lambda_j| <= 4 E with
               E = ||C^ - C||_F + D u lambda_1 (the iteration's own rounding) and gap_j the distance from lambda_j to its nearest
               neighbour in the float64 spectrum; total_variance: the covariance bound summed over the diagonal.
  projection   (D / 64 + 8) u sum_d |x_d - mu^_d| |q_d| against float64 (x - mu^) . q^ with the device's own mu^ and q^: a lane's
               fmaf chain of D / 64 terms, the subtraction's rounding, a 6-level tree.
The largest error / bound of each case is printed (run with -s)."""
import numpy as np
import pytest
import torch

import patch_pca_ref as R
from cbas_amd import _lib, attention_maps as A, config as C, weights as W, synth
from cbas_amd.encoder import PCA_DEFAULT_ITERS, DinoEncoder, PatchPCABasis, token_grid

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FRAME, BATCH = _lib.PCA_FRAME, _lib.PCA_BATCH
SENTINEL = np.float32(1.0e30)             # in the prefix rows and the columns past D: read into any sum, it shows


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32)


def fit(rows, n_prefix, D, k, scope, iters=PCA_DEFAULT_ITERS):
    """cbas_patch_pca_fit on a float32 (n, T, ld) numpy image.  Returns numpy mean (b, D), components (b, k, D), eigenvalues (b, k),
    total_variance (b,), the covariances (b, D, D) read back from the workspace, and the device tensors of the basis."""
    lib = _lib.load()
    n, T, ld = rows.shape
    dev = torch.from_numpy(rows).cuda()
    b = 1 if scope == BATCH else n
    M = (T - n_prefix) * (n if scope == BATCH else 1)
    need = int(lib.cbas_patch_pca_workspace_bytes(n, T, n_prefix, D, k, scope))
    assert need > 0, lib.cbas_last_error()
    ws = torch.zeros(need // 4, dtype=torch.float32, device="cuda")
    mean, comp = torch.empty(b, D, device="cuda"), torch.empty(b, k, D, device="cuda")
    eig, tv = torch.empty(b, k, device="cuda"), torch.empty(b, device="cuda")
    _lib.check(lib.cbas_patch_pca_fit(dev.data_ptr(), n, T, n_prefix, D, ld, k, scope, iters, mean.data_ptr(), comp.data_ptr(),
                                      eig.data_ptr(), tv.data_ptr(), ws.data_ptr(), need, None), "cbas_patch_pca_fit")
    torch.cuda.synchronize()
    nch = -(-M // R.CHUNK)
    cov = ws[:b * nch * D * D].reshape(b, nch, D, D)[:, 0].cpu().numpy()
    return dict(mean=mean.cpu().numpy(), comp=comp.cpu().numpy(), eig=eig.cpu().numpy(), tv=tv.cpu().numpy(), cov=cov,
                dev=(dev, mean, comp))


def project(dev_rows, n_prefix, D, k, mean, comp):
    lib = _lib.load()
    n, T, ld = dev_rows.shape
    scores = torch.empty(n, T - n_prefix, k, device="cuda")
    _lib.check(lib.cbas_patch_pca_project(dev_rows.data_ptr(), n, T, n_prefix, D, ld, k, mean.shape[0], mean.data_ptr(), comp.data_ptr(),
                                          scores.data_ptr(), None), "cbas_patch_pca_project")
    torch.cuda.synchronize()
    return scores


def random_rows(seed, n, P, n_prefix, D, ld):
    rng = np.random.default_rng(seed)
    x = np.full((n, n_prefix + P, ld), SENTINEL, np.float32)
    scale = rng.uniform(0.2, 3.0, D)
    x[:, n_prefix:, :D] = (rng.standard_normal((n, P, D)) * scale + rng.uniform(-5.0, 5.0, D)).astype(np.float32)
    return x


def problems(rows, n_prefix, D, scope):
    """The (M, D) float32 row sets of the problems of an (n, T, ld) image."""
    patches = rows[:, n_prefix:, :D]
    return [patches.reshape(-1, D)] if scope == BATCH else list(patches)


# ---- a. mean and covariance -----------------------------------------------------------------------------------------------------
# (D, P, n, n_prefix, ld - D, scope): every D, P, n, n_prefix and ld of the issue at least once; P around one and two row chunks; a
# BATCH problem whose chunk boundary falls inside a frame (683 x 3 = 2049 rows); D = 32 (one partly filled tile), 96, 384 (3 x 3
# tiles) and 1280 (10 x 10)
COV_CASES = [(32, 2, 1, 0, 0, FRAME), (32, 5, 3, 1, 32, FRAME), (96, 63, 3, 5, 0, BATCH), (96, 64, 1, 0, 32, FRAME),
             (96, 65, 3, 1, 0, FRAME), (384, 257, 1, 5, 32, BATCH), (384, 64, 3, 1, 0, BATCH), (1280, 65, 1, 1, 0, FRAME),
             (1280, 5, 3, 0, 32, BATCH), (32, R.CHUNK - 1, 1, 0, 0, FRAME), (96, R.CHUNK + 1, 1, 1, 32, FRAME),
             (32, 2 * R.CHUNK + 1, 1, 5, 0, BATCH), (96, 683, 3, 0, 0, BATCH)]


@pytest.mark.parametrize("D,P,n,n_prefix,pad,scope", COV_CASES)
def test_mean_and_covariance(D, P, n, n_prefix, pad, scope):
    rows = random_rows(7 * D + P, n, P, n_prefix, D, D + pad)
    out = fit(rows, n_prefix, D, 1, scope, iters=1)
    worst_m = worst_c = worst_t = 0.0
    for b, X in enumerate(problems(rows, n_prefix, D, scope)):
        M = X.shape[0]
        mu, C64 = R.covariance64(X)
        bound, d = R.cov_bound(X)
        worst_m = max(worst_m, float((np.abs(out["mean"][b] - mu) / d).max()))
        worst_c = max(worst_c, float((np.abs(out["cov"][b] - C64) / bound).max()))
        assert np.array_equal(bits(out["cov"][b]), bits(out["cov"][b].T.copy())), "covariance is not symmetric bit for bit"
        tb = np.trace(bound)
        worst_t = max(worst_t, abs(float(out["tv"][b]) - np.trace(C64)) / tb)
    print(f"[cov D {D} P {P} n {n} prefix {n_prefix} ld {D + pad} scope {scope}] error / bound: mean {worst_m:.3f}, covariance {worst_c:.3f}, "
          f"total variance {worst_t:.3f}")
    assert worst_m <= 1.0 and worst_c <= 1.0 and worst_t <= 1.0


# ---- b. eigenpairs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,k,M", R.EIGEN_CASES)
def test_eigenpairs(D, k, M):
    X = R.eigen_fixture(D, k, M)
    out = fit(X[None], 0, D, k, FRAME)
    _, C64 = R.covariance64(X)
    lam, V, spectrum = R.eigh_topk(C64, k)
    E = np.linalg.norm(out["cov"][0].astype(np.float64) - C64) + D * U * lam[0]
    comp = out["comp"][0].astype(np.float64)
    sines = R.sines(comp / np.linalg.norm(comp, axis=1, keepdims=True), V)
    worst_s = worst_l = 0.0
    for j in range(k):
        gap = min(abs(spectrum[j] - spectrum[i]) for i in (j - 1, j + 1) if 0 <= i < len(spectrum))
        worst_s = max(worst_s, sines[j] / (4 * E / gap))
        worst_l = max(worst_l, abs(float(out["eig"][0][j]) - lam[j]) / (4 * E))
        assert comp[j] @ V[j] > 0, f"component {j}: the sign rule gave the opposite sign"
    bound, _ = R.cov_bound(X)
    tb = np.trace(bound)
    worst_t = abs(float(out["tv"][0]) - np.trace(C64)) / tb
    norms = np.abs(np.linalg.norm(comp, axis=1) - 1).max()
    print(f"[eig D {D} k {k} M {M}] error / bound: sine {worst_s:.3f} (largest sine {sines.max():.2e}), eigenvalue {worst_l:.3f}, "
          f"total variance {worst_t:.3f}; | |q| - 1 | {norms:.1e}")
    assert worst_s <= 1.0 and worst_l <= 1.0 and worst_t <= 1.0
    assert norms <= (D / 256 + 2 * k + 16) * U and (np.diff(out["eig"][0]) <= 0).all()
    # the sign rule itself: the entry of largest magnitude is positive
    assert all(out["comp"][0][j][np.argmax(np.abs(out["comp"][0][j]))] > 0 for j in range(k))


# ---- c. projection --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [96, 384])
def test_projection(D):
    n, P, n_prefix, k = 3, 37, 1, 3
    rows = random_rows(11 + D, n, P, n_prefix, D, D + 32)
    other = random_rows(12 + D, 2, P, n_prefix, D, D + 32)
    worst = {}
    for scope in (FRAME, BATCH):
        out = fit(rows, n_prefix, D, k, scope)
        dev, mean, comp = out["dev"]
        scores = project(dev, n_prefix, D, k, mean, comp).cpu().numpy().astype(np.float64)
        for f in range(n):
            b = f if scope == FRAME else 0
            xc = rows[f, n_prefix:, :D].astype(np.float64) - out["mean"][b].astype(np.float64)
            q = out["comp"][b].astype(np.float64)
            bound = (D / 64 + 8) * U * (np.abs(xc) @ np.abs(q).T)
            worst[scope] = max(worst.get(scope, 0.0), float((np.abs(scores[f] - xc @ q.T) / bound).max()))
        if scope == BATCH:
            # a basis fitted on one batch colours another: the same bits as projecting both batches together
            od = torch.from_numpy(other).cuda()
            both = project(torch.cat([dev, od]), n_prefix, D, k, mean, comp)
            assert np.array_equal(bits(both[:n]), bits(project(dev, n_prefix, D, k, mean, comp)))
            assert np.array_equal(bits(both[n:]), bits(project(od, n_prefix, D, k, mean, comp)))
    print(f"[project D {D}] error / bound: n_bases = n {worst[FRAME]:.3f}, n_bases = 1 {worst[BATCH]:.3f}")
    assert worst[FRAME] <= 1.0 and worst[BATCH] <= 1.0


# ---- d. batch invariance and reproducibility ------------------------------------------------------------------------------------
def test_frame_scope_does_not_depend_on_the_batch():
    D, P, n_prefix, k = 96, 70, 5, 3
    rows = random_rows(21, 5, P, n_prefix, D, D + 32)

    def run(sel):
        out = fit(np.ascontiguousarray(rows[sel]), n_prefix, D, k, FRAME)
        dev, mean, comp = out["dev"]
        out["scores"] = project(dev, n_prefix, D, k, mean, comp).cpu().numpy()
        return out
    alone, first, last = run([2]), run([2, 0, 1]), run([3, 4, 2])
    for name in ("mean", "comp", "eig", "tv", "cov", "scores"):
        assert np.array_equal(bits(alone[name][0]), bits(first[name][0])), name
        assert np.array_equal(bits(alone[name][0]), bits(last[name][2])), name


@pytest.mark.parametrize("scope", [FRAME, BATCH])
def test_two_calls_give_the_same_bits(scope):
    D, P, n_prefix, k = 384, 400, 1, 8
    rows = random_rows(22, 3, P, n_prefix, D, D)
    a, b = fit(rows, n_prefix, D, k, scope), fit(rows, n_prefix, D, k, scope)
    for name in ("mean", "comp", "eig", "tv", "cov"):
        assert np.array_equal(bits(a[name]), bits(b[name])), name
    dev, mean, comp = a["dev"]
    assert np.array_equal(bits(project(dev, n_prefix, D, k, mean, comp)), bits(project(dev, n_prefix, D, k, mean, comp)))


# ---- e. refusals: by return code and a word of the message; none of these calls runs a kernel ---------------------------------------
def _pca_calls(bufs):
    lib = _lib.load()

    def fit_rc(n=2, T=9, n_prefix=1, D=64, ld=64, k=3, scope=FRAME, iters=4, ws_bytes=4 << 16, null=None, shift=None):
        ptrs = {name: bufs[name].data_ptr() for name in ("rows", "mean", "comp", "eig", "tv", "ws")}
        if null:
            ptrs[null] = None
        if shift:
            ptrs[shift] += 4                                       # one float past a 16-byte boundary
        return lib.cbas_patch_pca_fit(ptrs["rows"], n, T, n_prefix, D, ld, k, scope, iters, ptrs["mean"], ptrs["comp"], ptrs["eig"],
                                      ptrs["tv"], ptrs["ws"], ws_bytes, None)

    def proj_rc(n=2, T=9, n_prefix=1, D=64, ld=64, k=3, n_bases=1, null=None, shift=None):
        ptrs = {name: bufs[name].data_ptr() for name in ("rows", "mean", "comp", "scores")}
        if null:
            ptrs[null] = None
        if shift:
            ptrs[shift] += 4
        return lib.cbas_patch_pca_project(ptrs["rows"], n, T, n_prefix, D, ld, k, n_bases, ptrs["mean"], ptrs["comp"], ptrs["scores"], None)
    return lib, fit_rc, proj_rc


def _pca_bufs(rows):
    bufs = {name: torch.zeros(1 << 16, device="cuda") for name in ("mean", "comp", "eig", "tv", "ws", "scores")}
    bufs["rows"] = rows
    return bufs


def test_refusals():
    lib, fit_rc, proj_rc = _pca_calls(_pca_bufs(torch.zeros(1 << 16, device="cuda")))

    def refused(rc, word):
        msg = lib.cbas_last_error().decode()
        assert rc == -1 and word in msg, (rc, word, msg)          # CBAS_EINVAL
    refused(fit_rc(D=48), "multiple of 32")
    refused(fit_rc(D=1568, ld=1568), "multiple of 32")
    refused(fit_rc(k=0), "components")
    refused(fit_rc(k=9, T=20), "components")
    refused(fit_rc(k=8), "min(M - 1, D)")                          # M = 8 rows per frame
    refused(fit_rc(T=2, k=1), "at least 2 rows")                   # M = 1
    refused(fit_rc(ld=32), "ld")
    refused(fit_rc(ld=66), "multiple of 4")
    refused(fit_rc(iters=0), "iters")
    need = int(lib.cbas_patch_pca_workspace_bytes(2, 9, 1, 64, 3, FRAME))
    assert need == 4 * 2 * (64 * 64 + 3 * 64 + 64)
    refused(fit_rc(ws_bytes=need - 4), "workspace")
    for name in ("rows", "mean", "comp", "eig", "tv", "ws"):
        refused(fit_rc(null=name), "NULL")
    for name in ("rows", "mean", "comp", "ws"):
        refused(fit_rc(shift=name), "16-byte aligned")
    refused(fit_rc(scope=2), "scope")
    refused(fit_rc(n=0), "frames")
    refused(fit_rc(n=65536), "frames")
    assert lib.cbas_patch_pca_workspace_bytes(2, 9, 1, 48, 3, FRAME) == -1 and "multiple of 32" in lib.cbas_last_error().decode()
    refused(proj_rc(D=48), "multiple of 32")
    refused(proj_rc(k=9), "components")
    refused(proj_rc(ld=32), "ld")
    refused(proj_rc(ld=66), "multiple of 4")
    refused(proj_rc(n_bases=3), "n_bases")
    refused(proj_rc(n=65536, n_bases=65536), "frames")
    for name in ("rows", "mean", "comp", "scores"):
        refused(proj_rc(null=name), "NULL")
    for name in ("rows", "mean", "comp"):
        refused(proj_rc(shift=name), "16-byte aligned")


def test_smallest_accepted_shapes():
    """The neighbours of the refused shapes that must be served: an exact workspace, M = 2 rows as one BATCH problem, both n_bases."""
    rows = torch.from_numpy(random_rows(31, 2, 8, 1, 64, 64)).cuda()
    lib, fit_rc, proj_rc = _pca_calls(_pca_bufs(rows))
    need = int(lib.cbas_patch_pca_workspace_bytes(2, 9, 1, 64, 3, FRAME))
    assert fit_rc(ws_bytes=need) == 0 and proj_rc(n_bases=2) == 0
    assert fit_rc(scope=BATCH) == 0 and proj_rc() == 0
    assert fit_rc(T=2, k=1, scope=BATCH) == 0                      # P = 1 row per frame: M = 2 only as one problem
    torch.cuda.synchronize()


# ---- f. through the encoder -------------------------------------------------------------------------------------------------------
ENC_SEED = 1234
_WEIGHTS = {}


def make_enc(cfg, hw, max_batch, precision):
    if cfg not in _WEIGHTS:
        _WEIGHTS[cfg] = (W.synth_convnext_weights if C.is_convnext(cfg) else W.synth_encoder_weights)(cfg, ENC_SEED)
    return DinoEncoder.from_weights(cfg, _WEIGHTS[cfg], "cuda", max_batch=max_batch, max_frame=hw, precision=precision)


@pytest.mark.parametrize("name,cfg,precision", [("vit_tiny", C.VIT_TINY, 0), ("vit_tiny", C.VIT_TINY, 4), ("convnext_tiny", C.CONVNEXT_TINY, 4)])
def test_through_the_encoder(name, cfg, precision, tmp_path):
    hw, n = (64, 64), 3
    frames = synth.cage_frames(191, n, *hw)
    dev = torch.from_numpy(frames).cuda()
    enc = make_enc(cfg, hw, 4, precision)
    try:
        a16, a32 = enc.encode_u8(dev)
        nh, nw, P0 = token_grid(cfg, *hw)
        D = cfg.hidden_size
        tokens = enc.hidden_state(dev)
        for scope, sc in (("frame", FRAME), ("batch", BATCH)):
            scores, basis = enc.patch_pca(dev, 3, scope)
            assert scores.shape == (n, nh, nw, 3) and scores.dtype == torch.float32 and scores.is_cuda and torch.isfinite(scores).all()
            assert basis.scope == scope and basis.stamp == enc.stamp and basis.n_bases == (n if scope == "frame" else 1) and basis.dim == D
            ratio = basis.explained_variance_ratio.cpu().numpy().astype(np.float64)
            M = nh * nw * (n if scope == "batch" else 1)
            print(f"[patch_pca {name} p{precision} {scope}] M {M}: explained variance ratios sum to {ratio.sum(axis=1)}")
            assert (ratio >= 0).all(), ratio
            if M - 1 > 3:
                assert (ratio.sum(axis=1) <= 1).all(), ratio
            else:
                # k = M - 1: the components span all the variance there is, so the sum IS 1 and only rounding decides the side.
                # Its own tolerance: for a positive semidefinite C, |q|^T |C| |q| <= trace C (|C_de| <= sqrt(C_dd C_ee), then
                # Cauchy-Schwarz), so each of the k Rayleigh quotients is off by at most g trace C, g = the roundings on one
                # product's way through C q (a chain of D / 64, a 6-level tree) and q . (C q) (a chain of D / 256, 6 levels, 3
                # adds), plus 16 u for the Jacobi rotations and Q's own departure from orthonormal; the trace by (D / 256 + 9) u
                assert (ratio.sum(axis=1) <= 1 + (3 + 1) * (D / 64 + D / 256 + 32) * U).all(), ratio
            # bit for bit the two entry points called directly on hidden_state(frames)
            direct = fit(tokens.cpu().numpy(), P0, D, 3, sc)
            _, mean, comp = direct["dev"]
            assert np.array_equal(bits(basis.components), bits(comp)) and np.array_equal(bits(basis.mean), bits(mean))
            assert np.array_equal(bits(scores.reshape(n, nh * nw, 3)), bits(project(tokens, P0, D, 3, mean, comp)))
            # a given basis is applied, not refitted; a foreign one is refused
            again, same = enc.patch_pca(dev[:2], basis=basis if scope == "batch" else PatchPCABasis(
                basis.mean[:2], basis.components[:2], basis.eigenvalues[:2], basis.total_variance[:2], "frame", basis.stamp))
            assert np.array_equal(bits(again), bits(scores[:2])) and same.stamp == basis.stamp
            print(f"[patch_pca {name} p{precision} {scope}] explained variance ratio of frame 0: {ratio[0]}")
        with pytest.raises(ValueError, match="fitted on encoder"):
            enc.patch_pca(dev, basis=PatchPCABasis(basis.mean, basis.components, basis.eigenvalues, basis.total_variance, "batch", "other"))
        with pytest.raises(ValueError, match="width"):
            z = torch.zeros(1, 3, D + 32, device="cuda")
            enc.patch_pca(dev, basis=PatchPCABasis(z[:, 0], z, basis.eigenvalues, basis.total_variance, "batch", enc.stamp))
        with pytest.raises(ValueError, match="scope"):
            enc.patch_pca(dev, scope="clip")
        b16, b32 = enc.encode_u8(dev)
        assert np.array_equal(bits(a32), bits(b32)) and np.array_equal(a16.cpu().numpy().view(np.uint16), b16.cpu().numpy().view(np.uint16))
        # the pictures: (H, W, 3) in [0, 1] per frame, in both scopes
        vid = str(tmp_path / "clip.npy")
        np.save(vid, frames)
        for scope in A.PCA_SCOPES:
            maps, green = A.frame_maps(enc, vid, [2, 0], kind="pca", pca_scope=scope)
            assert maps.shape == (2, hw[0], hw[1], 3) and maps.dtype == np.float32 and maps.min() >= 0.0 and maps.max() <= 1.0
            assert green.shape == (2, *hw) and np.array_equal(green[0], frames[2, :, :, 1])
    finally:
        enc.close()
