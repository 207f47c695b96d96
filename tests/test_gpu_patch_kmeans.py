"""Patch-feature k-means on the GPU (csrc/patch_kmeans.hip through cbas_patch_kmeans_fit / cbas_patch_kmeans_assign), against float64
computed from the very fp32 rows handed to the device, then through DinoEncoder.patch_clusters and attention_maps.  Every bound
was fixed before the first run from the summation forms the header states (patch_kmeans_ref.dist2_bound, mean_bound, seed_bound;
DESIGN.md section 18; u1 = 1.01 * 2^-24):

  dist2      u1 ((D / 2 + 12) sum |u_d| |c_d| + (D / 64 + 9) |c|^2 + 2 |u|^2): the score u . c - |c|^2 / 2 as four fmaf chains of D / 4
             terms, a chain of D / 64 and a 6-level tree for |c|^2, the factor rn, two fmaf roundings, doubled by dist2 = |u|^2 - 2 score
  assignment the float64 distance to the chosen centroid <= the float64 minimum + dist2 bound(chosen) + dist2 bound(nearest)
  centroid   (64 + chunks + 3) u1 mean |u_d| over the cluster's rows: one fmaf chain of at most 64 rows per chunk, chunks in order,
             a division, the factor rn
  inertia    the rows' dist2 bounds added, + (64 + chunks + 1) u1 inertia for the two-level sum
  seeding    (D / 64 + 8) u1 d + 4 u1 sqrt(d) (|u| + |t|) per distance (+ the mean's own rounding at step 0): the chosen row's float64
             objective is within twice the largest such bound of the float64 maximum, so a near-tie cannot fail
Each test prints its largest error / bound (run with -s)."""
import numpy as np
import pytest
import torch

import patch_kmeans_ref as R
from cbas_amd import _lib, attention_maps as A, config as C, weights as W, synth
from cbas_amd.encoder import KMEANS_DEFAULT_ITERS, DinoEncoder, PatchClusters, token_grid

pytestmark = pytest.mark.gpu

FRAME, BATCH = _lib.PCA_FRAME, _lib.PCA_BATCH
CH = R.CHUNK
SENTINEL = np.float32(1.0e30)             # in the prefix rows and the columns past D: read into any sum, it shows


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32)


def fit(rows, n_prefix, D, k, scope, iters, normalize):
    """cbas_patch_kmeans_fit on a float32 (n, T, ld) numpy image (or device tensor).  numpy centroids (b, k, D), counts (b, k), inertia
    (b, iters + 1), init_index (b, k), and from the workspace cur (b, k, D) - the centroids in seeding order - and order (b, k)."""
    lib = _lib.load()
    dev = torch.from_numpy(rows).cuda() if isinstance(rows, np.ndarray) else rows
    n, T, ld = dev.shape
    b = 1 if scope == BATCH else n
    need = int(lib.cbas_patch_kmeans_workspace_bytes(n, T, n_prefix, D, k, scope))
    assert need > 0, lib.cbas_last_error()
    ws = torch.zeros(need // 4, dtype=torch.float32, device="cuda")
    cent = torch.empty(b, k, D, device="cuda")
    counts, init = torch.empty(b, k, dtype=torch.int32, device="cuda"), torch.empty(b, k, dtype=torch.int32, device="cuda")
    inertia = torch.empty(b, iters + 1, device="cuda")
    _lib.check(lib.cbas_patch_kmeans_fit(dev.data_ptr(), n, T, n_prefix, D, ld, k, scope, iters, normalize, cent.data_ptr(), counts.data_ptr(),
                                         inertia.data_ptr(), init.data_ptr(), ws.data_ptr(), need, None), "cbas_patch_kmeans_fit")
    torch.cuda.synchronize()
    cur = ws[:b * k * D].reshape(b, k, D)
    off = -(-(b * k * D) // 4) * 4
    order = ws[off:off + b * 16].view(torch.int32).reshape(b, 16)[:, :k]
    return dict(cent=cent.cpu().numpy(), counts=counts.cpu().numpy(), inertia=inertia.cpu().numpy(), init=init.cpu().numpy(),
                cur=cur.cpu().numpy(), order=order.cpu().numpy(), dev=dev, cent_dev=cent, cur_dev=cur.clone())


def assign(dev_rows, n_prefix, D, normalize, cent, want_dist=True):
    """cbas_patch_kmeans_assign with the (sets, k, D) device centroids: numpy labels (n, P) and dist2 (n, P)."""
    lib = _lib.load()
    n, T, ld = dev_rows.shape
    labels = torch.full((n, T - n_prefix), -7, dtype=torch.int32, device="cuda")
    dist = torch.empty(n, T - n_prefix, device="cuda") if want_dist else None
    _lib.check(lib.cbas_patch_kmeans_assign(dev_rows.data_ptr(), n, T, n_prefix, D, ld, cent.shape[1], cent.shape[0], normalize, cent.data_ptr(),
                                            labels.data_ptr(), dist.data_ptr() if want_dist else None, None), "cbas_patch_kmeans_assign")
    torch.cuda.synchronize()
    return labels.cpu().numpy(), dist.cpu().numpy() if want_dist else None


def image(patches, n_prefix, pad):
    """(n, P, D) float32 patch rows as an (n, n_prefix + P, D + pad) image with the sentinel everywhere else."""
    n, P, D = patches.shape
    x = np.full((n, n_prefix + P, D + pad), SENTINEL, np.float32)
    x[:, n_prefix:, :D] = patches
    return x


def random_image(seed, n, P, n_prefix, D, pad):
    return image(np.stack([R.tiny_patch_rows(seed * 16 + f, P, D, parts=4) for f in range(n)]), n_prefix, pad)


def problems(rows, n_prefix, D, scope):
    patches = rows[:, n_prefix:, :D]
    return [patches.reshape(-1, D)] if scope == BATCH else list(patches)


def labels_by_problem(lab, scope):
    return [lab.reshape(-1)] if scope == BATCH else list(lab)


# (D, k, P, n, scope, normalize, n_prefix, pad): every P of {k, 20, chunk - 1, chunk, chunk + 1, 2 chunk + 3}, every D of {32, 96, 1536},
# every k of {2, 5, 16}, n of {1, 3}, both scopes and both normalize values at least once; ld > D and a prefix in every case; a
# BATCH problem whose chunk boundary falls inside a frame (3 x 63 rows)
CASES = [(32, 2, 2, 1, FRAME, 0, 1, 32), (32, 5, 5, 3, FRAME, 1, 2, 4), (96, 16, 16, 3, BATCH, 1, 1, 32), (96, 5, 20, 3, FRAME, 0, 5, 4),
         (96, 2, CH - 1, 3, BATCH, 1, 1, 32), (32, 16, CH, 1, FRAME, 1, 1, 4), (1536, 5, CH + 1, 1, FRAME, 1, 1, 32),
         (96, 16, 2 * CH + 3, 3, FRAME, 0, 2, 4), (1536, 16, 20, 3, BATCH, 0, 1, 32), (1536, 2, 2 * CH + 3, 1, BATCH, 1, 5, 32),
         (32, 5, 2 * CH + 3, 3, BATCH, 0, 1, 4)]
_IMAGES = {}


def case_image(case):
    if case not in _IMAGES:
        D, k, P, n, scope, normalize, n_prefix, pad = case
        _IMAGES[case] = random_image(D + 7 * k + P, n, P, n_prefix, D, pad)
    return _IMAGES[case]


# ---- a. seeding -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_seeding(case):
    D, k, P, n, scope, normalize, n_prefix, pad = case
    rows = case_image(case)
    out = fit(rows, n_prefix, D, k, scope, 0, normalize)
    worst = 0.0
    for b, X in enumerate(problems(rows, n_prefix, D, scope)):
        M, idx = len(X), out["init"][b]
        assert ((0 <= idx) & (idx < M)).all() and sorted(out["order"][b].tolist()) == list(range(k))
        U = R.working_rows(X, normalize)
        # iters = 0: the centroids are the seed rows, in seeding order in the workspace and by descending count in the output
        assert np.array_equal(bits(out["cent"][b]), bits(out["cur"][b][out["order"][b]]))
        if normalize:
            ulp = np.spacing(np.abs(U[idx]).astype(np.float32)).astype(np.float64)
            assert (np.abs(out["cur"][b].astype(np.float64) - U[idx]) <= 2 * ulp).all()
        else:
            assert np.array_equal(bits(out["cur"][b]), bits(X[idx]))
        objs = R.seed_objectives(U, list(idx))
        nch = -(-M // CH)
        for j in range(k):
            targets = [U.mean(axis=0)] if j == 0 else [U[i] for i in idx[:j]]
            bound = R.seed_bound(U, objs[j], targets, D, nch if j == 0 else None)
            short = objs[j].max() - objs[j][idx[j]]
            worst = max(worst, short / (2 * bound))
            assert short <= 2 * bound, (b, j, short, bound)
        assert out["counts"][b].sum() == M and (np.diff(out["counts"][b]) <= 0).all()
    print(f"[seeding {case}] (largest objective - chosen row's) / bound: {worst:.3f}")


# ---- b. one round at a time -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_rounds(case):
    D, k, P, n, scope, normalize, n_prefix, pad = case
    rows = case_image(case)
    runs = [fit(rows, n_prefix, D, k, scope, t, normalize) for t in range(4)]
    probs = problems(rows, n_prefix, D, scope)
    worst_c = worst_i = 0.0
    for t in range(4):
        # the labels of the iters = t result, in seeding names: its centroids before the reorder are in the workspace
        cur = runs[t]["cur_dev"]
        lab, _ = assign(runs[t]["dev"], n_prefix, D, normalize, cur if scope == FRAME else cur[:1])
        for b, (X, lb) in enumerate(zip(probs, labels_by_problem(lab, scope))):
            M, nch = len(X), -(-len(X) // CH)
            U = R.working_rows(X, normalize)
            counts = np.bincount(lb, minlength=k)
            order = np.array(sorted(range(k), key=lambda j: (-counts[j], j)))
            assert np.array_equal(runs[t]["order"][b], order) and np.array_equal(runs[t]["counts"][b], counts[order])
            assert np.array_equal(bits(runs[t]["cent"][b]), bits(runs[t]["cur"][b][order]))
            c64 = runs[t]["cur"][b].astype(np.float64)
            d2 = R.assign(U, c64)[1][np.arange(M), lb]
            ibound = R.dist2_bound(U, c64, D)[np.arange(M), lb].sum() + (CH + nch + 1) * R.U1 * d2.sum()
            worst_i = max(worst_i, abs(float(runs[t]["inertia"][b][t]) - d2.sum()) / ibound)
            for s in range(t):
                assert np.array_equal(bits(runs[t]["inertia"][b][:s + 1]), bits(runs[s]["inertia"][b]))      # a longer run repeats a shorter one
            if t == 3:
                continue
            for j in range(k):
                got = runs[t + 1]["cur"][b][j]
                if counts[j] == 0:
                    assert np.array_equal(bits(got), bits(runs[t]["cur"][b][j]))
                    continue
                err = np.abs(got.astype(np.float64) - U[lb == j].mean(axis=0))
                bound = R.mean_bound(U, lb == j, nch)
                worst_c = max(worst_c, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"[rounds {case}] error / bound: centroid {worst_c:.3f}, inertia {worst_i:.3f}")
    assert worst_c <= 1.0 and worst_i <= 1.0


def test_an_emptied_cluster_keeps_its_centroid():
    # three distinct integer points, k = 4: seed 3 repeats the lowest row, loses every tie to its twin and never owns a row
    D, n_prefix = 32, 1
    pts = np.zeros((3, D), np.float32)
    pts[0, 0], pts[1, 1], pts[2, 2] = 8, 6, -4                    # squared distances to the mean 38.56, 20.16, 19.36: no tie
    X = pts[np.array([0, 1, 2, 1, 0, 2, 2, 0, 1, 1])]
    rows = image(X[None], n_prefix, 4)
    for iters in (0, 2):
        out = fit(rows, n_prefix, D, 4, FRAME, iters, 0)
        ref = R.fit(X, 4, iters, 0)
        assert np.array_equal(out["init"][0], ref["init_index"]) and out["init"][0][3] == 0
        assert out["counts"][0].tolist() == ref["counts"].tolist() and out["counts"][0][3] == 0 and out["order"][0][3] == 3
        assert np.array_equal(bits(out["cur"][0][3]), bits(X[0])) and np.array_equal(bits(out["cent"][0][3]), bits(X[0]))
        assert np.array_equal(out["cent"][0].astype(np.float64), ref["centroids"])


# ---- c. assignment ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_assignment(case):
    D, k, P, n, scope, normalize, n_prefix, pad = case
    rows = case_image(case)
    out = fit(rows, n_prefix, D, k, scope, 2, normalize)
    lab, dist = assign(out["dev"], n_prefix, D, normalize, out["cent_dev"])      # n_sets = n for FRAME, 1 for BATCH
    assert lab.min() >= 0 and lab.max() < k
    worst_a = worst_d = 0.0
    for b, (X, lb, db) in enumerate(zip(problems(rows, n_prefix, D, scope), labels_by_problem(lab, scope), labels_by_problem(dist, scope))):
        M = len(X)
        U = R.working_rows(X, normalize)
        c64 = out["cent"][b].astype(np.float64)
        near, d2 = R.assign(U, c64)
        Bd = R.dist2_bound(U, c64, D)
        ar = np.arange(M)
        room = Bd[ar, lb] + Bd[ar, near]
        worst_a = max(worst_a, float(((d2[ar, lb] - d2[ar, near]) / room).max()))
        worst_d = max(worst_d, float((np.abs(db.astype(np.float64) - d2[ar, lb]) / Bd[ar, lb]).max()))
        assert (db >= 0).all() and np.array_equal(np.bincount(lb, minlength=k), out["counts"][b])
    print(f"[assignment {case}] (chosen - nearest) / bound: {worst_a:.3f}; dist2 error / bound: {worst_d:.3f}")
    assert worst_a <= 1.0 and worst_d <= 1.0
    # labels without the distances are the same labels
    assert np.array_equal(assign(out["dev"], n_prefix, D, normalize, out["cent_dev"], want_dist=False)[0], lab)


@pytest.mark.parametrize("D,k,P", [(32, 5, 20), (96, 16, 2 * CH + 3), (1536, 2, CH + 1)])
def test_integer_rows_are_labelled_exactly(D, k, P):
    # small integers: every product, chain and |c|^2 / 2 is exact in fp32, so the labels are the float64 reference's, ties included
    rng = np.random.default_rng(D + k)
    n, n_prefix = 3, 2
    cent = rng.integers(-3, 4, (k, D)).astype(np.float32)
    cent[1] = cent[0]
    cent[1, 0] += 2                                                         # centroid 1: centroid 0 moved two steps along column 0
    if k > 2:
        cent[k - 1] = cent[0]                                               # a repeated centroid: the lower index wins
    X = rng.integers(-3, 4, (n, P, D)).astype(np.float32)
    X[:, 0] = cent[0]                                                       # on centroid 0 (and on its copy)
    X[:, 1] = cent[0]
    X[:, 1, 0] += 1                                                         # one step from centroid 0 and from centroid 1
    dev = torch.from_numpy(image(X, n_prefix, 4)).cuda()
    lab, dist = assign(dev, n_prefix, D, 0, torch.from_numpy(cent[None]).cuda())
    ties = 0
    for f in range(n):
        ref, d2 = R.assign(X[f].astype(np.float64), cent.astype(np.float64))
        assert np.array_equal(lab[f], ref)
        assert np.array_equal(dist[f].astype(np.float64), d2[np.arange(P), ref])
        srt = np.sort(d2, axis=1)
        ties += int((srt[:, 0] == srt[:, 1]).sum())
        assert lab[f][0] == 0 and lab[f][1] == 0 and d2[1, 0] == d2[1, 1] == 1.0
    print(f"[integer rows D {D} k {k} P {P}] rows with an exact tie: {ties}")
    assert ties >= (2 if k > 2 else 1) * n


# ---- d. planted data --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,k,M,scope,normalize", [(32, 2, 70, FRAME, 0), (96, 5, 3 * 67, BATCH, 1), (1536, 16, 2 * CH + 16, FRAME, 1), (96, 16, 3 * 131, BATCH, 0)])
def test_planted_partition(D, k, M, scope, normalize):
    X, planted = R.planted(D + k, k, M, D)
    ref = R.fit(X, k, 3, normalize)
    assert ref["margin"] > 0.5 and np.array_equal(ref["labels"], planted)     # every row's nearest centroid leads by far more than any bound
    n = 3 if scope == BATCH else 1
    rows = image(X.reshape(n, M // n, D), 1, 32)
    out = fit(rows, 1, D, k, scope, 3, normalize)
    lab, _ = assign(out["dev"], 1, D, normalize, out["cent_dev"])
    assert np.array_equal(lab.reshape(-1), ref["labels"]) and np.array_equal(out["counts"][0], ref["counts"])
    assert np.array_equal(planted[out["init"][0]][out["order"][0]], np.arange(k))       # one seed per blob, ordered as the reference orders them
    U = R.working_rows(X, normalize)
    tol = 2 * (R.dist2_bound(U, out["cent"][0].astype(np.float64), D).max(axis=1).sum() + (CH + -(-M // CH) + 1) * R.U1 * out["inertia"][0][0])
    print(f"[planted D {D} k {k} M {M}] inertia {out['inertia'][0]}, reference {ref['inertia']}, tolerance {tol:.2e}")
    assert (np.diff(out["inertia"][0].astype(np.float64)) <= tol).all()


# ---- e. determinism and batch independence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scope", [FRAME, BATCH])
def test_two_calls_give_the_same_bits(scope):
    D, P, n_prefix, k = 384, 150, 1, 7
    rows = random_image(41, 3, P, n_prefix, D, 0)
    a, b = fit(rows, n_prefix, D, k, scope, 5, 1), fit(rows, n_prefix, D, k, scope, 5, 1)
    for name in ("cent", "counts", "inertia", "init", "cur", "order"):
        assert np.array_equal(bits(a[name]), bits(b[name])), name
    la, lb = assign(a["dev"], n_prefix, D, 1, a["cent_dev"]), assign(b["dev"], n_prefix, D, 1, b["cent_dev"])
    assert np.array_equal(la[0], lb[0]) and np.array_equal(bits(la[1]), bits(lb[1]))


def test_frame_scope_does_not_depend_on_the_batch():
    D, P, n_prefix, k = 96, 70, 5, 4
    rows = random_image(42, 8, P, n_prefix, D, 32)

    def run(sel):
        out = fit(np.ascontiguousarray(rows[sel]), n_prefix, D, k, FRAME, 4, 1)
        out["labels"], out["dist"] = assign(out["dev"], n_prefix, D, 1, out["cent_dev"])
        return out
    alone, third, eight = run([2]), run([0, 1, 2]), run([3, 4, 2, 5, 6, 7, 0, 1])
    for name in ("cent", "counts", "inertia", "init", "cur", "order", "labels", "dist"):
        assert np.array_equal(bits(alone[name][0]), bits(third[name][2])), name
        assert np.array_equal(bits(alone[name][0]), bits(eight[name][2])), name


# ---- f. refusals: by return code and a word of the message; none of these calls runs a kernel -----------------------------------------
def test_refusals():
    lib = _lib.load()
    names = ("rows", "cent", "counts", "inertia", "init", "ws", "labels", "dist")
    bufs = {name: torch.full((1 << 16,), 3.0, device="cuda") for name in names}

    def fit_rc(n=2, T=9, n_prefix=1, D=64, ld=64, k=3, scope=FRAME, iters=2, normalize=1, ws_bytes=4 << 16, null=None, shift=None):
        p = {name: bufs[name].data_ptr() for name in names}
        if null:
            p[null] = None
        if shift:
            p[shift] += 4
        return lib.cbas_patch_kmeans_fit(p["rows"], n, T, n_prefix, D, ld, k, scope, iters, normalize, p["cent"], p["counts"], p["inertia"],
                                         p["init"], p["ws"], ws_bytes, None)

    def assign_rc(n=2, T=9, n_prefix=1, D=64, ld=64, k=3, n_sets=1, normalize=1, null=None, shift=None):
        p = {name: bufs[name].data_ptr() for name in names}
        if null:
            p[null] = None
        if shift:
            p[shift] += 4
        return lib.cbas_patch_kmeans_assign(p["rows"], n, T, n_prefix, D, ld, k, n_sets, normalize, p["cent"], p["labels"], p["dist"], None)

    def refused(rc, word):
        msg = lib.cbas_last_error().decode()
        assert rc == -1 and word in msg, (rc, word, msg)          # CBAS_EINVAL
    for call in (fit_rc, assign_rc):
        refused(call(k=1), "clusters")
        refused(call(k=17, T=40), "clusters")
        refused(call(D=48), "multiple of 32")
        refused(call(D=1568, ld=1568), "multiple of 32")
        refused(call(ld=32), "ld")
        refused(call(ld=66), "multiple of 4")
        refused(call(n=0), "frames")
        refused(call(n=65536), "frames")
        refused(call(T=1), "no patch row")
        refused(call(normalize=2), "normalize")
        refused(call(null="rows"), "NULL")
        refused(call(null="cent"), "NULL")
        refused(call(shift="rows"), "16-byte aligned")
        refused(call(shift="cent"), "16-byte aligned")
    refused(fit_rc(k=9), "exceed")                                 # M = 8 rows per frame
    refused(fit_rc(iters=-1), "iters")
    refused(fit_rc(scope=2), "scope")
    need = int(lib.cbas_patch_kmeans_workspace_bytes(2, 9, 1, 64, 3, FRAME))
    assert need > 0
    refused(fit_rc(ws_bytes=need - 4), "workspace")
    for name in ("counts", "inertia", "init", "ws"):
        refused(fit_rc(null=name), "NULL")
    refused(fit_rc(shift="ws"), "16-byte aligned")
    refused(assign_rc(n_sets=3), "n_sets")
    refused(assign_rc(null="labels"), "NULL")
    assert lib.cbas_patch_kmeans_workspace_bytes(2, 9, 1, 48, 3, FRAME) == -1 and "multiple of 32" in lib.cbas_last_error().decode()
    assert lib.cbas_patch_kmeans_workspace_bytes(2, 9, 1, 64, 9, FRAME) == -1 and lib.cbas_patch_kmeans_workspace_bytes(2, 9, 1, 64, 9, BATCH) > 0
    torch.cuda.synchronize()
    for name in names:                                             # nothing was queued: every output is as it was
        assert bool((bufs[name] == 3.0).all()), name
    # the neighbours that must be served: an exact workspace, iters = 0, k = M, no distances
    bufs["rows"].copy_(torch.from_numpy(np.resize(R.tiny_patch_rows(3, 64, 64), 1 << 16)).cuda())
    assert fit_rc(ws_bytes=need) == 0 and fit_rc(iters=0) == 0 and fit_rc(k=8) == 0 and fit_rc(k=16, scope=BATCH) == 0
    assert assign_rc(null="dist") == 0 and assign_rc(n_sets=2) == 0
    torch.cuda.synchronize()


# ---- g. through the encoder -------------------------------------------------------------------------------------------------------
ENC_SEED = 1234
_WEIGHTS = {}


def make_enc(cfg, hw, max_batch, precision):
    if cfg not in _WEIGHTS:
        _WEIGHTS[cfg] = (W.synth_convnext_weights if C.is_convnext(cfg) else W.synth_encoder_weights)(cfg, ENC_SEED)
    return DinoEncoder.from_weights(cfg, _WEIGHTS[cfg], "cuda", max_batch=max_batch, max_frame=hw, precision=precision)


ENCODERS = [(name, cfg, hw, n, p) for name, cfg, hw, n, ps in (
    ("vit_tiny", C.VIT_TINY, (72, 88), 3, (0, 1, 3, 4)), ("dinov2reg_tiny", C.DINOV2_REG_TINY, (72, 88), 3, (0, 1, 3, 4)),
    ("convnext_tiny", C.CONVNEXT_TINY, (72, 88), 3, (3, 4)), ("vitb16", C.VIT_B16, (224, 224), 8, (0,))) for p in ps]


@pytest.mark.parametrize("name,cfg,hw,n,precision", ENCODERS)
def test_through_the_encoder(name, cfg, hw, n, precision, tmp_path):
    frames = synth.cage_frames(191, n + 2, *hw)
    dev, other = torch.from_numpy(frames[:n]).cuda(), torch.from_numpy(frames[n:]).cuda()
    enc = make_enc(cfg, hw, n, precision)
    try:
        a16, a32 = enc.encode_u8(dev)
        nh, nw, P0 = token_grid(cfg, *hw)
        D, k = cfg.hidden_size, 3
        tokens = enc.hidden_state(dev)
        for scope, sc in (("frame", FRAME), ("batch", BATCH)):
            labels, cl = enc.patch_clusters(dev, k, scope)
            assert labels.shape == (n, nh, nw) and labels.dtype == torch.int32 and labels.is_cuda
            assert (cl.scope, cl.normalize, cl.stamp, cl.n_sets, cl.n_clusters, cl.dim) == (scope, True, enc.stamp, n if scope == "frame" else 1, k, D)
            assert cl.inertia.shape[1] == KMEANS_DEFAULT_ITERS + 1 and int(cl.counts.sum()) == n * nh * nw
            # bit for bit the two entry points called directly on hidden_state(frames)
            direct = fit(tokens, P0, D, k, sc, KMEANS_DEFAULT_ITERS, 1)
            assert np.array_equal(bits(cl.centroids), bits(direct["cent"])) and np.array_equal(cl.counts.cpu().numpy(), direct["counts"])
            assert np.array_equal(cl.init_index.cpu().numpy(), direct["init"]) and np.array_equal(bits(cl.inertia), bits(direct["inertia"]))
            lab = assign(tokens, P0, D, 1, direct["cent_dev"], want_dist=False)[0]
            assert np.array_equal(labels.cpu().numpy().reshape(n, nh * nw), lab)
            print(f"[patch_clusters {name} p{precision} {scope}] counts {cl.counts.cpu().numpy().tolist()}")
            # a given set is applied, not refitted: another batch, and the same one again
            given = cl if scope == "batch" else PatchClusters(cl.centroids[:2], cl.counts[:2], cl.inertia[:2], cl.init_index[:2], "frame", True, cl.stamp)
            again, same = enc.patch_clusters(dev[:2], clusters=given)
            assert np.array_equal(again.cpu().numpy(), labels[:2].cpu().numpy()) and same is given
            if scope == "batch":
                far, _ = enc.patch_clusters(other, clusters=cl)
                expect = assign(enc.hidden_state(other), P0, D, 1, cl.centroids, want_dist=False)[0]
                assert np.array_equal(far.cpu().numpy().reshape(2, nh * nw), expect)
        with pytest.raises(ValueError, match="fitted on encoder"):
            enc.patch_clusters(dev, clusters=PatchClusters(cl.centroids, cl.counts, cl.inertia, cl.init_index, "batch", True, "other"))
        with pytest.raises(ValueError, match="width"):
            enc.patch_clusters(dev, clusters=PatchClusters(torch.zeros(1, k, D + 32, device="cuda"), cl.counts, cl.inertia, cl.init_index, "batch", True, enc.stamp))
        with pytest.raises(ValueError, match="scope"):
            enc.patch_clusters(dev, scope="clip")
        b16, b32 = enc.encode_u8(dev)
        assert np.array_equal(bits(a32), bits(b32)) and np.array_equal(a16.cpu().numpy().view(np.uint16), b16.cpu().numpy().view(np.uint16))
        if precision == max(p for nm, _, _, _, p in ENCODERS if nm == name):
            vid = str(tmp_path / "clip.npy")
            np.save(vid, frames)
            for scope in A.CLUSTER_SCOPES:
                maps, green = A.frame_maps(enc, vid, [2, 0], kind="clusters", n_clusters=k, cluster_scope=scope)
                assert maps.shape == (2, nh, nw) and maps.dtype == np.int32 and maps.min() >= 0 and maps.max() < k
                assert green.shape == (2, *hw) and np.array_equal(green[0], frames[2, :, :, 1])
                assert A.render_labels(maps[0], (hw[1], hw[0])).shape == (*hw, 3)
    finally:
        enc.close()


def test_precision_2_is_refused():
    enc = make_enc(C.VIT_B16, (64, 64), 2, 2)
    try:
        with pytest.raises(ValueError, match="precision 2 serves CLS rows only"):
            enc.patch_clusters(torch.zeros(2, 64, 64, dtype=torch.uint8, device="cuda"))
    finally:
        enc.close()
