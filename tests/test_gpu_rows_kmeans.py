"""k-means over resident CLS rows on the GPU (csrc/rows_kmeans.hip through cbas_rows_kmeans_fit / _assign, then cbas_amd.motifs).

  assignment   labels against the float64 argmax of the very fp16 rows handed to the device; a row whose float64 top-2 gap is within
               twice the score bound may take either of the two; dist2 within its bound
  exact        small-integer rows whose cluster means are integers: every product and sum is exact, so seeds, labels, counts,
               centroids and inertia equal the float64 restatement bit for bit, through rounds and across segments
  update       from the device's own labels the centroids agree with the float64 means within the derived bound
  invariance   bit for bit: two fits, fit against assign, a slice, another ld, a continued fit
The bounds are derived in rows_kmeans_ref.py.  Cases print their largest error / bound (run with -s)."""
import csv
import os

import numpy as np
import pytest
import torch

import rows_kmeans_ref as R
from cbas_amd import _lib, motifs, pipeline, postprocess, search as S, synth

pytestmark = pytest.mark.gpu

TILE, SEGMENT = R.TILE, R.SEGMENT
PAD = np.float16(60000.0)                  # in the columns past D: read into any sum, it shows


def store(x, pad=8):
    """The fp16 rows as a device tensor with `pad` columns of PAD after the D."""
    img = np.full((x.shape[0], x.shape[1] + pad), PAD, np.float16)
    img[:, :x.shape[1]] = x
    return torch.from_numpy(img).cuda()


def no_subnormals(x):
    x = np.asarray(x, np.float16)
    tiny = np.float16(6.2e-5)              # no fp16 subnormals: what the MFMA does with them is not part of the contract
    x[(np.abs(x) < tiny) & (x != 0)] = tiny
    return x


def fit(rows, D, k, iters, normalize, init=None, want_labels=True):
    """cbas_rows_kmeans_fit on a (N, ld) fp16 device tensor; numpy outputs, `cur` / `order` from the workspace."""
    lib = _lib.load()
    N = rows.shape[0]
    need = int(lib.cbas_rows_kmeans_workspace_bytes(N, D, k))
    assert need > 0, lib.cbas_last_error()
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    cent = torch.full((k, D), 7.0, device="cuda")
    counts = torch.full((k,), -7, dtype=torch.int64, device="cuda")
    inertia = torch.full((iters + 1,), 7.0, device="cuda")
    seeds = torch.full((k,), -7, dtype=torch.int64, device="cuda")
    labels = torch.full((N,), -7, dtype=torch.int32, device="cuda") if want_labels else None
    dist2 = torch.full((N,), 7.0, device="cuda") if want_labels else None
    start = None if init is None else torch.from_numpy(np.ascontiguousarray(init, np.float32)).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _lib.check(lib.cbas_rows_kmeans_fit(rows.data_ptr(), N, D, rows.shape[1], k, iters, int(normalize), ptr(start), cent.data_ptr(),
                                        counts.data_ptr(), inertia.data_ptr(), seeds.data_ptr(), ptr(labels), ptr(dist2), ws.data_ptr(), need,
                                        None), "cbas_rows_kmeans_fit")
    torch.cuda.synchronize()
    out = {"centroids": cent.cpu().numpy(), "counts": counts.cpu().numpy(), "inertia": inertia.cpu().numpy(), "init_index": seeds.cpu().numpy(),
           "cur": ws[:k * D * 4].cpu().numpy().view(np.float32).reshape(k, D).copy(),
           "order": ws[k * D * 4:k * D * 4 + 256].cpu().numpy().view(np.int32).copy()}
    if want_labels:
        out["labels"], out["dist2"] = labels.cpu().numpy(), dist2.cpu().numpy()
    return out


def assign(rows, D, cent, normalize, first=0, n=None, want_dist2=True):
    lib = _lib.load()
    n = rows.shape[0] - first if n is None else n
    c = torch.from_numpy(np.ascontiguousarray(cent, np.float32)).cuda()
    labels = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    dist2 = torch.full((n,), 7.0, device="cuda") if want_dist2 else None
    _lib.check(lib.cbas_rows_kmeans_assign(rows.data_ptr() + first * rows.shape[1] * 2, n, D, rows.shape[1], c.shape[0], int(normalize),
                                           c.data_ptr(), labels.data_ptr(), None if dist2 is None else dist2.data_ptr(), None),
               "cbas_rows_kmeans_assign")
    torch.cuda.synchronize()
    return labels.cpu().numpy(), (dist2.cpu().numpy() if want_dist2 else None)


def planted(seed, N, D, k, noise=0.15, scale=1.0, lengths=(0.5, 1.0, 3.0)):
    """Rows around k prototypes, group sizes falling geometrically, every row times one of `lengths`; the fp16 rows, the group of
    every row, the prototypes."""
    rng = np.random.default_rng(seed)
    proto = rng.standard_normal((k, D)) * scale
    share = 0.8 ** np.arange(k)
    group = rng.choice(k, N, p=share / share.sum())
    group[:k] = np.arange(k)                                                   # every group has a row
    x = no_subnormals((proto[group] + noise * scale * rng.standard_normal((N, D))) * rng.choice(list(lengths), (N, 1)))
    return rng, x, group, proto


# ---- a. assignment and dist2 against float64 ---------------------------------------------------------------------------------------------
SHAPES = [(32, 2, 2), (32, 64, 64), (96, 16, TILE - 1), (96, 17, TILE + 1), (768, 64, SEGMENT + 1), (1536, 17, 2 * SEGMENT + TILE + 3),
          (768, 2, TILE + 1)]


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("D,k,N", SHAPES)
def test_assignment(D, k, N, normalize):
    rng, x, group, proto = planted(D + 3 * k + N, N, D, k)
    if N > 4:
        x[N // 2] = 0                                                          # a zero row: rn = 0 with normalize, a defined label
    cent = (proto * (1.0 if not normalize else 1.0 / np.linalg.norm(proto, axis=1, keepdims=True))
            + 0.01 * rng.standard_normal((k, D))).astype(np.float32)
    labels, dist2 = assign(store(x), D, cent, normalize)
    want, want_d2, gap = R.assign(x, cent, normalize)
    sb = R.score_bound(x, cent, normalize)
    sc = R.scores(R.working_rows(x, normalize), cent)
    idx = np.arange(N)
    second = sc.copy()
    second[idx, want] = -np.inf
    runner = second.argmax(axis=1)
    loose = gap <= 2.0 * np.maximum(sb[idx, want], sb[idx, runner])
    assert loose.mean() <= 0.01, loose.mean()
    assert np.array_equal(labels[~loose], want[~loose])
    assert ((labels[loose] == want[loose]) | (labels[loose] == runner[loose])).all()
    assert labels.min() >= 0 and labels.max() < k
    got_sc = sc[idx, labels]
    ref_d2 = np.maximum(0.0, (R.working_rows(x, normalize) ** 2).sum(axis=1) - 2.0 * got_sc)
    bound = R.dist2_bound(x, cent, normalize, labels)
    ratio = (np.abs(dist2.astype(np.float64) - ref_d2) / bound).max()
    print(f"D={D} k={k} N={N} normalize={normalize}: {int(loose.sum())} rows within the bound of a tie; dist2 error / bound {ratio:.3f}")
    assert ratio <= 1.0
    if N > 4 and normalize:
        j = int(np.argmin((cent.astype(np.float64) ** 2).sum(axis=1)))
        assert labels[N // 2] == want[N // 2] == j


# ---- b. exact: integer rows whose means are integers ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def integers():
    """Four groups of 4096, 4096, 256 and 64 rows around integer centres, the noise of a group in pairs (+n, -n) so that its mean IS the
    centre, shuffled over three segments; one far row, twice (rows 5000 and 7000): the farthest from the mean, a tie."""
    rng = np.random.default_rng(5)
    D, sizes = 32, (4096, 4096, 256, 64)
    centres = rng.integers(-8, 9, (len(sizes), D))
    parts = []
    for c, n in zip(centres, sizes):
        half = rng.integers(-1, 2, (n // 2, D))
        parts.append(c + np.concatenate([half, -half]))
    x = np.concatenate(parts)[rng.permutation(sum(sizes))]
    far = np.full(D, 40)
    x = np.insert(x, 5000, far, axis=0)
    x = np.insert(x, 7000, far, axis=0)
    assert x.shape[0] == 2 * SEGMENT + 322 and np.abs(x).max() <= 40
    x = x.astype(np.float16)
    return store(x), x, D


@pytest.mark.parametrize("iters", [0, 1, 3])
def test_exact(integers, iters):
    rows, x, D = integers
    k = 5
    got = fit(rows, D, k, iters, 0)
    want = R.fit(x, k, iters, 0)
    assert got["init_index"].tolist() == want["init_index"].tolist() and got["init_index"][0] == 5000           # the tie: the lowest row
    assert np.array_equal(got["labels"], want["labels"]) and np.array_equal(got["counts"], want["counts"])
    assert got["counts"].tolist() == [4096, 4096, 256, 64, 2]                  # by descending count, ties by seeding order
    assert np.array_equal(got["centroids"].astype(np.float64), want["centroids"])
    assert np.array_equal(got["cur"].astype(np.float64), want["cur"]) and got["order"][:k].tolist() == want["order"].tolist()
    assert (got["order"][k:] == -1).all()
    assert np.array_equal(got["inertia"].astype(np.float64), want["inertia"]) and np.array_equal(got["dist2"].astype(np.float64), want["dist2"])
    if iters == 0:                                                             # the start is returned: the seed rows themselves
        assert np.array_equal(got["cur"], x[got["init_index"]].astype(np.float32))


# ---- c. seeding on data with clear margins ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [0, 1])
def test_seeding(normalize):
    rng = np.random.default_rng(17)
    D, k, N = 96, 6, SEGMENT + 77
    proto = rng.standard_normal((k, D)) * np.arange(1, k + 1)[:, None]         # distinct lengths: clear margins without normalize too
    group = rng.integers(0, k, N)
    x = no_subnormals(proto[group] + 0.01 * rng.standard_normal((N, D)))
    got = fit(store(x), D, k, 0, normalize)
    want = R.fit(x, k, 0, normalize)
    assert got["init_index"].tolist() == want["init_index"].tolist()
    assert sorted(group[got["init_index"]].tolist()) == list(range(k))         # one seed in every group
    u = R.working_rows(x, normalize)[got["init_index"]]
    assert np.abs(got["cur"] - u).max() <= 2.0 ** -10 * np.abs(u).max()


# ---- d. the update, from the device's own labels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("D,k,N", [(96, 17, 2 * SEGMENT + TILE + 3), (768, 64, SEGMENT + 1), (1536, 2, TILE + 1)])
def test_update(D, k, N, normalize):
    rng, x, group, proto = planted(2 * D + k + N, N, D, k)
    rows = store(x)
    c0 = (proto + 0.05 * rng.standard_normal((k, D))).astype(np.float32)
    c0[k - 1] = 500.0                                                          # an emptied cluster keeps its centroid
    labels0, d0 = assign(rows, D, c0, normalize)
    assert not (labels0 == k - 1).any()
    got = fit(rows, D, k, 1, normalize, init=c0)
    assert (got["init_index"] == -1).all()
    want = R.update(x, labels0, c0, normalize)
    bound = R.centroid_bound(x, labels0, k, normalize)
    err = np.abs(got["cur"].astype(np.float64) - want)
    assert np.array_equal(got["cur"][k - 1], c0[k - 1]) and got["counts"][-1] == 0 and np.array_equal(got["centroids"][-1], c0[k - 1])
    ratio = (err[:k - 1] / np.maximum(bound[:k - 1], 1e-300)).max()
    print(f"D={D} k={k} N={N} normalize={normalize}: centroid error / bound {ratio:.3f}")
    assert ratio <= 1.0
    # inertia[0] is the sum of the first assignment's dist2: N fp32 additions
    s = d0.astype(np.float64).sum()
    assert abs(got["inertia"][0] - s) <= R.g(min(N, SEGMENT) + -(-N // SEGMENT)) * s
    assert got["counts"].sum() == N and (np.diff(got["counts"]) <= 0).all()


# ---- e. a planted partition is recovered ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [0, 1])
def test_planted_partition(normalize):
    D, k, N = 96, 7, 2 * SEGMENT + TILE + 3
    # noise around every prototype; rows of several lengths only where the direction is what is clustered
    rng, x, group, proto = planted(41, N, D, k, noise=0.1, lengths=(0.5, 1.0, 3.0) if normalize else (1.0,))
    got = fit(store(x), D, k, 8, normalize)
    sizes = np.bincount(group, minlength=k)
    for j in range(k):                                                         # every found cluster is one planted group
        inside = np.bincount(group[got["labels"] == j], minlength=k)
        assert inside.max() >= 0.98 * inside.sum() and inside.max() >= 0.98 * sizes[inside.argmax()]
    assert np.array_equal(got["counts"], np.bincount(got["labels"], minlength=k)) and (np.diff(got["counts"]) <= 0).all()
    assert got["counts"][0] == got["counts"].max() and abs(int(got["counts"][0]) - int(sizes.max())) <= 0.02 * N
    assert (np.diff(got["inertia"]) <= 1e-4 * got["inertia"][:-1]).all()       # Lloyd rounds never raise the inertia beyond rounding


# ---- f. invariance, bit for bit -------------------------------------------------------------------------------------------------------
def test_invariance():
    D, k, N = 96, 17, 2 * SEGMENT + TILE + 3
    rng, x, group, proto = planted(77, N, D, k, noise=0.4)
    rows = store(x)
    a, b = fit(rows, D, k, 4, 1), fit(rows, D, k, 4, 1)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    labels, dist2 = assign(rows, D, a["centroids"], 1)
    assert np.array_equal(labels, a["labels"]) and dist2.tobytes() == a["dist2"].tobytes()
    assert np.array_equal(assign(rows, D, a["centroids"], 1, want_dist2=False)[0], labels)
    for first, n in ((0, 1), (5, TILE), (TILE - 3, SEGMENT + 9), (N - 7, 7)):
        part = assign(rows, D, a["centroids"], 1, first=first, n=n)
        assert np.array_equal(part[0], labels[first:first + n]) and part[1].tobytes() == dist2[first:first + n].tobytes()
    wide = fit(store(x, pad=40), D, k, 4, 1)
    for key in a:
        assert a[key].tobytes() == wide[key].tobytes(), key
    t2 = fit(rows, D, k, 2, 1)
    more = fit(rows, D, k, 2, 1, init=t2["cur"])                               # continued from the centroids in seeding order
    for key in ("cur", "order", "centroids", "counts", "labels", "dist2"):
        assert a[key].tobytes() == more[key].tobytes(), key
    assert a["inertia"][2:].tobytes() == more["inertia"].tobytes()
    quiet = fit(rows, D, k, 4, 1, want_labels=False)
    assert quiet["centroids"].tobytes() == a["centroids"].tobytes()


# ---- g. refusals: by return code and a word of the message; none of these calls writes an output ---------------------------------------------
def test_refusals():
    lib = _lib.load()
    names = ("rows", "init", "cent", "counts", "inertia", "seeds", "labels", "dist2", "ws")
    bufs = {name: torch.full((1 << 18,), 3.0, device="cuda") for name in names}

    def rc_fit(n=100, D=64, ld=64, k=5, iters=2, normalize=1, ws_bytes=4 << 18, null=("init",), shift=None):
        p = {name: bufs[name].data_ptr() for name in names}
        for name in null:
            p[name] = None
        if shift:
            p[shift] += 4
        return lib.cbas_rows_kmeans_fit(p["rows"], n, D, ld, k, iters, normalize, p["init"], p["cent"], p["counts"], p["inertia"], p["seeds"],
                                        p["labels"], p["dist2"], p["ws"], ws_bytes, None)

    def rc_assign(n=100, D=64, ld=64, k=5, normalize=1, null=(), shift=None):
        p = {name: bufs[name].data_ptr() for name in names}
        for name in null:
            p[name] = None
        if shift:
            p[shift] += 4
        return lib.cbas_rows_kmeans_assign(p["rows"], n, D, ld, k, normalize, p["cent"], p["labels"], p["dist2"], None)

    def refused(code, word):
        msg = lib.cbas_last_error().decode()
        assert code == -1 and word in msg, (code, word, msg)           # CBAS_EINVAL
    for rc in (rc_fit, rc_assign):
        refused(rc(k=1), "k =")
        refused(rc(k=65), "k =")
        refused(rc(D=48), "multiple of 32")
        refused(rc(D=0), "multiple of 32")
        refused(rc(D=1568, ld=1568), "multiple of 32")
        refused(rc(ld=32), "ld =")
        refused(rc(ld=68), "multiple of 8")
        refused(rc(n=0), "n_rows")
        refused(rc(n=-1), "n_rows")
        refused(rc(normalize=2), "normalize")
        refused(rc(normalize=-1), "normalize")
        refused(rc(shift="rows"), "16-byte aligned")
        refused(rc(shift="cent"), "16-byte aligned")
        refused(rc(null=("rows",)), "NULL")
    refused(rc_fit(n=4, k=5), "clusters of")
    refused(rc_fit(iters=-1), "iters")
    refused(rc_fit(shift="ws"), "16-byte aligned")
    refused(rc_fit(null=(), shift="init"), "16-byte aligned")
    for name in ("cent", "counts", "inertia", "seeds", "ws"):
        refused(rc_fit(null=("init", name)), "NULL")
    for name in ("cent", "labels"):
        refused(rc_assign(null=(name,)), "NULL")
    need = int(lib.cbas_rows_kmeans_workspace_bytes(100, 64, 5))
    assert 0 < need <= 4 << 18
    refused(rc_fit(ws_bytes=need - 1), "workspace")
    for args in ((0, 64, 5), (100, 48, 5), (100, 1568, 5), (100, 64, 1), (100, 64, 65), (4, 64, 5)):
        assert lib.cbas_rows_kmeans_workspace_bytes(*args) == -1
    # O(n_rows) plus one (k, D) block per SEGMENT: not one per 64 rows
    big = int(lib.cbas_rows_kmeans_workspace_bytes(2_000_000, 768, 64))
    assert big <= 17 * 2_000_000 + (4 * 64 * 768 + 260) * (-(-2_000_000 // SEGMENT) + 2)
    torch.cuda.synchronize()
    for name in names:                                                 # every buffer is as it was
        assert bool((bufs[name] == 3.0).all()), name
    # the neighbours that must be served: an exact workspace, every optional pointer NULL; fewer rows than centroids in _assign
    bufs["rows"].copy_(torch.from_numpy(np.resize(np.random.default_rng(1).standard_normal(1 << 15).astype(np.float16).view(np.float32), 1 << 18)).cuda())
    assert rc_fit(ws_bytes=need, null=("init", "labels", "dist2")) == 0
    assert rc_assign(n=3, null=("dist2",)) == 0
    torch.cuda.synchronize()
    assert bool((bufs["dist2"] == 3.0).all()) and int(bufs["counts"][:10].view(torch.int64).sum()) == 100


# ---- h. through the Python layer ------------------------------------------------------------------------------------------------------
def test_python_layer(tmp_path):
    C, D, k = 4, 64, 4
    sizes = (300, 420, 3)                                                      # the last file is shorter than the smoothing window
    paths, truth = synth.cls_project(str(tmp_path), sizes, D, C, seed=3)
    index = S.FrameIndex(paths, "cuda:0")
    N = index.n_rows
    labels, dist2, clusters = index.cluster(n_clusters=k, iters=10)
    assert labels.dtype == torch.int32 and labels.shape == (N,) and labels.is_cuda and dist2.shape == (N,)
    assert clusters.centroids.shape == (k, D) and clusters.counts.sum() == N and len(clusters.seed_rows) == k and clusters.normalize
    assert all(p in paths and 0 <= f < sizes[paths.index(p)] for p, f in clusters.seed_rows)
    host = labels.cpu().numpy()
    direct = fit(index.rows, D, k, 10, 1)
    assert np.array_equal(host, direct["labels"]) and clusters.centroids.tobytes() == direct["centroids"].tobytes()
    assert np.array_equal(clusters.counts, direct["counts"]) and clusters.inertia.tobytes() == direct["inertia"].tobytes()
    # the labels are the float64 assignment to the returned centroids, but for rows within the bound of a tie
    x = index.rows.cpu().numpy()
    want, _, gap = R.assign(x, clusters.centroids, 1)
    clear = gap > 2.0 * R.score_bound(x, clusters.centroids, 1).max(axis=1)
    assert clear.mean() >= 0.99 and np.array_equal(host[clear], want[clear])
    assert (np.diff(clusters.counts) <= 0).all() and (np.diff(clusters.inertia) <= 1e-4 * clusters.inertia[:-1]).all()
    # later recordings: the same numbers
    clusters.save(str(tmp_path / "clusters.npz"))
    loaded = motifs.FrameClusters.load(str(tmp_path / "clusters.npz"))
    second = S.FrameIndex(paths[1:], "cuda:0")
    l2, d2, same = motifs.cluster_frames(second, clusters=loaded)
    assert same is loaded and np.array_equal(l2.cpu().numpy(), host[300:]) and d2.cpu().numpy().tobytes() == dist2.cpu().numpy()[300:].tobytes()
    with pytest.raises(ValueError, match="width"):
        motifs.cluster_frames(index, clusters=motifs.FrameClusters(np.zeros((k, 32)), np.zeros(k), np.zeros(1), None, 32, True))
    cont = motifs.cluster_frames(index, n_clusters=k, iters=0, init=clusters.centroids)[2]
    assert cont.seed_rows is None and cont.centroids.tobytes() == clusters.centroids.tobytes()
    by_span = motifs.cluster_frames(index, n_clusters=2, iters=1, init=[(paths[0], 0, 20), (paths[1], 30)])[2]
    assert by_span.n_clusters == 2 and by_span.seed_rows is None
    # bouts: no bout crosses a file, and they are the host's
    for w, least in ((1, 1), (5, 3)):
        runs = motifs.motif_runs(index, labels, clusters, smooth_window=w, min_frames=least)
        assert runs == motifs.runs_host(host, index._table, w, least) and len(runs) == 3
        for n, file_runs in zip(sizes, runs):
            assert all(0 <= a <= b < n and 0 <= m < k and b - a + 1 >= least for m, a, b in file_runs)
    with pytest.raises(ValueError, match="odd"):
        motifs.motif_runs(index, labels, clusters, smooth_window=4)
    # transitions within files
    want = np.zeros((k, k), np.int64)
    for first, n in index._table:
        seg = host[first:first + n]
        np.add.at(want, (seg[:-1], seg[1:]), 1)
    trans = motifs.transition_counts(index, labels, k)
    assert trans.is_cuda and trans.dtype == torch.int64 and np.array_equal(trans.cpu().numpy(), want) and want.sum() == N - 3
    # exemplars: frames of the right motif
    ex = motifs.exemplars(index, clusters, per_motif=3, min_gap=5)
    assert len(ex) == k
    for j, hits in enumerate(ex):
        assert 1 <= len(hits) <= 3
        first = {p: int(f) for p, (f, _) in zip(index.files, index._table)}
        assert host[first[hits[0]["file"]] + hits[0]["frame"]] == j
    # the files read back one-hot
    out = motifs.write_outputs(index, labels, clusters, "motifs")
    for path, (first, n) in zip(out, index._table):
        names, _, f32 = pipeline.read_outputs_csv(path)
        assert names == motifs.motif_names(k) and np.array_equal(f32.argmax(axis=1), host[first:first + n])
        assert ((f32 == 0) | (f32 == 1)).all() and (f32.sum(axis=1) == 1).all()
    bins = postprocess.activity_bins_device(torch.from_numpy(f32).cuda(), 0, 0.5, 2)
    assert int(bins.sum()) == int((host[first:first + n] == 0).sum())
    # the command line, end to end
    frames, runs_csv, ex_csv = (str(tmp_path / name) for name in ("frames.csv", "runs.csv", "exemplars.csv"))
    assert motifs.main(["--files", *paths, "--clusters", str(k), "--iters", "10", "--out", frames, "--runs", runs_csv, "--smooth", "5",
                        "--exemplars", ex_csv, "--per-motif", "3", "--save", str(tmp_path / "cli.npz"), "--write-outputs", "cli"]) == 0
    with open(frames, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == motifs.FRAME_COLUMNS and len(rows) == N + 1 and [int(r[2]) for r in rows[1:]] == host.tolist()
    assert rows[1][0] == paths[0] and rows[-1][:2] == [paths[2], "2"]
    with open(runs_csv, newline="") as f:
        assert next(csv.reader(f)) == motifs.RUN_COLUMNS
    assert motifs.FrameClusters.load(str(tmp_path / "cli.npz")).centroids.tobytes() == clusters.centroids.tobytes()
    assert os.path.exists(paths[0].replace("_cls.h5", "_cli_outputs.csv"))
    assert motifs.main(["--files", *paths[1:], "--load", str(tmp_path / "cli.npz"), "--out", frames]) == 0
    with open(frames, newline="") as f:
        assert [int(r[2]) for r in list(csv.reader(f))[1:]] == host[300:].tolist()
