"""The k-NN labels over resident CLS rows on the GPU (csrc/rows_knn.hip through cbas_rows_knn, then knn.LabelBank / FrameIndex.knn_labels).

  cosines      sims against float64 cosines of the very fp16 rows handed to the device: |sims - cos64| <= (2 D + 8) 2^-24
  selection    nn_index and nn_score equal, bit for bit, rows_knn_ref.select applied to the DEVICE's sims
  vote         probs against rows_knn_ref.vote64 on the DEVICE's neighbours: |p - p64| <= (8 / T + 2 k + 8) 2^-24
  invariance   bit for bit: two calls, another first row, another N, a longer bank, a permuted bank
The bounds are derived in rows_knn_ref.py.  Each cosine and vote case prints its largest error / bound (run with -s)."""
import numpy as np
import pytest
import torch

import rows_knn_ref as K
from cbas_amd import _lib, knn, pipeline, postprocess, search as S, synth

pytestmark = pytest.mark.gpu

TILE, BLOCK = K.TILE, K.BLOCK
PAD = np.float16(60000.0)                  # in the columns past D: read into any sum, it shows


def store(x, pad=8):
    """The fp16 rows as a device tensor with `pad` columns of PAD after the D."""
    img = np.full((x.shape[0], x.shape[1] + pad), PAD, np.float16)
    img[:, :x.shape[1]] = x
    return torch.from_numpy(img).cuda()


def dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def run(rows, D, bank, labels, C, k=20, T=0.07, bank_group=None, row_group=None, cw=None, first=0, n=None, full=True):
    """cbas_rows_knn on rows [first, first + n) of a (rows, ld) fp16 device tensor against a (M, bank_ld) device bank.
    numpy probs (n, C), and with `full` nn_index (n, k), nn_score (n, k), sims (n, M)."""
    lib = _lib.load()
    n = rows.shape[0] - first if n is None else n
    M = bank.shape[0]
    lab, bg, rg, w = dev(labels, np.int32), dev(bank_group, np.int32), dev(row_group, np.int32), dev(cw, np.float32)
    need = int(lib.cbas_rows_knn_workspace_bytes(n, M, k))
    assert need > 0, lib.cbas_last_error()
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    probs = torch.full((n, C), 7.0, device="cuda")
    index = torch.full((n, k), -7, dtype=torch.int32, device="cuda") if full else None
    score = torch.full((n, k), 7.0, device="cuda") if full else None
    sims = torch.full((n, M), 7.0, device="cuda") if full else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _lib.check(lib.cbas_rows_knn(rows.data_ptr() + first * rows.shape[1] * 2, n, D, rows.shape[1], bank.data_ptr(), M, bank.shape[1], lab.data_ptr(),
                                 ptr(bg), ptr(rg), C, ptr(w), k, float(T), probs.data_ptr(), ptr(index), ptr(score), ptr(sims), ws.data_ptr(), need,
                                 None), "cbas_rows_knn")
    torch.cuda.synchronize()
    if not full:
        return probs.cpu().numpy()
    return probs.cpu().numpy(), index.cpu().numpy(), score.cpu().numpy(), sims.cpu().numpy()


def data(seed, N, M, D):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, D)) * rng.choice([0.01, 1.0, 30.0], (N, 1))).astype(np.float16)
    y = (rng.standard_normal((M, D)) * rng.choice([0.01, 1.0, 30.0], (M, 1))).astype(np.float16)
    tiny = np.float16(6.2e-5)              # no fp16 subnormals: what the MFMA does with them is not part of the contract
    x[(np.abs(x) < tiny) & (x != 0)] = tiny
    y[(np.abs(y) < tiny) & (y != 0)] = tiny
    return rng, x, y


def check_vote(probs, index, score, labels, cw, T, C, k):
    ref = K.vote64(index, score, labels, cw, float(np.float32(T)), C)       # the temperature the device was handed
    err = np.abs(probs.astype(np.float64) - ref).max()
    has = index[:, 0] >= 0
    rows_err = np.abs(probs[has].astype(np.float64).sum(axis=1) - 1.0).max() if has.any() else 0.0
    assert err <= K.prob_bound(T, k) and rows_err <= K.prob_bound(T, k), (err, rows_err, K.prob_bound(T, k))
    assert (probs[~has] == 0).all()
    return err


# ---- a. cosines ------------------------------------------------------------------------------------------------------------------------
COS_CASES = [(32, 1, 1), (32, 17, 63), (32, 65, 65), (384, 63, 129), (768, TILE + 1, 3 * BLOCK + 1), (1536, 2 * TILE - 1, BLOCK - 1),
             (1536, 16, 2 * BLOCK)]


@pytest.mark.parametrize("D,N,M", COS_CASES)
def test_cosines_selection_and_vote(D, N, M):
    rng, x, y = data(D + 7 * N + M, N, M, D)
    if N > 2:
        x[N // 2] = 0                                                         # a zero store row
    if M > 1:
        y[M - 1] = 0                                                          # a zero bank row
    C, k = 7, 5
    labels = rng.integers(0, C, M)
    probs, index, score, sims = run(store(x), D, store(y, pad=16), labels, C, k=k)
    ref = K.cos64(x, y)
    err = np.abs(sims.astype(np.float64) - ref).max()
    print(f"D={D} N={N} M={M}: largest error {err:.3e} = {err / K.cos_bound(D):.3f} of the bound {K.cos_bound(D):.3e}")
    assert err <= K.cos_bound(D)
    if N > 2:
        assert (sims[N // 2] == 0).all()
    if M > 1:
        assert (sims[:, M - 1] == 0).all()
    want = K.select(sims, None, None, k)
    assert np.array_equal(index, want[0]) and score.tobytes() == want[1].tobytes()
    check_vote(probs, index, score, labels, None, 0.07, C, k)


# ---- b. selection, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tied():
    """A bank of 3 BLOCK + 5 entries drawn from 40 distinct rows: ties within a block and across block boundaries."""
    rng = np.random.default_rng(11)
    pool = rng.standard_normal((40, 32)).astype(np.float16)
    M, N = 3 * BLOCK + 5, TILE + 9
    y = pool[rng.integers(0, 40, M)]
    y[BLOCK - 2:BLOCK + 2] = pool[9]                                          # duplicates across a block boundary
    y[[3, 2 * BLOCK + 1, 3 * BLOCK + 4]] = pool[3] * 2                        # the same direction in three blocks
    x = rng.standard_normal((N, 32)).astype(np.float16)
    x[0], x[1] = pool[9], pool[3]
    bank_group = rng.integers(0, 6, M).astype(np.int32)
    row_group = rng.integers(-1, 6, N).astype(np.int32)
    bank_group[rng.random(M) < 0.1] = -1
    return store(x), store(y), x, y, bank_group, row_group, rng.integers(0, 7, M)


@pytest.mark.parametrize("k", [1, 5, 20, 64])
@pytest.mark.parametrize("groups", [False, True])
def test_selection_bit_for_bit(tied, k, groups):
    rows, bank, x, y, bank_group, row_group, labels = tied
    bg, rg = (bank_group, row_group) if groups else (None, None)
    probs, index, score, sims = run(rows, 32, bank, labels, 7, k=k, bank_group=bg, row_group=rg)
    assert len(np.unique(sims[0])) <= 41
    want = K.select(sims, bg, rg, k)
    assert np.array_equal(index, want[0]) and score.tobytes() == want[1].tobytes()
    if not groups:                                                            # equal scores: the lowest index wins
        for m, planted in ((0, [BLOCK - 2, BLOCK - 1, BLOCK, BLOCK + 1]), (1, [3, 2 * BLOCK + 1, 3 * BLOCK + 4])):
            top = np.flatnonzero(sims[m] == sims[m].max())                    # the planted copies, and the pool's own draws of that row
            assert set(planted) <= set(top.tolist()) and index[m, :min(k, top.size)].tolist() == top[:k].tolist()
        alone = run(rows, 32, bank, labels, 7, k=k, bank_group=bank_group)    # one group array alone excludes nothing
        assert np.array_equal(alone[1], index) and alone[0].tobytes() == probs.tobytes()
    else:
        m, r = np.nonzero(index >= 0)
        assert not ((bank_group[index[m, r]] == row_group[m]) & (row_group[m] >= 0)).any()
    check_vote(probs, index, score, labels, None, 0.07, 7, k)


def test_short_and_excluded_banks(tied):
    rows, bank, x, y, _, _, labels = tied
    N = x.shape[0]
    for M in (1, 3, 19):                                                      # M < k: -1 / -inf past the last
        probs, index, score, sims = run(rows, 32, bank[:M].contiguous(), labels[:M], 7, k=20)
        want = K.select(sims, None, None, 20)
        assert np.array_equal(index, want[0]) and score.tobytes() == want[1].tobytes()
        assert (index[:, M:] == -1).all() and np.isneginf(score[:, M:]).all() and (index[:, :M] >= 0).all()
        check_vote(probs, index, score, labels[:M], None, 0.07, 7, 20)
    # rows whose whole bank is excluded: every row of group 0 when all of the bank is group 0
    row_group = np.where(np.arange(N) % 3 == 0, 0, np.where(np.arange(N) % 3 == 1, 1, -1)).astype(np.int32)
    bank_group = np.zeros(y.shape[0], np.int32)
    probs, index, score, sims = run(rows, 32, bank, labels, 7, k=5, bank_group=bank_group, row_group=row_group)
    out = row_group == 0
    assert (index[out] == -1).all() and np.isneginf(score[out]).all() and (probs[out] == 0).all() and (index[~out] >= 0).all()
    want = K.select(sims, bank_group, row_group, 5)
    assert np.array_equal(index, want[0]) and score.tobytes() == want[1].tobytes()
    check_vote(probs, index, score, labels, None, 0.07, 7, 5)


# ---- c. probabilities ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def voters():
    rng, x, y = data(31, TILE + 3, 2 * BLOCK + 7, 64)
    y[:40] = x[:40]                                                           # exact copies: cosines of 1 at the top of some lists
    return rng, store(x), store(y), x, y


@pytest.mark.parametrize("T", [0.07, 1.0])
@pytest.mark.parametrize("C", [1, 2, 7, 64])
def test_probabilities(voters, T, C):
    rng, rows, bank, x, y = voters
    M = y.shape[0]
    labels = np.random.default_rng(C).integers(0, C, M)
    for k in (1, 20, 64):
        for cw in (None, np.random.default_rng(C + k).uniform(0.25, 4.0, C).astype(np.float32)):
            probs, index, score, sims = run(rows, 64, bank, labels, C, k=k, T=T, cw=cw)
            err = check_vote(probs, index, score, labels, cw, T, C, k)
            print(f"T={T} C={C} k={k} cw={'yes' if cw is not None else 'no'}: largest error {err:.3e} = {err / K.prob_bound(T, k):.3f} of the bound")
            bare = run(rows, 64, bank, labels, C, k=k, T=T, cw=cw, full=False)      # sims == NULL, neighbours == NULL
            assert bare.tobytes() == probs.tobytes()


# ---- d. invariance, bit for bit --------------------------------------------------------------------------------------------------------
def test_invariance():
    rng, x, y = data(5, TILE + 77, 2 * BLOCK + 11, 96)
    N, M, D, C = x.shape[0], y.shape[0], 96, 5
    labels = rng.integers(0, C, M)
    bg, rg = rng.integers(0, 9, M).astype(np.int32), rng.integers(-1, 9, N).astype(np.int32)
    rows, bank = store(x), store(y)
    a = run(rows, D, bank, labels, C, bank_group=bg, row_group=rg)
    b = run(rows, D, bank, labels, C, bank_group=bg, row_group=rg)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()                                     # two calls: the same bytes
    for first in (1, 5, 16, TILE - 1):                                        # the store starts at another row
        t = run(rows, D, bank, labels, C, bank_group=bg, row_group=rg[first:], first=first)
        for u, v in zip(t, a):
            assert u.tobytes() == np.ascontiguousarray(v[first:]).tobytes(), first
    for n in (1, 15, 17, TILE, TILE + 1):                                     # another N
        t = run(rows, D, bank, labels, C, bank_group=bg, row_group=rg[:n], n=n)
        for u, v in zip(t, a):
            assert u.tobytes() == np.ascontiguousarray(v[:n]).tobytes(), n
    # the bank followed by entries that lose everywhere: zero rows in a group no row has, against rows whose neighbours all score above 0
    plain = run(rows, D, bank, labels, C, k=3)
    assert (plain[2] > 0).all()
    extra = np.concatenate([y, np.zeros((BLOCK + 3, D), np.float16)])
    longer = run(rows, D, store(extra), np.concatenate([labels, np.zeros(BLOCK + 3, np.int64)]), C, k=3)
    assert longer[0].tobytes() == plain[0].tobytes() and np.array_equal(longer[1], plain[1]) and longer[2].tobytes() == plain[2].tobytes()
    assert longer[3][:, :M].tobytes() == plain[3].tobytes()
    # a permuted bank: the same score bits per (row, entry)
    perm = rng.permutation(M)
    shuffled = run(rows, D, store(y[perm]), labels[perm], C, k=3)
    assert shuffled[3].tobytes() == np.ascontiguousarray(plain[3][:, perm]).tobytes()


# ---- e. refusals: by return code and a word of the message; none of these calls writes an output -------------------------------------------
def test_refusals():
    lib = _lib.load()
    names = ("rows", "bank", "label", "bgroup", "rgroup", "cw", "probs", "index", "score", "sims", "ws")
    bufs = {name: torch.full((1 << 16,), 3.0, device="cuda") for name in names}
    bufs["label"] = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")

    def rc(n=100, D=64, ld=64, M=50, bank_ld=64, C=4, k=5, T=0.07, ws_bytes=4 << 16, null=(), shift=None):
        p = {name: bufs[name].data_ptr() for name in names}
        for name in null:
            p[name] = None
        if shift:
            p[shift] += 4
        return lib.cbas_rows_knn(p["rows"], n, D, ld, p["bank"], M, bank_ld, p["label"], p["bgroup"], p["rgroup"], C, p["cw"], k, T, p["probs"],
                                 p["index"], p["score"], p["sims"], p["ws"], ws_bytes, None)

    def refused(code, word):
        msg = lib.cbas_last_error().decode()
        assert code == -1 and word in msg, (code, word, msg)           # CBAS_EINVAL
    refused(rc(D=48), "multiple of 32")
    refused(rc(D=0), "multiple of 32")
    refused(rc(D=1568, ld=1568, bank_ld=1568), "multiple of 32")
    refused(rc(ld=32), "ld =")
    refused(rc(ld=68), "multiple of 8")
    refused(rc(bank_ld=32), "bank_ld")
    refused(rc(bank_ld=68), "bank_ld")
    refused(rc(M=0), "M =")
    refused(rc(M=65537), "M =")
    refused(rc(k=0), "k =")
    refused(rc(k=65), "k =")
    refused(rc(C=0), "C =")
    refused(rc(C=65), "C =")
    refused(rc(n=-1), "N =")
    for T in (0.0, -1.0, float("inf"), float("nan")):
        refused(rc(T=T), "temperature")
    for name in ("rows", "bank", "label", "probs", "ws"):
        refused(rc(null=(name,)), "NULL")
    for name in ("rows", "bank", "ws"):
        refused(rc(shift=name), "16-byte aligned")
    need = int(lib.cbas_rows_knn_workspace_bytes(100, 50, 5))
    assert 0 < need <= 4 << 16
    refused(rc(ws_bytes=need - 1), "workspace")
    for args in ((-1, 50, 5), (100, 0, 5), (100, 65537, 5), (100, 50, 0), (100, 50, 65)):
        assert lib.cbas_rows_knn_workspace_bytes(*args) == -1
    assert lib.cbas_rows_knn_workspace_bytes(0, 1, 1) > 0
    # a label outside [0, C) is found on the device before it is used as an index
    for bad in (4, -1, 1 << 30):
        bufs["label"][37] = bad
        refused(rc(), "label")
    bufs["label"][37] = 0
    assert rc(n=0) == 0                                                # N = 0: nothing is done
    torch.cuda.synchronize()
    for name in ("rows", "bank", "bgroup", "rgroup", "cw", "probs", "index", "score", "sims"):      # every output is as it was
        assert bool((bufs[name] == 3.0).all()), name
    # the neighbours that must be served: an exact workspace, every optional pointer NULL
    bufs["rows"].copy_(torch.from_numpy(np.resize(np.random.default_rng(1).standard_normal(1 << 15).astype(np.float16).view(np.float32), 1 << 16)).cuda())
    bufs["bank"].copy_(bufs["rows"])
    assert rc(ws_bytes=need, null=("bgroup", "rgroup", "cw", "index", "score", "sims")) == 0
    torch.cuda.synchronize()
    assert bool((bufs["probs"][:400].reshape(100, 4)[:, 0] == 1.0).all()) and bool((bufs["probs"][400:] == 3.0).all())


# ---- f. through the public interface -----------------------------------------------------------------------------------------------------
def test_public_interface(tmp_path):
    C, D = 4, 64
    paths, labels = synth.cls_project(str(tmp_path), (300, 420, 260), D, C, seed=3)
    behaviors = [f"b{c}" for c in range(C)]
    instances = [(p, a, b, behaviors[c]) for p, lab in zip(paths, labels) for a, b, c in synth.label_runs(lab)]
    index = S.FrameIndex(paths, "cuda:0")
    bank = knn.LabelBank.from_instances(index, instances, behaviors, stride=3, group="file")
    M, N = len(bank), index.n_rows
    assert N == 980 and M > 2 * BLOCK and bank.rows.shape == (M, D)
    probs, nn_index, nn_score = index.knn_labels(bank, k=20, temperature=0.07, exclude=True, return_neighbours=True)
    direct = run(index.rows, D, bank.rows, bank.label.cpu().numpy(), C, k=20, T=0.07, bank_group=bank.group.cpu().numpy(),
                 row_group=bank.row_group.cpu().numpy())
    assert probs.cpu().numpy().tobytes() == direct[0].tobytes() and np.array_equal(nn_index.cpu().numpy(), direct[1])
    assert nn_score.cpu().numpy().tobytes() == direct[2].tobytes() and probs.shape == (N, C) and probs.dtype == torch.float32
    file_of = np.repeat(np.arange(3), (300, 420, 260))
    assert (file_of[bank.store_row[direct[1]]] != file_of[:, None]).all()     # leave-one-file-out: no neighbour of a row's own file
    assert index.knn_labels(bank, k=20).cpu().numpy().tobytes() == run(index.rows, D, bank.rows, bank.label.cpu().numpy(), C, full=False).tobytes()
    # the report: the numpy report of the same probabilities
    report = knn.knn_report(index, bank, k=20, temperature=0.07)
    own = direct[0][bank.store_row]
    pred = np.where(own.max(axis=1) > 0, own.argmax(axis=1), -1)
    assert report == knn.report_from_predictions(bank.label.cpu().numpy(), pred, behaviors)
    assert 0.0 <= report["accuracy"] <= 1.0 and report["weighted avg"]["support"] == M
    # the files, and the probabilities as events
    plain = index.knn_labels(bank, k=20)
    out = knn.write_outputs(index, plain, behaviors, "knn")
    host = plain.cpu().numpy()
    for path, (first, n) in zip(out, index._table):
        names, _, f32 = pipeline.read_outputs_csv(path)
        assert names == behaviors and f32 is not None and f32.tobytes() == host[first:first + n].tobytes()
    events = postprocess.predictions_to_instances(plain[:300].contiguous(), behaviors, "clip0.mp4")
    assert events == postprocess.predictions_to_instances(host[:300], behaviors, "clip0.mp4") and len(events) > 0
    with pytest.raises(ValueError, match="width"):
        other = knn.LabelBank(bank.rows, bank.label, bank.group, bank.row_group, bank.store_row, behaviors, 32, "file")
        index.knn_labels(other)
