"""The search over resident CLS rows on the GPU (csrc/rows_search.hip through cbas_rows_search, then search.FrameIndex).

  scores      against float64 cosines of the very fp16 rows handed to the device: |score - cosine| <= (2 D + 8) 2^-24, fixed before the
              first run from the sums the header states (gamma_D sum |x_d q_d| rn rq <= gamma_D by Cauchy-Schwarz, gamma_D / 2 + u for
              each reciprocal norm, two roundings); a zero row and a zero query score exactly 0
  selection   index and score equal, bit for bit, rows_search_ref.select applied to the DEVICE trace
  invariance  bit for bit: two calls, another first row, another N, another slot or group of 16 for the query
Each score case prints its largest error / bound (run with -s)."""
import numpy as np
import pytest
import torch

import rows_search_ref as R
from cbas_amd import _lib, h5io, search as S

pytestmark = pytest.mark.gpu

CH = R.CHUNK
PAD = np.float16(60000.0)                  # in the columns past D: read into any sum, it shows


def run(rows, D, queries, table, mask=None, gap=15, threshold=None, k=20, first=0, n=None):
    """cbas_rows_search on rows [first, first + n) of a (rows, ld) fp16 device tensor.  numpy trace (Q, n), index (Q, k), score (Q, k)."""
    lib = _lib.load()
    n = rows.shape[0] - first if n is None else n
    ld = rows.shape[1]
    q = torch.from_numpy(np.ascontiguousarray(queries, np.float32)).cuda()
    Q = q.shape[0]
    tab = torch.from_numpy(np.asarray(table, np.int64).reshape(-1, 2)).cuda()
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda()
    need = int(lib.cbas_rows_search_workspace_bytes(n, Q, k))
    assert need > 0, lib.cbas_last_error()
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    trace = torch.full((Q, n), 7.0, device="cuda")
    index = torch.full((Q, k), -7, dtype=torch.int64, device="cuda")
    score = torch.full((Q, k), 7.0, device="cuda")
    _lib.check(lib.cbas_rows_search(rows.data_ptr() + first * ld * 2, n, D, ld, q.data_ptr(), Q, tab.data_ptr(), tab.shape[0],
                                    None if m is None else m.data_ptr(), gap, int(threshold is not None), float(threshold or 0.0), k,
                                    trace.data_ptr(), index.data_ptr(), score.data_ptr(), ws.data_ptr(), need, None), "cbas_rows_search")
    torch.cuda.synchronize()
    return trace.cpu().numpy(), index.cpu().numpy(), score.cpu().numpy()


def store(x, pad=0):
    """The fp16 rows as a device tensor with `pad` columns of PAD after the D."""
    img = np.full((x.shape[0], x.shape[1] + pad), PAD, np.float16)
    img[:, :x.shape[1]] = x
    return torch.from_numpy(img).cuda()


def same(got, want):
    return np.array_equal(got[0], want[0]) and got[1].tobytes() == np.asarray(want[1], np.float32).tobytes()


# ---- a. scores -------------------------------------------------------------------------------------------------------------------------
SCORE_CASES = [(32, 1, 1, 1), (32, 15, 3, 5), (32, 16, 16, 5), (32, 17, 17, 64), (384, 63, 1, 1), (384, 64, 64, 5), (384, 65, 3, 64),
               (768, CH + 1, 16, 5), (768, 3 * CH - 1, 17, 64), (1536, 17, 3, 1), (1536, CH + 1, 64, 5), (1536, 3 * CH - 1, 1, 64)]


@pytest.mark.parametrize("D,N,Q,k", SCORE_CASES)
def test_scores_and_selection(D, N, Q, k):
    rng = np.random.default_rng(D + 7 * N + Q)
    x = (rng.standard_normal((N, D)) * rng.choice([0.01, 1.0, 30.0], (N, 1))).astype(np.float16)
    q = (rng.standard_normal((Q, D)) * 3).astype(np.float32)
    if N > 2:
        x[N // 2] = 0                                                         # a zero row
    if Q > 1:
        q[Q - 1] = 0                                                          # a zero query
    table = [(0, N)]
    trace, index, score = run(store(x, pad=8 if D < 1536 else 0), D, q, table, gap=2, k=k)
    ref = R.scores64(x, q)
    err = np.abs(trace.astype(np.float64) - ref).max()
    print(f"D={D} N={N} Q={Q}: largest error {err:.3e} = {err / R.score_bound(D):.3f} of the bound {R.score_bound(D):.3e}")
    assert err <= R.score_bound(D)
    if N > 2:
        assert (trace[:, N // 2] == 0).all()
    if Q > 1:
        assert (trace[Q - 1] == 0).all()
    assert same((index, score), R.select(trace, table, None, 2, None, k))


# ---- b. selection, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tied():
    """3 CH - 1 rows drawn from 40 distinct ones: equal scores everywhere, within every gap and across it; the device trace of 3 queries."""
    rng = np.random.default_rng(11)
    pool = rng.standard_normal((40, 32)).astype(np.float16)
    N = 3 * CH - 1
    x = pool[rng.integers(0, 40, N)]
    x[100:140] = pool[7]                                                      # a plateau longer than the gap of 15
    x[CH - 3:CH + 3] = pool[9]                                                # duplicates across a chunk boundary
    x[[500, 510, 530]] = pool[3] * 2                                          # duplicated rows 10 apart (within the gap) and 20 apart (across)
    q = np.stack([pool[7], pool[9] + pool[3], rng.standard_normal(32)]).astype(np.float32)
    rows = store(x)
    trace = run(rows, 32, q, [(0, N)], gap=0, k=1)[0]
    assert len(np.unique(trace[0])) <= 41 and trace[1, 500] == trace[1, 510] == trace[1, 530]
    return rows, q, trace, N


UNEVEN = [(3, 1), (10, 700), (710, 15), (CH - 20, 40), (CH + 30, 2 * CH - 100)]      # rows 0 - 2, 4 - 9, ... lie outside every clip


@pytest.mark.parametrize("gap", [0, 1, 15, 64, 5000])
@pytest.mark.parametrize("clips", ["one", "uneven"])
def test_selection_bit_for_bit(tied, gap, clips):
    rows, q, trace, N = tied
    table = [(0, N)] if clips == "one" else UNEVEN
    rng = np.random.default_rng(gap)
    mask = (rng.random(N) > 0.3).astype(np.uint8)
    mask[100] = 0                                                             # the plateau's winner is masked: nothing of it comes back
    for k, m, thr in ((1, None, None), (5, mask, None), (64, mask, float(np.median(trace))), (64, None, 2.0)):
        t, index, score = run(rows, 32, q, table, mask=m, gap=gap, threshold=thr, k=k)
        assert t.tobytes() == trace.tobytes()
        want = R.select(trace, table, m, gap, thr, k)
        assert same((index, score), want), (gap, clips, k, thr)
        if m is not None:
            assert not np.isin(index, np.flatnonzero(mask == 0)).any()
        if clips == "one" and m is None and thr is None:
            for qi in range(3):                                               # equal scores: the lowest index wins
                assert index[qi, 0] == np.flatnonzero(trace[qi] == trace[qi].max())[0]
    if clips == "uneven":
        inside = np.zeros(N, bool)
        for a, n in UNEVEN:
            inside[a:a + n] = True
        index = run(rows, 32, q, table, gap=gap, k=64)[1]
        assert inside[index[index >= 0]].all()
        if 0 < gap:
            for a, n in UNEVEN:                                               # any two results of one clip are more than the gap apart
                for qi in range(3):
                    hit = np.sort(index[qi][(index[qi] >= a) & (index[qi] < a + n)])
                    assert (np.diff(hit) > gap).all()


def test_gap_limits():
    x = np.random.default_rng(2).standard_normal((70, 32)).astype(np.float16)
    rows = store(x)
    trace, index, score = run(rows, 32, x[:2].astype(np.float32), [(0, 70)], gap=65535, k=3)
    assert same((index, score), R.select(trace, [(0, 70)], None, 65535, None, 3)) and (index[:, 1:] == -1).all() and index[:, 0].tolist() == [0, 1]
    lib = _lib.load()
    assert lib.cbas_rows_search(rows.data_ptr(), 70, 32, 32, rows.data_ptr(), 1, rows.data_ptr(), 1, None, 70000, 0, 0.0, 3, rows.data_ptr(),
                                rows.data_ptr(), rows.data_ptr(), rows.data_ptr(), 1 << 20, None) == -1
    assert "min_gap" in lib.cbas_last_error().decode()


# ---- c. invariance, bit for bit --------------------------------------------------------------------------------------------------------
def test_invariance():
    rng = np.random.default_rng(5)
    N, D = CH + 77, 32                                                        # rows of 64 bytes
    x = rng.standard_normal((N, D)).astype(np.float16)
    q = rng.standard_normal((17, D)).astype(np.float32)
    rows = store(x)
    a = run(rows, D, q, [(0, N)])
    b = run(rows, D, q, [(0, N)])
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()                                     # two calls: the same bytes
    for first in (1, 5, 16, CH - 1):                                          # the store starts at another row
        t = run(rows, D, q, [(0, N - first)], first=first)[0]
        assert t.tobytes() == np.ascontiguousarray(a[0][:, first:]).tobytes(), first
    for n in (1, 15, 17, CH, CH + 1):                                         # another N
        t = run(rows, D, q, [(0, n)], n=n)[0]
        assert t.tobytes() == np.ascontiguousarray(a[0][:, :n]).tobytes(), n
    # the query in another slot and another group of 16
    perm = np.roll(np.arange(17), 1)                                          # slot j holds query j - 1; slot 0 of group 0 holds query 16
    t = run(rows, D, q[perm], [(0, N)])[0]
    assert t.tobytes() == a[0][perm].tobytes()
    alone = run(rows, D, q[16:17], [(0, N)])[0]
    assert alone.tobytes() == a[0][16:17].tobytes()
    wide = run(rows, D, np.concatenate([q, q, q, q[:13]]), [(0, N)])[0]      # 64 queries: four groups
    assert wide[17:34].tobytes() == a[0].tobytes() and wide[51:].tobytes() == a[0][:13].tobytes()


# ---- d. planted neighbours through FrameIndex.search -----------------------------------------------------------------------------------
def test_planted_neighbours(tmp_path):
    rng = np.random.default_rng(21)
    D, sizes = 256, (400, 700, 300)
    a = rng.standard_normal(D)
    a /= np.linalg.norm(a)
    files = [rng.standard_normal((n, D)) for n in sizes]
    planted = {(0, 50): 0.02, (0, 200): 0.10, (1, 10): 0.06, (1, 600): 0.14, (2, 100): 0.18,
               (1, 300): 0.30, (1, 301): 0.26, (1, 302): 0.22, (1, 303): 0.27, (1, 304): 0.31}     # a bout: frame 302 is its peak
    for (f, frame), noise in planted.items():
        e = rng.standard_normal(D)
        e -= (e @ a) * a                                                      # orthogonal noise: the cosine is 1 / sqrt(1 + noise^2)
        files[f][frame] = 9.0 * (a + noise * e / np.linalg.norm(e))
    files = [x.astype(np.float16) for x in files]
    paths = []
    for i, x in enumerate(files):
        paths.append(str(tmp_path / f"rec{i}_cls.h5"))
        with h5io.ClsWriter(paths[-1], D) as w:
            w.append(x)
    q = a.astype(np.float32)
    cos = [R.scores64(x, q[None])[0] for x in files]
    keys = sorted(planted, key=lambda fk: -cos[fk[0]][fk[1]])
    vals = np.array([cos[f][k] for f, k in keys])
    assert vals.min() > 0.95 and (-np.diff(vals)).min() > 1e-3                # the data: planted rows far over the rest and well apart
    for f, x in enumerate(cos):
        rest = np.delete(x, [k for ff, k in planted if ff == f])
        assert np.abs(rest).max() < 0.5
    peaks = [fk for fk in keys if not (fk[0] == 1 and fk[1] in (300, 301, 303, 304))]

    index = S.FrameIndex(paths, "cuda:0")
    assert (index.n_rows, index.dim, index.files) == (1400, D, paths)
    (hits,), trace = index.search(q, k=20, min_gap=15, return_trace=True)
    assert [(h["file"], h["frame"]) for h in hits[:len(peaks)]] == [(paths[f], k) for f, k in peaks]
    assert all(h["score"] < 0.5 for h in hits[len(peaks):]) and len(hits) == 20
    assert all(abs(h["score"] - cos[f][k]) <= R.score_bound(D) for h, (f, k) in zip(hits, peaks))
    # the same through query_from: the planted row itself as the query
    (hits2,) = index.search([(paths[2], 100)], k=3, min_gap=15)
    assert (hits2[0]["file"], hits2[0]["frame"]) == (paths[2], 100) and abs(hits2[0]["score"] - 1.0) <= R.score_bound(D)
    # excluding the bout removes it AND its neighbours: the masked rows still suppress them
    (hits3,) = index.search(q, k=20, min_gap=15, exclude=[(paths[1], 300, 304)])
    got = [(h["file"], h["frame"]) for h in hits3]
    assert got[:len(peaks) - 1] == [(paths[f], k) for f, k in peaks if (f, k) != (1, 302)]
    assert not any(p == paths[1] and 287 <= fr <= 317 for p, fr in got)
    # a threshold keeps the planted peaks only; two queries at once
    both = index.search(np.stack([q, -q]), k=20, min_gap=15, threshold=0.9)
    assert [(h["file"], h["frame"]) for h in both[0]] == [(paths[f], k) for f, k in peaks] and both[1] == []
    # the trace is the C call's
    table = [(0, 400), (400, 700), (1100, 300)]
    t, idx, sc = run(index.rows, D, q[None], table, gap=15, k=20)
    assert trace.cpu().numpy().tobytes() == t.tobytes() and trace.shape == (1, 1400)
    assert [index.locate(m) for m in idx[0]] == [(h["file"], h["frame"]) for h in hits]
    assert np.array_equal(sc[0], np.array([h["score"] for h in hits], np.float32))


# ---- e. refusals: by return code and a word of the message; none of these calls writes an output -------------------------------------------
def test_refusals():
    lib = _lib.load()
    names = ("rows", "q", "table", "mask", "trace", "index", "score", "ws")
    bufs = {name: torch.full((1 << 16,), 3.0, device="cuda") for name in names}
    bufs["table"] = torch.tensor([[0, 40], [40, 60]], dtype=torch.int64, device="cuda")
    good_table = bufs["table"].clone()

    def rc(n=100, D=64, ld=64, Q=2, n_clips=2, gap=15, k=5, ws_bytes=4 << 16, null=None, shift=None):
        p = {name: bufs[name].data_ptr() for name in names}
        if null:
            p[null] = None
        if shift:
            p[shift] += 4
        return lib.cbas_rows_search(p["rows"], n, D, ld, p["q"], Q, p["table"], n_clips, p["mask"], gap, 0, 0.0, k, p["trace"], p["index"],
                                    p["score"], p["ws"], ws_bytes, None)

    def refused(code, word):
        msg = lib.cbas_last_error().decode()
        assert code == -1 and word in msg, (code, word, msg)           # CBAS_EINVAL
    refused(rc(D=48), "multiple of 32")
    refused(rc(D=1568, ld=1568), "multiple of 32")
    refused(rc(D=0), "multiple of 32")
    refused(rc(ld=32), "ld")
    refused(rc(ld=68), "multiple of 8")
    refused(rc(n=0), "n_rows")
    refused(rc(Q=0), "n_queries")
    refused(rc(Q=65), "n_queries")
    refused(rc(k=0), "k =")
    refused(rc(k=65), "k =")
    refused(rc(gap=-1), "min_gap")
    refused(rc(gap=65536), "min_gap")
    refused(rc(n_clips=0), "n_clips")
    for name in ("rows", "q", "table", "trace", "index", "score", "ws"):
        refused(rc(null=name), "NULL")
    for name in ("rows", "q", "trace", "ws"):
        refused(rc(shift=name), "16-byte aligned")
    need = int(lib.cbas_rows_search_workspace_bytes(100, 2, 5))
    assert 0 < need <= 4 << 16
    refused(rc(ws_bytes=need - 1), "workspace")
    for args in ((0, 2, 5), (100, 0, 5), (100, 65, 5), (100, 2, 0), (100, 2, 65)):
        assert lib.cbas_rows_search_workspace_bytes(*args) == -1
    # a bad clip table is found on the device before anything is indexed with it
    for bad, word in (([[0, 40], [40, 61]], "outside"), ([[-1, 40], [40, 60]], "outside"), ([[0, 40], [1 << 62, 1 << 62]], "outside"),
                      ([[0, 40], [90, -5]], "outside"), ([[0, 41], [40, 60]], "overlap"), ([[10, 50], [20, 5]], "overlap"),
                      ([[0, 100], [0, 100]], "overlap")):
        bufs["table"].copy_(torch.tensor(bad, dtype=torch.int64))
        refused(rc(), word)
    bufs["table"].copy_(good_table)
    torch.cuda.synchronize()
    for name in ("rows", "q", "mask", "trace", "index", "score"):      # every output is as it was
        assert bool((bufs[name] == 3.0).all()), name
    # the neighbours that must be served: an exact workspace, no mask, an empty clip beside the others
    bufs["rows"].copy_(torch.from_numpy(np.resize(np.random.default_rng(1).standard_normal(1 << 15).astype(np.float16).view(np.float32), 1 << 16)).cuda())
    assert rc(ws_bytes=need, null="mask") == 0
    bufs["table"].copy_(torch.tensor([[0, 100], [50, 0]], dtype=torch.int64))
    assert rc(ws_bytes=need, null="mask") == 0
    torch.cuda.synchronize()
