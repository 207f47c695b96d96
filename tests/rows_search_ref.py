"""What cbas_rows_search must give, written from the comment in include/cbas_mi355x.h (not from the kernels): the float64 cosines,
and the peak and top-k rules restated on a GIVEN float32 trace - comparisons and integers only, so it is exact.  A helper, not a
test."""
import numpy as np

CHUNK = 1024                 # rows per first-stage list of csrc/rows_search.hip: the sizes at which the selection takes another path
MAX_Q, MAX_K, MAX_GAP = 64, 64, 65535


def scores64(rows_f16, queries):
    """(Q, N) float64 cosines of fp16 rows (N, D) and queries (Q, D); a zero row or a zero query scores 0."""
    x = np.asarray(rows_f16).astype(np.float64)
    q = np.asarray(queries).astype(np.float64)
    xn = np.sqrt((x * x).sum(axis=1))
    qn = np.sqrt((q * q).sum(axis=1))
    den = qn[:, None] * xn[None, :]
    return np.divide(q @ x.T, den, out=np.zeros((q.shape[0], x.shape[0])), where=den > 0)


def score_bound(D):
    """|score - cosine| <= (2 D + 8) 2^-24: gamma_D sum |x_d q_d| rn rq <= gamma_D by Cauchy-Schwarz, gamma_D / 2 + u for each
    reciprocal norm, two roundings."""
    return (2 * D + 8) * 2.0 ** -24


def peaks(trace_row, clip_table, min_gap):
    """bool (N): row m of a clip is a peak iff every m' of the same clip with 0 < |m - m'| <= min_gap has a lower score, or
    an equal score and m' > m.  Rows outside every clip are no peaks."""
    t = np.asarray(trace_row, np.float32)
    out = np.zeros(t.shape[0], bool)
    for first, n in np.asarray(clip_table, np.int64).reshape(-1, 2):
        first, n = int(first), int(n)
        s = t[first:first + n]
        ok = np.ones(n, bool)
        for d in range(1, min(int(min_gap), n - 1) + 1):
            ok[d:] &= s[:-d] < s[d:]             # the neighbour d rows before: strictly lower
            ok[:-d] &= s[d:] <= s[:-d]           # the neighbour d rows after: lower or equal
        out[first:first + n] = ok
    return out


def select(trace_f32, clip_table, mask, min_gap, threshold, k):
    """index (Q, k) int64 and score (Q, k) float32: per query the k best unmasked peaks with score >= threshold (None: no
    threshold) by (score descending, row ascending); (-1, -inf) past the last."""
    trace = np.asarray(trace_f32, np.float32)
    if trace.ndim == 1:
        trace = trace[None]
    Q, N = trace.shape
    index = np.full((Q, k), -1, np.int64)
    score = np.full((Q, k), -np.inf, np.float32)
    for q in range(Q):
        cand = peaks(trace[q], clip_table, min_gap)
        if mask is not None:
            cand &= np.asarray(mask).astype(bool)
        if threshold is not None:
            cand &= trace[q] >= np.float32(threshold)
        rows = np.flatnonzero(cand)
        order = np.lexsort((rows, -trace[q][rows].astype(np.float64)))[:k]
        index[q, :order.size] = rows[order]
        score[q, :order.size] = trace[q][rows[order]]
    return index, score
