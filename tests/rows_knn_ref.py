"""What cbas_rows_knn must give, written from the comment in include/cbas_mi355x.h (not from the kernels).  A helper, not a test.

THE DEFINITION
  cos[m][j]   = fl(fl(dot * rn_row[m]) * rn_bank[j]); dot the fp32-accumulated sum of the exact fp16 products on the fp16 matrix pipe
                over D in ascending blocks of 32; rn = fp32(1 / sqrt((double)s)), 0 for a zero row, s the fp32 sum of squares in
                rows_search's order.  A zero row scores exactly 0.  sims holds every pair's cosine, excluded ones included.
  excluded    bank entry j for row m when both group arrays are given and bank_group[j] == row_group[m] >= 0
  neighbours  the k best entries that are not excluded; a beats b when cos[a] > cos[b], or cos[a] == cos[b] and a < b; in that order;
              (-1, -inf) past the last.  A function of the cosine bits and the bank indices alone.
  vote        s_0 the best score; w_r = expf(__fdiv_rn(s_r - s_0, T)) * cw[label_r]; Z = the fp32 sum of w_r in ascending rank; num_c
              that of the neighbours with label c; probs[m][c] = num_c / Z; zeros for a row without a neighbour.

THE BOUNDS, fixed before the first run
  cosine      |sims - cos64| <= (2 D + 8) 2^-24 = rows_search_ref.score_bound(D): the dot's D u32 S (oracle/kernel_ref.gemm_acc's bound
              for the fp16 pipe, u32 = 2^-24, S = sum |x_d y_d|) times rn rn, and S rn rn <= 1 by Cauchy-Schwarz; D / 2 u32 + u32 for
              each reciprocal norm (the sum of squares' D u32 halved by the square root, one rounding to fp32); two roundings.
  vote        |p - p64| <= (8 / T + 2 k + 8) 2^-24 against vote64 on the device's own neighbours.  The exponent's argument
              (s_r - s_0) / T: |s_r - s_0| <= 2 is rounded once (2 u32 absolute at most) and the quotient once more (relative u32 of
              at most 2 / T), so the argument is off by at most 4 u32 / T and exp, at most 1 there, by as much relatively; twice
              that, 8 u32 / T, covers numerator and denominator.  The two sums of at most k positive terms add k u32 each, relative.
              expf's own rounding, the product with cw and the division are the constant 8 u32.  p <= 1, so relative is absolute.
"""
import numpy as np

from cbas_amd.knn import BLOCK, TILE  # noqa: F401  (the sizes at which the kernel takes another path)
from rows_search_ref import score_bound as cos_bound  # noqa: F401

MAX_M, MAX_K, MAX_C = 65536, 64, 64


def cos64(rows_f16, bank_f16):
    """(N, M) float64 cosines of fp16 rows (N, D) and bank rows (M, D); a zero row scores 0 with everything."""
    x = np.asarray(rows_f16).astype(np.float64)
    y = np.asarray(bank_f16).astype(np.float64)
    den = np.sqrt((x * x).sum(axis=1))[:, None] * np.sqrt((y * y).sum(axis=1))[None, :]
    return np.divide(x @ y.T, den, out=np.zeros((x.shape[0], y.shape[0])), where=den > 0)


def prob_bound(T, k):
    return (8.0 / T + 2 * k + 8) * 2.0 ** -24


def select(sims_f32, bank_group, row_group, k):
    """index (N, k) int32 and score (N, k) float32 from a GIVEN float32 (N, M) matrix: comparisons and integers only."""
    sims = np.asarray(sims_f32, np.float32)
    N, M = sims.shape
    index = np.full((N, k), -1, np.int32)
    score = np.full((N, k), -np.inf, np.float32)
    for m in range(N):
        ok = np.ones(M, bool)
        if bank_group is not None and row_group is not None and row_group[m] >= 0:
            ok = np.asarray(bank_group) != row_group[m]
        j = np.flatnonzero(ok)
        order = np.lexsort((j, -sims[m][j].astype(np.float64)))[:k]
        index[m, :order.size] = j[order]
        score[m, :order.size] = sims[m][j[order]]
    return index, score


def vote64(index, score, labels, cw, T, C):
    """(N, C) float64 probabilities of GIVEN neighbours (index (N, k), -1 past the last; score float32)."""
    index, score = np.asarray(index), np.asarray(score).astype(np.float64)
    labels = np.asarray(labels)
    cw = np.ones(C) if cw is None else np.asarray(cw, np.float64)
    out = np.zeros((index.shape[0], C))
    for m in range(index.shape[0]):
        n = int((index[m] >= 0).sum())
        if n == 0:
            continue
        lab = labels[index[m, :n]]
        w = np.exp((score[m, :n] - score[m, 0]) / float(T)) * cw[lab]
        np.add.at(out[m], lab, w)
        out[m] /= w.sum()
    return out
