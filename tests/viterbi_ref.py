"""The definition ``cbasx_viterbi_scores`` / ``cbasx_viterbi_decode`` implement (include/cbas_mi355x_ext.h), serial, in numpy
int64 and written for clarity, not speed.  The tests of cbas_amd/bouts.py compare against it; ``brute_force`` enumerates every
path and is what the reference itself is checked against."""
import itertools

import numpy as np

UNIT = 256
SCORE_MIN = -8192
TRANS_LIMIT = 1 << 20


def scores_exact(probs):
    """256 * log2(max(p, 2^-32)) in float64, not yet rounded; a NaN and a negative p count as 2^-32."""
    p = np.asarray(probs, np.float64)
    p = np.where(np.isnan(p) | (p < 2.0 ** -32), 2.0 ** -32, p)
    return UNIT * np.log2(p)


def scores_ref(probs):
    """``e = clamp(rint(256 * log2(max(p, 2^-32))), -8192, 0)`` as int32."""
    return np.clip(np.rint(scores_exact(probs)), SCORE_MIN, 0).astype(np.int32)


def viterbi_clip(e, A, prior=None):
    """One clip: ``e`` (T, C) scores, ``A`` (C, C) with A[i][j] the score of i -> j, ``prior`` (C,) or None.
    ``(labels (T,) int32, score)``; T = 0 gives no label and score 0."""
    e = np.asarray(e, np.int64)
    A = np.asarray(A, np.int64)
    T, C = e.shape
    if T == 0:
        return np.empty(0, np.int32), 0
    d = (np.zeros(C, np.int64) if prior is None else np.asarray(prior, np.int64)) + e[0]
    bp = np.zeros((T, C), np.int64)
    for t in range(1, T):
        cand = d[:, None] + A                                  # cand[i][j] = d_{t-1}[i] + A[i][j]
        bp[t] = cand.argmax(axis=0)                            # numpy's argmax is the FIRST maximum: the lowest i keeps a tie
        d = cand.max(axis=0) + e[t]
    end = 0
    for j in range(1, C):
        if d[j] > d[end]:                                      # the lowest j keeps a tie
            end = j
    labels = np.empty(T, np.int32)
    labels[T - 1] = end
    for t in range(T - 1, 0, -1):
        labels[t - 1] = bp[t, labels[t]]
    return labels, int(d[end])


def viterbi_ref(scores, clip_table, A, prior=None):
    """All clips of a call: ``(labels (N,) int32 with -1 outside every clip, clip_score (n_clips,) int64)``."""
    scores = np.asarray(scores)
    labels = np.full(scores.shape[0], -1, np.int32)
    table = np.asarray(clip_table, np.int64).reshape(-1, 2)
    clip_score = np.zeros(table.shape[0], np.int64)
    for c, (first, n) in enumerate(table):
        labels[first:first + n], clip_score[c] = viterbi_clip(scores[first:first + n], A, prior)
    return labels, clip_score


def path_score(path, e, A, prior=None):
    s = (0 if prior is None else int(prior[path[0]])) + int(e[0, path[0]])
    for t in range(1, len(path)):
        s += int(A[path[t - 1], path[t]]) + int(e[t, path[t]])
    return s


def brute_force(e, A, prior=None):
    """Every one of the C^T paths.  ``(labels, score)``: the best score, and among the paths that attain it the one the
    definition picks - the lowest end state, then at every frame, going backwards, the lowest predecessor from which the
    best score of the prefix is still attained."""
    e = np.asarray(e, np.int64)
    T, C = e.shape
    best_prefix = {}                                           # (t, j) -> best score of a path over frames 0 .. t that ends in j
    for t in range(T):
        for j in range(C):
            best_prefix[t, j] = max(path_score(list(p) + [j], e, A, prior) for p in itertools.product(range(C), repeat=t))
    score = max(best_prefix[T - 1, j] for j in range(C))
    labels = np.empty(T, np.int32)
    labels[T - 1] = min(j for j in range(C) if best_prefix[T - 1, j] == score)
    for t in range(T - 1, 0, -1):
        j = int(labels[t])
        labels[t - 1] = min(i for i in range(C) if best_prefix[t - 1, i] + int(A[i, j]) + int(e[t, j]) == best_prefix[t, j])
    assert path_score(labels, e, A, prior) == score
    return labels, score
