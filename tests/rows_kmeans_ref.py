"""cbas_rows_kmeans_* (include/cbas_mi355x.h, csrc/rows_kmeans.hip) restated in float64 numpy, and the error bounds of the device.

The restatement computes what the header defines with every sum in float64: the tie rules (the lowest centroid, the lowest row),
farthest-point seeding, Lloyd rounds from given centroids (an empty cluster keeps its centroid), the ordering of the clusters.

THE BOUNDS, derived before the first run.  e = 2^-24 (fp32 unit roundoff), g(n) = n e / (1 - n e) (a chain of n fp32 additions).
  dot       x . c on the device: two fmaf chains of D / 64 blocks x 32 exact products = D / 2 terms each, then one addition:
            |dot - x . c| <= g(D / 2 + 1) sum_d |x_d c_d|.
  rn        s is four fmaf chains of D / 4 squares and two additions: relative error g(D / 4 + 2); 1 / sqrt halves it; the division and
            square root run in double (2^-52, neglected against e) and one rounding to fp32 follows: r = g(D / 4 + 2) / 2 + e.
  h         |c|^2 is one fmaf chain of D squares: relative error g(D); halving is exact.
  score     fmaf(rn, dot, -h) rounds once: with A = sum_d |u_d c_d| (u the exact working row)
            |score - score64| <= A (g(D / 2 + 1) + r) + g(D) h + e (A + h)            (r = 0 without normalize)
  dist2     max(0, fmaf(-2, score, |u|^2)); |u|^2 is s (relative error g(D / 4 + 2)) without normalize and exactly 1 with it:
            |dist2 - dist2_64| <= 2 score_bound + g(D / 4 + 2) |u|^2 [normalize = 0] + e (|u|^2 + 2 |score|)
  centroid  every u = fl(x rn) has relative error r + e; a cluster's n rows are added one by one inside a segment (at most SEGMENT
            additions) and the segments one by one (ceil(N / SEGMENT) more), then one division:
            |c - c64| <= ((r + e) + g(min(n, SEGMENT) + ceil(N / SEGMENT)) + e) * (sum of |u| over the cluster) / n
"""
import numpy as np

TILE = 128                 # rows per workgroup of the pass (RKM_TILE)
SEGMENT = 4096             # CBAS_ROWS_KMEANS_SEGMENT
MAX_K, MAX_D = 64, 1536
E = 2.0 ** -24


def g(n):
    return n * E / (1.0 - n * E)


def working_rows(x, normalize):
    """float64 u of fp16 (or any) rows x: x itself, or x / |x| with a zero row left zero."""
    x = np.asarray(x, np.float64)
    if not normalize:
        return x
    norm = np.sqrt((x * x).sum(axis=1, keepdims=True))
    return np.divide(x, norm, out=np.zeros_like(x), where=norm > 0)


def scores(u, cent):
    cent = np.asarray(cent, np.float64)
    return u @ cent.T - 0.5 * (cent * cent).sum(axis=1)[None, :]


def assign(x, cent, normalize):
    """labels (the lowest j of the largest score), dist2, and the gap between the two best scores of every row."""
    u = working_rows(x, normalize)
    sc = scores(u, cent)
    labels = sc.argmax(axis=1)                                   # numpy: the first of equal maxima
    best = sc[np.arange(len(sc)), labels]
    dist2 = np.maximum(0.0, (u * u).sum(axis=1) - 2.0 * best)
    part = np.partition(sc, -2, axis=1)
    return labels.astype(np.int64), dist2, part[:, -1] - part[:, -2]


def score_bound(x, cent, normalize):
    """(N, k): the bound on |device score - float64 score| of every pair."""
    D = np.asarray(x).shape[1]
    u = np.abs(working_rows(x, normalize))
    c = np.abs(np.asarray(cent, np.float64))
    A = u @ c.T
    h = 0.5 * (c * c).sum(axis=1)[None, :]
    r = (g(D / 4 + 2) / 2 + E) if normalize else 0.0
    return A * (g(D / 2 + 1) + r) + g(D) * h + E * (A + h)


def dist2_bound(x, cent, normalize, labels):
    D = np.asarray(x).shape[1]
    u = working_rows(x, normalize)
    idx = np.arange(len(u))
    sb = score_bound(x, cent, normalize)[idx, labels]
    un2 = (u * u).sum(axis=1)
    sc = np.abs(scores(u, cent)[idx, labels])
    return 2.0 * sb + (0.0 if normalize else g(D / 4 + 2)) * un2 + E * (un2 + 2.0 * sc)


def centroid_bound(x, labels, k, normalize, n_rows=None):
    """(k, D): the bound on |device centroid - float64 mean| given the SAME labels."""
    x = np.asarray(x)
    N, D = x.shape
    n_rows = N if n_rows is None else n_rows
    u = np.abs(working_rows(x, normalize))
    r = (g(D / 4 + 2) / 2 + E) if normalize else 0.0
    out = np.zeros((k, D))
    nseg = -(-n_rows // SEGMENT)
    for j in range(k):
        n = int((labels == j).sum())
        if n:
            out[j] = ((r + E) + g(min(n, SEGMENT) + nseg) + E) * u[labels == j].sum(axis=0) / n
    return out


def update(x, labels, cent, normalize):
    """The means of the working rows; a cluster without rows keeps its centroid."""
    u = working_rows(x, normalize)
    new = np.array(cent, np.float64, copy=True)
    for j in range(new.shape[0]):
        mine = labels == j
        if mine.any():
            new[j] = u[mine].sum(axis=0) / mine.sum()
    return new


def seed(x, k, normalize):
    """The rows farthest-point seeding picks: the farthest from the column mean, then the largest minimum distance; ties to the
    lowest row."""
    u = working_rows(x, normalize)
    d = ((u - u.mean(axis=0)) ** 2).sum(axis=1)
    picks = [int(d.argmax())]
    mind = None
    for _ in range(1, k):
        d = ((u - u[picks[-1]]) ** 2).sum(axis=1)
        mind = d if mind is None else np.minimum(mind, d)
        picks.append(int(mind.argmax()))
    return picks


def order(counts):
    """Output cluster r is seeding position order[r]: descending count, ties by seeding order."""
    return np.argsort(-np.asarray(counts, np.int64), kind="stable")


def lloyd(x, cent0, iters, normalize):
    """`iters` rounds from cent0.  Returns the dict the device's outputs are compared with: centroids and counts in the OUTPUT
    numbering, labels in it, inertia (iters + 1), `cur` = the final centroids in seeding order, `order`."""
    cur = np.array(cent0, np.float64, copy=True)
    inertia = []
    for _ in range(iters):
        labels, d2, _ = assign(x, cur, normalize)
        inertia.append(d2.sum())
        cur = update(x, labels, cur, normalize)
    labels, d2, gap = assign(x, cur, normalize)
    inertia.append(d2.sum())
    k = cur.shape[0]
    counts = np.bincount(labels, minlength=k)
    o = order(counts)
    pos = np.empty(k, np.int64)
    pos[o] = np.arange(k)
    return {"centroids": cur[o], "counts": counts[o], "labels": pos[labels], "dist2": d2, "gap": gap, "inertia": np.array(inertia),
            "cur": cur, "order": o}


def fit(x, k, iters, normalize):
    picks = seed(x, k, normalize)
    out = lloyd(x, working_rows(x, normalize)[picks], iters, normalize)
    out["init_index"] = np.array(picks, np.int64)
    return out


def brute_assign(x, cent, normalize):
    """Plain squared distances, one pair at a time: what `assign` is checked against on tiny problems."""
    u = working_rows(x, normalize)
    cent = np.asarray(cent, np.float64)
    labels, dist2 = [], []
    for row in u:
        d = [float(((row - c) ** 2).sum()) for c in cent]
        labels.append(int(np.argmin(d)))
        dist2.append(min(d))
    return np.array(labels), np.array(dist2)
