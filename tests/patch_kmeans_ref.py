"""Float64 restatement of cbas_patch_kmeans_fit / _assign, written from the comment in include/cbas_mi355x.h (not from the kernels):
the working row, farthest-point seeding, Lloyd rounds with empty clusters kept, the final reorder, the inertia - plus the error
bounds the GPU tests hold the device to and the fixtures they share.  numpy only."""
import numpy as np

CHUNK = 64                      # CBAS_KMEANS_CHUNK
MAX_K = 16                      # CBAS_KMEANS_MAX_K
U1 = 1.01 * 2.0 ** -24          # the fp32 unit roundoff with room for the second-order terms of gamma_n = n u / (1 - n u), n <= 500


def working_rows(X, normalize):
    """u = x, or x / |x| with a zero row left zero, in float64."""
    X = np.asarray(X, dtype=np.float64)
    if not normalize:
        return X
    nrm = np.sqrt((X * X).sum(axis=1, keepdims=True))
    return np.divide(X, nrm, out=np.zeros_like(X), where=nrm > 0)


def sqdist(U, t):
    d = U - t
    return (d * d).sum(axis=1)


def seed_objectives(U, chosen):
    """The objective every row had at each seeding step GIVEN the rows chosen before it: step 0 the squared distance to the column
    mean, step j the least squared distance to seeds 0 .. j - 1.  (k, M)."""
    out = [sqdist(U, U.mean(axis=0))]
    mind = None
    for i in chosen[:-1]:
        d = sqdist(U, U[i])
        mind = d if mind is None else np.minimum(mind, d)
        out.append(mind.copy())
    return np.stack(out)


def seed(U, k):
    """Farthest-point seeding: the chosen rows (np.argmax: ties to the lowest row) and the least margin (largest objective minus the
    second largest, over the steps)."""
    chosen, margin = [], np.inf
    for j in range(k):
        obj = seed_objectives(U, chosen + [0])[j]
        i = int(np.argmax(obj))
        if len(obj) > 1:
            margin = min(margin, obj[i] - np.delete(obj, i).max())
        chosen.append(i)
    return chosen, margin


def assign(U, C):
    """labels (least squared distance, ties to the lowest centroid), the squared distances (M, k)."""
    d2 = np.stack([sqdist(U, c) for c in C], axis=1)
    return np.argmin(d2, axis=1).astype(np.int32), d2


def lloyd(U, chosen, iters):
    """`iters` rounds from the seeds U[chosen].  Returns a dict: centroids and counts in the output order (descending count, ties by
    seeding order), order (output position -> seeding position), labels in output names, inertia (iters + 1), seeding_centroids, and
    margin: the least gap between a row's nearest and second nearest centroid over every assignment made."""
    C = U[list(chosen)].copy()
    k = len(C)
    inertia, margin = [], np.inf
    for t in range(iters + 1):
        lab, d2 = assign(U, C)
        srt = np.sort(d2, axis=1)
        margin = min(margin, float((srt[:, 1] - srt[:, 0]).min()))
        inertia.append(float(d2[np.arange(len(U)), lab].sum()))
        if t == iters:
            break
        for j in range(k):
            if (lab == j).any():
                C[j] = U[lab == j].mean(axis=0)            # a cluster without rows keeps its centroid
    counts = np.bincount(lab, minlength=k)
    order = np.array(sorted(range(k), key=lambda j: (-counts[j], j)), dtype=np.int32)
    inv = np.empty(k, np.int32)
    inv[order] = np.arange(k, dtype=np.int32)
    return dict(centroids=C[order], counts=counts[order].astype(np.int32), order=order, labels=inv[lab], inertia=np.array(inertia),
                seeding_centroids=C, margin=margin)


def fit(X, k, iters, normalize):
    U = working_rows(X, normalize)
    chosen, seed_margin = seed(U, k)
    out = lloyd(U, chosen, iters)
    out.update(init_index=np.array(chosen, np.int32), seed_margin=seed_margin)
    return out


def rounds_until_stable(X, k, normalize, limit=64):
    """The smallest t such that the labels after t updates equal those after t + 1 (Lloyd is then at its fixed point)."""
    U = working_rows(X, normalize)
    chosen, _ = seed(U, k)
    C = U[chosen].copy()
    prev = None
    for t in range(limit + 1):
        lab, _ = assign(U, C)
        if prev is not None and np.array_equal(lab, prev):
            return t - 1
        prev = lab
        for j in range(k):
            if (lab == j).any():
                C[j] = U[lab == j].mean(axis=0)
    raise AssertionError(f"labels still change after {limit} rounds")


# ---- the bounds (u1 = U1; derivations: DESIGN.md section 18) ---------------------------------------------------------------------
def dist2_bound(U, C, D):
    """(M, k): how far the device's dist2 of row m to centroid j may lie from the float64 squared distance.  score = fmaf(rn, x . c,
    -h): x . c is four fmaf chains of at most D / 4 terms and three additions, (D / 4 + 3) u1 a with a = sum |u_d| |c_d| after
    the factor rn, whose own rounding and the fmaf's add 2 u1 a; h = |c|^2 / 2 is a chain of D / 64 and a 6-level tree with one
    halving (exact) and the fmaf's rounding, (D / 64 + 7) u1 |c|^2 / 2.  dist2 = fmaf(-2, score, |u|^2) doubles that, rounds |u|^2
    (u1 |u|^2) and rounds once more (u1 (|u|^2 + 2 a + |c|^2)): (D / 2 + 12) a + (D / 64 + 8) |c|^2 + 2 |u|^2, all times u1; one more
    |c|^2 is room for max(0, .) on a row that coincides with its centroid."""
    a = np.abs(U) @ np.abs(C).T
    c2 = (C * C).sum(axis=1)[None, :]
    u2 = (U * U).sum(axis=1)[:, None]
    return U1 * ((D / 2 + 12) * a + (D / 64 + 9) * c2 + 2 * u2)


def mean_bound(U, members, nch):
    """(D,): a device centroid against the float64 mean of its rows: per chunk one fmaf chain of at most 64 terms, nch chunks added
    in order, one division, and each term's factor rn rounded once: (64 + nch + 3) u1 mean |u_d|."""
    return (CHUNK + nch + 3) * U1 * np.abs(U[members]).mean(axis=0)


def seed_bound(U, obj, targets, D, step0_chunks=None):
    """A scalar: how far the device's seeding objective may lie from the float64 one at a step, the largest over the rows.  One
    distance is 64 fmaf chains of D / 64 terms and a 6-level tree over squares of differences rounded once: (D / 64 + 8) u1 d; the
    row and the target each carry a relative 2 u1 (rn, the product), which moves d by at most 4 u1 sqrt(d) (|u| + |t|).  At step 0
    the target is the device's mean, off the float64 mean by delta with |delta_d| <= (64 + chunks + 2) u1 mean |u_d|: d moves by at
    most 2 sqrt(d) |delta| + |delta|^2."""
    un = np.sqrt((U * U).sum(axis=1))
    tn = max(float(np.sqrt((t * t).sum())) for t in targets)
    b = (D / 64 + 8) * U1 * obj + 4 * U1 * np.sqrt(obj) * (un + tn)
    if step0_chunks is not None:
        delta = (CHUNK + step0_chunks + 2) * U1 * np.linalg.norm(np.abs(U).mean(axis=0))
        b = b + 2 * np.sqrt(obj) * delta + delta * delta
    return float(b.max())


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
def planted(seed_, k, M, D, spread=0.05):
    """k well separated blobs of unequal sizes (size_j strictly decreasing, so the output order is decided by the counts) in a
    shuffled order: float32 (M, D) rows and the planted labels.  Centres are +-1 patterns scaled 3, the noise `spread`."""
    rng = np.random.default_rng(seed_)
    w = np.arange(k, 0, -1, dtype=np.float64) + 1.0
    sizes = np.floor(w / w.sum() * M).astype(int)
    sizes[0] += M - sizes.sum()
    assert (np.diff(sizes) < 0).all() and sizes[-1] >= 1, sizes
    centres = 3.0 * rng.choice([-1.0, 1.0], size=(k, D))
    lab = np.repeat(np.arange(k), sizes)
    rng.shuffle(lab)
    X = centres[lab] + spread * rng.standard_normal((M, D))
    return X.astype(np.float32), lab.astype(np.int32)


def tiny_patch_rows(seed_, M, D, parts=3):
    """Rows shaped like a small encoder's patch features, for choosing the default number of rounds: `parts` overlapping groups on
    a smooth background drift - clusters that touch, so Lloyd needs several rounds."""
    rng = np.random.default_rng(seed_)
    centres = rng.standard_normal((parts, D))
    lab = rng.integers(0, parts, M)
    drift = np.linspace(-1, 1, M)[:, None] * rng.standard_normal((1, D))
    return (centres[lab] + 0.5 * drift + 0.6 * rng.standard_normal((M, D))).astype(np.float32)
