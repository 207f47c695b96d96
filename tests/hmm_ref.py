"""The forward-backward pass of DESIGN.md section 25 in float64, written from the definition and independent of
``cbas_amd.bouts.posteriors_host``, a brute-force enumeration of all C^T paths for tiny cases, and the inputs the host and the
device tests share."""
import itertools

import numpy as np

FLOOR = 2.0 ** -32
INPUTS = ["softmax", "one_hot", "uniform"]
TRANSITIONS = ["sticky", "positive", "forbidden"]


def emissions(probs):
    p = np.asarray(probs, np.float64)
    return np.where(np.isnan(p) | (p < FLOOR), FLOOR, p)


def posteriors_ref(probs, clip_table, A, prior=None):
    """``(gamma (N, C), Xi (C, C), Pi (C,), loglik (n_clips,))`` in float64: per clip the scaled forward pass, a backward pass
    held below its own maximum, and every xi_t formed and normalised on its own."""
    b_all = emissions(probs)
    N, C = b_all.shape
    A = np.asarray(A, np.float64)
    pri = np.full(C, 1.0 / C) if prior is None else np.asarray(prior, np.float64)
    table = np.asarray(clip_table, np.int64).reshape(-1, 2)
    gamma, Xi, Pi, loglik = np.zeros((N, C)), np.zeros((C, C)), np.zeros(C), np.zeros(len(table))
    for c, (first, T) in enumerate(table):
        if T == 0:
            continue
        b = b_all[first:first + T]
        alpha, beta = np.zeros((T, C)), np.ones((T, C))
        for t in range(T):
            a = (pri if t == 0 else alpha[t - 1] @ A) * b[t]
            loglik[c] += np.log2(a.sum())
            alpha[t] = a / a.sum()
        for t in range(T - 2, -1, -1):
            v = A @ (b[t + 1] * beta[t + 1])
            beta[t] = v / v.max()
        g = alpha * beta
        gamma[first:first + T] = g / g.sum(axis=1, keepdims=True)
        for t in range(T - 1):
            xi = alpha[t][:, None] * A * (b[t + 1] * beta[t + 1])[None, :]
            Xi += xi / xi.sum()
        Pi += gamma[first]
    return gamma, Xi, Pi, loglik


def enumerate_paths(probs, A, prior=None):
    """One clip, all C^T paths: ``(gamma, Xi, loglik)`` from the definition of a hidden Markov model and nothing else."""
    b = emissions(probs)
    T, C = b.shape
    A = np.asarray(A, np.float64)
    pri = np.full(C, 1.0 / C) if prior is None else np.asarray(prior, np.float64)
    gamma, Xi, total = np.zeros((T, C)), np.zeros((C, C)), 0.0
    for path in itertools.product(range(C), repeat=T):
        w = pri[path[0]] * b[0, path[0]]
        for t in range(1, T):
            w *= A[path[t - 1], path[t]] * b[t, path[t]]
        total += w
        for t in range(T):
            gamma[t, path[t]] += w
        for t in range(T - 1):
            Xi[path[t], path[t + 1]] += w
    return gamma / total, Xi / total, np.log2(total)


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------
def make_transitions(kind, C, rng):
    """Float32 row-stochastic ``(C, C)``: sticky with stay 0.975; random and strictly positive; or random with single forbidden
    transitions (0 -> 0, and for C >= 3 also 1 -> 2 and C-1 -> 0) that leave the chain irreducible."""
    if C == 1:
        return np.ones((1, 1), np.float32)
    if kind == "sticky":
        A = np.full((C, C), 0.025 / (C - 1))
        A[np.diag_indices(C)] = 0.975
    else:
        A = rng.random((C, C)) + 0.05
        if kind == "forbidden":
            A[0, 0] = 0.0
            if C >= 3:
                A[1, 2] = 0.0
                A[C - 1, 0] = 0.0
    A = (A / A.sum(axis=1, keepdims=True)).astype(np.float32)
    return A


def make_probs(kind, N, C, rng):
    """Float32 ``(N, C)``: softmax rows of logits with standard deviation 4; near-one-hot rows along a sticky random path whose
    other entries sit at, below and on the 2^-32 floor (2^-32, 0, 2^-33); or uniform rows."""
    if kind == "softmax":
        z = rng.normal(0.0, 4.0, size=(N, C))
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    if kind == "uniform":
        return np.full((N, C), 1.0 / C, np.float32)
    state = np.zeros(N, np.int64)
    jump = rng.random(N) < 0.1
    fresh = rng.integers(0, C, size=N)
    for t in range(1, N):
        state[t] = fresh[t] if jump[t] else state[t - 1]
    p = rng.choice(np.array([FLOOR, 0.0, FLOOR / 2]), size=(N, C))
    p[np.arange(N), state] = 0.0
    p[np.arange(N), state] = 1.0 - p.sum(axis=1)
    return p.astype(np.float32)


def identities(gamma, Xi, Pi, table):
    """The four identities of the definition as ``(worst row-sum error, |sum Xi - sum (T - 1)|, worst |Xi.sum(1) - sum_{t<T-1}
    gamma_t|, |sum Pi - non-empty clips|)``."""
    owned = np.zeros(gamma.shape[0], bool)
    occupancy = np.zeros(gamma.shape[1])
    for first, T in table:
        owned[first:first + T] = True
        if T > 1:
            occupancy += gamma[first:first + T - 1].astype(np.float64).sum(axis=0)
    rows = np.abs(gamma[owned].astype(np.float64).sum(axis=1) - 1.0).max() if owned.any() else 0.0
    steps = sum(max(int(T) - 1, 0) for _, T in table)
    return rows, abs(Xi.sum() - steps), np.abs(Xi.sum(axis=1) - occupancy).max(), abs(Pi.sum() - sum(1 for _, T in table if T > 0))
