"""Float64 restatement, fixtures and a-priori bounds for the PCA over resident CLS rows (csrc/rows_pca.hip).
Not collected.  Every bound below was written down before the first device run, and none was widened after it; the working row's
restatement was corrected after it (see there).  e = E = 2^-24, g(n) = n e / (1 - n e).

  the working row   as the header defines it.  normalize = 0: u = x.  normalize = 1: u = fl(x * rn), the fp32 product, with the fp32
                    rn restated bit for bit (`reciprocal_norms`: squares of fp16 values are exact in fp32, so an fmaf chain of them
                    is a chain of fp32 additions; numpy's float32 product is the correctly rounded one).  The PCA is that of these
                    rows: what is bounded below is the arithmetic after them.  (Against x * rn left UNROUNDED the covariance form
                    below does not hold: that rounding is relative to |u|, not to |u - mu|, and where two rows nearly agree in a
                    column it exceeds gamma a_mi by any factor - 38 x at N = 2 on the device.)
  mean              the bound of section 16 with the chunk depth of 1024: the device adds min(M, 1024) terms per chunk, the
                    ceil(M / 1024) chunk sums, and divides once:
                        d_i = (ceil(M / 1024) + min(M, 1024) + 1) e mean_m |u_mi|
  covariance        cov_bound of section 16: per element the M products run as fmaf chains of at most 1024 terms (the fp32 MFMA is an
                    fmaf chain), at most chunks_per_part chain results are added within a part, the parts are added, one division;
                    each factor is fl(u - mu^), the subtraction's rounding (the fifth unit is the issue's, kept as slack):
                        |C^_ij - C_ij| <= gamma sum_m a_mi a_mj / (M - 1) + M d_i d_j / (M - 1),   a_mi = |u_mi - mu_i| + d_i
                        gamma = (min(M, 1024) + chunks_per_part + parts + 5) e
                    (the second term is the rounded mean's: the centred rows sum to zero, so a shift d of the mean adds exactly
                    M d_i d_j to the sum of products).  The trace: the bound's diagonal summed, plus (D / 256 + 9) e trace C for the
                    solver's own sum of the diagonal (section 16).
  scores            against c . q in float64 with the device's own mean and components, c = u - mu^: the dot bound of sections 19 /
                    22 - two fmaf chains of at most D / 2 terms and their sum - on the factors fl(u - mu^):
                        |s^ - s| <= g(D / 2 + 2) sum_d |c_d| |q_d|
  residual          r = max(0, n2 - q2), n2 = |c|^2 (four fmaf chains of D / 4 terms, two additions), q2 = the scores' squares (one
                    chain of k terms); max(0, .) moves nothing apart:
                        |r^ - r| <= g(D / 4 + 5) n2 + g(k + 1) sum_j (|s_j| + b_j)^2 + sum_j (2 |s_j| b_j + b_j^2),   b_j the score's bound
  solver            `ritz_tolerance`: ||C q_j - lambda_j q_j||_2 <= 4 (D / 64 + D / 256 + 2 k + 48) e trace C against the device's own C,
                    once the iteration has converged - the roundings on one product's way through C q (a chain of D / 64, a 6-level
                    tree) and q . (C q) (a chain of D / 256, 6 levels, 3 additions), the Jacobi rotations and Q's departure from
                    orthonormal (2 k + 16 from the two Gram-Schmidt passes), with section 16's margin of 4; || |C| ||_2 <= trace C for
                    a positive semidefinite C.
"""
import numpy as np

import patch_pca_ref as P

CHUNK, MAX_PARTS, TILE = 1024, 64, 128       # CBAS_ROWS_PCA_CHUNK, CBAS_ROWS_PCA_MAX_PARTS; rows per workgroup of the projection
MAX_K, MAX_D = 8, 1536
E = 2.0 ** -24

sign_rule, eigh_topk = P.sign_rule, P.eigh_topk


def g(n):
    return n * E / (1.0 - n * E)


def partition(n_rows):
    """(chunks, chunks per part, parts)."""
    chunks = -(-int(n_rows) // CHUNK)
    per = -(-chunks // MAX_PARTS)
    return chunks, per, -(-chunks // per)


def part_spans(n_rows):
    """[(first row, rows)] of every part."""
    _, per, parts = partition(n_rows)
    step = per * CHUNK
    return [(p * step, min(step, n_rows - p * step)) for p in range(parts)]


def reciprocal_norms(x):
    """The device's fp32 rn of fp16 rows, bit for bit (csrc/rows_rn.h): s = (l0 + l1) + (l2 + l3), l_j the chain over the columns d with
    (d % 32) / 8 = j ascending; rn = fp32(1 / sqrt((double)s)), 0 for s = 0."""
    x = np.asarray(x, np.float16)
    N, D = x.shape
    sq = (x.astype(np.float32) * x.astype(np.float32)).reshape(N, D // 32, 4, 8)        # exact: 22-bit products
    lanes = np.zeros((N, 4), np.float32)
    for c in range(D // 32):
        for e in range(8):
            lanes = lanes + sq[:, c, :, e]
    s = (lanes[:, 0] + lanes[:, 1]) + (lanes[:, 2] + lanes[:, 3])
    assert s.dtype == np.float32
    s64 = s.astype(np.float64)
    return np.where(s64 > 0, 1.0 / np.sqrt(np.where(s64 > 0, s64, 1.0)), 0.0).astype(np.float32)


def working_rows(x, normalize):
    """float64 u of fp16 rows x: x itself, or fl(x * rn): the fp32 product with the fp32 rn, widened."""
    if not normalize:
        return np.asarray(x, np.float64)
    u = np.asarray(x, np.float16).astype(np.float32) * reciprocal_norms(x)[:, None]
    assert u.dtype == np.float32
    return u.astype(np.float64)


def mean_cov(x, normalize):
    """(mean, C) in float64 of the working rows."""
    return P.covariance64(working_rows(x, normalize))


def fit(x, k, normalize):
    """The oracle: dict of mean, cov, eigenvalues (k), components (k, D) with the sign rule, the whole spectrum descending,
    total_variance."""
    mu, C = mean_cov(x, normalize)
    lam, V, spectrum = eigh_topk(C, k)
    return {"mean": mu, "cov": C, "eigenvalues": lam, "components": V, "spectrum": spectrum, "total_variance": float(np.trace(C))}


def project(x, normalize, mean, comp, scale=None):
    """(scores (N, k), residual (N,), c (N, D), u (N, D)) in float64 against a given mean and components."""
    u = working_rows(x, normalize)
    c = u - np.asarray(mean, np.float64)
    q = np.asarray(comp, np.float64)
    s = c @ q.T
    resid = np.maximum(0.0, (c * c).sum(axis=1) - (s * s).sum(axis=1))
    return (s if scale is None else s * np.asarray(scale, np.float64)), resid, c, u


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
def mean_bound(x, normalize):
    u = working_rows(x, normalize)
    M = u.shape[0]
    return (-(-M // CHUNK) + min(M, CHUNK) + 1) * E * np.abs(u).mean(axis=0)


def cov_bound(x, normalize):
    """((D, D) bound on |C_device - C_float64|, (D,) bound on the mean)."""
    u = working_rows(x, normalize)
    M = u.shape[0]
    _, per, parts = partition(M)
    gamma = (min(M, CHUNK) + per + parts + 5) * E
    d = mean_bound(x, normalize)
    A = np.abs(u - u.mean(axis=0)) + d
    return (gamma * (A.T @ A) + M * np.outer(d, d)) / (M - 1), d


def trace_bound(x, normalize):
    bound, _ = cov_bound(x, normalize)
    D = bound.shape[0]
    return float(np.trace(bound)) + g(D / 256 + 9) * float(np.trace(mean_cov(x, normalize)[1]))


def score_bound(x, normalize, mean, comp):
    """(N, k) on the UNSCALED scores."""
    _, _, c, u = project(x, normalize, mean, comp)
    D = c.shape[1]
    q = np.abs(np.asarray(comp, np.float64))
    return g(D / 2 + 2) * (np.abs(c) @ q.T)


def residual_bound(x, normalize, mean, comp):
    s, _, c, u = project(x, normalize, mean, comp)
    D, k = c.shape[1], s.shape[1]
    b = score_bound(x, normalize, mean, comp)
    return g(D / 4 + 5) * (c * c).sum(axis=1) + g(k + 1) * ((np.abs(s) + b) ** 2).sum(axis=1) + (2 * np.abs(s) * b + b * b).sum(axis=1)


def ritz_tolerance(C, k):
    D = np.asarray(C).shape[0]
    return 4 * (D / 64 + D / 256 + 2 * k + 48) * E * float(np.trace(np.asarray(C, np.float64)))


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------
def no_subnormals(x):
    x = np.asarray(x, np.float16)
    tiny = np.float16(6.2e-5)              # no fp16 subnormals: what the MFMA does with them is not part of the contract
    x[(np.abs(x) < tiny) & (x != 0)] = tiny
    return x


PLANTED, RATIO = 8, 2.5                      # planted directions; between consecutive planted standard deviations' squares


def planted(seed, N, D, noise=0.02, offset=1.0):
    """fp16 rows (N, D): min(PLANTED, N - 1, D) orthonormal directions whose variances fall by RATIO from 4.0, isotropic noise, and
    a mean of norm `offset` x the largest standard deviation - a fit that forgets to centre fails loudly."""
    rng = np.random.default_rng(seed)
    r = max(1, min(PLANTED, N - 1, D))
    var = 4.0 * RATIO ** -np.arange(r, dtype=np.float64)
    dirs = np.linalg.qr(rng.standard_normal((D, r)))[0]
    lat = rng.standard_normal((N, r)) * np.sqrt(var)
    mean = rng.standard_normal(D)
    mean *= offset * 2.0 / np.linalg.norm(mean)
    return no_subnormals(lat @ dirs.T + noise * rng.standard_normal((N, D)) + mean)


def exact_rows(seed, N, D, spread=3, centre=6):
    """Small-integer fp16 rows (N odd) whose column mean is an integer: (N - 1) / 2 pairs (c + n, c - n) and the centre c itself,
    shuffled.  Every product and partial sum of the device's fit is an integer below 2^24: exact."""
    assert N % 2 == 1
    rng = np.random.default_rng(seed)
    c = rng.integers(-centre, centre + 1, D)
    half = rng.integers(-spread, spread + 1, ((N - 1) // 2, D))
    x = np.concatenate([c + half, c - half, c[None]])[rng.permutation(N)]
    assert np.abs(x).max() * N < 2 ** 24 and (2 * spread) ** 2 * N < 2 ** 24
    return x.astype(np.float16), c
