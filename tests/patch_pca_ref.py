"""Float64 references and fixtures for the patch-feature PCA (csrc/patch_pca.hip).  Not collected.

  start_pattern / subspace_fit   the device's fit restated in float64: the same start pattern, the same rounds (Z = C Q, modified
                                 Gram-Schmidt twice), a Rayleigh-Ritz step, the same sign rule
  eigh_topk                      the oracle: the top k of numpy.linalg.eigh with the same sign rule
  planted_rows                   synthetic rows with planted structure: r orthonormal directions whose SAMPLE variances are the
                                 prescribed ones (the latent scores are centred and orthogonalised), isotropic noise, and a
                                 mean of 10 x the largest standard deviation - a fit that forgets to centre fails loudly
"""
import numpy as np

CHUNK, MEAN_CHUNK = 1024, 64            # PCA_CHUNK / PCA_MEAN_CHUNK of csrc/kernels.h
NOISE_VAR = 0.01
RATIO = 3.0                             # between consecutive planted variances; the fixtures' condition is a ratio >= 2 AFTER noise
SMALLEST_VAR = 4.0                      # of the planted ones: with M - 1 = 3 rows' worth of noise in D = 384 columns every sample
                                        # eigenvalue gains about NOISE_VAR D / (M - 1) = 1.3, which a ratio of 3 above 4 survives
U = 2.0 ** -24


def start_pattern(D, k):
    """(k, D) float64: pca_start of csrc/patch_pca.hip - a 32-bit hash of (d, j) mapped to [-1, 1)."""
    d = np.arange(D, dtype=np.uint64)[None, :]
    j = np.arange(k, dtype=np.uint64)[:, None]
    m = np.uint64(0xFFFFFFFF)
    u = (((d + np.uint64(1)) * np.uint64(2654435761)) & m) ^ (((j + np.uint64(1)) * np.uint64(2246822519)) & m)
    u ^= u >> np.uint64(15)
    u = (u * np.uint64(2246822519)) & m
    u ^= u >> np.uint64(13)
    return (u >> np.uint64(8)).astype(np.float64) * 2.0 ** -23 - 1.0


def sign_rule(components):
    """Each row's entry of largest magnitude positive; ties to the lowest index (argmax returns the first)."""
    c = np.array(components, dtype=np.float64, copy=True)
    for row in c:
        if row[np.argmax(np.abs(row))] < 0:
            row *= -1.0
    return c


def mgs(Z):
    """Modified Gram-Schmidt over the rows of Z (k, D)."""
    Q = np.array(Z, dtype=np.float64, copy=True)
    for j in range(Q.shape[0]):
        for i in range(j):
            Q[j] -= (Q[i] @ Q[j]) * Q[i]
        nrm = np.sqrt(Q[j] @ Q[j])
        Q[j] = Q[j] / nrm if nrm > 0 else 0.0
    return Q


def covariance64(X):
    """(mean, C) in float64 of rows X (M, D) given in any dtype."""
    X = np.asarray(X, dtype=np.float64)
    mu = X.mean(axis=0)
    Xc = X - mu
    return mu, Xc.T @ Xc / (X.shape[0] - 1)


def subspace_fit(C, k, iters):
    """(eigenvalues (k,), components (k, D)) of the symmetric C by the device's algorithm in float64."""
    C = np.asarray(C, dtype=np.float64)
    Q = mgs(mgs(start_pattern(C.shape[0], k)))
    for _ in range(iters):
        Q = mgs(mgs(Q @ C))              # rows of Q: (C q)^T = q^T C
    B = Q @ C @ Q.T
    w, V = np.linalg.eigh((B + B.T) / 2)
    order = np.argsort(-w, kind="stable")
    return w[order], sign_rule((Q.T @ V[:, order]).T)


def eigh_topk(C, k):
    """(eigenvalues (k,), components (k, D), all eigenvalues descending) from numpy.linalg.eigh of C in float64."""
    w, V = np.linalg.eigh(np.asarray(C, dtype=np.float64))
    w, V = w[::-1], V[:, ::-1]
    return w[:k], sign_rule(V[:, :k].T), w


def sines(comp, ref):
    """sin of the angle between corresponding unit rows: || q - (q . v) v ||."""
    comp, ref = np.asarray(comp, np.float64), np.asarray(ref, np.float64)
    return np.array([np.linalg.norm(q - (q @ v) * v) for q, v in zip(comp, ref)])


def planted_rows(M, D, k, seed, ld=None):
    """float32 rows (M, ld or D); columns D .. ld - 1 hold a sentinel no kernel may read into a result.  r = min(k + 1, M - 1, D)
    planted directions of sample variances SMALLEST_VAR x (RATIO^(r-1), ..., RATIO, 1), noise of variance NOISE_VAR per element, and a mean of
    norm 10 x the largest standard deviation."""
    rng = np.random.default_rng(seed)
    r = max(1, min(k + 1, M - 1, D))
    var = SMALLEST_VAR * RATIO ** np.arange(r - 1, -1, -1, dtype=np.float64)
    dirs = np.linalg.qr(rng.standard_normal((D, r)))[0]                      # (D, r) orthonormal
    lat = rng.standard_normal((M, r))
    lat -= lat.mean(axis=0)
    lat = np.linalg.qr(lat)[0]                                               # centred, orthonormal columns (M - 1 >= r)
    lat -= lat.mean(axis=0)                                                  # QR keeps the centring up to rounding; make it exact again
    signal = (lat * np.sqrt(var * (M - 1))) @ dirs.T
    mean = rng.standard_normal(D)
    mean *= 10.0 * np.sqrt(var[0]) / np.linalg.norm(mean)
    X = signal + np.sqrt(NOISE_VAR) * rng.standard_normal((M, D)) + mean
    out = np.full((M, ld or D), 1.0e30, np.float32)
    out[:, :D] = X.astype(np.float32)
    return out


# the eigenpair fixtures of tests/test_gpu_patch_pca.py and tests/test_patch_pca_host.py: (D, k, M)
EIGEN_CASES = [(D, k, M) for D in (96, 384) for k in (1, 3, 8) for M in (k + 1, 65, 1000)]


def eigen_fixture(D, k, M):
    return planted_rows(M, D, k, seed=1000 * D + 10 * k + (M % 7))


def cov_bound(X, chunk=CHUNK, mean_chunk=MEAN_CHUNK):
    """The a-priori bound on |C_device - C_float64| per element, for fp32 rows X (M, D).

    The device sums M products per element as ceil(M / chunk) fmaf chains of at most `chunk` terms (the fp32 MFMA is an fmaf
    chain), adds the chains in order and divides once; each factor is fl(x - mu_hat), one rounding each.  With
    x~ = x - mu (float64 mean), d_i = |mu_hat_i - mu_i| <= gamma_mean mean_m |x_mi| (two-stage sum: mean_chunk terms, then
    ceil(M / mean_chunk) partials, one division) and a_mi = |x~_mi| + d_i:
        |C_ij - C64_ij| <= gamma sum_m a_mi a_mj / (M - 1)  +  M d_i d_j / (M - 1)
        gamma      = (ceil(M / chunk) + min(M, chunk) + 4) 2^-24        chains + chain depth + 2 subtractions + division + slack
        gamma_mean = (ceil(M / mean_chunk) + min(M, mean_chunk) + 1) 2^-24
    The second term is the rounded mean's: sum_m (x~_mi - d_i)(x~_mj - d_j) = sum_m x~_mi x~_mj + M d_i d_j because the x~ sum to 0."""
    X = np.asarray(X, dtype=np.float64)
    M = X.shape[0]
    gamma = (-(-M // chunk) + min(M, chunk) + 4) * U
    gamma_mean = (-(-M // mean_chunk) + min(M, mean_chunk) + 1) * U
    d = gamma_mean * np.abs(X).mean(axis=0)
    A = np.abs(X - X.mean(axis=0)) + d
    return (gamma * (A.T @ A) + M * np.outer(d, d)) / (M - 1), d
