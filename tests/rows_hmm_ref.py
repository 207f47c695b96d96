"""cbasx_rows_emissions / cbasx_rows_weighted_sums (include/cbas_mi355x_ext.h, csrc/rows_hmm.hip) and one EM round of
cbas_amd/motif_hmm.py restated in float64 numpy, and the error bounds of the device.

THE BOUNDS, derived from the sum orders before the first run.  e = 2^-24 (fp32 unit roundoff), g(n) = n e / (1 - n e) (a chain of n
fp32 additions), r = g(D / 4 + 2) / 2 + e the relative error of rn (rows_kmeans_ref.py), 0 without normalize.
  cos       the device forms fl(rn * dot), dot two fmaf chains of D / 2 exact products and one addition (rows_kmeans_ref.py: dot):
            with A = sum_d |u_d mu_d| (u the exact working row)   |cos - u . mu| <= A (g(D / 2 + 1) + r) + e A
            - rows_kmeans_ref.score_bound with h = 0.
  z         fmaf(kappa, cos, logw) rounds once:   zb = kappa * cos_bound + e |z|
  softmax   a shift common to all z cancels, so the device's probs are p_j (1 + a_j) / sum_i p_i (1 + a_i) with
            |a_j| <= alpha_j = expm1(zb_j + e |z_j - max z|) + ULP_EXP * 2 e: the error of z, the rounding of z_j - max, expf.  The
            sum of at most 4 + 4 terms and the division add g(7) + e:
            |probs_j - p_j| <= p_j (alpha_j + abar + g(7) + e) / (1 - abar - g(7)) + 2^-120,  abar = sum_i p_i alpha_i
            (2^-120: where expf leaves the normal range).
  lognorm   log sum exp is 1-Lipschitz in the largest error of z; evaluated on the device's z the sum S in [1, C] has the relative
            error rho = ULP_EXP * 2 e + g(7) + 0.37 C e (the last: sum_j p_j e |z_j - max| <= C e max_t t exp(-t)); logf adds
            ULP_LOG * 2 e |log S|, the addition e |m + log S|, the constant and the product 2 e |lognorm|:
            |lognorm - L| <= log2(e) (max_j zb_j + rho + ULP_LOG * 2 e log C + e |L / log2(e)|) + 2 e |L|
  sums      u = fl(x rn) has relative error r + e.  A lane's chain takes a quarter of the part's rows (block b to lane b % 4), the
            products are exact inside the fused multiply-add, three more additions join the lanes and the float64 addition of at most
            256 parts adds 256 * 2^-53:
            |sums - S| <= (r + e + g(rpp / 4 + 3) + e) sum_t |w_tc| |u_td|;     mass likewise with |u| = 1 and r = 0
ULP_EXP = ULP_LOG = 2: the HIP math API documents expf and logf to 1 ulp; one more is allowed for.
"""
import numpy as np

import rows_kmeans_ref as R
from cbas_amd import bouts

E = R.E
g = R.g
MAX_PARTS, PART_ROWS = 256, 64             # CBASX_ROWS_HMM_MAX_PARTS, CBASX_ROWS_HMM_PART_ROWS
MAX_C, MAX_D = 64, 1536
ULP_EXP = ULP_LOG = 2
LOG2E = 1.0 / np.log(2.0)
MASS_MIN = 1e-6


def parts(n_rows):
    """(rows per part, parts): a function of n_rows alone."""
    per = -(-n_rows // MAX_PARTS)
    rpp = max(PART_ROWS, -(-per // PART_ROWS) * PART_ROWS)
    return rpp, -(-n_rows // rpp)


def workspace_bytes(n_rows, dim, C):
    n = max(parts(n_rows)[1], 1)
    return n * C * dim * 4 + n * 256


def logits(x, means, kappa, logw, normalize):
    u = R.working_rows(x, normalize)
    z = kappa * (u @ np.asarray(means, np.float64).T)
    return z + (0.0 if logw is None else np.asarray(logw, np.float64)[None, :])


def emissions(x, means, kappa, logw=None, normalize=1):
    """(probs (N, C), lognorm (N,) in bits) in float64."""
    z = logits(x, means, kappa, logw, normalize)
    m = z.max(axis=1, keepdims=True)
    ex = np.exp(z - m)
    s = ex.sum(axis=1, keepdims=True)
    return ex / s, ((m + np.log(s)) * LOG2E)[:, 0]


def rn_error(D, normalize):
    return (g(D / 4 + 2) / 2 + E) if normalize else 0.0


def z_bound(x, means, kappa, logw, normalize):
    D = np.asarray(x).shape[1]
    A = np.abs(R.working_rows(x, normalize)) @ np.abs(np.asarray(means, np.float64)).T
    cos_bound = A * (g(D / 2 + 1) + rn_error(D, normalize)) + E * A
    return kappa * cos_bound + E * np.abs(logits(x, means, kappa, logw, normalize))


def emissions_bound(x, means, kappa, logw=None, normalize=1):
    """((N, C) bound on |device probs - float64 probs|, (N,) bound on |device lognorm - float64 lognorm|)."""
    C = np.asarray(means).shape[0]
    z = logits(x, means, kappa, logw, normalize)
    zb = z_bound(x, means, kappa, logw, normalize)
    p, L = emissions(x, means, kappa, logw, normalize)
    alpha = np.expm1(zb + E * np.abs(z - z.max(axis=1, keepdims=True))) + ULP_EXP * 2 * E
    abar = (p * alpha).sum(axis=1, keepdims=True)
    pb = p * (alpha + abar + g(7) + E) / (1.0 - abar - g(7)) + 2.0 ** -120
    rho = ULP_EXP * 2 * E + g(7) + 0.37 * C * E
    lb = LOG2E * (zb.max(axis=1) + rho + ULP_LOG * 2 * E * np.log(C) + E * np.abs(L / LOG2E)) + 2 * E * np.abs(L)
    return pb, lb


def weighted_sums(x, w, normalize=1):
    """(sums (C, D), mass (C,)) in float64."""
    w = np.asarray(w, np.float64)
    return w.T @ R.working_rows(x, normalize), w.sum(axis=0)


def sums_bound(x, w, normalize=1, n_rows=None):
    x = np.asarray(x)
    N, D = x.shape
    rpp, nparts = parts(N if n_rows is None else n_rows)
    aw = np.abs(np.asarray(w, np.float64))
    chain = g(rpp / 4 + 3) + MAX_PARTS * 2.0 ** -53
    sb = (rn_error(D, normalize) + E + chain + E) * (aw.T @ np.abs(R.working_rows(x, normalize)))
    return sb, (chain + E) * aw.sum(axis=0)


def owned(table, N):
    mask = np.zeros(N, bool)
    for first, n in np.asarray(table, np.int64).reshape(-1, 2):
        mask[first:first + n] = True
    return mask


def update(means, S, mass, Xi, Pi, prior, smoothing, fit_prior):
    """The M step: mu = S / |S| (a state of mass below 1e-6 keeps its mean), A = rows of (Xi + smoothing) normalised, the prior
    likewise when it is fitted."""
    norm = np.sqrt((S * S).sum(axis=1, keepdims=True))
    keep = (mass < MASS_MIN)[:, None] | ~(norm > 0)
    new = np.where(keep, np.asarray(means, np.float64), S / np.where(norm > 0, norm, 1.0))
    A = Xi + smoothing
    A = A / A.sum(axis=1, keepdims=True)
    pri = (Pi + smoothing) / (Pi + smoothing).sum() if fit_prior else prior
    return new, A, pri


def em_round(x, table, means, A, prior, kappa, normalize=1, smoothing=1.0, fit_prior=False):
    """One round in float64: (gamma, new means, new A, new prior, the likelihood in bits under the parameters given)."""
    N = np.asarray(x).shape[0]
    probs, lognorm = emissions(x, means, kappa, None, normalize)
    gamma, Xi, Pi, loglik, _ = bouts.posteriors_host(probs, table, A, prior)
    S, mass = weighted_sums(x, gamma, normalize)
    new, A2, pri2 = update(means, S, mass, Xi, Pi, prior, smoothing, fit_prior)
    return gamma, new, A2, pri2, loglik.sum() + lognorm[owned(table, N)].sum()


def fit(x, table, means, A, kappa, iters, normalize=1, smoothing=1.0, fit_prior=False):
    """`iters` rounds and the closing E step, then the states by descending occupancy: the dict motif_hmm.fit is compared with."""
    x = np.asarray(x)
    C = np.asarray(means).shape[0]
    means, A = np.asarray(means, np.float64), np.asarray(A, np.float64)
    prior = np.full(C, 1.0 / C)
    history = []
    for _ in range(iters):
        _, means, A, prior, ll = em_round(x, table, means, A, prior, kappa, normalize, smoothing, fit_prior)
        history.append(ll)
    probs, _ = emissions(x, means, kappa, None, normalize)
    gamma = bouts.posteriors_host(probs, table, A, prior)[0]
    occupancy = gamma.sum(axis=0)
    order = np.argsort(-occupancy, kind="stable")
    return {"gamma": gamma[:, order], "means": means[order], "transitions": A[np.ix_(order, order)], "prior": prior[order],
            "occupancy": occupancy[order], "loglik": np.array(history), "order": order}


def planted(seed, lengths, D, C, noise=0.08, mean_bout=60):
    """fp16 rows of `lengths` clips back to back, each frame a noisy copy of its state's direction times a random length, the states
    in bouts of a geometric length; (rows, table, states, directions)."""
    rng = np.random.default_rng(seed)
    dirs = rng.standard_normal((C, D))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rows, states, table, at = [], [], [], 0
    for n in lengths:
        s = np.empty(n, np.int64)
        t, cur = 0, int(rng.integers(C))
        while t < n:
            run = int(rng.geometric(1.0 / mean_bout))
            s[t:t + run] = cur
            t += run
            cur = (cur + int(rng.integers(1, C))) % C if C > 1 else 0
        v = dirs[s] + noise * rng.standard_normal((n, D))
        rows.append((v * rng.uniform(0.5, 3.0, size=(n, 1))).astype(np.float16))
        states.append(s)
        table.append((at, n))
        at += n
    return np.concatenate(rows), np.array(table, np.int64), np.concatenate(states), dirs
