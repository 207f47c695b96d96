"""cbas_rows_probe_* (include/cbas_mi355x.h, csrc/rows_probe.hip) restated in float64 numpy, and the error bounds of the device.

The restatement computes what the header defines with every sum in float64: the normalised working rows (a zero row stays zero), the
logits, the softmax, the objective with the bias regularised like a weight, its gradient, Nesterov's constant-step iteration with its
loss history, predict, and the dealing of groups to folds.

THE BOUNDS, derived before the first run.  e = 2^-24 (fp32 unit roundoff), g(n) = n e / (1 - n e) (a chain of n fp32 additions).
  dot       x . w on the device: two fmaf chains of D / 64 blocks x 32 exact products = D / 2 terms each, then one addition: relative
            to sum_d |x_d w_d| at most gd = g(D / 2 + 1).
  rn        s is four fmaf chains of D / 4 squares and two additions: relative error g(D / 4 + 2); 1 / sqrt halves it; the division and
            square root run in double (2^-52, neglected against e) and one rounding to fp32 follows: r = g(D / 4 + 2) / 2 + e.
  logit     z = fmaf(rn, dot, b) rounds once: with A = sum_d |u_d w_d| (u the exact working row)
              dz = A ((1 + gd)(1 + r) - 1) + e (A (1 + gd)(1 + r) + |b|).           A zero row: rn = 0, z = b exactly, dz = 0.
  softmax   with mx the DEVICE's largest logit, softmax and lse are what they are for any shift, so only z_c - mx matters: the
            device forms t_c = fl(z^_c - mx) = (z_c - mx) + d_c + e |t_c| (|d_c| <= dz_c) and e^_c = expf(t_c).  HIP documents expf
            and logf to 1 ulp, and one ulp of an fp32 number is at most 2^-23 = 2 e of it:
              e^_c = exp(z_c - mx) (1 + rho_c),   rho_c <= exp(dz_c + e |t_c|) (1 + 2 e) - 1,   |t_c| <= (z_max - z_c) + dz_c + dz_max.
            S adds at most NG = ceil(C / 16) terms in a lane and four tree levels: gs = g(NG + 3); all terms are positive, so
              S^ = S (1 + rho_S),   |rho_S| <= rs = (1 + max_c rho_c)(1 + gs) - 1   (below: >= -(max_c rho_c + gs)).
  prob      p^_c = fl(e^_c / S^):  |p^_c - p_c| <= p_c ((1 + rho_c)(1 + e) / (1 - max rho - gs) - 1) + 2^-126
            (the last term: an e^_c below the normal range may come out as zero).
  loss term lse^ = fl(mx + logf(S^)): |lse^ - lse| <= dl = -log(1 - max rho - gs) + 2 e (log C + 1) + e (|z_max| + dz_max + log C + 1);
            ell^ = fl(omega fl(lse^ - z^_y)): |ell^ - ell| <= omega ((dl + dz_y)(1 + 2 e) + 2 e (lse - z_y)).
  chains    a segment's chain has at most min(M, SEGMENT) terms and the segments add ceil(M / SEGMENT) more: gl = g(min(M, SEGMENT) +
            ceil(M / SEGMENT)), relative to the sum of the terms' magnitudes.  Omega's terms are exact and positive: relative gl.
  loss      data = sum ell / Omega: |data^ - data| <= (sum d_ell + gl sum (ell + d_ell)) / Omega (1 + ro) + data ro, ro = (1 + gl / (1 -
            gl))(1 + e) - 1 (Omega's sum, one division).  |W|^2 + |b|^2: chains of D squares, C additions, a chain of C squares, one
            addition: relative g(D + C + 1).  F = fmaf(0.5 l2, reg, data) rounds once:
              dF = (that) + 0.5 l2 g(D + C + 1) reg + e (F + that).
  gradient  r^ = fl(omega fl(p^ - [c = y])): |r^ - r| <= dr = omega dp (1 + 2 e) + 2 e (|r| + omega dp).  u^ = fl(x rn^): relative
            ru = (1 + r)(1 + e) - 1.  Per element the products carry sum_m dr |u| (1 + ru) + |r| |u| ru, the fmaf chain and the
            segments gl sum_m (|r| + dr) |u| (1 + ru); the bias column has u = 1, ru = 0.  Scaling by fl(1 / Omega^) and the product
            round: rO = (1 + gl / (1 - gl))(1 + e)^2 - 1; g = fmaf(l2, v, .) rounds once:
              dg = dS / Omega (1 + rO) + |S| / Omega rO + e (|g| + the former).
  one step  w1^ = fl(v - fl32(1 / L) g^): (w0 - w1^) L = g^ (1 + theta) + L eps, |theta| <= e, |eps| <= e |w1^|:
              |(w0 - w1^) L - g| <= dg (1 + e) + e |g| + L e |w1^|.
  theorem   Nesterov's constant-step scheme on an L-smooth, mu-strongly convex F from w_0 = v_0:
              F(w_k) - F* <= (1 - sqrt(mu / L))^k (F(w_0) - F* + mu / 2 |w_0 - w*|^2) <= 2 (1 - sqrt(mu / L))^k (F(w_0) - F*).
"""
import numpy as np

TILE = 128                 # rows per workgroup of the pass (RP_TILE)
SEGMENT = 1024             # CBAS_ROWS_PROBE_SEGMENT
MAX_C, MAX_D = 64, 1536
E = 2.0 ** -24
TINY = 2.0 ** -126


def g(n):
    return n * E / (1.0 - n * E)


def working_rows(x):
    """float64 u of fp16 (or any) rows x: x / |x| with a zero row left zero."""
    x = np.asarray(x, np.float64)
    norm = np.sqrt((x * x).sum(axis=1, keepdims=True))
    return np.divide(x, norm, out=np.zeros_like(x), where=norm > 0)


def logits(x, W, b):
    return working_rows(x) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)[None, :]


def log_softmax(z):
    mx = z.max(axis=1, keepdims=True)
    lse = mx + np.log(np.exp(z - mx).sum(axis=1, keepdims=True))
    return z - lse, lse[:, 0]


def predict(x, W, b):
    """(probs, logits) in float64."""
    z = logits(x, W, b)
    return np.exp(log_softmax(z)[0]), z


def _omega(omega, M):
    return np.ones(M) if omega is None else np.asarray(omega, np.float64)


def objective(x, y, omega, W, b, l2):
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    om = _omega(omega, len(y))
    logp, _ = log_softmax(logits(x, W, b))
    data = -(om * logp[np.arange(len(y)), y]).sum() / om.sum()
    return data + 0.5 * float(l2) * ((W * W).sum() + (b * b).sum())


def gradient(x, y, omega, W, b, l2):
    """(dF / dW, dF / db)."""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    om = _omega(omega, len(y))
    u = working_rows(x)
    r = np.exp(log_softmax(u @ W.T + b[None, :])[0])
    r[np.arange(len(y)), y] -= 1.0
    r *= om[:, None]
    return r.T @ u / om.sum() + float(l2) * W, r.sum(axis=0) / om.sum() + float(l2) * b


def constants(l2):
    """(L, 1 / L, beta) of the iteration."""
    L = 1.0 + float(l2)
    sq = np.sqrt(float(l2) / L)
    return L, 1.0 / L, (1.0 - sq) / (1.0 + sq)


def fit(x, y, omega, l2, iters, W0=None, b0=None, C=None, tol=None):
    """`iters` steps from (W0, b0) (zeros when None); with `tol` it stops early once the gradient norm at w is below tol.  Returns
    (W, b, loss): loss[t] = F(v_t) for t < steps taken, then F at the weights returned."""
    D = np.asarray(x).shape[1]
    C = (np.asarray(W0).shape[0] if W0 is not None else C)
    W = np.zeros((C, D)) if W0 is None else np.array(W0, np.float64, copy=True)
    b = np.zeros(C) if b0 is None else np.array(b0, np.float64, copy=True)
    _, inv_l, beta = constants(l2)
    vW, vb = W.copy(), b.copy()
    loss = []
    for _ in range(iters):
        if tol is not None:
            gW, gb = gradient(x, y, omega, W, b, l2)
            if np.sqrt((gW * gW).sum() + (gb * gb).sum()) < tol:
                break
        loss.append(objective(x, y, omega, vW, vb, l2))
        gW, gb = gradient(x, y, omega, vW, vb, l2)
        nW, nb = vW - inv_l * gW, vb - inv_l * gb
        vW, vb = nW + beta * (nW - W), nb + beta * (nb - b)
        W, b = nW, nb
    loss.append(objective(x, y, omega, W, b, l2))
    return W, b, np.array(loss)


def optimum(x, y, omega, l2, C):
    """F* and its weights: the restatement run until its gradient norm is below 1e-10."""
    W, b, loss = fit(x, y, omega, l2, 100000, C=C, tol=1e-10)
    gW, gb = gradient(x, y, omega, W, b, l2)
    assert np.sqrt((gW * gW).sum() + (gb * gb).sum()) < 1e-10
    return loss[-1], W, b


def theorem_bound(l2, iters, f0, fstar):
    """2 (1 - sqrt q')^iters (F(w_0) - F*), q' = l2 / (L (1 + 2^-20)): the 2^-20 covers |u| being 1 only to rounding."""
    L = 1.0 + float(l2)
    q = float(l2) / (L * (1.0 + 2.0 ** -20))
    return 2.0 * (1.0 - np.sqrt(q)) ** iters * (f0 - fstar)


def deal_folds(groups, folds):
    """The i-th of the sorted unique group ids goes to fold i % folds; the fold of every entry."""
    groups = np.asarray(groups, np.int64)
    ids = sorted(set(groups.tolist()))
    if not 2 <= folds <= len(ids):
        raise ValueError(f"folds = {folds}: 2 .. {len(ids)}")
    fold = {gid: i % folds for i, gid in enumerate(ids)}
    return np.array([fold[v] for v in groups.tolist()], np.int64)


def planted(seed, M, D, C, noise=1.0):
    """Rows around C prototypes plus noise, class sizes falling geometrically, every class present, no fp16 subnormals (what the MFMA
    does with them is not part of the contract); (rng, fp16 rows, int64 labels)."""
    rng = np.random.default_rng(seed)
    proto = rng.standard_normal((C, D))
    share = 0.85 ** np.arange(C)
    y = rng.choice(C, M, p=share / share.sum())
    y[:C] = np.arange(C)
    x = (proto[y] + noise * rng.standard_normal((M, D))).astype(np.float16)
    tiny = np.float16(6.2e-5)
    x[(np.abs(x) < tiny) & (x != 0)] = tiny
    return rng, x, y.astype(np.int64)


def planted_project(seed, sizes, D, C, block=20, scale=2.0, noise=0.3):
    """Per file of `sizes` frames the fp16 rows and int64 labels of a planted, well-separated project: frame t of file i has class
    (t // block + i) % C and the row scale * prototype + noise."""
    rng = np.random.default_rng(seed)
    proto = rng.standard_normal((C, D))
    rows, labels = [], []
    for i, n in enumerate(sizes):
        lab = (np.arange(n) // block + i) % C
        rows.append((scale * proto[lab] + noise * rng.standard_normal((n, D))).astype(np.float16))
        labels.append(lab.astype(np.int64))
    return rows, labels


def project_bank(rows_of, labels_of, stride):
    """(x, y, group) of the bank knn.LabelBank.from_instances builds from the label runs of such a project with group='instance':
    every stride-th frame of a run, the runs numbered file by file."""
    x, y, group = [], [], []
    number = 0
    for rows, lab in zip(rows_of, labels_of):
        cuts = np.flatnonzero(np.diff(lab)) + 1
        for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(lab)]])):
            frames = np.arange(a, b, stride)
            x.append(rows[frames])
            y.append(lab[frames])
            group.append(np.full(frames.size, number, np.int64))
            number += 1
    return np.concatenate(x), np.concatenate(y), np.concatenate(group)


def balanced(labels, C):
    labels = np.asarray(labels, np.int64)
    return np.array([labels.size / (C * (labels == c).sum()) if (labels == c).any() else 0.0 for c in range(C)])


# ---- the bounds ----------------------------------------------------------------------------------------------------------------------
def _rn_rel(D):
    return g(D / 4 + 2) / 2 + E


def logit_bound(x, W, b):
    """(N, C): the bound on |device logit - float64 logit|."""
    D = np.asarray(x).shape[1]
    u = np.abs(working_rows(x))
    A = u @ np.abs(np.asarray(W, np.float64)).T
    f = (1.0 + g(D / 2 + 1)) * (1.0 + _rn_rel(D))
    bound = A * (f - 1.0) + E * (A * f + np.abs(np.asarray(b, np.float64))[None, :])
    bound[~(u > 0).any(axis=1)] = 0.0                            # a zero row: the bias exactly
    return bound


def _softmax_terms(x, W, b):
    """z, dz, p, and per row the largest rho and gs."""
    z = logits(x, W, b)
    dz = logit_bound(x, W, b)
    C = z.shape[1]
    zmax, dzmax = z.max(axis=1, keepdims=True), dz.max(axis=1, keepdims=True)
    t = (zmax - z) + dz + dzmax
    rho = np.exp(dz + E * t) * (1.0 + 2.0 * E) - 1.0
    gs = g(-(-C // 16) + 3)
    p = np.exp(log_softmax(z)[0])
    return z, dz, p, rho, rho.max(axis=1, keepdims=True), gs


def prob_bound(x, W, b):
    """(N, C): the bound on |device probability - float64 probability|."""
    z, dz, p, rho, rmax, gs = _softmax_terms(x, W, b)
    return p * ((1.0 + rho) * (1.0 + E) / (1.0 - rmax - gs) - 1.0) + TINY


def _gl(M):
    return g(min(M, SEGMENT) + -(-M // SEGMENT))


def loss_bound(x, y, omega, W, b, l2):
    """The bound on |device F - float64 F| at (W, b)."""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    M, D = np.asarray(x).shape
    C = W.shape[0]
    om = _omega(omega, M)
    z, dz, p, rho, rmax, gs = _softmax_terms(x, W, b)
    idx = np.arange(M)
    logC = np.log(C)
    dl = -np.log(1.0 - rmax[:, 0] - gs) + 2.0 * E * (logC + 1.0) + E * (np.abs(z).max(axis=1) + dz.max(axis=1) + logC + 1.0)
    _, lse = log_softmax(z)
    ell = lse - z[idx, y]
    d_ell = om * ((dl + dz[idx, y]) * (1.0 + 2.0 * E) + 2.0 * E * ell)
    gl = _gl(M)
    Om = om.sum()
    ro = (1.0 + gl / (1.0 - gl)) * (1.0 + E) - 1.0
    data = (om * ell).sum() / Om
    d_data = (d_ell.sum() + gl * (om * ell + d_ell).sum()) / Om * (1.0 + ro) + data * ro
    reg = (W * W).sum() + (b * b).sum()
    F = data + 0.5 * float(l2) * reg
    rest = d_data + 0.5 * float(l2) * g(D + C + 1) * reg
    return rest + E * (F + rest)


def gradient_bound(x, y, omega, W, b, l2):
    """((C, D), (C,)): the bounds on |device gradient - float64 gradient| at (W, b)."""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    M, D = np.asarray(x).shape
    om = _omega(omega, M)
    u = np.abs(working_rows(x))
    p = predict(x, W, b)[0]
    dp = prob_bound(x, W, b)
    r = p.copy()
    r[np.arange(M), y] -= 1.0
    r = np.abs(r) * om[:, None]
    dr = om[:, None] * dp * (1.0 + 2.0 * E) + 2.0 * E * (r + om[:, None] * dp)
    ru = (1.0 + _rn_rel(D)) * (1.0 + E) - 1.0
    gl = _gl(M)
    Om = om.sum()
    rO = (1.0 + gl / (1.0 - gl)) * (1.0 + E) ** 2 - 1.0
    gW, gb = gradient(x, y, omega, W, b, l2)
    out = []
    for cols, rel, grad, weight in ((u, ru, gW, W), (np.ones((M, 1)), 0.0, gb[:, None], b[:, None])):
        dS = dr.T @ cols * (1.0 + rel) + r.T @ cols * rel + gl * ((r + dr).T @ cols) * (1.0 + rel)
        S = np.abs(grad - float(l2) * weight) * Om                # |sum_m r u| of the float64 gradient
        first = dS / Om * (1.0 + rO) + S / Om * rO
        out.append(first + E * (np.abs(grad) + first))
    return out[0], out[1][:, 0]


def step_bound(x, y, omega, W0, b0, l2, W1, b1):
    """((C, D), (C,)): the bounds on |(w0 - w1) L - gradient(w0)| for the device's one step w1."""
    L = 1.0 + float(l2)
    dW, db = gradient_bound(x, y, omega, W0, b0, l2)
    gW, gb = gradient(x, y, omega, W0, b0, l2)
    return (dW * (1.0 + E) + E * np.abs(gW) + L * E * np.abs(np.asarray(W1, np.float64)),
            db * (1.0 + E) + E * np.abs(gb) + L * E * np.abs(np.asarray(b1, np.float64)))
