"""The references and bounds of oracle/kernel_ref.py on the CPU (no GPU): the fmaf-chain emulation equals exact rational
arithmetic, every bound accepts a numpy simulation of its kernel's roundings, and rejects the same output with a planted
defect - so tests/test_gpu_kernel_reference.py's bounds are neither wrong nor vacuous."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import kernel_ref as R


@pytest.fixture(autouse=True, scope="module")
def _one_blas_thread():
    """These checks are small: keep them on one core so that they cost the rest of a CPU suite (its wall-clock legs
    included, should a runner interleave files) nothing but their own ~1 s."""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:                      # pragma: no cover - numpy's own thread count then
        yield
        return
    with threadpool_limits(limits=1):
        yield


def _round_f32(v: Fraction) -> np.float32:
    """Correct rounding of a rational to fp32 (nearest, ties to even)."""
    f = np.float32(float(v))                      # within one fp32 ulp of the answer
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - v), int(np.float32(c).view(np.uint32)) & 1))


def _exact_chain(A, W, order):
    out = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for i in range(A.shape[0]):
        for j in range(W.shape[0]):
            acc = np.float32(0.0)
            for k in order:
                acc = _round_f32(Fraction(float(acc)) + Fraction(float(A[i, k])) * Fraction(float(W[j, k])))
            out[i, j] = acc
    return out


def test_fmaf_chain_equals_exact_rational_arithmetic():
    rng = np.random.default_rng(1)
    A = rng.standard_normal((3, 64)).astype(np.float32)
    W = rng.standard_normal((3, 64)).astype(np.float32)
    A[0] *= np.exp2(rng.integers(-20, 20, 64)).astype(np.float32)             # wide dynamic range
    # constructed ties: 1 + 2^-24 is an fp32 midpoint; the products 2^-24 (exact) land on it, and a later tiny product
    # (2^-60) decides the side - only a chain that keeps the TwoSum residual rounds those correctly
    A[1, :4] = [1.0, 2.0 ** -24, 2.0 ** -60, 3.0]
    W[1, :4] = [1.0, 1.0, 1.0, -3.0]
    A[2, :6] = [1.0, 2.0 ** -24, -2.0 ** -60, 1.0, 3.0 * 2.0 ** -25, 2.0 ** -70]
    W[2, :6] = [1.0, 1.0, 1.0, -1.0, 1.0, 1.0]
    # cancellation: a large sum that cancels to a small remainder
    A[1, 4:8] = [1e8, 3.14159, -1e8, 1e-3]
    W[1, 4:8] = [1.0, 1.0, 1.0, 1.0]
    for order in (None, R.f32_mfma_k_order(64)):
        o = range(64) if order is None else order
        assert np.array_equal(R.fmaf_chain(A, W, order).view(np.uint32), _exact_chain(A, W, o).view(np.uint32))


def test_tie_rounding_decided_by_the_residual():
    s = np.array([1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24])
    e = np.array([1e-30, -1e-30, 0.0, 0.0])
    r = R.round_f32_with_residual(s, e)
    assert r[0] == np.nextafter(np.float32(1), np.float32(2)) and r[1] == np.float32(1.0)
    assert r[2] == np.float32(1.0 + 4 * 2.0 ** -24) and r[3] == np.float32(1.0)     # ties to even without a residual


# ---- GEMM: simulated kernels, planted defects ------------------------------------------------------------------------
def _case(epi, M=257, N=768, K=256, seed=0):          # an M edge and the tile-form shape of the GPU tests
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    d = dict(A=A, W=W, bias=(0.5 * rng.standard_normal(N)).astype(np.float32), M=M)
    if epi == R.EPI_RESID:
        d.update(lam=(0.3 * rng.standard_normal(N)).astype(np.float32), x0=rng.standard_normal((M, N)).astype(np.float32))
    if epi == R.EPI_QKV:
        cos, sin = R.rope_cos_sin(14, 14, 64, 100.0)
        d.update(D=N // 3, T=201, n_prefix=5, cos=cos, sin=sin)
    return d


def _reference(arith, epi, d, **kw):
    acc, E, S = R.gemm_acc(arith, d["A"], d["W"], **kw)
    y, Ey, _ = R.gemm_epilogue_ref(epi, acc, E, S, bias=d["bias"], lam=d.get("lam"), x0=d.get("x0"), T=d.get("T"),
                                   n_prefix=d.get("n_prefix", 0), cos=d.get("cos"), sin=d.get("sin"), D=d.get("D"))
    return acc, y, Ey


def _simulate(arith, epi, d, acc32, *, shift_bias=False, swap_rope=False, rope_prefix=False, no_q_scale=False):
    """The kernel's epilogue in float32 on an fp32 accumulator, then its output rounding; optional planted defects."""
    f = np.float32
    b = d["bias"].astype(f)
    if shift_bias:
        b = np.roll(b, 1)
    v = acc32 + b[None, :]
    if epi == R.EPI_RESID:
        return ((v * d["lam"][None, :]) + d["x0"]).astype(np.float64)
    if epi == R.EPI_GELU:
        y = R.gelu_erf(v)
        return (y.astype(np.float16) if arith == 0 else y).astype(np.float64)
    M, N = v.shape
    y = v.copy()
    t = np.arange(M) % d["T"]
    rows = np.nonzero(t >= (d["n_prefix"] - (1 if rope_prefix else 0)))[0]
    tt = np.maximum(t[rows] - d["n_prefix"], 0)
    c, s = d["cos"][tt], d["sin"][tt]
    for h0 in range(0, 2 * d["D"], 64):
        vh = v[rows, h0:h0 + 64]
        rot = R._rotate_half(vh)
        y[rows, h0:h0 + 64] = (vh * s + rot * c) if swap_rope else (vh * c + rot * s)
    if not no_q_scale:
        y[:, :d["D"]] *= f(0.125)
    return (y.astype(np.float16) if arith == 0 else y).astype(np.float64)


def _bound_out(arith, epi, y, Ey):
    if arith == 0 and epi in (R.EPI_QKV, R.EPI_GELU):
        return Ey + R.out_rounding(y, "f16")
    return Ey + R.out_rounding(y, "f32")


@pytest.mark.parametrize("arith", [0, 3])
@pytest.mark.parametrize("epi", [R.EPI_QKV, R.EPI_RESID, R.EPI_GELU])
def test_gemm_bound_accepts_the_simulated_kernel_and_rejects_planted_defects(arith, epi):
    d = _case(epi, seed=10 * arith + epi)
    acc, y, Ey = _reference(arith, epi, d)
    if epi == R.EPI_GELU:
        v = acc + d["bias"][None, :]
        Ey = Ey + 2e-7 * np.abs(v) + 8 * R.U32 * (np.abs(v) + np.abs(y))
    bound = _bound_out(arith, epi, y, Ey)
    a = R.f16(d["A"]).astype(np.float32) if arith == 0 else d["A"]
    w = R.f16(d["W"]).astype(np.float32) if arith == 0 else d["W"]
    acc32 = a @ w.T                                                         # fp32 accumulation (BLAS order)
    assert R.ratio(_simulate(arith, epi, d, acc32), y, bound) <= 1.0
    K = d["A"].shape[1]
    defects = {"last K-tile dropped": _simulate(arith, epi, d, a[:, :K - 32] @ w[:, :K - 32].T),
               "bias shifted one column": _simulate(arith, epi, d, acc32, shift_bias=True)}
    last = _simulate(arith, epi, d, acc32)
    last[-1] = last[-2]
    defects["last row copied from the row before"] = last
    if epi == R.EPI_QKV:
        defects["RoPE halves swapped"] = _simulate(arith, epi, d, acc32, swap_rope=True)
        defects["RoPE on a prefix row"] = _simulate(arith, epi, d, acc32, rope_prefix=True)
        defects["q's 1/8 missing"] = _simulate(arith, epi, d, acc32, no_q_scale=True)
    for name, out in defects.items():
        r = R.ratio(out, y, bound)
        assert r > 1.0, (name, r)


def test_split_bound_accepts_simulated_split_products_and_rejects_a_dropped_k_tile():
    rng = np.random.default_rng(4)
    M, N, K = 300, 256, 768
    A = rng.standard_normal((M, K)).astype(np.float32)
    A[7] *= 2.0 ** -16                                                      # low halves in fp16's subnormal range
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    acc, E, S = R.gemm_acc(4, A, W, 2.0, 4.0)
    ah, al = R.split_halves(A, 2.0)
    wh, wl = R.split_halves(W, 4.0)
    sim = ((ah @ wh.T + ah @ wl.T + al @ wh.T) / 8.0).astype(np.float32).astype(np.float64)   # a_lo w_lo dropped
    bound = E + R.out_rounding(acc, "f32")
    assert R.ratio(sim, acc, bound) <= 1.0
    cut = ((ah[:, :-32] @ wh[:, :-32].T + ah[:, :-32] @ wl[:, :-32].T + al[:, :-32] @ wh[:, :-32].T) / 8.0)
    assert R.ratio(cut, acc, bound) > 1.0


def test_split_decoders_invert_the_store_layouts():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 64)).astype(np.float32)
    hi, lo = R.split_halves(x, 4.0)
    raw = np.zeros((3, 64), np.float32)
    h = raw.view(np.float16).reshape(3, 2, 2, 32)                           # [row][K-tile][hi | lo][32]
    k = np.arange(32)
    pos = 8 * ((k % 16) // 4) + 4 * (k // 16) + k % 4
    for t in range(2):
        h[:, t, 0, pos] = hi[:, t * 32:(t + 1) * 32]
        h[:, t, 1, pos] = lo[:, t * 32:(t + 1) * 32]
    assert np.array_equal(R.decode_split_operand(raw, 64, 4.0), (hi + lo) / 4.0)
    raw2 = np.zeros((3, 64), np.float32)
    h2 = raw2.view(np.float16).reshape(3, 2, 64)
    h2[:, 0], h2[:, 1] = hi, lo
    assert np.array_equal(R.decode_head_split(raw2, 64, [4.0]), (hi + lo) / 4.0)


# ---- attention -------------------------------------------------------------------------------------------------------
def _qkv(n, T, D, seed):
    rng = np.random.default_rng(seed)
    rows = n * T
    q = rng.standard_normal((rows, D)) * 0.3
    k = rng.standard_normal((rows, D))
    k[np.arange(n) * T + T - 1] *= 3.0                                      # strong keys in the last, partial tile
    v = rng.standard_normal((rows, D))
    return np.concatenate([q, k, v], axis=1).astype(np.float32)


def _sim_attention(qkv, n, T, D, *, leak=False, drop_last=False, no_q_scale=False):
    """The fp16 kernel's roundings: fp16 q, k, v; fp32 scores; unnormalised p rounded to fp16; fp32 P.V and row sum;
    fp16 output.  leak: frame b also attends to the next frame's first key."""
    q, k, v = R.attention_operands(0, qkv, D)
    if no_q_scale:
        q = q * 8.0
    H = D // 64
    out = np.zeros((n * T, D))
    for b in range(n):
        keys = list(range(b * T, (b + 1) * T - (1 if drop_last else 0)))
        if leak and b + 1 < n:
            keys.append((b + 1) * T)
        for h in range(H):
            c = slice(h * 64, (h + 1) * 64)
            s = (q[b * T:(b + 1) * T, c].astype(np.float32) @ k[keys, c].astype(np.float32).T)
            p = np.exp(s - s.max(axis=1, keepdims=True)).astype(np.float16).astype(np.float32)
            o = (p @ v[keys, c].astype(np.float32)) / p.sum(axis=1, keepdims=True, dtype=np.float32)
            out[b * T:(b + 1) * T, c] = o.astype(np.float16)
    return out


@pytest.mark.parametrize("T", [33, 201, 289])
def test_attention_bound_accepts_the_simulated_kernel_and_rejects_planted_defects(T):
    n, D = 3, 128
    qkv = _qkv(n, T, D, T)
    ref, bound = R.attention_ref(0, qkv, n, T, D)
    assert R.ratio(_sim_attention(qkv, n, T, D), ref, bound) <= 1.0
    for name, kw in (("a key of the next frame unmasked", dict(leak=True)), ("the last key dropped", dict(drop_last=True)),
                     ("q's 1/8 missing", dict(no_q_scale=True))):
        r = R.ratio(_sim_attention(qkv, n, T, D, **kw), ref, bound)
        assert r > 1.0, (name, r)


# ---- row-wise kernels: LayerNorm forms, the MX-fp8 row, the ConvNeXt producers ----------------------------------------
F32 = np.float32


def _sim_ln(x, gamma, beta, eps, *, unbiased=False, no_eps=False, one_pass=False, drop_last_vec=False):
    """ln_row / layernorm_f32_kernel / cnx_ln in numpy float32 with the kernels' reduction order: a lane adds its 4-vectors
    pairwise, accumulates them in order, then the xor butterfly 32, 16, .., 1 over the 64 lanes.  Optional planted defects."""
    x = np.asarray(x, F32)
    M, D = x.shape
    nvec = D // 4
    NV = (nvec + 63) // 64
    valid = (np.arange(NV * 64) < nvec).reshape(NV, 64)
    xp = np.zeros((M, NV * 256), F32)
    xp[:, :D] = x
    xp = xp.reshape(M, NV, 64, 4)

    def wave_sum(vec4, mask):                                     # vec4 [M][NV][64][4] -> [M]
        pair = (vec4[..., 0] + vec4[..., 1]) + (vec4[..., 2] + vec4[..., 3])
        s = np.zeros((M, 64), F32)
        for k in range(NV):
            s = s + np.where(mask[k], pair[:, k], F32(0))
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, np.arange(64) ^ o]
        return s[:, 0]

    mmask = valid.copy()
    if drop_last_vec:
        mmask[NV - 1] = False
    with np.errstate(all="ignore"):
        mean = (wave_sum(xp, mmask) / F32(D))[:, None, None, None]
        d = xp - mean
        if one_pass:
            q = wave_sum(xp * xp, valid) / F32(D) - mean[:, 0, 0, 0] * mean[:, 0, 0, 0]
        else:
            q = wave_sum(d * d, valid) / F32(D - 1 if unbiased else D)
        rstd = F32(1) / np.sqrt(q + (F32(0) if no_eps else F32(eps)))
        g = np.zeros(NV * 256, F32)
        g[:D] = gamma
        b = np.zeros(NV * 256, F32)
        b[:D] = beta
        y = d * rstd[:, None, None, None] * g.reshape(NV, 64, 4) + b.reshape(NV, 64, 4)
    return y.reshape(M, NV * 256)[:, :D]


def _store(y32, kind):
    """The output format's rounding of an fp32 row: fp16, fp32, or the split pair at scale 1."""
    if kind == "f16":
        return y32.astype(np.float16).astype(np.float64)
    if kind == "split":
        return R.split_value(y32, 1.0)
    return y32.astype(np.float64)


LN_DEFECTS = ("unbiased", "no_eps", "one_pass", "drop_last_vec")


@pytest.mark.parametrize("kind", ["f16", "f32", "split"])
@pytest.mark.parametrize("D", [128, 256, 384, 768, 1024, 1280, 96, 800, 1536])
def test_layernorm_bound_accepts_the_simulated_kernel_and_rejects_planted_defects(kind, D):
    """ViT widths (NV 1 .. 5) and ConvNeXt widths (96: a partial only vector, 800: a partial vector at NV 4, 1536: NV 6)."""
    rejected = set()
    for eps in (1e-5, 1e-6):
        x, gamma, beta = R.rows_case(9, D, 1000 + D)
        ref, E = R.ln_ref(x, gamma, beta, eps)
        bound = R.stored_bound(ref, E, kind)
        r = R.ratio(_store(_sim_ln(x, gamma, beta, eps), kind), ref, bound)
        print(f"[ln {kind} D {D} eps {eps:g}] simulated kernel: max err / bound {r:.3f}")
        assert r <= 1.0
        for name in LN_DEFECTS:
            if name == "drop_last_vec" and (D // 4) % 64 == 0:
                continue
            if R.ratio(_store(_sim_ln(x, gamma, beta, eps, **{name: True}), kind), ref, bound) > 1.0:
                rejected.add(name)
    expect = set(LN_DEFECTS) - ({"drop_last_vec"} if (D // 4) % 64 == 0 else set())
    if kind == "f16" and D >= 1024:
        expect.discard("unbiased")           # 1 / (2 D) of the value is below fp16's own rounding there; caught at every D < 1024
    assert rejected >= expect, expect - rejected


def test_each_layernorm_defect_is_caught_where_it_should_be():
    """Per trap row: the constant row catches the dropped eps, the mean-1e3 row the one-pass variance."""
    D = 384
    x, gamma, beta = R.rows_case(4, D, 7)
    ref, E = R.ln_ref(x, gamma, beta, 1e-6)
    bound = R.stored_bound(ref, E, "f32")
    err = lambda **kw: np.abs(_sim_ln(x, gamma, beta, 1e-6, **kw) - ref) / bound    # noqa: E731
    with np.errstate(invalid="ignore"):
        assert not (np.nan_to_num(err(no_eps=True)[1], nan=np.inf) <= 1.0).all()
        assert err(one_pass=True)[0].max() > 1.0
        assert err(drop_last_vec=True).max(axis=1).min() > 1.0                     # every row
        assert err(unbiased=True)[3].max() > 1.0                                   # a plain random row


# MX-fp8 row
def _sim_mx_row(y32, *, neighbour_block=False):
    """layernorm_f8_kernel's store on the fp32 LayerNorm rows: block maximum -> scale byte -> e4m3 bytes, and the scale
    image [D/128][sc_ld] dwords.  neighbour_block: each scale byte lands in the next 32-column block's slot."""
    from oracle import mx_oracle as MX
    M, D = y32.shape
    sc_ld = M + 3
    yb = y32.reshape(M, D // 32, 32)
    sb = MX.mx_scale_exp(np.abs(yb).max(-1))
    inv = np.exp2(127.0 - sb).astype(F32)
    q = MX.e4m3_round(yb * inv[:, :, None])
    # e4m3 value -> byte: sign | exponent | mantissa
    a = np.abs(q).astype(np.float64)
    e = np.where(a >= 2.0 ** -6, np.floor(np.log2(np.maximum(a, 2.0 ** -9))), -7)
    ef = (e + 7).astype(np.int64)
    m = np.where(ef > 0, a / 2.0 ** e * 8 - 8, a * 2.0 ** 9).astype(np.int64)
    byte = ((np.signbit(q).astype(np.int64) << 7) | (ef << 3) | m).astype(np.uint8).reshape(M, D)
    img = np.full((D // 128, sc_ld, 4), 0xA5, np.uint8)
    for blk in range(D // 32):
        dst = (blk + 1) % (D // 32) if neighbour_block else blk
        img[dst // 4, :M, dst % 4] = sb[:, blk]
    return byte, img.view(np.uint32).reshape(D // 128, sc_ld)


@pytest.mark.parametrize("D", [256, 384, 768, 1024])
def test_mx_row_bound_and_scale_bytes(D):
    M = 64
    tolerated = total = 0
    for eps in (1e-5, 1e-6):
        x, gamma, beta = R.rows_case(M, D, 2000 + D)
        ref, E = R.ln_ref(x, gamma, beta, eps)
        y32 = _sim_ln(x, gamma, beta, eps)
        byte, img = _sim_mx_row(y32)
        val, sb = R.mx_row_decode(byte, img, M, D)
        r = R.ratio(val, ref, R.mx_row_bound(ref, E, sb))
        print(f"[ln f8 D {D} eps {eps:g}] simulated kernel: max err / bound {r:.3f}")
        assert r <= 1.0
        want, lo, hi = R.mx_scale_window(ref, E)
        assert ((sb >= lo) & (sb <= hi)).all()
        tolerated += int((lo != hi).sum())
        total += lo.size
        # planted: the scale byte written to the neighbouring 32-column block
        byte2, img2 = _sim_mx_row(y32, neighbour_block=True)
        val2, sb2 = R.mx_row_decode(byte2, img2, M, D)
        assert not ((sb2 >= lo) & (sb2 <= hi)).all()
        assert R.ratio(val2, ref, R.mx_row_bound(ref, E, sb2)) > 1.0
    assert tolerated <= 0.01 * total, (tolerated, total)


def test_the_gpu_cases_of_the_mx_row_have_few_blocks_at_a_scale_boundary():
    """tests/test_gpu_rows_reference.py accepts either neighbour where the reference's block maximum lies within the bound of
    a scale boundary; with its seeds (kernel_ref.mx_row_seed) the reference alone keeps such blocks under 1 % per case."""
    for D in (256, 384, 768, 1024):
        for M in (1, 3, 4, 5, 1023):
            x, gamma, beta = R.rows_case(M, D, R.mx_row_seed(D, M))
            ref, E = R.ln_ref(x, gamma, beta, 1e-5 if M % 2 else 1e-6)
            _, lo, hi = R.mx_scale_window(ref, E)
            assert (lo != hi).sum() <= 0.01 * lo.size, (D, M, int((lo != hi).sum()), lo.size)


# ConvNeXt producers
def _cnx_case(n, h, w, C, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, h, w, C)) * 1.5 + 0.3).astype(F32)
    gamma = (1.0 + 0.5 * rng.standard_normal(C)).astype(F32)
    beta = (0.3 * rng.standard_normal(C)).astype(F32)
    wt = (rng.standard_normal((49, C)) / 7.0).astype(F32)
    bias = (0.2 * rng.standard_normal(C)).astype(F32)
    return x, gamma, beta, wt, bias


def _sim_dwconv(x, wt, bias, *, shift=False, clamp=False):
    """The kernel's fmaf chain over the taps inside the frame (ky, then kx), then the bias: each step's exact product and
    sum in float64, rounded once to fp32.  shift: the taps read one pixel to the right; clamp: edge clamping for zero padding."""
    n, h, w, C = x.shape
    acc = np.zeros((n, h, w, C), F32)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    for ky in range(7):
        for kx in range(7):
            iy, ix = ys + ky - 3, xs + kx - 3 + (1 if shift else 0)
            inside = ((iy >= 0) & (iy < h) & (ix >= 0) & (ix < w))[None, :, :, None]
            a = x[:, np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1)]
            step = (acc.astype(np.float64) + a.astype(np.float64) * wt[7 * ky + kx].astype(np.float64)).astype(F32)
            acc = step if clamp else np.where(inside, step, acc)
    return acc + bias


@pytest.mark.parametrize("C", [32, 96, 800])
def test_dwconv_ln_bound_accepts_the_simulated_kernel_and_rejects_planted_defects(C):
    for (h, w) in ((1, 1), (2, 3), (7, 7), (8, 5)):
        x, gamma, beta, wt, bias = _cnx_case(2, h, w, C, 10 * h + w)
        ref, E = R.cnx_dwconv_ln_ref(x, wt, bias, gamma, beta, 1e-6)
        bound = R.stored_bound(ref, E, "f32")
        sim = lambda **kw: _sim_ln(_sim_dwconv(x, wt, bias, **kw).reshape(-1, C), gamma, beta, 1e-6).astype(np.float64)   # noqa: E731
        r = R.ratio(sim(), ref, bound)
        print(f"[dwconv C {C} {h}x{w}] simulated kernel: max err / bound {r:.3f}")
        assert r <= 1.0
        if h * w > 1:                           # a 1 x 1 frame has one tap: nothing to shift or clamp to
            assert R.ratio(sim(shift=True), ref, bound) > 1.0
            assert R.ratio(sim(clamp=True), ref, bound) > 1.0
    # the 1 x 1 frame's only tap is the centre one: a kernel that took tap 0 instead is rejected
    x, gamma, beta, wt, bias = _cnx_case(2, 1, 1, C, 11)
    ref, E = R.cnx_dwconv_ln_ref(x, wt, bias, gamma, beta, 1e-6)
    wrong = _sim_ln((x * wt[0] + bias).reshape(-1, C), gamma, beta, 1e-6)
    assert R.ratio(wrong, ref, R.stored_bound(ref, E, "f32")) > 1.0


@pytest.mark.parametrize("C", [32, 192, 1536])
def test_downsample_bound_accepts_the_simulated_kernel_and_rejects_swapped_kh_kw(C):
    x, gamma, beta, _, _ = _cnx_case(2, 5, 7, C, 5)
    x[:, 4], x[:, :, 6] = np.nan, np.nan                                  # the odd grid's last row / column: never read
    ref, E = R.cnx_downsample_ref(x, gamma, beta, 1e-6)
    assert np.isfinite(ref).all() and np.isfinite(E).all()
    bound = R.stored_bound(ref, E, "f32")
    y = _sim_ln(x[:, :4, :6].reshape(-1, C), gamma, beta, 1e-6).reshape(2, 2, 2, 3, 2, C)       # [b][oy][kh][ox][kw][C]
    good = y.transpose(0, 1, 3, 2, 4, 5).reshape(-1, 4 * C)
    swapped = y.transpose(0, 1, 3, 4, 2, 5).reshape(-1, 4 * C)
    assert R.ratio(good, ref, bound) <= 1.0
    assert R.ratio(swapped, ref, bound) > 1.0
    assert R.ratio(_store(good, "split"), ref, R.stored_bound(ref, E, "split")) <= 1.0


@pytest.mark.parametrize("hw", [1, 3, 4, 5, 49, 196])
def test_pool_ln_bound_accepts_the_kernel_order_and_rejects_a_dropped_pixel(hw):
    C = 384
    x, gamma, beta, _, _ = _cnx_case(3, 1, hw, C, hw)
    x = x.reshape(3, hw, C)
    ref, E = R.cnx_pool_ln_ref(x, gamma, beta, 1e-6)
    bound = R.stored_bound(ref, E, "f32")
    r = R.ratio(_sim_ln(R.pool_order_f32(x), gamma, beta, 1e-6), ref, bound)
    print(f"[pool hw {hw}] simulated kernel: max err / bound {r:.3f}")
    assert r <= 1.0
    if hw > 1:
        dropped = R.pool_order_f32(x[:, :-1]) * F32(hw - 1) / F32(hw)       # the last pixel (a partial round of 4) left out
        assert R.ratio(_sim_ln(dropped, gamma, beta, 1e-6), ref, bound) > 1.0
    # (a wrong divisor is no defect here: LayerNorm undoes a common factor)  The next frame's first pixel summed as well:
    leak = R.pool_order_f32(np.concatenate([x, np.roll(x, -1, axis=0)[:, :1]], axis=1)) * F32(hw + 1) / F32(hw)
    assert R.ratio(_sim_ln(leak, gamma, beta, 1e-6), ref, bound) > 1.0


def test_stem_reference_gathers_4x4_patches_and_ignores_the_remainder():
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, (2, 9, 14), dtype=np.uint8)
    f[:, 8:], f[:, :, 12:] = 255, 255                                      # the remainder of a 9 x 14 frame: never read
    A = R.cnx_stem_ref(f, True)
    assert A.shape == (2 * 2 * 3, 32) and not A[:, 16:].any()
    m = (1 * 2 + 1) * 3 + 2                                               # frame 1, oy 1, ox 2
    assert np.array_equal(A[m, :16].reshape(4, 4), (f[1, 4:8, 8:12] / 255.0).astype(F32))
    g = rng.standard_normal((2, 9, 14)).astype(F32)
    assert np.array_equal(R.cnx_stem_ref(g, False)[m, :16].reshape(4, 4), g[1, 4:8, 8:12])


# ---- classifier head: the exact-fp32 GEMM and the small training kernels (tests/test_gpu_head_kernels_reference.py) ----
# Same inputs as the GPU tests (the case builders of oracle/kernel_ref.py).  Where the GPU test asks for equal bits, a planted
# defect must change bits; where it asks for a bound, a float32 simulation in the kernel's order must pass and the defect fail.
def _f32_gelu(v32):
    return (F32(0.5) * v32 * (F32(1.0) + R._erf64(v32.astype(np.float64) / np.sqrt(2.0)).astype(F32))).astype(F32)


def test_head_gemm_reference_rejects_planted_defects():
    M, N, K = 129, 132, 96
    A, W, b = R.head_gemm_case(M, N, K, 1000 * M + 10 * N + K, N_alloc=N + 4, lda=K + 4)
    A, W = A[:, :K], W[:N, :K]
    pre, _ = R.head_gemm_exact(A, W, b, K)
    acc, _ = R.head_gemm_exact(A, W, None, K)
    y, bound = R.head_gemm_gelu_ref(pre)
    assert R.ratio(_f32_gelu(pre), y, bound) <= 1.0
    same = lambda t: np.array_equal(t.view(np.uint32), pre.view(np.uint32))     # noqa: E731
    assert not same((R.fmaf_chain(A, W) + b[None, :]).astype(F32)), "k order 0 .. K-1 must differ from the MFMA's in some bits"
    dropped = (R.fmaf_chain(A[:, :K - 32], W[:, :K - 32], R.f32_mfma_k_order(K - 32)) + b[None, :]).astype(F32)
    shifted = (acc + np.roll(b, 4)[None, :]).astype(F32)
    before = (_f32_gelu(acc) + b[None, :]).astype(F32)
    assert not same(dropped) and not same(shifted)
    for name, out in (("last K-tile dropped", _f32_gelu(dropped)), ("bias shifted by 4 columns", _f32_gelu(shifted)),
                      ("GELU before the bias", before)):
        assert R.ratio(out, y, bound) > 1.0, name
    # split-K: a partial added twice / skipped changes the sum's bits
    Kt, splits = 1024, 4
    A, W, _ = R.head_gemm_case(12, 128, Kt, Kt + splits + 12, bias=False)
    want, parts = R.head_gemm_exact(A, W, None, Kt // splits, splits)
    twice = ((((parts[0] + parts[1]) + parts[1]) + parts[2]) + parts[3]).astype(F32)
    skipped = ((parts[0] + parts[1]) + parts[3]).astype(F32)
    backwards = (((parts[3] + parts[2]) + parts[1]) + parts[0]).astype(F32)
    for t in (twice, skipped, backwards):
        assert not np.array_equal(t.view(np.uint32), want.view(np.uint32))
    # ... and against the float64 product those two are far outside fp32 accumulation's K u32 sum |a w|
    acc64, E, _ = R.gemm_acc(3, A, W)
    assert R.ratio(want, acc64, E) <= 1.0 and R.ratio(twice, acc64, E) > 1.0 and R.ratio(skipped, acc64, E) > 1.0


@pytest.mark.parametrize("rows", [1, 37, 63, 64, 65, 1000])
def test_colsum_bound_accepts_the_kernel_order_and_rejects_planted_defects(rows):
    for cols in (1, 65):
        src, _ = R.colsum_case(rows, cols, 7 * rows + cols)
        x = src[:, :cols]
        for scale in (1.0, 1.0 / 37.0):
            tmp, dst = R.colsum_f32(x, scale)
            ref, bound = R.colsum_ref(x, scale)
            assert R.ratio(dst, ref, bound) <= 1.0
            per = -(-rows // 64)
            if rows > 63 * per:                                              # chunk 63 holds rows: drop it
                assert R.ratio((tmp[:63].sum(0, dtype=F32) * F32(scale)), ref, bound) > 1.0, "last chunk dropped"
            if rows % 64:                                                    # per = rows / chunks rounded down loses the tail
                lost = x[:(rows // 64) * 64].sum(0, dtype=F32) * F32(scale)
                assert R.ratio(lost, ref, bound) > 1.0, "per rounded down"
            if scale != 1.0:
                assert R.ratio(R.colsum_f32(x, 1.0)[1], ref, bound) > 1.0, "scale ignored"


@pytest.mark.parametrize("n", [32, 100, 256])
def test_cov_offdiag_reference_rejects_planted_defects(n):
    cov, cs, gs = R.cov_case(n, n)
    ref, bound = R.cov_sq_ref(cov, cs)
    sim = R.cov_sq_f32(cov, cs)
    assert R.ratio(sim, ref, bound) <= 1.0
    v = (cov * cs).astype(F32)
    kept = (sim + np.diagonal(v) ** 2).astype(F32)
    assert R.ratio(kept, ref, bound) > 1.0, "diagonal kept"
    assert R.ratio((gs * gs) * sim, ref, bound) > 1.0 and R.ratio(gs * sim, ref, bound) > 1.0, "gscale applied to sq"
    G = R.cov_offdiag_f32(cov, cs, gs)
    assert (np.diagonal(G).view(np.uint32) == 0).all() and not np.array_equal(G, (gs * v).astype(F32))


def _sim_ce(z, y, cw, eps, sums=None, *, no_max=False, c_minus_1=False, no_w_smooth=False, no_div=False):
    """ce_terms_window / ce_grad_window in numpy float32 (the kernels' loops, sums in class order), optional planted defects."""
    n, Cc = z.shape
    w = np.ones(Cc, F32) if cw is None else cw.astype(F32)
    ws = np.ones(Cc, F32) if no_w_smooth else w
    eps = F32(eps)
    ec = eps / F32(Cc - 1 if c_minus_1 else Cc)
    rows = np.arange(n)
    with np.errstate(over="ignore", invalid="ignore"):
        mx = np.zeros((n, 1), F32) if no_max else z.max(1, keepdims=True)
        ex = np.exp((z - mx).astype(F32)).astype(F32)
        den = np.zeros(n, F32)
        for c in range(Cc):
            den = den + ex[:, c]
        wy = w[y]
        if sums is None:
            lse = mx[:, 0] + np.log(den).astype(F32)
            sm = np.zeros(n, F32)
            for c in range(Cc):
                sm = sm + ws[c] * (lse - z[:, c])
            return np.stack([(F32(1.0) - eps) * wy * (lse - z[rows, y]) + ec * sm, wy], 1)
        wsum = F32(0.0)
        for c in range(Cc):
            wsum = wsum + ws[c]
        p = ex / den[:, None]
        oh = np.zeros_like(p)
        oh[rows, y] = 1.0
        inv = F32(1.0) if no_div else F32(1.0) / F32(sums[1])
        return (((F32(1.0) - eps) * wy[:, None] * (p - oh) + ec * (p * wsum - ws[None, :])) * inv).astype(F32)


@pytest.mark.parametrize("Cc", [2, 9, 12, 64])
def test_cross_entropy_bounds_accept_the_simulated_kernels_and_reject_planted_defects(Cc):
    for n in (1, 129):
        for with_cw in (False, True):
            for eps in (0.0, 0.1):
                z, y, cw = R.ce_case(n, Cc, 100 * n + Cc, with_cw)
                ref, bound = R.ce_terms_ref(z, y, cw, eps)
                sums = ref.sum(0).astype(F32) * F32(3.0)                      # not 1: the division shows
                gref, gbound = R.ce_grad_ref(z, y, cw, eps, sums)
                assert R.ratio(_sim_ce(z, y, cw, eps)[:, 0], ref[:, 0], bound[:, 0]) <= 1.0
                assert R.ratio(_sim_ce(z, y, cw, eps, sums), gref, gbound) <= 1.0
                defects = [dict(no_div=True)] + ([dict(no_max=True)] if n > 3 else [])      # row 3 (+-100) shows it: see ce_case
                if eps:
                    defects.append(dict(c_minus_1=True))
                    if with_cw:
                        defects.append(dict(no_w_smooth=True))
                for d in defects:
                    if "no_div" not in d:
                        assert R.ratio(_sim_ce(z, y, cw, eps, **d)[:, 0], ref[:, 0], bound[:, 0]) > 1.0, ("terms", d)
                    assert R.ratio(_sim_ce(z, y, cw, eps, sums, **d), gref, gbound) > 1.0, ("grad", d)


def _sim_gelu_dropout(z, d, key, thr, scale, *, backward, strict=False, offset=0, no_mask=False):
    keep = R.dropout_keep_mask(key, z.size, thr + (1 if strict else 0), offset)          # hash > thr <=> hash >= thr + 1
    ds = np.where(keep | no_mask, F32(scale), F32(0.0)).astype(F32)
    if backward:
        return ((d * ds) * R.gelu_grad64(z).astype(F32)).astype(F32)
    return (_f32_gelu(z) * ds).astype(F32)


def _gelu_passes(z, d, key, thr, scale, backward, **kw):
    out = _sim_gelu_dropout(z, d, key, thr, scale, backward=backward, **kw)
    ref, bound, keep = (R.gelu_dropout_bwd_ref(z, d, key, thr, scale) if backward else R.gelu_dropout_fwd_ref(z, key, thr, scale))
    return bool((out[~keep] == 0).all()) and R.ratio(out[keep], ref[keep], bound[keep]) <= 1.0


@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
def test_gelu_dropout_reference_accepts_the_simulated_kernel_and_rejects_planted_defects(backward):
    for n in (1, 255, 256, 257, 5000):
        for thr in (0, int(0.1 * 2 ** 24), 2 ** 24 - 1):
            for which in (0, 1):
                z, d, key, scale = R.gelu_case(n, thr, which)
                assert _gelu_passes(z, d, key, thr, scale, backward)
                assert not _gelu_passes(z, d, key, thr, scale, backward, strict=True), ("> thr", n, thr, which)
                if n >= 255 and thr == int(0.1 * 2 ** 24):
                    assert not _gelu_passes(z, d, key, thr, scale, backward, offset=1), ("index + 1", n, which)
                if backward and not R.dropout_keep_mask(key, n, thr).all():
                    assert not _gelu_passes(z, d, key, thr, scale, backward, no_mask=True), ("no mask", n, thr, which)


def test_mix64_is_the_training_oracles_hash():
    from oracle.head_train_oracle import _mix64
    z = np.random.default_rng(0).integers(0, 2 ** 64, 4096, dtype=np.uint64)
    z[:3] = [0, 1, 2 ** 64 - 1]
    assert np.array_equal(R.mix64(z), _mix64(z))
    assert all(int(R.mix64(np.array([R.mix64_inverse(int(h))], np.uint64))[0]) == int(h) for h in z[:64])


ADAM_DEFECTS = ["closed range", "open range", "range shifted", "wd swapped", "no decay", "step1 corrections", "eps in sqrt"]


def _adam_defect(d, ins, lr, wd, lo, hi, wds, step):
    """The float64 Adam step with one planted defect: a wrong decay range / factor or stale corrections go in through
    adam_ref_core's inputs; eps inside the square root is its own arithmetic."""
    n = ins[0].size
    dlo, dhi = {"closed range": (lo, hi + 1), "open range": (lo + 1, hi), "range shifted": (lo + 1, hi + 1)}.get(d, (lo, hi))
    a, b = {"wd swapped": (wds, wd), "no decay": (0.0, 0.0)}.get(d, (wd, wds))
    wdv = R.adam_decay(n, a, dlo, dhi, b)
    lr_c1, c2 = R.adam_corrections(lr, 1 if d == "step1 corrections" else step)
    if d != "eps in sqrt":
        return R.adam_ref_core(*ins, lr_c1, c2, wdv)[0]
    p, g, m, v = (t.astype(np.float64) for t in ins)
    b1, b2, eps = float(F32(0.9)), float(F32(0.999)), float(F32(1e-8))
    gi = g + wdv * p
    mi = b1 * m + float(F32(1.0) - F32(0.9)) * gi
    vi = b2 * v + float(F32(1.0) - F32(0.999)) * gi * gi
    return p - float(lr_c1) * mi / (np.sqrt(vi + eps) * float(c2)), mi, vi


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_adam_bounds_accept_the_simulated_kernel_and_reject_planted_defects(n):
    ins = R.adam_case(n, n)
    caught = set()
    for step in (1, 2, 1000):
        for lo, hi in [(0, 0), (0, 1), (255, 257), (n - 1, n)]:
            for wd in (0.0, 1e-2):
                args = (1e-3, wd, lo, hi, 1e-3, step)
                ref, E = R.adam_ref(*ins, *args)
                sim = R.adam_f32(*ins, *args)
                assert all(R.ratio(s, r, e) <= 1.0 for s, r, e in zip(sim, ref, E)), (n, step, lo, hi, wd)
                for d in ADAM_DEFECTS:
                    bad = _adam_defect(d, ins, *args)
                    out = max(R.ratio(b, r, e) for b, r, e in zip(bad, ref, E))
                    # a defect must show wherever it changes the arithmetic at all: which elements decay and by how much,
                    # the corrections (equal at step 1), eps's place (always)
                    i = np.arange(n)
                    dlo, dhi = {"closed range": (lo, hi + 1), "open range": (lo + 1, hi), "range shifted": (lo + 1, hi + 1)}.get(d, (lo, hi))
                    changes = {"wd swapped": True, "no decay": wd > 0 or lo < min(hi, n), "step1 corrections": step > 1,
                               "eps in sqrt": n > 3}.get(d,      # the quiet elements (adam_case) show eps's place
                                                         bool((((i >= lo) & (i < hi)) != ((i >= dlo) & (i < dhi))).any()))
                    assert (out > 1.0) == changes, (d, n, step, lo, hi, wd, out)
                    if out > 1.0:
                        caught.add(d)
    assert caught == set(ADAM_DEFECTS) - ({"eps in sqrt"} if n <= 3 else set())


# ---- classifier head: LSTM, BPTT, attention pooling, centre (tests/test_gpu_head_seq_reference.py) ---------------------------
F32 = np.float32


def _sig32(x):
    with np.errstate(over="ignore"):
        return (F32(1) / (F32(1) + np.exp(-x, dtype=F32))).astype(F32)


def _emu_lstm(gin, W, lo=None, hi=None, defect=None):
    """fp32 numpy emulation of the LSTM forward kernels (sum order and tanh form differ from the device's within the bounds).
    Returns act, cst, hout [w][T][..] of the full run; with (lo, hi) also the inference kernel's truncated output.  defect: one
    planted mistake."""
    gin = np.asarray(gin, F32)
    W = np.asarray(W, F32)
    nw, T, G8 = gin.shape
    H = G8 // 8
    if defect == "swap_dirs":
        W = W[::-1]
    if defect == "window_15_for_16" and nw > 16:
        gin = gin.copy()
        gin[16] = gin[15]
    act = np.zeros((nw, T, 8 * H), F32)
    cst = np.zeros((nw, T, 2 * H), F32)
    hout = np.zeros((nw, T, 2 * H), F32)
    for d in range(2):
        hp = np.zeros((nw, H), F32)
        c = np.zeros((nw, H), F32)
        for s in range(T):
            t = T - 1 - s if d else s
            pre = (gin[:, t, d * 4 * H:(d + 1) * 4 * H] + hp @ W[d].T).astype(F32)
            a = _sig32(pre)
            gg, oo = (3, 2) if defect == "swap_g_o" else (2, 3)
            a[:, gg * H:(gg + 1) * H] = np.tanh(pre[:, gg * H:(gg + 1) * H], dtype=F32)
            if defect == "c_not_carried" and s == 1:
                c = np.zeros_like(c)
            c = (a[:, H:2 * H] * c + a[:, :H] * a[:, gg * H:(gg + 1) * H]).astype(F32)
            hp = (a[:, oo * H:(oo + 1) * H] * np.tanh(c, dtype=F32)).astype(F32)
            ts = T - 1 - t if (defect == "reverse_stored_mirrored" and d) else t
            act[:, ts, d * 4 * H:(d + 1) * 4 * H] = a
            cst[:, ts, d * H:(d + 1) * H] = c
            hout[:, ts, d * H:(d + 1) * H] = hp
    if lo is None:
        return act, cst, hout
    out = hout[:, lo:hi].copy()
    if defect == "reverse_lo_off_by_one":          # the reverse direction stops one step early and indexes its rows from lo + 1
        out[:, :, H:] = 0
        out[:, :hi - lo - 1, H:] = hout[:, lo + 1:hi, H:]
    return act, cst, hout, out


LSTM_FWD_DEFECTS = ("swap_g_o", "swap_dirs", "reverse_stored_mirrored", "c_not_carried", "window_15_for_16")


def test_lstm_suite_covers_every_value_with_two_hidden_sizes_and_stays_conditioned():
    """Coverage of the covering set, and the conditioning the issue asks for: at every case the propagated bound (doubled) at
    any step is at most 64 x the largest one-step bound, forward (both kinds) and BPTT."""
    cases = R.lstm_suite_cases()
    assert len(cases) == 40
    for idx, values in ((0, R.LSTM_H), (1, R.LSTM_NW_INFER), (2, R.LSTM_NW_TRAIN), (3, R.LSTM_T), (4, R.RANGE_KINDS)):
        for v in values:
            assert len({c[0] for c in cases if c[idx] == v}) >= (1 if idx == 0 else 2), (idx, v)
    worst = 0.0
    for (h, nwi, nwt, T, kind, lo, hi) in cases:
        gin, W = R.lstm_case(nwt, T, h, 7 * h + T)
        assert np.abs(W).sum(2).max() <= 0.5 and np.abs(gin).max() <= 3.0 and T <= 31
        for k in ("infer", "train"):
            r = R.lstm_fwd_ref(gin, W, k)
            worst = max(worst, r["E_h"].max() / r["S_h"].max(), r["E_c"].max() / r["S_c"].max())
        dh = np.random.default_rng(h + T).standard_normal(r["h"].shape).astype(F32)
        _, _, E, S = R.lstm_bwd_ref(dh, r["act"].astype(F32), r["c"].astype(F32), r["h"].astype(F32), W)
        worst = max(worst, E.max() / S.max())
    print(f"[lstm conditioning] propagated / one-step bound, worst {worst:.2f} (limit 64)")
    assert worst <= 64.0


def _torch_lstm(gin, W, dh):
    """torch.nn.LSTM (float64, bidirectional) fed the precomputed gate inputs through identity input weights: output and the
    gradient of sum(dh * output) with respect to gin."""
    import torch
    nw, T, G8 = gin.shape
    H = G8 // 8
    m = torch.nn.LSTM(8 * H, H, batch_first=True, bidirectional=True).double()
    eye = torch.eye(4 * H, dtype=torch.float64)
    zero = torch.zeros(4 * H, 4 * H, dtype=torch.float64)
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.cat([eye, zero], 1))
        m.weight_ih_l0_reverse.copy_(torch.cat([zero, eye], 1))
        m.weight_hh_l0.copy_(torch.from_numpy(W[0].astype(np.float64)))
        m.weight_hh_l0_reverse.copy_(torch.from_numpy(W[1].astype(np.float64)))
        for b in (m.bias_ih_l0, m.bias_hh_l0, m.bias_ih_l0_reverse, m.bias_hh_l0_reverse):
            b.zero_()
    x = torch.from_numpy(gin.astype(np.float64)).requires_grad_(True)
    y, _ = m(x)
    (y * torch.from_numpy(dh)).sum().backward()
    return y.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize("h,T,nw", [(16, 1, 1), (16, 7, 3), (48, 31, 2), (128, 3, 1)])
def test_lstm_references_agree_with_torch_autograd_in_float64(h, T, nw):
    gin, W = R.lstm_case(nw, T, h, h + T)
    r = R.lstm_fwd_ref(gin, W, "train")
    dh = np.random.default_rng(T).standard_normal((nw, T, 2 * h))
    y, dgin_t = _torch_lstm(gin, W, dh)
    assert np.abs(r["h"] - y).max() <= 1e-12 * np.abs(y).max()
    dgin, hprev, _, _ = R.lstm_bwd_ref(dh, r["act"], r["c"], r["h"], W)          # float64 images: nothing is rounded
    assert np.abs(dgin - dgin_t).max() <= 1e-12 * np.abs(dgin_t).max(), np.abs(dgin - dgin_t).max()
    assert (hprev[:, 0, :h] == 0).all() and (hprev[:, T - 1, h:] == 0).all()
    if T > 1:
        assert np.array_equal(hprev[:, 1:, :h], r["h"][:, :-1, :h]) and np.array_equal(hprev[:, :-1, h:], r["h"][:, 1:, h:])


def test_lstm_forward_bounds_accept_the_emulation_and_reject_planted_defects():
    """At the suite's own shapes: the correct fp32 emulation lies within the free-running bound (inference rows [lo, hi)) and
    the teacher-forced one-step bound (training forward); each planted defect leaves it at a case that can show it."""
    worst = 0.0
    caught = {d: 0 for d in LSTM_FWD_DEFECTS + ("reverse_lo_off_by_one",)}
    for (h, nwi, nwt, T, kind, lo, hi) in R.lstm_suite_cases():
        gin, W = R.lstm_case(nwi, T, h, 7 * h + T + nwi)
        ref, E, _ = R.lstm_infer_ref(gin, W, lo, hi)
        act, cst, hout, out = _emu_lstm(gin, W, lo, hi)
        worst = max(worst, R.ratio(out, ref, E))
        tf = R.lstm_train_fwd_teacher_ref(gin, W, cst, hout)
        worst = max(worst, R.ratio(act, tf["act"], tf["S_act"]), R.ratio(cst, tf["c"], tf["S_c"]), R.ratio(hout, tf["h"], tf["S_h"]))
        for d in caught:
            shows = {"c_not_carried": T >= 2, "swap_dirs": T >= 2, "reverse_stored_mirrored": T >= 2, "window_15_for_16": nwi > 16}.get(d, True)
            if not shows:
                continue
            a2, c2, h2, o2 = _emu_lstm(gin, W, lo, hi, defect=d)
            bad = R.ratio(o2, ref, E) > 1.0
            if d not in ("reverse_lo_off_by_one",):
                tf2 = R.lstm_train_fwd_teacher_ref(gin, W, c2, h2)
                bad_t = max(R.ratio(a2, tf2["act"], tf2["S_act"]), R.ratio(c2, tf2["c"], tf2["S_c"]), R.ratio(h2, tf2["h"], tf2["S_h"])) > 1.0
                assert bad_t, (d, h, T)
            # what [lo, hi) observes may hide one: the dropped step lies past it, or the mirror of a single centre row is itself
            if not bad and (d == "c_not_carried" or (d == "reverse_stored_mirrored" and (lo, hi) == (T // 2, T // 2 + 1) and T % 2)):
                continue
            assert bad, (d, h, nwi, T, lo, hi)
            caught[d] += 1
    print(f"[lstm forward emulation] worst error / bound {worst:.3f}; defects caught at {caught} cases")
    assert worst <= 1.0
    assert all(v >= 2 for v in caught.values()), caught


def _emu_bptt(dh, act, cst, hout, W, defect=None):
    dh, act, cst, hout, W = (np.asarray(x, F32) for x in (dh, act, cst, hout, W))
    nw, T, G8 = act.shape
    H = G8 // 8
    dgin = np.zeros_like(act)
    hprev = np.zeros_like(hout)
    one = F32(1)
    for d in range(2):
        dh_rec = np.zeros((nw, H), F32)
        dc_rec = np.zeros((nw, H), F32)
        sl4, sl = slice(d * 4 * H, (d + 1) * 4 * H), slice(d * H, (d + 1) * H)
        for st in range(T - 1, -1, -1):
            t = T - 1 - st if d else st
            tp = t + 1 if d else t - 1
            a = act[:, t, sl4]
            ig, fg, gg, og = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
            c = cst[:, t, sl]
            cp = cst[:, t if defect == "cp_from_t" else tp, sl] if st else np.zeros_like(c)
            hprev[:, t, sl] = hout[:, tp, sl] if st else (hout[:, t, sl] if defect == "hprev_first_not_zero" else 0)
            dhh = dh[:, t, sl] + dh_rec
            tc = np.tanh(c, dtype=F32)
            dc = dc_rec + dhh * og * (one - tc * tc)
            da = np.concatenate([dc * gg * ig * (one - ig), dc * cp * fg * (one - fg), dc * ig * (one - gg * gg), dhh * tc * og * (one - og)], 1).astype(F32)
            dc_rec = dc if defect == "dc_rec_without_f" else dc * fg
            dgin[:, t, sl4] = da
            dh_rec = (da @ W[d]).astype(F32)
    return dgin, hprev


def test_bptt_bounds_accept_the_emulation_and_reject_planted_defects():
    worst = 0.0
    caught = {"dc_rec_without_f": 0, "cp_from_t": 0, "hprev_first_not_zero": 0}
    for (h, nwi, nwt, T, kind, lo, hi) in R.lstm_suite_cases():
        gin, W = R.lstm_case(nwt, T, h, 11 * h + T)
        r = R.lstm_fwd_ref(gin, W, "train")
        act, cst, hout = (r[k].astype(F32) for k in ("act", "c", "h"))
        dh = np.random.default_rng(h * T).standard_normal(hout.shape).astype(F32)
        dgin, hprev, E, _ = R.lstm_bwd_ref(dh, act, cst, hout, W)
        g, hp = _emu_bptt(dh, act, cst, hout, W)
        worst = max(worst, R.ratio(g, dgin, E))
        assert np.array_equal(hp.view(np.uint32), hprev.astype(F32).view(np.uint32))
        for d in caught:
            g2, hp2 = _emu_bptt(dh, act, cst, hout, W, defect=d)
            if d == "hprev_first_not_zero":
                assert not np.array_equal(hp2.view(np.uint32), hprev.astype(F32).view(np.uint32)), (d, h, T)
            elif T >= 2:                      # both recurrences need a second step to show ("at small T": T = 2 is in the suite)
                assert R.ratio(g2, dgin, E) > 1.0, (d, h, T)
            else:
                continue
            caught[d] += 1
    print(f"[bptt emulation] worst error / bound {worst:.3f}; defects caught at {caught} cases")
    assert worst <= 1.0 and all(v >= 8 for v in caught.values())


# pooling: the GPU suite's shapes (H2, C, nc, T, raw att_temp) - tests/test_gpu_head_seq_reference.py imports them from here
def _emu_pool_fwd(hout, lin, wa, b_att, raw_temp, W2, b2, raw_gate, lo, hi, *, max_over_T=False, dead_threads=False):
    hout, lin, wa, W2, b2 = (np.asarray(x, F32) for x in (hout, lin, wa, W2, b2))
    nw, T, H2 = hout.shape
    raw = F32(raw_temp)
    temp = (raw if raw > 20 else np.log1p(np.exp(raw, dtype=F32), dtype=F32)) + F32(1e-3)
    flat = hout.reshape(nw, -1)
    block = -(-H2 // 64) * 64

    def score(t):
        s = hout[:, t] @ wa
        if dead_threads and block > H2:           # threads u >= 2h add hout[.. u]: the next row's first columns (w_att taken as 1)
            idx = t * H2 + np.arange(H2, block)
            s = s + flat[:, np.minimum(idx, flat.shape[1] - 1)].sum(1)
        return ((s + F32(b_att)) / temp).astype(F32)

    sc = np.stack([score(t) for t in range(lo, hi)], 1)
    with np.errstate(all="ignore"):
        mx = (np.stack([score(t) for t in range(T)], 1) if max_over_T else sc).max(1, keepdims=True)
        e = np.exp(sc - mx, dtype=F32)
        aw = (e / e.sum(1, keepdims=True)).astype(F32)
    lat = np.einsum("wt,wtu->wu", aw, hout[:, lo:hi]).astype(F32)
    lstm = (lat @ W2.T + b2).astype(F32)
    g = _sig32(F32(raw_gate))
    return aw, sc, lat, lstm, (lin + g * (lstm - lin)).astype(F32)


def test_pool_train_forward_bound_accepts_the_emulation_and_rejects_planted_defects():
    worst = 0.0
    for (H2, C, nc, raw) in R.POOL_TRAIN_CASES:
        c = R.pool_case(3, H2, C, nc, H2 + C + nc, train=True, temp=R.softplus_temp_ref(raw)[0])
        ref, E = R.pool_train_fwd_ref(c["hout"], c["lin"], c["w_att"], c["b_att"], raw, c["w_lin2"], c["b_lin2"], c["gate"], c["lo"], c["hi"])
        args = (c["hout"], c["lin"], c["w_att"], c["b_att"], raw, c["w_lin2"], c["b_lin2"], c["gate"], c["lo"], c["hi"])
        got = _emu_pool_fwd(*args)
        for name, y, r_, e_ in zip(("attw", "scores", "latent", "lstm", "final"), got, ref, E):
            assert abs(ref[0].sum(1) - 1).max() < 1e-12
            rr = R.ratio(y, r_, e_)
            worst = max(worst, rr)
            assert rr <= 1.0, (name, H2, C, nc, raw, rr)
        if H2 % 64:                                # a dead thread's addend reaches the scores
            bad = _emu_pool_fwd(*args, dead_threads=True)
            assert R.ratio(bad[1], ref[1], E[1]) > 1.0, ("dead threads", H2)
        hot = c["hout"].copy()                     # rows outside [lo, hi) score 200 higher: a max over T underflows every weight
        out_rows = np.r_[0:c["lo"], c["hi"]:hot.shape[1]]
        hot[:, out_rows] = (200.0 * float(R.softplus_temp_ref(raw)[0]) * np.sign(c["w_att"]) / np.abs(c["w_att"]).sum()).astype(F32)
        bad = _emu_pool_fwd(hot, *args[1:], max_over_T=True)
        assert R.ratio(bad[0], ref[0], E[0]) > 1.0, ("max over T", H2, nc)
        assert R.ratio(_emu_pool_fwd(hot, *args[1:])[0], ref[0], E[0]) <= 1.0
    print(f"[pool train forward emulation] worst error / bound {worst:.3f}")


def _emu_pool_infer(c, g, temperature, *, ge=False, exchanged=False):
    hout, lin, wa, W2, b2 = (np.asarray(c[k], F32) for k in ("hout_c", "lin", "w_att", "w_lin2", "b_lin2"))
    sc = ((hout @ wa + F32(c["b_att"])) / F32(c["att_temp"])).astype(F32)
    with np.errstate(all="ignore"):
        e = np.exp(sc - sc.max(1, keepdims=True), dtype=F32)
    lat = (np.einsum("wt,wtu->wu", e, hout) / e.sum(1, keepdims=True)).astype(F32)
    lstm = (lat @ W2.T + b2).astype(F32)
    g = F32(g)
    low = (g <= F32(0.5)) if ge else (g < F32(0.5))          # ge: the branch chosen by <= instead of <
    if exchanged:
        low = not low
    fin = (lin + g * (lstm - lin)) if low else (lstm - (lstm - lin) * (F32(1) - g))
    fin = fin.astype(F32)
    z = (fin / max(F32(1e-3), F32(temperature))).astype(F32)
    ez = np.exp(z - z.max(1, keepdims=True), dtype=F32)
    return (ez / ez.sum(1, keepdims=True)).astype(F32), fin, lat


def test_pool_inference_bound_accepts_both_lerp_forms():
    """The two forms of torch.lerp are one value mathematically, and the bound is the larger of the two forms' roundings: the
    emulation passes with the branch chosen by < or by <= at g = 0.5 (must be accepted), and ALSO with the branches' formulas
    exchanged at every g - exchanging them does not leave the bound, so this check cannot see it (stated, as the issue asks)."""
    worst = 0.0
    for (H2, C, nc, nw, g, temperature) in R.POOL_INFER_CASES:
        c = R.pool_case(nw, H2, C, nc, H2 + C + nc + nw, train=False)
        ref, E = R.pool_infer_ref(c["hout_c"], c["lin"], c["w_att"], c["b_att"], c["att_temp"], c["w_lin2"], c["b_lin2"], g, temperature)
        for kw in ({}, {"ge": True}, {"exchanged": True}):
            got = _emu_pool_infer(c, g, temperature, **kw)
            for y, r_, e_ in zip(got, ref, E):
                rr = R.ratio(y, r_, e_)
                worst = max(worst, rr)
                assert rr <= 1.0, (H2, C, nc, nw, g, temperature, kw, rr)
        if C > 1 and temperature >= 1e-3:                                # a wrong divisor is seen
            assert R.ratio(_emu_pool_infer(c, g, temperature * 2)[0], ref[0], E[0]) > 1.0
    print(f"[pool inference emulation] worst error / bound {worst:.3f}")


def _torch_pool(c, raw_temp, dfinal, dlat_cov):
    import torch
    t = lambda x: torch.tensor(np.asarray(x, np.float64), dtype=torch.float64, requires_grad=True)
    hout, lin, wa, W2, b2 = (t(c[k]) for k in ("hout", "lin", "w_att", "w_lin2", "b_lin2"))
    b_att, raw, gate = t([c["b_att"]]), t([float(F32(raw_temp))]), t([c["gate"]])
    lo, hi = c["lo"], c["hi"]
    sp = raw if float(F32(raw_temp)) > 20 else torch.nn.functional.softplus(raw)
    temp = sp + float(F32(1e-3))
    hc = hout[:, lo:hi]
    sc = (hc @ wa + b_att) / temp
    aw = torch.softmax(sc, 1)
    lat = (aw[:, :, None] * hc).sum(1)
    lstm = lat @ W2.T + b2
    fin = torch.lerp(lin, lstm, torch.sigmoid(gate))
    loss = (fin * torch.from_numpy(dfinal)).sum()
    if dlat_cov is not None:
        loss = loss + (lat * torch.from_numpy(dlat_cov)).sum()
    lstm.retain_grad()
    loss.backward()
    return dict(aw=aw, sc=sc, lstm=lstm, dhout=hout.grad, dlstm=lstm.grad, dlin=lin.grad, dwatt=wa.grad, dbatt=b_att.grad, dgate=gate.grad,
                dtemp=raw.grad)


@pytest.mark.parametrize("with_cov", [False, True])
def test_pool_backward_reference_agrees_with_torch_autograd_in_float64(with_cov):
    for (H2, C, nc, raw) in R.POOL_TRAIN_CASES:
        nw = 1                                         # part is per window: one window makes it the parameter gradient
        c = R.pool_case(nw, H2, C, nc, H2 + C + nc, train=True, temp=R.softplus_temp_ref(raw)[0])
        rng = np.random.default_rng(H2 + nc)
        dfinal = rng.standard_normal((nw, C))
        dcov = rng.standard_normal((nw, H2)) if with_cov else None
        tt = _torch_pool(c, raw, dfinal, dcov)
        n = lambda x: x.detach().numpy()
        (dh, dl, dlin, part), _ = R.pool_train_bwd_ref(c["hout"], c["lin"], c["w_att"], raw, c["w_lin2"], c["gate"], c["lo"], c["hi"], n(tt["aw"]),
                                                       n(tt["sc"]), n(tt["lstm"]), dfinal, dcov)
        close = lambda a, b, scale=None: np.abs(a - n(b)).max() <= 1e-12 * (scale or max(np.abs(n(b)).max(), 1e-300))
        assert close(dh, tt["dhout"]) and close(dl, tt["dlstm"]) and close(dlin, tt["dlin"]), (H2, C, nc, raw)
        # d b_att = sum_t q_t is identically zero (a softmax ignores a shift of its scores): what is left is rounding, measured
        # against sum_t |q_t| >= |sum_t q_t h_tu| = |d w_att[u]| (|h| <= 1)
        assert close(part[0, :H2], tt["dwatt"]) and close(part[0, H2:H2 + 1], tt["dbatt"], np.abs(part[0, :H2]).max()), (H2, C, nc, raw)
        assert close(part[0, H2 + 4:H2 + 5], tt["dgate"]) and close(part[0, H2 + 8:H2 + 9], tt["dtemp"]), (H2, C, nc, raw)
        assert (dh[:, :c["lo"]] == 0).all() and (dh[:, c["hi"]:] == 0).all()
        assert (part[0, [H2 + i for i in (1, 2, 3, 5, 6, 7, 9, 10, 11)]] == 0).all()
        (aw, sc, lat, lstm, fin), _ = R.pool_train_fwd_ref(c["hout"], c["lin"], c["w_att"], c["b_att"], raw, c["w_lin2"], c["b_lin2"], c["gate"],
                                                          c["lo"], c["hi"])
        assert close(aw, tt["aw"]) and close(sc, tt["sc"]) and close(lstm, tt["lstm"])


def test_pool_backward_bound_rejects_a_missing_softplus_factor():
    """d att_temp without softplus' factor: seen where the factor is not 1 (raw <= 20); at raw = 25 the kernel's switch makes the
    factor exactly 1 and the two agree; a single step (hi - lo = 1) has no temperature gradient at all."""
    for (H2, C, nc, raw) in R.POOL_TRAIN_CASES:
        c = R.pool_case(3, H2, C, nc, H2 + C + nc, train=True, temp=R.softplus_temp_ref(raw)[0])
        fw, _ = R.pool_train_fwd_ref(c["hout"], c["lin"], c["w_att"], c["b_att"], raw, c["w_lin2"], c["b_lin2"], c["gate"], c["lo"], c["hi"])
        aw, sc, _, lstm, _ = (x.astype(F32) for x in fw)
        df = np.random.default_rng(C).standard_normal((3, C)).astype(F32)
        (_, _, _, part), (_, _, _, E) = R.pool_train_bwd_ref(c["hout"], c["lin"], c["w_att"], raw, c["w_lin2"], c["gate"], c["lo"], c["hi"], aw, sc,
                                                             lstm, df, None)
        col = H2 + 8
        wrong = part[:, col] / R.softplus_temp_ref(raw)[1]
        assert (R.ratio(wrong.astype(F32), part[:, col], E[:, col]) > 1.0) == (raw <= 20 and nc > 1), (H2, nc, raw)
        assert R.ratio(part[:, col].astype(F32), part[:, col], E[:, col] + R.U32 * np.abs(part[:, col])) <= 1.0


def test_centre_reference():
    x = np.random.default_rng(0).standard_normal((2, 31, 260)).astype(F32) + F32(3)
    y, E = R.centre_ref(x)
    assert np.abs(y.mean(1)).max() < 1e-12
    got = (x - (x.sum(1, keepdims=True, dtype=F32) / F32(31))).astype(F32)
    assert R.ratio(got, y, E) <= 1.0
    assert R.ratio(x, y, E) > 1.0                     # the mean not subtracted


# ---- classifier head: the expand kernels (tests/test_gpu_head_expand_reference.py) ---------------------------------------------
EXP_ALPHA, EXP_SLIDING = R.EXPAND_ALPHA, R.EXPAND_SLIDING


def _f64sum32(x, axis):
    return np.sum(x, axis=axis, keepdims=True, dtype=F32)


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _ln32(u, g, b, Bn, defect):
    """Two-pass fp32 LayerNorm of rows [..][Bn] (numpy's pairwise sums stand in for the lane partials and the butterfly)."""
    div = F32(3 * Bn) if defect == "mean_over_F" else F32(Bn)
    mean = (_f64sum32(u, -1) / div).astype(F32)
    dv = (u - mean).astype(F32)
    q = _f64sum32((dv * dv).astype(F32), -1)
    eps = F32(0) if defect == "no_eps" else F32(R.EXPAND_EPS)
    with np.errstate(divide="ignore"):
        rstd = (F32(1) / np.sqrt(((q / F32(Bn)).astype(F32) + eps).astype(F32))).astype(F32)
    return mean, rstd, ((((dv * rstd).astype(F32) * g).astype(F32)) + b).astype(F32)


def _ema32(x, alpha, contract):
    al = F32(alpha)
    s = np.empty_like(x)
    s[:, 0] = x[:, 0]
    for t in range(1, x.shape[1]):
        d = (x[:, t] - s[:, t - 1]).astype(F32)
        s[:, t] = _fma32(al, d, s[:, t - 1]) if contract else (s[:, t - 1] + (al * d).astype(F32)).astype(F32)
    return s


def _emu_expand_infer(img, p, Bn, NS, C, lo, hi, nw, T, contract, sliding=None, defect=None):
    """fp32 emulation of head_expand_kernel on the proj image [rows][NPROJ]; sliding = (w0, r0, n_frames).  A row the defective
    row map takes from outside the image reads as 0."""
    F_ = NS * Bn
    if sliding is None:
        rows = R.expand_rows(nw, T, False)
    else:
        w0, r0, nf = sliding
        f = w0 + np.arange(nw)[:, None] + np.arange(T)[None, :] - T // 2
        f = np.clip(f, -10 ** 9 if defect == "no_clamp_first" else 0, 10 ** 9 if defect == "no_clamp_last" else nf - 1)
        rows = f - r0
    ok = (rows >= 0) & (rows < img.shape[0])
    X = np.where(ok[:, :, None], img[np.clip(rows, 0, img.shape[0] - 1)], F32(0)).astype(F32)
    s = _ema32(X[:, :, :F_], EXP_ALPHA, contract)
    i1, i2 = np.abs(np.arange(T) - 1), np.abs(np.arange(T) - 2)
    if defect == "reflect_t0":
        i1 = i1.copy(); i1[0] = 0                            # replicate: s_{-1} = s_0
    if defect == "reflect_t1":
        i2 = i2.copy(); i2[1] = 0                            # s_{-1} = s_0 again
    if defect == "reflect_t2":
        i2 = i2.copy(); i2[2] = 1                            # the padding's mirror applied where the interior stencil belongs
    b, c = s[:, i1], s[:, i2]
    d1 = (s - b).astype(F32)
    d2 = (d1 - (b - c).astype(F32)).astype(F32)
    k = (np.arange(F_) // Bn)[None, None, :]
    v = np.where(k == 0, s, np.where(k == 1, d1, d2))
    g = R.gelu64((v + p["b_bott"]).astype(F32)).astype(F32).reshape(nw, T, NS, Bn)
    aug = _ln32(g, p["ln_w"].reshape(NS, Bn), p["ln_b"].reshape(NS, Bn), Bn, defect)[2].reshape(nw, T, F_)
    sl = _ema32(X[:, :, F_:F_ + C], EXP_ALPHA, contract)
    a, z = (lo, hi + 1) if defect == "mean_lo_hi_inclusive" else ((0, T) if defect == "mean_0_T" else (lo, hi))
    acc = np.zeros((nw, C), F32)
    for t in range(a, z):
        acc = (acc + sl[:, t]).astype(F32)
    return aug, ((acc / F32(z - a)).astype(F32) + p["b_lin1"]).astype(F32)


def _emu_keep(keys, nw, T, Bn, NS, thr, defect):
    if defect == "keys_permuted":
        keys = [keys[1], keys[0], keys[2]]
    if defect == "drop_idx_F":                               # the index taken in the fused F-wide row
        F_ = NS * Bn
        idx = (np.arange(nw * T, dtype=np.uint64)[:, None] * np.uint64(F_) + np.arange(F_, dtype=np.uint64)[None, :]).reshape(nw, T, NS, Bn)
        with np.errstate(over="ignore"):
            return np.stack([(R.mix64(np.uint64(keys[k]) + idx[:, :, k]) >> np.uint64(40)).astype(np.int64) >= thr for k in range(NS)], 2)
    return R.expand_keep_mask(keys, nw, T, Bn, NS, thr)


def _emu_expand_train_fwd(Y, p, Bn, NS, defect=None):
    """fp32 emulation of train_expand_fwd_kernel after its (bit-exact) fmaf chain: GELU, dropout, LayerNorm."""
    nw, T, F_ = Y.shape
    keep = _emu_keep(p["keys"], nw, T, Bn, NS, p["thr"], defect)
    u = (R.gelu64(Y).astype(F32).reshape(nw, T, NS, Bn) * np.where(keep, F32(p["scale"]), F32(0))).astype(F32)
    return _ln32(u, p["ln_w"].reshape(NS, Bn), p["ln_b"].reshape(NS, Bn), Bn, defect)[2].reshape(nw, T, F_)


def _emu_expand_train_bwd(Y, p, tm, lv, Bn, NS, C, defect=None):
    """fp32 emulation of train_expand_bwd_kernel (numpy's sums stand in for the kernel's orders)."""
    nw, T, F_ = Y.shape
    NP = p["NPROJ"]
    keep = _emu_keep(p["keys"], nw, T, Bn, NS, p["thr"], defect)
    ds = np.where(keep, F32(p["scale"]), F32(0))
    y = Y.reshape(nw, T, NS, Bn)
    u = (R.gelu64(y).astype(F32) * ds).astype(F32)
    gam = p["ln_w"].reshape(NS, Bn)
    dy = p["daug"].reshape(nw, T, NS, Bn)
    mean, rstd, xh = _ln32(u, F32(1), F32(0), Bn, defect)
    dxh = (dy * gam).astype(F32)
    s1 = (_f64sum32(dxh, -1) / F32(Bn)).astype(F32)
    s2 = (_f64sum32((dxh * xh).astype(F32), -1) / F32(Bn)).astype(F32)
    if defect == "st_slots":                                 # streams 0 and 1 read each other's row statistics
        sw = [1, 0, 2][:NS]
        mean, rstd, s1, s2 = (a[:, :, sw] for a in (mean, rstd, s1, s2))
        xh = ((u - mean).astype(F32) * rstd).astype(F32)
    du = (rstd * ((dxh - s1).astype(F32) - (xh * s2).astype(F32)).astype(F32)).astype(F32)
    dyv = ((du * ds).astype(F32) * R.gelu_grad64(y).astype(F32)).astype(F32)
    dgam, dbet = (dy * xh).astype(F32).sum(1, dtype=F32), dy.sum(1, dtype=F32)
    if defect == "dgam_dbet":
        dgam, dbet = dbet, dgam
    part = np.concatenate([dyv.sum(1, dtype=F32).reshape(nw, F_), dgam.reshape(nw, F_), dbet.reshape(nw, F_)], 1)
    dproj = np.zeros((nw, T, NP), F32)
    dproj[:, :, :F_] = np.einsum("kts,wtkc->wskc", tm.reshape(3, T, T)[:NS], dyv).astype(F32).reshape(nw, T, F_)
    dproj[:, :, F_:F_ + C] = (lv[None, :, None] * p["dlin"][:, None, :]).astype(F32)
    return dproj, part


_expand_infer_case, _expand_train_case = R.expand_infer_suite_case, R.expand_train_suite_case


def test_expand_suites_cover_every_value_and_both_storage_forms():
    ic, tc = R.expand_infer_cases(), R.expand_train_cases()
    for bn_ns in R.EXPAND_BN_NS:
        mine = [c for c in ic if c[:2] == bn_ns]
        assert {c[2] for c in mine} >= set(R.EXPAND_INFER_T) and {c[3] for c in mine} >= set(R.EXPAND_INFER_C)
        assert {c[4] for c in mine} >= set(R.RANGE_KINDS) and {c[7] for c in mine} >= set(R.EXPAND_NW)
        mine = [c for c in tc if c[:2] == bn_ns]
        assert {c[2] for c in mine} >= set(R.EXPAND_TRAIN_T) and {c[3] for c in mine} >= set(R.EXPAND_TRAIN_C) and {c[4] for c in mine} == {0, R.EXPAND_THR_HALF}
        assert {R.round_up(c[0] * c[1] + c[3], 4) - c[0] * c[1] - c[3] for c in tc} == {0, 1, 2, 3}          # padding columns
    assert (64, 2, 15, 64) in {c[:4] for c in ic} and (64, 2, 15, 64) in {c[:4] for c in tc}
    lo_T, hi_T = R.expand_big_threshold(256, 3, 4)
    NP = R.round_up(3 * 256 + 4, 4)
    assert NP == 772 and not R.expand_is_big(lo_T, 256, NP) and R.expand_is_big(hi_T, 256, NP) and hi_T == lo_T + 1
    assert R.expand_lds_bytes(lo_T, 256, NP, True, False) <= 160 * 1024 < R.expand_lds_bytes(hi_T, 256, NP, True, False)
    assert {(256, 3, lo_T, 4), (256, 3, hi_T, 4)} <= {c[:4] for c in tc} and (256, 3, hi_T, 4) in {c[:4] for c in ic}
    big64 = [c for c in tc if c[0] == 64 and R.expand_is_big(c[2], 64, R.round_up(c[0] * c[1] + c[3], 4))]
    assert big64 and big64[0][2] == R.EXPAND_T_MAX and R.expand_lds_bytes(R.EXPAND_T_MAX, 64, 196, True, True) <= 160 * 1024
    for c in tc:                                             # every training case is served: its LDS need fits
        NPc = R.round_up(c[0] * c[1] + c[3], 4)
        big = R.expand_is_big(c[2], c[0], NPc)
        assert max(R.expand_lds_bytes(c[2], c[0], NPc, True, big), R.expand_lds_bytes(c[2], c[0], NPc, False, big)) <= 160 * 1024


def test_ln_stats_ref_restates_ln_ref():
    rng = np.random.default_rng(5)
    x, ex = rng.standard_normal((7, 128)), np.abs(rng.standard_normal((7, 128))) * 1e-6
    y, E = R.ln_ref(x, 1.0, 0.0, 1e-5, ex)
    st = R.ln_stats_ref(x, 1e-5, ex)
    ac = np.abs(st["c"])
    E2 = st["rstd"] * ((1 + st["rel"]) * (st["K"] + st["r"]) + ac * st["rel"])
    E2 = E2 + 2 * R.U32 * (np.abs(st["c"] * st["rstd"]) + E2) + R.U32 * (np.abs(y) + E2)
    assert np.array_equal(y, st["c"] * st["rstd"]) and np.allclose(E, E2, rtol=1e-12, atol=0)


def test_expand_temporal_ref_is_the_models_padding_and_differences():
    """x_smooth, dx[:, 1:], ddx of _calculate_robust_deltas (torch, float64, the model's own pad / slice / lerp calls) on the
    identity: its columns are the operators' columns."""
    import torch
    for T in (3, 4, 15):
        a = float(F32(EXP_ALPHA))
        x = torch.eye(T, dtype=torch.float64)[None]
        xs = torch.zeros_like(x)
        xs[:, 0] = x[:, 0]
        for t in range(1, T):
            xs[:, t] = torch.lerp(xs[:, t - 1], x[:, t], a)
        padded = torch.nn.functional.pad(xs.permute(0, 2, 1), (2, 0), "reflect").permute(0, 2, 1)
        dx = padded[:, 1:] - padded[:, :-1]
        ddx = dx[:, 1:] - dx[:, :-1]
        lo, hi = R.centre_range("centre3", T)
        E, D, A, lv = R.expand_temporal_ref(T, EXP_ALPHA, lo, hi)
        for got, want in ((E, xs[0]), (D, dx[0, 1:]), (A, ddx[0]), (lv, xs[0, lo:hi].mean(0))):
            assert np.abs(got - want.numpy()).max() <= 1e-15


def _torch_model(P, p, Bn, NS, C, lo, hi, mask):
    """A direct transcription of ClassifierLSTMDeltas.forward up to x_augmented and linear_logits on projected rows, float64."""
    import torch
    Fn = torch.nn.functional
    F_ = NS * Bn
    a = float(F32(EXP_ALPHA))
    x = P[:, :, :F_ + C]
    xs = [x[:, 0]]
    for t in range(1, x.shape[1]):
        xs.append(torch.lerp(xs[-1], x[:, t], a))
    xs = torch.stack(xs, 1)
    padded = Fn.pad(xs.permute(0, 2, 1), (2, 0), "reflect").permute(0, 2, 1)
    dx = padded[:, 1:] - padded[:, :-1]
    ddx = dx[:, 1:] - dx[:, :-1]
    outs, pre = [], []
    for k, st in enumerate((xs, dx[:, 1:], ddx)[:NS]):
        sl = slice(k * Bn, (k + 1) * Bn)
        v = st[:, :, sl] + p["b_bott"][sl]
        pre.append(v)
        outs.append(Fn.layer_norm(Fn.gelu(v) * mask[:, :, k], (Bn,), p["ln_w"][sl], p["ln_b"][sl], float(F32(R.EXPAND_EPS))))
    return torch.cat(outs, -1), xs[:, lo:hi, F_:F_ + C].mean(1) + p["b_lin1"], torch.cat(pre, -1)


@pytest.mark.parametrize("Bn,NS,T,C,thr,nw", [(64, 2, 3, 3, 0, 1), (64, 3, 15, 64, R.EXPAND_THR_HALF, 2), (128, 3, 7, 1, R.EXPAND_THR_HALF, 1)])
def test_expand_references_agree_with_autograd_on_the_model(Bn, NS, T, C, thr, nw):
    import torch
    c = R.expand_case(nw, T, Bn, NS, C, 11 + T, thr)
    lo, hi = R.centre_range("centre3", T)
    F_ = NS * Bn
    tp = {k: torch.tensor(np.asarray(c[k], np.float64), requires_grad=True) for k in ("b_bott", "ln_w", "ln_b", "b_lin1")}
    P = torch.tensor(c["proj"].astype(np.float64), requires_grad=True)
    keep = R.expand_keep_mask(c["keys"], nw, T, Bn, NS, thr)
    ones = torch.ones((nw, T, NS, Bn), dtype=torch.float64)
    aug_i, lin_i, _ = _torch_model(P, tp, Bn, NS, C, lo, hi, ones)
    (ra, rl), _ = R.expand_infer_ref(c["proj"].astype(np.float64), EXP_ALPHA, c["b_bott"], c["ln_w"], c["ln_b"], c["b_lin1"], Bn, NS, C, lo, hi)
    assert np.abs(ra - aug_i.detach().numpy()).max() <= 1e-11 and np.abs(rl - lin_i.detach().numpy()).max() <= 1e-12
    aug, lin, pre = _torch_model(P, tp, Bn, NS, C, lo, hi, torch.tensor(keep * float(F32(c["scale"]))))
    E, D, A, lv = R.expand_temporal_ref(T, EXP_ALPHA, lo, hi)
    tm = np.stack([E, D, A])
    f64 = lambda k: np.asarray(c[k], np.float64)
    fw = R.expand_train_fwd_ref(f64("proj"), tm, lv, f64("b_bott"), f64("ln_w"), f64("ln_b"), f64("b_lin1"), Bn, NS, C, c["keys"], thr, c["scale"])
    assert np.abs(fw["Y"] - pre.detach().numpy()).max() <= 1e-12 and np.abs(fw["lin"] - lin.detach().numpy()).max() <= 1e-12
    assert np.abs(fw["aug"] - aug.detach().numpy()).max() <= 1e-11
    ((aug * torch.tensor(f64("daug"))).sum() + (lin * torch.tensor(f64("dlin"))).sum()).backward()
    (dp, part), _, _ = R.expand_train_bwd_ref(fw["Y"], f64("daug"), f64("dlin"), tm, lv, f64("ln_w"), Bn, NS, C, c["NPROJ"], c["keys"], thr, c["scale"])
    assert np.abs(dp - P.grad.numpy()).max() <= 1e-10 and not dp[:, :, F_ + C:].any()
    for i, k in enumerate(("b_bott", "ln_w", "ln_b")):       # the per-window sums against the parameter gradients
        assert np.abs(part[:, i * F_:(i + 1) * F_].sum(0) - tp[k].grad.numpy()).max() <= 1e-10, k
    if nw == 1:
        assert np.abs(part[0, :F_] - tp["b_bott"].grad.numpy()).max() <= 1e-10


EXP_INFER_DEFECTS = ("reflect_t0", "reflect_t1", "reflect_t2", "mean_lo_hi_inclusive", "mean_0_T", "no_eps", "mean_over_F")
EXP_TRAIN_FWD_DEFECTS = ("drop_idx_F", "keys_permuted", "no_eps", "mean_over_F")
EXP_TRAIN_BWD_DEFECTS = EXP_TRAIN_FWD_DEFECTS + ("st_slots", "dgam_dbet")
_expand_worst = {}


@pytest.mark.parametrize("case", R.expand_infer_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_expand_inference_bound_accepts_both_lerp_forms_and_rejects_the_defects(case):
    Bn, NS, T, C, kind, lo, hi, nw = case
    p, ref, E = _expand_infer_case(case)
    assert np.isfinite(E[0]).all() and E[0].max() < 1e-3, "a LayerNorm row's variance is lost: the bound is vacuous"
    img = p["proj"].reshape(nw * T, -1)
    for contract in (False, True):
        aug, lin = _emu_expand_infer(img, p, Bn, NS, C, lo, hi, nw, T, contract)
        r = max(R.ratio(aug, ref[0], E[0]), R.ratio(lin, ref[1], E[1]))
        _expand_worst["infer"] = max(_expand_worst.get("infer", 0.0), r)
        assert r <= 1.0, (case, contract, r)
    for defect in EXP_INFER_DEFECTS:
        if (defect == "mean_lo_hi_inclusive" and hi == T) or (defect == "mean_0_T" and (lo, hi) == (0, T)) or (defect in ("reflect_t1", "reflect_t2") and NS == 2):
            continue                                         # the defect does not exist at this shape (the second difference: stream 2 only)
        aug, lin = _emu_expand_infer(img, p, Bn, NS, C, lo, hi, nw, T, False, defect=defect)
        assert max(R.ratio(aug, ref[0], E[0]), R.ratio(lin, ref[1], E[1])) > 1.0, (case, defect)


@pytest.mark.parametrize("sl", EXP_SLIDING, ids=lambda s: "-".join(str(v) for v in s))
def test_expand_sliding_row_map_and_its_clamps(sl):
    """The sliding cases of the GPU suite: the reference on the gathered rows accepts the emulation reading through the row
    map, and rejects a map without its clamp wherever a window of the case crosses that end of the clip."""
    nf, w0, nw = sl
    T, Bn, NS, C = 7, 64, 3, 3
    r0, rows, n_img = R.expand_sliding_layout(nf, w0, nw, T)
    assert np.array_equal(rows, R.expand_rows(nw, T, True, w0, r0, nf)) and rows.min() == (1 if r0 else 0) and rows.max() == n_img - 3
    p = R.expand_case(1, n_img, Bn, NS, C, 40 + nf + w0)
    img = p["proj"][0]
    lo, hi = R.centre_range("centre3", T)
    ref, E = R.expand_infer_ref(img[rows], EXP_ALPHA, p["b_bott"], p["ln_w"], p["ln_b"], p["b_lin1"], Bn, NS, C, lo, hi)
    aug, lin = _emu_expand_infer(img, p, Bn, NS, C, lo, hi, nw, T, True, sliding=(w0, r0, nf))
    assert max(R.ratio(aug, ref[0], E[0]), R.ratio(lin, ref[1], E[1])) <= 1.0
    f = w0 + np.arange(nw)[:, None] + np.arange(T)[None, :] - T // 2
    for defect, crosses in (("no_clamp_first", (f < 0).any()), ("no_clamp_last", (f > nf - 1).any())):
        if crosses:
            aug, lin = _emu_expand_infer(img, p, Bn, NS, C, lo, hi, nw, T, True, sliding=(w0, r0, nf), defect=defect)
            assert R.ratio(aug, ref[0], E[0]) > 1.0, (sl, defect)
    if nf <= 5:                                              # the short clips: every window crosses an end
        assert ((f < 0) | (f > nf - 1)).any(1).all()


def test_expand_sliding_cases_cover_both_ends_the_interior_and_r0():
    lay = {sl: R.expand_sliding_layout(*sl, 7) for sl in EXP_SLIDING}
    assert {sl[0] for sl in EXP_SLIDING} == {1, 2, 5, 40}
    assert any(r0 > 0 for r0, _, _ in lay.values()) and any(r0 == 0 for r0, _, _ in lay.values())
    f = lambda sl: sl[1] + np.arange(sl[2])[:, None] + np.arange(7)[None, :] - 3
    assert any((f(sl) >= 0).all() and (f(sl) <= sl[0] - 1).all() for sl in EXP_SLIDING)           # interior
    assert any(sl[1] > 0 and (f(sl) > sl[0] - 1).any() and sl[0] == 40 for sl in EXP_SLIDING)


@pytest.mark.parametrize("case", R.expand_train_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_expand_training_bounds_accept_the_emulations_and_reject_the_defects(case):
    Bn, NS, T, C, thr, nw = case
    p, tm, lv, fw, Yb, ((dp, part), (Edp, Epart), info) = _expand_train_case(case)
    F_ = NS * Bn
    # conditioning: no row's variance is lost, and the threshold element of each stream exists (kept: hash == thr)
    assert np.isfinite(fw["E_aug"]).all() and fw["E_aug"].max() < 1e-3 and info["rel"].max() < 1e-5 and info["var"].min() > 1e-3
    for k in range(NS):
        h = int(R.mix64(np.uint64((p["keys"][k] + 7 + k) & ((1 << 64) - 1))) >> np.uint64(40))
        assert h == thr and fw["keep"].reshape(-1, NS, Bn)[0, k, 7 + k]
    assert len(set(p["keys"])) == 3
    aug = _emu_expand_train_fwd(fw["Y"], p, Bn, NS)
    r = R.ratio(aug, fw["aug"], fw["E_aug"])
    _expand_worst["fwd"] = max(_expand_worst.get("fwd", 0.0), r)
    assert r <= 1.0, (case, r)
    m = Edp > 0
    g, pt = _emu_expand_train_bwd(Yb, p, tm, lv, Bn, NS, C)
    r = max(R.ratio(g[m], dp[m], Edp[m]), R.ratio(pt, part, Epart))
    _expand_worst["bwd"] = max(_expand_worst.get("bwd", 0.0), r)
    assert r <= 1.0, (case, r)
    assert np.array_equal(g[~m].view(np.uint32), dp[~m].astype(F32).view(np.uint32))
    for defect in EXP_TRAIN_BWD_DEFECTS:
        if defect in ("drop_idx_F", "keys_permuted") and thr == 0:
            continue                                         # nothing is dropped: the index and the key are not used
        if defect in EXP_TRAIN_FWD_DEFECTS:
            assert R.ratio(_emu_expand_train_fwd(fw["Y"], p, Bn, NS, defect), fw["aug"], fw["E_aug"]) > 1.0, (case, defect, "forward")
        g, pt = _emu_expand_train_bwd(Yb, p, tm, lv, Bn, NS, C, defect)
        assert max(R.ratio(g[m], dp[m], Edp[m]), R.ratio(pt, part, Epart)) > 1.0, (case, defect, "backward")


def test_expand_temporal_defects_leave_the_rounded_reference():
    """What the GPU suite's bit-for-bit check of build_temporal would see of a wrong stencil row or a wrong centre mean."""
    for T in (3, 15, 31, 101):
        for kind in R.RANGE_KINDS:
            lo, hi = R.centre_range(kind, T)
            E, D, A, lv = R.expand_temporal_ref(T, EXP_ALPHA, lo, hi)
            interior_D = np.concatenate([np.zeros((1, T)), E[1:] - E[:-1]])                      # replicate instead of reflect at t = 0
            interior_A = A.copy()
            interior_A[1] = E[1] - E[0]                                                          # likewise at t = 1
            assert not np.array_equal(D.astype(F32), interior_D.astype(F32)) and not np.array_equal(A.astype(F32), interior_A.astype(F32))
            if hi < T:
                assert not np.array_equal(lv.astype(F32), E[lo:hi + 1].mean(0).astype(F32))
            if (lo, hi) != (0, T):
                assert not np.array_equal(lv.astype(F32), E.mean(0).astype(F32))


def test_zz_expand_print_the_largest_emulation_ratios():
    print(f"[expand bounds] largest emulation error / bound: {_expand_worst}")


# ---- ViT ingest and the create-time weight packers (tests/test_gpu_ingest_reference.py): the exact references ----------------------
@pytest.mark.parametrize("ps", [14, 16])
def test_ingest_slot_layout_is_the_models_patch_convolution(ps):
    """vit_im2col_ref(g) @ patch_weight_ref(w).T against oracle/vit_oracle.embeddings on the 3-times repeated green plane: ties the
    slot layout of the two references to the model definition, not to each other.  Pixels are bytes and the weights multiples of
    2^-4 below 2, so every product, every channel sum and every dot product (below 2^19, in steps of 2^-4: 23 bits) is exact in
    float32 and float64 alike, whatever the order - embeddings rounds its result to float32 - and the comparison is equality."""
    from oracle import vit_oracle as V
    rng = np.random.default_rng(50 + ps)
    n, h, w, D = 2, 2 * ps + 3, 3 * ps + 5, 5
    g = rng.integers(0, 256, (n, h, w)).astype(np.float64)
    wt = (rng.integers(-31, 32, (D, 3, ps, ps)) / 16.0).astype(F32)
    A, owned = R.vit_im2col_ref(g, ps)
    assert owned.sum() == 16 * ps and not A[:, ~owned].any()
    for wide in (False, True):
        got = A @ R.patch_weight_ref(wt, ps, wide).astype(np.float64).T
        weights = {"embeddings.patch_embeddings.weight": wt.astype(np.float64), "embeddings.patch_embeddings.bias": np.zeros(D),
                   "embeddings.cls_token": np.zeros((1, 1, D)), "embeddings.register_tokens": np.zeros((1, 0, D))}
        want = V.embeddings(np.repeat(g[:, None], 3, axis=1), weights, ps)[:, 1:]
        assert want.shape == (n, 6, D) and np.array_equal(got.reshape(n, 6, D), want.astype(np.float64))
    # a py / px swap or a transposed slot is another matrix
    swapped = A.reshape(n, 2, 3, 256).transpose(0, 2, 1, 3).reshape(n * 6, 256)
    assert not np.array_equal(swapped, A) and not np.array_equal(A.reshape(-1, 16, 16).transpose(0, 2, 1).reshape(-1, 256), A)


def test_patch_weight_sums_differ_between_float32_and_float64_on_cancelling_triples():
    w = np.zeros((1, 3, 14, 14), F32)
    w[0, :, 0, 0] = [1.0, 2.0 ** -30, -1.0]                       # float32: (1 + 2^-30) - 1 = 0; float64: 2^-30
    w[0, :, 0, 1] = [16777216.0, 1.0, 1.0]                        # float32: 2^24 + 1 -> 2^24 (tie to even), + 1 -> 2^24; float64: 2^24 + 2
    n32, n64 = R.patch_weight_ref(w, 14, False), R.patch_weight_ref(w, 14, True)
    assert n32[0, 0] == 0.0 and n64[0, 0] == F32(2.0 ** -30)
    assert n32[0, 1] == F32(16777216.0) and n64[0, 1] == F32(16777218.0)
    assert not n32[0, 14:16].any() and not n32[0, 14 * 16:].any()


@pytest.mark.parametrize("ps", [14, 16])
def test_ingest_hi_lo_reproduce_the_float_inputs(ps):
    """hi + lo against v on the float frames of the GPU suite.  hi is off by at most 2^-11 |v|; lo rounds that residual to 2^-11 of
    itself - 2^-22 |v| in all - wherever the residual is a normal fp16 (>= 2^-14) or zero.  A smaller residual lands on fp16's
    subnormal grid (step 2^-24) and is off by up to F16_SUB = 2^-25 instead: no pair of fp16 values does better there (a value below
    2^-25 is lost whole), which is why kernels.h promises x = hi + lo to about 2^-22 for pixels in [0, 1], not relative to x."""
    g = R.ingest_float_planes(3, 2 * ps + 3, 3 * ps + 5, ps, 700 + ps)
    v, _ = R.vit_im2col_ref(g, ps)
    assert np.isfinite(v).all(), "the NaN remainder was gathered"
    hi, lo = R.f16_pair(v)
    v64 = v.astype(np.float64)
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - v64)
    resid = np.abs((v - hi.astype(F32)).astype(np.float64))
    normal = (resid >= 2.0 ** -14) | (resid == 0)
    assert normal.sum() > 100 and (~normal).sum() > 100
    assert (err[normal] <= 2.0 ** -22 * np.abs(v64[normal])).all()
    assert (err[~normal] <= R.F16_SUB).all()
    assert np.array_equal(R.split_value(v, 1.0), hi.astype(np.float64) + lo.astype(np.float64))
    # the inputs do reach the edges they are there for: hi subnormal, hi zero with v != 0, -0.0 kept
    assert ((np.abs(hi) < 2.0 ** -14) & (hi != 0)).any() and ((hi == 0) & (v != 0)).any()
    assert (np.signbit(v) & (v == 0)).any() and np.array_equal(hi[v == 0].view(np.uint16), v[v == 0].view(np.uint32) >> 16)
    # the split image is the same pair, placed: decode_split_operand undoes split_operand_bits
    img = R.split_operand_bits(v, 1.0).view(F32)
    assert np.array_equal(R.decode_split_operand(img, 256, 1.0), R.split_value(v, 1.0))


def test_u8_to_unit_f32_is_the_reference_preprocessing():
    from oracle import vit_oracle as V
    p = np.arange(256, dtype=np.uint8)
    want = V.preprocess_green(np.repeat(p.reshape(1, 16, 16, 1), 3, axis=3)).reshape(-1)
    assert np.array_equal(R.u8_to_unit_f32(p).view(np.uint32), want.view(np.uint32))
    # a kernel that multiplied by the rounded reciprocal instead of dividing would show on these 256 values
    assert (R.u8_to_unit_f32(p) != p.astype(F32) * F32(1.0 / 255.0)).any()


@pytest.mark.parametrize("F,K", [(32, 1), (32, 5), (96, 40)])
def test_interleave_ref_is_a_permutation_with_an_inverse(F, K):
    gate = (np.arange(F * K, dtype=np.int64).reshape(F, K)).astype(F32)
    up = gate + F32(F * K)
    out = R.interleave_ref(gate, up)
    assert out.shape == (2 * F, K) and np.array_equal(np.sort(out.reshape(-1)), np.arange(2 * F * K, dtype=F32))
    blocks = out.reshape(F // 32, 2, 32, K)
    assert np.array_equal(blocks[:, 0].reshape(F, K), gate) and np.array_equal(blocks[:, 1].reshape(F, K), up)
    # the index formula of kernels.h, element by element
    for r in range(2 * F):
        src = (gate if r % 64 < 32 else up)[32 * (r // 64) + r % 32]
        assert np.array_equal(out[r], src)


def test_fp8_weight_ref_routes_three_calls_into_one_scale_image():
    from oracle.mx_oracle import mx_quant
    rng = np.random.default_rng(81)
    N, K = 3, 256
    nt = 3 * N + 4
    img = np.full((K // 128, nt), 0xA5A5A5A5, np.uint32)
    ws = [rng.standard_normal((N, K)).astype(F32) * F32(10.0 ** i) for i in range(3)]
    for i, n0 in enumerate((0, N, 2 * N + 4)):
        q, img = R.fp8_weight_ref(ws[i], img, nt, n0)
        assert np.array_equal(q, mx_quant(ws[i])[1])
    by = img.view(np.uint8).reshape(K // 128, nt, 4)
    for i, n0 in enumerate((0, N, 2 * N + 4)):
        sb = mx_quant(ws[i])[2]
        for n in range(N):
            for k in range(0, K, 32):
                assert by[k // 128, n0 + n, (k % 128) // 32] == sb[n, k // 32]
    assert (img[:, 2 * N:2 * N + 4] == 0xA5A5A5A5).all()


# ---- the MX-fp8 GEMM: the bound of tests/test_gpu_fp8_gemm_reference.py at its cap, MX_ACC_U = 2^-11 ----------------------------
MX_CAP = 2.0 ** -11


def _mx_bytes(q) -> np.ndarray:
    """e4m3 codes of values that ARE e4m3 numbers (mx_quant's elements)."""
    from oracle.mx_oracle import e4m3_decode
    table = e4m3_decode(np.arange(256, dtype=np.uint8)).astype(np.float64)
    codes = np.concatenate([np.arange(0, 0x7F), np.arange(0x81, 0xFF)])           # no NaN codes, one zero
    order = np.argsort(table[codes])
    idx = np.searchsorted(table[codes][order], np.asarray(q, np.float64))
    out = codes[order][idx].astype(np.uint8)
    assert np.array_equal(table[out], np.asarray(q, np.float64))
    return out


def _mx_case(epi, seed, n_total=256, n0=0, D=128, sec0=0):
    """Random operands as the GPU cases draw them (rows of different scale, every 7th column x 30, one all-zero row), quantised
    on the CPU: K = 256, N = 256, M = 64 of M_alloc = 128 rows (rows 64 .. 127 are other rows' worth of scales)."""
    from oracle.mx_oracle import mx_quant
    rng = np.random.default_rng(seed)
    M, M_alloc, N, K = 64, 128, 256, 256
    A = (rng.standard_normal((M_alloc, K)) * np.exp(rng.standard_normal((M_alloc, 1)))).astype(np.float32)
    A[:, ::7] *= 30.0
    A[3] = 0.0
    W = (rng.standard_normal((n_total, K)) * 0.05).astype(np.float32)
    _, qa, sa = mx_quant(A)
    _, qw, sw = mx_quant(W)
    d = dict(M=M, N=N, K=K, n0=n0, A8=_mx_bytes(qa), W8=_mx_bytes(qw), sa=sa.astype(np.uint8), sw=sw.astype(np.uint8),
             A_sc=R.mx_scale_image(sa, M_alloc + 128), W_sc=R.mx_scale_image(sw, n_total), sc_lda=M_alloc + 128, n_total=n_total,
             bias=(0.5 * rng.standard_normal(N)).astype(np.float32))
    if epi == R.EPI_RESID:
        d.update(lam=(0.3 * rng.standard_normal(N)).astype(np.float32), x0=rng.standard_normal((M, N)).astype(np.float32))
    if epi == R.EPI_QKV:
        cos, sin = R.rope_cos_sin(5, 7, 64, 100.0)
        d.update(D=D, sec0=sec0, T=40, n_prefix=5, cos=cos, sin=sin)
    return d


def _mx_operands(d, *, a_sc=None, a8=None, w_n0=None):
    M, N = d["M"], d["N"]
    n0 = d["n0"] if w_n0 is None else w_n0
    a = R.mx_dequant((d["A8"] if a8 is None else a8)[:M], d["A_sc"] if a_sc is None else a_sc, M, d["sc_lda"])
    w = R.mx_dequant(d["W8"][d["n0"]:d["n0"] + N], d["W_sc"][:, n0:n0 + N], N, N)
    return a, w


def _mx_acc32(a, w):
    """fp32 accumulation block by block: each block's 32 products summed in fp32, the blocks chained in fp32."""
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for k in range(0, a.shape[1], 32):
        acc = acc + a[:, k:k + 32].astype(np.float32) @ w[:, k:k + 32].astype(np.float32).T
    return acc


def _mx_reference(epi, d):
    a, w = _mx_operands(d)
    acc = a @ w.T
    S = np.abs(a) @ np.abs(w).T
    y, Ey, _ = R.gemm_epilogue_ref(epi, acc, MX_CAP * S, S, bias=d["bias"], lam=d.get("lam"), x0=d.get("x0"), T=d.get("T"),
                                   n_prefix=d.get("n_prefix", 0), cos=d.get("cos"), sin=d.get("sin"), D=d.get("D"), sec0=d.get("sec0", 0))
    if epi == R.EPI_GELU:
        v = acc + d["bias"][None, :]
        Ey = Ey + 2e-7 * np.abs(v) + 8 * R.U32 * (np.abs(v) + np.abs(y))
    return y, Ey + R.out_rounding(y, "f32" if epi == R.EPI_RESID else "f16")


def _rows_rejected(out, y, bound):
    return (np.where(np.isfinite(out), np.abs(out - y), np.inf) / bound).max(axis=1) > 1.0


def test_mx_acc_u_is_within_the_cap_the_defect_tests_are_written_for():
    assert R.MX_ACC_U <= MX_CAP and np.log2(R.MX_ACC_U) == round(np.log2(R.MX_ACC_U))
    assert R.MX_ACC_MEASURED is None or 2.0 * R.MX_ACC_MEASURED <= R.MX_ACC_U < 4.0 * R.MX_ACC_MEASURED


@pytest.mark.parametrize("epi", [R.EPI_QKV, R.EPI_RESID, R.EPI_GELU])
def test_mx_gemm_bound_accepts_the_simulated_launch_and_rejects_operand_defects_row_by_row(epi):
    d = _mx_case(epi, 300 + epi)
    y, bound = _mx_reference(epi, d)
    a, w = _mx_operands(d)
    assert R.ratio(_simulate(0, epi, d, _mx_acc32(a, w)), y, bound) <= 1.0
    M, K = d["M"], d["K"]
    nz = np.any(a != 0.0, axis=1)
    assert not nz[3] and nz.sum() == M - 1
    sa = d["sa"].astype(np.int64)
    # block b of an A row takes the scale byte of block b ^ 1
    swapped = sa.reshape(sa.shape[0], -1, 2)[:, :, ::-1].reshape(sa.shape)
    a_def, _ = _mx_operands(d, a_sc=R.mx_scale_image(swapped, d["sc_lda"]))
    hit = np.any(a_def != a, axis=1)
    assert hit.sum() >= M // 4                                                 # enough rows have neighbouring blocks of different scale
    rej = _rows_rejected(_simulate(0, epi, d, _mx_acc32(a_def, w)), y, bound)
    assert np.all(rej[hit]) and not np.any(rej[~hit]), "scale byte of block b ^ 1"
    # a row's scale dword taken from row + 64
    a_def, _ = _mx_operands(d, a_sc=R.mx_scale_image(np.roll(sa, -64, axis=0), d["sc_lda"]))
    hit = np.any(a_def != a, axis=1)
    assert hit.sum() >= M - 2
    rej = _rows_rejected(_simulate(0, epi, d, _mx_acc32(a_def, w)), y, bound)
    assert np.all(rej[hit]) and not np.any(rej[~hit]), "scale dword of row + 64"
    # one e4m3 byte of a row replaced by its neighbour code: the row's largest element (a SMALL element's neighbour code moves the
    # row by far less than S / 256 - no per-element bound at K = 256 can see that, and none is claimed)
    a8 = d["A8"].copy()
    k = np.argmax(np.abs(a), axis=1)
    r = np.arange(M)
    mag = a8[r, k] & 0x7F
    a8[r, k] = (a8[r, k] & 0x80) | np.where(mag < 0x7E, mag + 1, mag - 1)
    a_def, _ = _mx_operands(d, a8=a8)
    rej = _rows_rejected(_simulate(0, epi, d, _mx_acc32(a_def, w)), y, bound)
    assert np.all(rej[nz]), "neighbour code"


def test_mx_gemm_bound_rejects_w_scales_read_at_column_0_of_the_fused_image():
    """The k | v launch: n0 = D of a 3 D-wide image; the defect reads the q columns' scales."""
    d = _mx_case(R.EPI_QKV, 41, n_total=384, n0=128, D=128, sec0=1)
    y, bound = _mx_reference(R.EPI_QKV, d)
    a, w = _mx_operands(d)
    # _simulate rotates columns [0, 2 D) and scales [0, D): told D = 64 without the q scale it rotates k (columns [0, 128)) alone
    def run(aa, ww):
        return _simulate(0, R.EPI_QKV, dict(d, D=64), _mx_acc32(aa, ww), no_q_scale=True)

    assert R.ratio(run(a, w), y, bound) <= 1.0
    _, w_def = _mx_operands(d, w_n0=0)
    assert np.any(w_def != w)
    rej = _rows_rejected(run(a, w_def), y, bound)
    nz = np.any(a != 0.0, axis=1)
    assert np.all(rej[nz]) and not np.any(rej[~nz])


def test_mx_gemm_bound_rejects_rope_on_a_prefix_row_and_a_missing_q_scale():
    d = _mx_case(R.EPI_QKV, 42)
    y, bound = _mx_reference(R.EPI_QKV, d)
    a, w = _mx_operands(d)
    acc32 = _mx_acc32(a, w)
    rej = _rows_rejected(_simulate(0, R.EPI_QKV, d, acc32, rope_prefix=True), y, bound)
    t = np.arange(d["M"]) % d["T"]
    assert np.array_equal(rej, t == d["n_prefix"] - 1)                        # the last prefix row of each frame, nothing else
    rej = _rows_rejected(_simulate(0, R.EPI_QKV, d, acc32, no_q_scale=True), y, bound)
    assert np.all(rej)                                                        # the all-zero row too: its q is the bias


@pytest.mark.parametrize("K", [256, 768])
def test_mx_lossless_operands_are_the_integers_that_generated_them(K):
    M_alloc, n_total, ld = 384, 768, 512
    L = R.mx_lossless_case(M_alloc, n_total, K, 40 + K, ld)
    a = R.mx_dequant(L["A8"], L["A_sc"], M_alloc, ld)
    w = R.mx_dequant(L["W8"], L["W_sc"], n_total, n_total)
    assert np.array_equal(a, R.mx_lossless_values(L["ai"], L["sa"])) and np.array_equal(w, R.mx_lossless_values(L["wi"], L["sw"]))
    assert set(np.unique(L["ai"])) == set(range(-4, 5)) and set(np.unique(L["sa"])) == set(range(125, 130))
    assert np.all(L["A_sc"][:, M_alloc:] == 0xFFFFFFFF)
    # every partial sum, in any order, is an integer number of the smallest product 2^(2 * 125 - 254) = 2^-4 and below 2^24 of them
    unit = 2.0 ** -4
    S = (np.abs(a) @ np.abs(w).T) / unit
    assert np.array_equal(S, np.round(S)) and S.max() < 2.0 ** 24
    assert 768 * 16 * 2.0 ** (2 * 129 - 254) / unit < 2.0 ** 24               # and so would the worst draw at K = 768
