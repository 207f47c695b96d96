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
