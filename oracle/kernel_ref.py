"""ORACLE (test infrastructure, not product code): float64 references of single GEMM and attention launches, the
exact precision-3 accumulator, the row-wise kernels between the GEMMs (LayerNorm forms, the MX-fp8 row, the ConvNeXt
producers), and element-wise error bounds derived from where each kernel rounds.

Used by tests/test_gpu_kernel_reference.py (the kernels through cbas_debug_gemm_run / cbas_debug_attention_run),
tests/test_gpu_fp8_gemm_reference.py (the MX-fp8 GEMM through cbas_debug_gemm_f8_run), tests/test_gpu_rows_reference.py (cbas_debug_rows_run), tests/test_gpu_head_kernels_reference.py (the classifier head's
exact-fp32 GEMM and small training kernels through cbas_debug_head_run), tests/test_gpu_head_seq_reference.py and
tests/test_gpu_head_expand_reference.py (the head's sequential and expand kernels through cbas_debug_head_seq_run /
cbas_debug_head_expand_run), tests/test_gpu_ingest_reference.py (the ViT ingest kernels and the create-time weight packers
through cbas_debug_pack_run: exact references, no bounds) and tests/test_kernel_reference_bounds.py (the
references and bounds themselves, on the CPU).

Units: u32 = 2^-24 (fp32 unit roundoff), u16 = 2^-11 (fp16).  A bound is a float64 array shaped like the output; a kernel
output y passes when |y - ref| <= bound everywhere (non-finite y never passes).  Every bound is a sum of the terms its
docstring names; no term is fitted to measured errors, except the device math library's budgets in the classifier-head
section and the scaled MFMA's accumulation (MX_ACC_U), which are measured as their comments describe.
"""
from __future__ import annotations

import math

import numpy as np

from oracle.vit_oracle import _rotate_half, gelu_erf, rope_cos_sin  # noqa: F401  (re-exported for the tests)

try:
    from scipy.special import erf as _erf64
except Exception:  # pragma: no cover
    _erf64 = np.vectorize(math.erf, otypes=[np.float64])

U32 = 2.0 ** -24
U16 = 2.0 ** -11
F16_SUB = 2.0 ** -25          # half of fp16's subnormal step: the absolute rounding error below 2^-14
EPI_PATCH, EPI_QKV, EPI_RESID, EPI_GELU = 0, 1, 2, 3
ATT_QS, ATT_KS, ATT_VS, ATT_CTX = 16.0, 4.0, 4.0, 16.0      # vit32_epilogue.h / api_enc.hip split scales
GELU_SLOPE = 1.13             # max |d gelu / dx| (at x ~ 1.5: 1.1289)


# ---- operand roundings ------------------------------------------------------------------------------------------------
def f16(x) -> np.ndarray:
    """fp32 -> fp16 (round to nearest even, as the device's conversion), returned as float64."""
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float64)


def split_halves(x, scale: float):
    """precision 4's split of an fp32 value (vit32_epilogue.h store_split4): s = x * scale (power of two, exact),
    hi = fp16(s), lo = fp16(s - hi) (the fp32 subtraction is exact by Sterbenz).  float64 hi, lo (scaled units)."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.asarray(x, np.float32) * np.float32(scale)
        hi = s.astype(np.float16)
        lo = (s - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def split_value(x, scale: float) -> np.ndarray:
    hi, lo = split_halves(x, scale)
    return (hi + lo) / scale


def decode_split_operand(raw: np.ndarray, ncols: int, scale: float) -> np.ndarray:
    """The GEMM-operand split image (store_split4: per 32-column K-tile 128 bytes = [hi 32 x fp16 | lo 32 x fp16], value
    k = 16 h + 4 g + e at position 8 g + 4 h + e) of rows [R][ld] float32 -> float64 [R][ncols] = (hi + lo) / scale."""
    R = raw.shape[0]
    h = np.ascontiguousarray(raw[:, :ncols]).view(np.float16).reshape(R, ncols // 32, 2, 32).astype(np.float64)
    k = np.arange(32)
    pos = 8 * ((k % 16) // 4) + 4 * (k // 16) + k % 4
    return ((h[:, :, 0, pos] + h[:, :, 1, pos]) / scale).reshape(R, ncols)


def decode_head_split(raw: np.ndarray, ncols: int, scales) -> np.ndarray:
    """The attention-operand split image (store_head_split4: per 64-column head 256 bytes = [hi 64 | lo 64] fp16 in d
    order) -> float64 (hi + lo) / scale; `scales` gives the scale per D-wide section (q | k | v) of the columns."""
    R = raw.shape[0]
    h = np.ascontiguousarray(raw[:, :ncols]).view(np.float16).reshape(R, ncols // 64, 2, 64).astype(np.float64)
    v = (h[:, :, 0] + h[:, :, 1]).reshape(R, ncols)
    sc = np.repeat(np.asarray(scales, np.float64), ncols // len(scales))
    return v / sc


# ---- exact fp32 accumulation ------------------------------------------------------------------------------------------
def f32_mfma_k_order(K: int) -> np.ndarray:
    """k order of the precision-3 GEMM (vit_f32.hip gemm_f32_vit_kernel): per 32-wide K-tile, kk = 0, 1 and e = 0..3 issue
    one v_mfma_f32_16x16x4_f32 each, whose four products are k = 16 kk + 4 g + e for lane groups g = 0..3 (the 16-byte
    chunk kk * 4 + g of the row).  The MFMA is a bitwise fmaf chain over its k index g (MI355X_MICROARCH.md, matrix cores)."""
    kt, kk, e, g = np.meshgrid(np.arange(K // 32), np.arange(2), np.arange(4), np.arange(4), indexing="ij")
    return (kt * 32 + kk * 16 + g * 4 + e).reshape(-1)


def round_f32_with_residual(s: np.ndarray, err: np.ndarray) -> np.ndarray:
    """Correctly rounded fp32 of the exact value s + err, where s = fl64(s + err) (a TwoSum pair).  fp32(s) is right
    unless s sits exactly on an fp32 midpoint (representable in float64): then the sign of err decides."""
    with np.errstate(over="ignore", invalid="ignore"):
        r = s.astype(np.float32)
        r64 = r.astype(np.float64)
        other = np.nextafter(r, np.where(s > r64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        tie = np.isfinite(s) & (s != r64) & (s - r64 == other.astype(np.float64) - s)
        # at a tie r is the even neighbour; the exact value lies on the side err points to
        pick = np.where(err > 0, np.maximum(r, other), np.minimum(r, other))
        r = np.where(tie & (err != 0), pick, r)
    return r


def fmaf_chain(A: np.ndarray, W: np.ndarray, order=None) -> np.ndarray:
    """C[m][n] = fmaf(a_k, w_k, C) over k in `order` (default 0..K-1), starting from +0, every step rounded once to fp32:
    the product a_k w_k is exact in float64 (24 + 24 bits), the sum is a TwoSum pair, rounded with
    round_f32_with_residual.  A [M][K], W [N][K] fp32; returns fp32 [M][N]."""
    A = np.asarray(A, np.float32).astype(np.float64)
    W = np.asarray(W, np.float32).astype(np.float64)
    ks = range(A.shape[1]) if order is None else order
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in ks:
            p = A[:, k:k + 1] * W[None, :, k]
            a = acc.astype(np.float64)
            s = a + p
            bb = s - a
            err = (a - (s - bb)) + (p - bb)
            acc = round_f32_with_residual(s, np.where(np.isfinite(err), err, 0.0))
    return acc


# ---- GEMM references --------------------------------------------------------------------------------------------------
def gemm_acc(arith: int, A, W, a_scale: float = 1.0, w_scale: float = 1.0):
    """float64 accumulator reference and its bound.  Returns (acc, E, S) with S = sum_k |a_k w_k| of the operands used.
      arith 0 / 1: products of the fp16-rounded operands (fp16 A; W fp16, or W hi + lo for arith 1, whose residual
                   2^-11 |w| rounding of lo adds 2^-22 |a w| per product); E = K u32 S (fp32 accumulation, products exact).
      arith 3:     exact products of the fp32 operands; E = K u32 S.
      arith 4:     exact products of the fp32 operands; each split product (a_hi w_hi + a_hi w_lo + a_lo w_hi) is off by
                   the two representation residues and the dropped a_lo w_lo: 3 * 2^-22 |a w|; a low half below fp16's
                   normal range rounds absolutely: 2^-25 / scale per operand, times the other operand; E adds K u32 S."""
    A32 = np.asarray(A, np.float32)
    W32 = np.asarray(W, np.float32)
    K = A32.shape[1]
    if arith in (0, 1):
        a = f16(A32)
        if arith == 1:
            hi, lo = f16(W32), f16(np.asarray(W32, np.float32) - np.asarray(W32, np.float32).astype(np.float16).astype(np.float32))
            w = hi + lo
        else:
            w = f16(W32)
        acc = a @ w.T
        S = np.abs(a) @ np.abs(w).T
        E = K * U32 * S + (2.0 ** -22 * S if arith == 1 else 0.0)
        return acc, E, S
    a = A32.astype(np.float64)
    w = W32.astype(np.float64)
    acc = a @ w.T
    S = np.abs(a) @ np.abs(w).T
    E = K * U32 * S
    if arith == 4:
        sub = (np.ones_like(a) / a_scale) @ np.abs(w).T + np.abs(a) @ (np.ones_like(w) / w_scale).T
        E = E + 3 * 2.0 ** -22 * S + 2 * F16_SUB * sub
    return acc, E, S


# ---- MX-fp8 operands (gemm_f16_8ph.hip, F8 = true) ---------------------------------------------------------------------
# Used by tests/test_gpu_fp8_gemm_reference.py through cbas_debug_gemm_f8_run.  The reference is the float64 product of exactly
# the e4m3 bytes and E8M0 scale bytes the launch was given; the epilogues and their bounds are those of the fp16 form above.
#
# MX_ACC_U: the accumulator's error per unit of S = sum_k |a_k w_k|.  v_mfma_scale_f32_16x16x128_f8f6f4 does not accumulate its
# 128 products as an fp32 fma chain, and no public document gives its internal alignment, so this ONE figure is measured, not
# derived: the largest |kernel - acc| / S of the accumulator-only launch (residual epilogue on x = 0, bias 0, lambda 1) against
# the float64 product of the dequantised operands, over every random-operand case and tile form of
# tests/test_gpu_fp8_gemm_reference.py (mx_random_cases), doubled for operand draws not in the suite and rounded up to a power
# of two.  Measured on an MI355X on 2026-10-21: see MX_ACC_MEASURED below.  It must stay <= 2^-11: above that a single
# mis-decoded element at K = 256 (~S / 256) is no longer reliably outside the bound (tests/test_kernel_reference_bounds.py).
MX_ACC_MEASURED = 1.18e-4     # = 2^-13.05: the largest |kernel - acc| / S seen (tile forms q|k|v operands, M 1015 N 768 K 256)
MX_ACC_U = 2.0 ** -12         # 2 x 1.18e-4 = 2.36e-4, rounded up to a power of two (2.44e-4)
MX_INT_BYTE = {0: 0x00, 1: 0x38, 2: 0x40, 3: 0x44, 4: 0x48}      # e4m3 codes of the lossless cases' magnitudes


def mx_dequant(bytes8, sc_image, rows: int, ld: int) -> np.ndarray:
    """float64 [rows][K] of e4m3 bytes [rows][K] and the scale image [K / 128][ld] dwords (byte b of dword (t, r) = the E8M0
    scale of block b of K-tile t of row r, GemmParams A_sc / W_sc): oracle.mx_oracle.e4m3_decode x 2^(scale byte - 127).
    The e4m3 NaN codes (0x7f, 0xff) and the E8M0 NaN (0xff) give NaN."""
    from oracle.mx_oracle import e4m3_decode
    b = np.asarray(bytes8, np.uint8)
    assert b.shape[0] == rows and b.shape[1] % 128 == 0
    K = b.shape[1]
    sb = np.ascontiguousarray(np.asarray(sc_image, np.uint32).reshape(K // 128, ld)).view(np.uint8).reshape(K // 128, ld, 4)
    sb = sb[:, :rows].transpose(1, 0, 2).reshape(rows, K // 32).astype(np.float64)
    scale = np.where(sb == 255.0, np.nan, np.exp2(sb - 127.0))
    el = np.where((b & 0x7f) == 0x7f, np.nan, e4m3_decode(b).astype(np.float64))
    return el * np.repeat(scale, 32, axis=1)


def mx_scale_image(sb, ld: int, fill: int = 0xFFFFFFFF) -> np.ndarray:
    """The inverse of mx_dequant's scale routing: scale bytes [rows][K / 32] -> dwords [K / 128][ld], rows past `rows` = fill."""
    sb = np.asarray(sb, np.uint8)
    rows, nb = sb.shape
    img = np.full((nb // 4, ld), fill, np.uint32)
    img.view(np.uint8).reshape(nb // 4, ld, 4)[:, :rows] = sb.reshape(rows, nb // 4, 4).transpose(1, 0, 2)
    return img


def gemm_acc_mx(a, w):
    """Accumulator reference of the MX-fp8 GEMM on dequantised operands a [M][K], w [N][K] (float64, mx_dequant): (acc, E, S)
    with acc = a w^T, S = |a| |w|^T and E = MX_ACC_U S; feeds gemm_epilogue_ref / out_rounding like gemm_acc's triple."""
    a = np.asarray(a, np.float64)
    w = np.asarray(w, np.float64)
    acc = a @ w.T
    S = np.abs(a) @ np.abs(w).T
    return acc, MX_ACC_U * S, S


def mx_int_bytes(v) -> np.ndarray:
    """e4m3 bytes of integers in [-4, 4] (exactly representable)."""
    v = np.asarray(v, np.int64)
    lut = np.array([MX_INT_BYTE[i] for i in range(5)], np.uint8)
    return (lut[np.abs(v)] | np.where(v < 0, 0x80, 0).astype(np.uint8)).astype(np.uint8)


def mx_lossless_case(M_alloc: int, n_total: int, K: int, seed: int, sc_lda: int, sb_lo: int = 125, sb_hi: int = 129):
    """The lossless operands of the bit-for-bit cases: elements drawn from {0, +-1, .., +-4}, every (row, block) scale byte
    drawn independently from sb_lo .. sb_hi, for A [M_alloc][K] and W [n_total][K].  Every product is an integer multiple of
    2^(2 sb_lo - 254) no larger than 16 x 2^(2 sb_hi - 254), so any partial sum over K <= 768 stays below 2^24 units: exact in
    fp32 in any order.  Returns dict(ai, wi (the integers), sa, sw (scale bytes), A8, W8, A_sc [K/128][sc_lda], W_sc [K/128][n_total])."""
    rng = np.random.default_rng(seed)
    ai = rng.integers(-4, 5, (M_alloc, K))
    wi = rng.integers(-4, 5, (n_total, K))
    sa = rng.integers(sb_lo, sb_hi + 1, (M_alloc, K // 32)).astype(np.uint8)
    sw = rng.integers(sb_lo, sb_hi + 1, (n_total, K // 32)).astype(np.uint8)
    return dict(ai=ai, wi=wi, sa=sa, sw=sw, A8=mx_int_bytes(ai), W8=mx_int_bytes(wi), A_sc=mx_scale_image(sa, sc_lda),
                W_sc=mx_scale_image(sw, n_total))


def mx_lossless_values(ints, sb) -> np.ndarray:
    """What mx_lossless_case's operands mean: integer x 2^(scale byte - 127), float64 (exact)."""
    return np.asarray(ints, np.float64) * np.repeat(np.exp2(np.asarray(sb, np.float64) - 127.0), 32, axis=1)


def out_rounding(ref: np.ndarray, kind: str) -> np.ndarray:
    """Rounding of the stored output: 'f16' 2^-11 |ref| + 2^-25 (subnormal step), 'f32' 2^-24 |ref| (+ fp32's tiny
    subnormal step), 'split' (hi + lo to 22 bits: 2^-22 |ref|, and 2^-25 / scale absolute - the caller adds the latter)."""
    r = np.abs(ref)
    if kind == "f16":
        return U16 * r + F16_SUB
    if kind == "split":
        return 2.0 ** -22 * r
    return U32 * r + 2.0 ** -149


def gemm_epilogue_ref(epi: int, acc, E, S, *, bias, lam=None, x0=None, pos=None, in_scale=1.0, frames_P=None, T=None,
                      n_prefix=0, cos=None, sin=None, D=None, sec0=0):
    """float64 epilogue on the reference accumulator, and the propagated bound (before the output's own rounding).
      PATCH  y = acc in_scale + b (+ pos[p]) scattered to row frame T + n_prefix + p; E' = in_scale E + 2 u32 (|acc in_scale| + |b| + |pos|)
      RESID  y = x + (acc + b) lam;   E' = |lam| (E + u32 |acc + b|) + 2 u32 (|(acc + b) lam| + |y|)
      QKV    v = acc + b; RoPE on patch rows of q, k: v c + rotate_half(v) s; q x 1/8;
             E' = |c| Ev + |s| Ev[partner] + 3 u32 (|v c| + |v_p s|), Ev = E + u32 |v|  (x 1/8 exact)
      GELU   y = gelu(acc + b) (float64 erf); E' = 1.13 (E + u32 |v|) + the caller's implementation term
    Returns (ref rows as stored: [rows][N], bound, valid-row index for PATCH or None)."""
    b = np.asarray(bias, np.float64)[None, :]
    M, N = acc.shape
    if epi == EPI_PATCH:
        v = acc * in_scale + b
        pe = np.zeros_like(v)
        if pos is not None:
            pe = np.asarray(pos, np.float64)[np.arange(M) % frames_P]
        y = v + pe
        Ey = in_scale * E + 2 * U32 * (np.abs(acc * in_scale) + np.abs(b) + np.abs(pe) + np.abs(y))
        frame, p = np.arange(M) // frames_P, np.arange(M) % frames_P
        return y, Ey, frame * T + n_prefix + p
    if epi == EPI_RESID:
        lamv = np.asarray(lam, np.float64)[None, :]
        v = acc + b
        y = np.asarray(x0, np.float64) + v * lamv
        Ey = np.abs(lamv) * (E + U32 * np.abs(v)) + 2 * U32 * (np.abs(v * lamv) + np.abs(y))
        return y, Ey, None
    if epi == EPI_GELU:
        v = acc + b
        y = 0.5 * v * (1.0 + _erf64(v / math.sqrt(2.0)))
        return y, GELU_SLOPE * (E + U32 * np.abs(v)), None
    # EPI_QKV
    v = acc + b
    Ev = E + U32 * np.abs(v)
    y = v.copy()
    Ey = Ev.copy()
    t = np.arange(M) % T
    rows = np.nonzero(t >= n_prefix)[0]
    if cos is not None and len(rows):
        c = np.asarray(cos, np.float64)[t[rows] - n_prefix]
        s = np.asarray(sin, np.float64)[t[rows] - n_prefix]
        for h0 in range(0, N, 64):
            sec = h0 // D + sec0
            if sec >= 2:
                continue
            vh = v[rows, h0:h0 + 64]
            rot = _rotate_half(vh)
            y[rows, h0:h0 + 64] = vh * c + rot * s
            eh = Ev[rows, h0:h0 + 64]
            ep = np.concatenate([eh[:, 32:], eh[:, :32]], axis=1)
            Ey[rows, h0:h0 + 64] = np.abs(c) * eh + np.abs(s) * ep + 3 * U32 * (np.abs(vh * c) + np.abs(rot * s))
    qcols = np.array([(c // D + sec0) == 0 for c in range(N)])
    y[:, qcols] *= 0.125
    Ey[:, qcols] *= 0.125
    return y, Ey, None


# ---- attention --------------------------------------------------------------------------------------------------------
def attention_operands(arith: int, qkv: np.ndarray, D: int):
    """The q, k, v values a kernel multiplies: fp16-rounded (arith 0), fp32 (3), split with the ATT_* scales (4)."""
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D]
    if arith == 0:
        return f16(q), f16(k), f16(v)
    if arith == 4:
        return split_value(q, ATT_QS), split_value(k, ATT_KS), split_value(v, ATT_VS)
    return (np.asarray(q, np.float32).astype(np.float64), np.asarray(k, np.float32).astype(np.float64),
            np.asarray(v, np.float32).astype(np.float64))


def attention_ref(arith: int, qkv: np.ndarray, n: int, T: int, D: int, q_cls=None):
    """softmax(q k^T) v per (frame, head) in float64 on the operands the kernel multiplies (q already carries 1/8), and
    the bound.  With P = softmax row, V = sum_j P_j |v_j| (per output element), Sq = max_j sum_d |q_d k_jd| (per query):
      scores: fp32 accumulation of 64 exact products, 64 u32 Sq (arith 4: + 3 * 2^-22 Sq for the split products), plus the
              exp argument's rounding (u32 |s - m| log2e) - a score error ds moves P_j by at most a factor e^(2 ds);
      probabilities: arith 0 rounds the unnormalised p to fp16 (u16 relative, 2^-25 absolute below 2^-14: T 2^-25 max|v| / l,
              l >= 1); arith 4 splits them x 1024 (2^-22 relative, 2^-25 / 1024 absolute); arith 3 keeps fp32 (exp: 2 u32);
      P.V: fp32 accumulation, T u32 V;   1 / l: the row sum rounded like P (same eta) times |O|;
      output: fp16 (arith 0), fp32 (3), split x 16 (4: 2^-22 |O| + 2^-25 / 16).
    Returns (O [rows][D], bound)."""
    hd = 64
    H = D // hd
    q, k, v = attention_operands(arith, qkv[: n * T], D)
    if q_cls is not None:
        q = attention_operands(arith, np.concatenate([q_cls, q_cls, q_cls], axis=1), D)[0]
        nq = 1
    else:
        nq = T
    qh = q.reshape(n, nq, H, hd).transpose(0, 2, 1, 3)
    kh = k.reshape(n, T, H, hd).transpose(0, 2, 1, 3)
    vh = v.reshape(n, T, H, hd).transpose(0, 2, 1, 3)
    s = qh @ kh.transpose(0, 1, 3, 2)                          # [n][H][nq][T]
    m = s.max(axis=-1, keepdims=True)
    e = np.exp(s - m)
    lsum = e.sum(axis=-1, keepdims=True)
    P = e / lsum
    O = P @ vh
    Vabs = P @ np.abs(vh)
    Sq = (np.abs(qh) @ np.abs(kh).transpose(0, 1, 3, 2)).max(axis=-1, keepdims=True)
    smax = np.abs(s - m).max(axis=-1, keepdims=True)
    ds = 64 * U32 * Sq + U32 * 1.45 * smax + (3 * 2.0 ** -22 * Sq if arith == 4 else 0.0)
    eta = {0: U16, 3: 2 * U32, 4: 2.0 ** -22}[arith]
    absP = {0: F16_SUB, 3: 0.0, 4: F16_SUB / 1024}[arith]
    vmax = np.abs(vh).max(axis=-2, keepdims=True)
    bound = ((eta + 2.5 * ds + T * U32 + 2 * U32) * Vabs + (eta + 2.5 * ds + T * U32) * np.abs(O)
             + T * absP * (vmax + np.abs(O)) / lsum)
    if arith == 0:
        bound = bound + U16 * np.abs(O) + F16_SUB
    elif arith == 4:
        bound = bound + 2.0 ** -22 * np.abs(O) + F16_SUB / ATT_CTX + 2.0 ** -22 * Vabs
    else:
        bound = bound + U32 * np.abs(O)
    to_rows = lambda x: x.transpose(0, 2, 1, 3).reshape(n * nq, D)   # noqa: E731
    return to_rows(O), to_rows(bound)


# ---- row-wise kernels: LayerNorm forms, the MX-fp8 row, the ConvNeXt producers -----------------------------------------
# Accuracy of the device's fp32 division and sqrtf, in units of u32 (half an ulp).  The library is built with hipcc -O3 and
# no fast-math switch (cbas_amd/build.py), so -fhip-fp32-correctly-rounded-divide-sqrt holds (hipcc's default): `/` is
# IEEE-correct (half an ulp = 1 u32); for sqrtf the HIP math API documents 1 ulp (= 2 u32), which is what is budgeted.
DIV_U = 1.0
SQRT_U = 2.0
DW_TAPS = 49


def ln_levels(D: int) -> int:
    """Depth of the kernels' sum over D terms (ln_row / layernorm_f32_kernel / cnx_ln): pairwise inside a 4-vector (2
    levels), one accumulation per vector a lane holds (NV = ceil(D / 256)), then the 6-step xor butterfly.  A value passes
    through at most that many fp32 additions, so the sum is off by at most levels u32 sum |x| to first order."""
    return 2 + (D // 4 + 63) // 64 + 6


def ln_ref(x, gamma, beta, eps, Ex=None):
    """LayerNorm over the last axis with the biased variance, float64: y = (x - mean) / sqrt(var + eps) gamma + beta, eps
    the fp32 value the kernel receives.  Returns (y, bound); the bound follows the kernels' two-pass form, L = ln_levels(D):
      mean   fp32 sum of D terms, then a division:         K = L u32 sum |x| / D + DIV_U u32 |mean|  (+ mean(Ex))
      centre d_i = fl(x_i - mean^): off by the common K (its effect on sum d^2 is D K^2 exactly, as sum c_i = 0) and by
             r_i = u32 (|c_i| + K) (+ Ex_i) of its own
      var    Eq = D K^2 + sum r_i (2 |c_i| + 2 K + r_i) + (L + 1) u32 sum (|c_i| + K + r_i)^2   (squares, sum), then
             t = fl(fl(q / D) + eps): Et = Eq / D + (DIV_U + 1) u32 (t + Eq / D)
      rstd   1 / sqrtf(t): relative rel = |sqrt(t / (t -+ Et)) - 1| + (SQRT_U + DIV_U) u32
      out    y = fl(fl(fl(d rstd) g) + b): E = |g| rstd ((1 + rel) (K + r_i) + |c_i| rel), + 2 u32 (|c rstd g| + E)
             + u32 (|y| + E) for the two products and the sum (a fused multiply-add only removes one of them)
    Ex (optional, shaped like x): what the kernel's input is already off by when x itself is computed on the device (the
    pooled mean, the depthwise convolution).  The output format's rounding is the caller's (out_rounding)."""
    x = np.asarray(x, np.float64)
    g = np.asarray(gamma, np.float64)
    b = np.asarray(beta, np.float64)
    D = x.shape[-1]
    L = ln_levels(D)
    e = float(np.float32(eps))
    ex = np.zeros_like(x) if Ex is None else np.asarray(Ex, np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        mean = x.mean(-1, keepdims=True)
        K = (L * U32 * (np.abs(x) + ex).sum(-1, keepdims=True) / D + DIV_U * U32 * np.abs(mean)) * (1 + 2 * L * U32) \
            + ex.mean(-1, keepdims=True)
        c = x - mean
        ac = np.abs(c)
        r = U32 * (ac + K + ex) + ex
        var = (c * c).mean(-1, keepdims=True)
        Eq = D * K * K + (r * (2 * ac + 2 * K + r)).sum(-1, keepdims=True) + (L + 1) * U32 * ((ac + K + r) ** 2).sum(-1, keepdims=True)
        t = var + e
        Et = Eq / D + (DIV_U + 1) * U32 * (t + Eq / D)
        lo = np.where(t > Et, t - Et, np.nan)                       # the bound is infinite where the variance is lost
        rel = np.maximum(np.sqrt(t / lo) - 1.0, 1.0 - np.sqrt(t / (t + Et))) + (SQRT_U + DIV_U) * U32 * (1 + 2.0 ** -20)
        rel = np.where(np.isfinite(rel), rel, np.inf)
        rstd = 1.0 / np.sqrt(t)
        y = c * rstd * g + b
        E = np.abs(g) * rstd * ((1 + rel) * (K + r) + ac * rel)
        E = E + 2 * U32 * (np.abs(c * rstd * g) + E) + U32 * (np.abs(y) + E)
    return y, E


def stored_bound(ref, E, kind: str) -> np.ndarray:
    """Bound of a row kernel's stored output: E, plus the format's rounding of a value within E of ref ('f16', 'f32', or
    'split' at scale 1: 2^-22 relative and 2^-25 where a half falls below fp16's normal range)."""
    return E + out_rounding(np.abs(ref) + E, kind) + (F16_SUB if kind == "split" else 0.0)


def rows_case(M: int, D: int, seed: int, ld: int | None = None, traps: bool = True):
    """The inputs of a LayerNorm case, shared by the GPU tests and the CPU validation: M random rows [M][ld] (columns past D
    hold 7.0 and are never read), gains and offsets that differ per column, and - when there is room - the trap rows: a
    large mean with a small spread (1e3, sd 1), a constant row, a row with one massive channel."""
    rng = np.random.default_rng(seed)
    ld = ld or D
    x = np.full((M, ld), 7.0, np.float32)
    x[:, :D] = (rng.standard_normal((M, D)) * rng.uniform(0.2, 3.0, (M, 1)) + rng.standard_normal((M, 1))).astype(np.float32)
    if traps:
        x[0, :D] = (1e3 + rng.standard_normal(D)).astype(np.float32)
        if M > 1:
            x[1, :D] = np.float32(2.7182817)
        if M > 2:
            x[2, int(rng.integers(D))] = np.float32(1.0e4)
    gamma = (1.0 + 0.5 * rng.standard_normal(D)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(D)).astype(np.float32)
    return x, gamma, beta


def mx_row_seed(D: int, M: int) -> int:
    """Seed of the LN_F8 GPU case (D, M): tests/test_kernel_reference_bounds.py checks on the CPU that the reference alone
    leaves at most 1 % of a case's blocks within the bound of a scale boundary."""
    return 3000 + D + M + (10000 if (D, M) == (384, 4) else 0)      # 3388 puts 1 of that case's 48 blocks at a boundary


# MX-fp8 row (layernorm_f8_kernel): e4m3 elements, one E8M0 scale byte per 32 columns
def e4m3_half_step(a) -> np.ndarray:
    """Half the spacing of e4m3 at magnitude a (in units of the block scale): 2^(floor(log2 a) - 4), 2^-10 in the subnormal
    range below 2^-6; a value that lands exactly on a power of two from below still rounds within the lower binade's step."""
    a = np.asarray(a, np.float64)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.maximum(a, 2.0 ** -6)))
    return 2.0 ** (np.clip(e, -6, 8) - 4)


def mx_row_decode(bytes8: np.ndarray, sc: np.ndarray, M: int, D: int):
    """out8 [M][D] e4m3 bytes + out_sc [D/128][sc_ld] dwords (byte b of dword (kt, row) = block 4 kt + b) ->
    (values float64 [M][D], scale bytes [M][D/32])."""
    from oracle.mx_oracle import e4m3_decode
    sb = np.ascontiguousarray(sc).view(np.uint8).reshape(D // 128, -1, 4)[:, :M, :]          # [kt][row][b]
    sb = sb.transpose(1, 0, 2).reshape(M, D // 32).astype(np.int32)
    s = 2.0 ** (sb.astype(np.float64) - 127.0)
    v = e4m3_decode(bytes8[:M, :D]).astype(np.float64).reshape(M, D // 32, 32) * s[:, :, None]
    return v.reshape(M, D), sb


def mx_row_bound(y: np.ndarray, E: np.ndarray, sb: np.ndarray) -> np.ndarray:
    """LayerNorm bound E plus the e4m3 half-step at the scale the kernel chose (sb [M][D/32]): the element rounded is
    within E of y, so its magnitude in scale units is at most (|y| + E) / s."""
    s = np.repeat(2.0 ** (sb.astype(np.float64) - 127.0), 32, axis=1)
    return E + s * e4m3_half_step((np.abs(y) + E) / s)


def mx_scale_window(y: np.ndarray, E: np.ndarray):
    """Scale bytes of the reference's 32-column block maxima, pushed down / up by the LayerNorm bound:
    (expected, lowest accepted, highest accepted) [M][D/32]; lowest != highest marks a block within the bound of a boundary."""
    from oracle.mx_oracle import mx_scale_exp
    M, D = y.shape
    a = np.abs(y).reshape(M, D // 32, 32)
    e = E.reshape(M, D // 32, 32)
    return mx_scale_exp(a.max(-1)), mx_scale_exp(np.maximum(a - e, 0.0).max(-1)), mx_scale_exp((a + e).max(-1))


# ConvNeXt producers.  Activations are channels-last [n][h][w][C] float64 views of the fp32 rows.
def cnx_stem_ref(frames: np.ndarray, u8: bool) -> np.ndarray:
    """Stem gather of [n][h][w] green planes: A[(b, oy, ox)][4 i + j] = pixel (4 oy + i, 4 ox + j), u8 as
    np.float32(px / 255.0); columns 16 .. 31 zero.  Exact: returns float32 [n (h/4) (w/4)][32]."""
    n, h, w = frames.shape
    ho, wo = h // 4, w // 4
    v = frames[:, :4 * ho, :4 * wo].reshape(n, ho, 4, wo, 4).transpose(0, 1, 3, 2, 4).reshape(n * ho * wo, 16)
    v = (v.astype(np.float64) / 255.0).astype(np.float32) if u8 else v.astype(np.float32)
    return np.concatenate([v, np.zeros_like(v)], axis=1)


def cnx_downsample_ref(x, gamma, beta, eps):
    """A[(b, oy, ox)][(2 kh + kw) C + c] = LayerNorm(x[b, 2 oy + kh, 2 ox + kw])[c]; the last row / column of an odd grid is
    not read.  Returns (A [n ho wo][4 C], bound)."""
    n, h, w, C = x.shape
    ho, wo = h // 2, w // 2
    y, E = ln_ref(x[:, :2 * ho, :2 * wo], gamma, beta, eps)
    win = lambda t: t.reshape(n, ho, 2, wo, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(n * ho * wo, 4 * C)   # noqa: E731
    return win(y), win(E)


def cnx_dwconv_ref(x, wt, bias):
    """Depthwise 7 x 7, zero padding 3, taps tap-major wt [49][C] (tap = 7 ky + kx reads pixel (y + ky - 3, x + kx - 3)),
    plus bias.  Returns (conv [n][h][w][C], Ex): the kernel's fmaf chain over at most 49 taps and the bias addition are off
    by at most (49 + 1) u32 (sum |w a| + |b|)."""
    x = np.asarray(x, np.float64)
    wt = np.asarray(wt, np.float64)
    n, h, w, C = x.shape
    xp = np.zeros((n, h + 6, w + 6, C))
    xp[:, 3:3 + h, 3:3 + w] = x
    acc = np.zeros_like(x)
    mag = np.zeros_like(x)
    for ky in range(7):
        for kx in range(7):
            p = xp[:, ky:ky + h, kx:kx + w] * wt[7 * ky + kx]
            acc += p
            mag += np.abs(p)
    b = np.asarray(bias, np.float64)
    return acc + b, (DW_TAPS + 1) * U32 * (mag + np.abs(b))


def cnx_dwconv_ln_ref(x, wt, bias, gamma, beta, eps):
    conv, Ex = cnx_dwconv_ref(x, wt, bias)
    n, h, w, C = conv.shape
    y, E = ln_ref(conv.reshape(n * h * w, C), gamma, beta, eps, Ex.reshape(n * h * w, C))
    return y, E


def cnx_pool_ln_ref(x, gamma, beta, eps):
    """LayerNorm(mean over the hw pixels of a frame), x [n][hw][C].  The kernel sums ceil(hw / 4) pixels per wave in order,
    adds the four partial sums in order and divides: Ex = (ceil(hw / 4) + 3) u32 sum |x| / hw + DIV_U u32 |mean|."""
    x = np.asarray(x, np.float64)
    hw = x.shape[1]
    p = x.mean(1)
    Ex = ((hw + 3) // 4 + 3) * U32 * np.abs(x).sum(1) / hw + DIV_U * U32 * np.abs(p)
    return ln_ref(p, gamma, beta, eps, Ex)


def pool_order_f32(x32: np.ndarray) -> np.ndarray:
    """The pooled mean in the kernel's own order, float32: wave w sums pixels w, w + 4, ... in order from +0, then
    ((p0 + p1) + p2) + p3, divided by hw.  x32 [n][hw][C]."""
    x32 = np.asarray(x32, np.float32)
    n, hw, C = x32.shape
    part = np.zeros((4, n, C), np.float32)
    for p in range(hw):
        part[p % 4] = part[p % 4] + x32[:, p]
    return (((part[0] + part[1]) + part[2]) + part[3]) / np.float32(hw)


# ---- classifier head: the exact-fp32 GEMM (gemm_f32.hip) and the small training kernels (head_train_kernels.hip) -------
# Used by tests/test_gpu_head_kernels_reference.py through cbas_debug_head_run.  gemm_f32_kernel issues its MFMAs in the order
# of vit_f32.hip's kernel (both read fragment chunk kk * 4 + (lane >> 4) of gemm_f32_tile.h's rows and loop kt, kk, e):
# f32_mfma_k_order is its k order too.
COLSUM_CHUNKS = 64            # kernels.h
TRAIN_MULTI_MAX = 8
ERF_BF_U = 4.0                # common.h erf_bf inside gelu_erf: the arith-3 budget of the encoder's GELU epilogue, u32 (|v| + |y|)
# Device math library (expf, logf, erff of head_train_kernels.hip).  The ROCm installation's documentation states no ulp
# figures for them, so each budget comes from a measurement on an MI355X against the float64 reference over the inputs of
# tests/test_gpu_head_kernels_reference.py, which prints the figure beside the budget.  A figure is what the library adds
# BEYOND the kernel's own fp32 roundings: from each stored value's error the roundings its bound itemises are taken off first
# (so nothing is budgeted twice), and the rest is divided by the unit the budget multiplies.  The budget is twice the figure,
# rounded up to a whole unit, and never below 1: no fp32 function returns better than half an ulp (1 u32 of its result).
#   GELU_LIB_U   erff and the three roundings inside gelu_erf_lib (x c, 1 + erf, the product); unit u32 (|z| + |gelu z|) scale;
#                itemised and taken off: the product with scale, u32 |ref|.                          measured 0.74 -> 2
#   GELU_GRAD_U  erff, expf and the roundings inside gelu_erf_grad; unit u32 |d| scale (1 + |gelu' z|); taken off: the two
#                products d scale gelu', 2 u32 |ref|.                                                measured 0.75 -> 2
#   CE_LSE_U     expf and logf in lse = mx + logf(sum expf(z - mx)); unit u32 (1 + |log den|); measured on fl(lse - z_y) (cw
#                NULL, eps 0); taken off: u32 (|lse| + |lse - z_y| + C).                              measured 0.00 -> 1
#   CE_P_U       expf in p = expf(z - mx) / den; unit u32 p; measured on p of the classes c != y (cw NULL, eps 0, sums[1] = 1)
#                against the fp32 argument z - mx; taken off: u32 p (C + 2) (the sum, the division).  measured 0.00 -> 1
# The two cross-entropy figures are zero because the itemised terms are worst cases (a sum of C terms seldom rounds C times
# the same way) and cover the library's share as well on these inputs; the budgets are the floor.
GELU_LIB_U = 2.0
GELU_GRAD_U = 2.0
CE_LSE_U = 1.0
CE_P_U = 1.0


def head_gemm_exact(A, W, bias, K: int, splits: int = 1):
    """launch_gemm_f32 without GELU, bit for bit: per split z the fmaf chain over k = z K + f32_mfma_k_order(K) from +0; the
    result is the fp32 sum of the partials, z ascending (launch_splitk_reduce), then ONE fp32 addition of the bias (plain GEMM
    only).  A [M][>= splits K], W [N][>= splits K] fp32 (unread columns are cut off here).  Returns (out fp32, [partials])."""
    A = np.asarray(A, np.float32)
    W = np.asarray(W, np.float32)
    order = f32_mfma_k_order(K)
    parts = [fmaf_chain(A[:, z * K:(z + 1) * K], W[:, z * K:(z + 1) * K], order) for z in range(splits)]
    out = parts[0]
    with np.errstate(over="ignore", invalid="ignore"):
        for z in range(1, splits):
            out = (out + parts[z]).astype(np.float32)
        if bias is not None:
            out = (out + np.asarray(bias, np.float32)[None, :]).astype(np.float32)
    return out, parts


def gelu64(v) -> np.ndarray:
    v = np.asarray(v, np.float64)
    return 0.5 * v * (1.0 + _erf64(v / math.sqrt(2.0)))


def gelu_grad64(v) -> np.ndarray:
    """d/dx gelu(x) = Phi(x) + x phi(x)."""
    v = np.asarray(v, np.float64)
    return 0.5 * (1.0 + _erf64(v / math.sqrt(2.0))) + v * np.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def head_gemm_gelu_ref(pre32):
    """The fused GELU on the EXACT fp32 pre-activation (head_gemm_exact's output): float64 gelu and the bound
    gemm_epilogue_ref + the GPU tests give EPI_GELU of arith 3 with no accumulator error left: the branch-free erf's
    ERF_BF_U u32 (|v| + |y|) and the stored value's fp32 rounding."""
    v = np.asarray(pre32, np.float32).astype(np.float64)
    y = gelu64(v)
    return y, ERF_BF_U * U32 * (np.abs(v) + np.abs(y)) + out_rounding(y, "f32")


def transpose_pad_ref(src, rows: int, cols: int, rows_pad: int) -> np.ndarray:
    """dst [cols][rows_pad] = src[:rows, :cols]^T, columns rows .. rows_pad exact +0."""
    out = np.zeros((cols, rows_pad), np.float32)
    out[:, :rows] = np.asarray(src, np.float32)[:rows, :cols].T
    return out


def colsum_f32(x, scale):
    """launch_colsum in its own order, float32: COLSUM_CHUNKS contiguous ranges of ceil(rows / 64) rows, each summed in row
    order from +0 (tmp [64][cols]; a range past the last row holds +0), the chunks added in order from +0, times scale.
    Returns (tmp, dst)."""
    x = np.asarray(x, np.float32)
    rows, cols = x.shape
    per = -(-rows // COLSUM_CHUNKS)
    tmp = np.zeros((COLSUM_CHUNKS, cols), np.float32)
    for ch in range(COLSUM_CHUNKS):
        for r in range(ch * per, min(ch * per + per, rows)):
            tmp[ch] = tmp[ch] + x[r]
    s = np.zeros(cols, np.float32)
    for ch in range(COLSUM_CHUNKS):
        s = s + tmp[ch]
    return tmp, (s * np.float32(scale)).astype(np.float32)


def colsum_ref(x, scale):
    """float64 column sums times scale, and the independent bound (rows + chunks) u32 sum |x| |scale|: no value passes
    through more than ceil(rows / 64) + 64 additions and one product."""
    x = np.asarray(x, np.float64)
    sc = float(np.float32(scale))
    return x.sum(0) * sc, (x.shape[0] + COLSUM_CHUNKS) * U32 * np.abs(x).sum(0) * abs(sc) + 2.0 ** -149


def sub_colmean_f32(src, colsum) -> np.ndarray:
    """src - colsum[c] / float(rows): one IEEE division and one subtraction per element (no fast-math in the build)."""
    src = np.asarray(src, np.float32)
    return (src - (np.asarray(colsum, np.float32) / np.float32(src.shape[0]))[None, :]).astype(np.float32)


def cov_offdiag_f32(cov, cscale, gscale) -> np.ndarray:
    """G = gscale * (cov * cscale) with the diagonal's factor replaced by +0, float32."""
    v = (np.asarray(cov, np.float32) * np.float32(cscale)).astype(np.float32)
    np.fill_diagonal(v, np.float32(0.0))
    return (np.float32(gscale) * v).astype(np.float32)


def cov_sq_ref(cov, cscale):
    """sq[i] = sum_{j != i} (cov[i][j] cscale)^2 in float64.  Kernel: v = fl(cov cscale) (1 u32), v v (1 u32, or fused), lane l
    adds j = l, l + 64, ... in order (ceil(n / 64) additions), then the 6-level wave_sum: (3 + ceil(n / 64) + 6) u32 sum v^2."""
    c = np.asarray(cov, np.float64) * float(np.float32(cscale))
    np.fill_diagonal(c, 0.0)
    q = (c * c).sum(1)
    n = c.shape[0]
    return q, (3 + (n + 63) // 64 + 6) * U32 * q + 2.0 ** -149


def cov_sq_f32(cov, cscale) -> np.ndarray:
    """cov_offdiag_row's sq in its own order, float32 (unfused): per-lane stride-64 sums, then the xor butterfly 32 .. 1."""
    v = (np.asarray(cov, np.float32) * np.float32(cscale)).astype(np.float32)
    np.fill_diagonal(v, np.float32(0.0))
    n = v.shape[0]
    s = np.zeros((n, 64), np.float32)
    for j0 in range(0, n, 64):
        blk = v[:, j0:j0 + 64]
        s[:, :blk.shape[1]] = s[:, :blk.shape[1]] + blk * blk
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, 0]


def _ce_parts(logits, cw, eps):
    z = np.asarray(logits, np.float32).astype(np.float64)
    C = z.shape[1]
    w = np.ones(C) if cw is None else np.asarray(cw, np.float32).astype(np.float64)
    e32 = np.float32(eps)
    one_m = float(np.float32(1.0) - e32)                      # (1.0f - eps) and eps / (float)C as the kernel forms them
    e_c = float(e32 / np.float32(C))
    mx = z.max(1, keepdims=True)
    ex = np.exp(z - mx)
    den = ex.sum(1, keepdims=True)
    return z, C, w, one_m, e_c, mx, ex, den


def ce_terms_ref(logits, labels, cw, eps):
    """nn.CrossEntropyLoss(weight, label_smoothing) per window, float64 (oracle/head_train_oracle.cross_entropy before its
    sums): terms[w] = [(1 - eps) w[y] (lse - z_y) + eps / C sum_c w[c] (lse - z_c), w[y]].  Bound of the numerator:
      lse = mx + logf(sum expf(z - mx)): E_lse = C u32 (the sum of C terms <= C; a relative error of den is an absolute one
            of its log) + u32 |lse| (the addition) + CE_LSE_U u32 (1 + |log den|) (expf, logf);
      a_c = lse - z_c: E_a = E_lse + u32 |a_c|;   (1 - eps) w[y] a_y: 3 u32 more;   the smoothing sum of C products:
      w_c (E_a + u32 |a_c|) each + (C + 3) u32 sum |w_c a_c| (sum, eps / C, product);   the last addition u32 |ref|.
    w[y] is exact.  Returns (terms [n][2], bound [n][2])."""
    z, C, w, one_m, e_c, mx, ex, den = _ce_parts(logits, cw, eps)
    y = np.asarray(labels, np.int64)
    rows = np.arange(len(y))
    lse = mx + np.log(den)
    a = lse - z
    wy = w[y]
    nll = one_m * wy * a[rows, y]
    smooth = e_c * (w[None, :] * a).sum(1)
    ref = nll + smooth
    E_lse = C * U32 + U32 * np.abs(lse) + CE_LSE_U * U32 * (1.0 + np.abs(np.log(den)))
    E_a = E_lse + U32 * np.abs(a)
    Eb = (one_m * wy * (E_a[rows, y] + 3 * U32 * np.abs(a[rows, y]))
          + e_c * ((w[None, :] * (E_a + U32 * np.abs(a))).sum(1) + (C + 3) * U32 * (w[None, :] * np.abs(a)).sum(1))
          + U32 * (np.abs(nll) + np.abs(smooth)))
    return np.stack([ref, wy], 1), np.stack([Eb * (1 + 2.0 ** -10), np.zeros_like(Eb)], 1)


def ce_grad_ref(logits, labels, cw, eps, sums):
    """d loss / d logits given sums = [sum of numerators, sum of w[y]], float64:
    ((1 - eps) w[y] (p - [c = y]) + eps / C (p sum(w) - w_c)) / sums[1].  Bound: p = expf(z - mx) / den is off by
    E_p = p u32 (CE_P_U + |z - mx| + C + 2) (expf, its argument's rounding, the sum, the division); the bracket adds
    3 u32 |(1 - eps) w[y] (p - [c = y])|, (C + 4) u32 (|p wsum| + |w_c|) eps / C and u32 of the sum; 1 / sums[1] and the last
    product 3 u32 |ref|."""
    z, C, w, one_m, e_c, mx, ex, den = _ce_parts(logits, cw, eps)
    y = np.asarray(labels, np.int64)
    p = ex / den
    oh = np.zeros_like(p)
    oh[np.arange(len(y)), y] = 1.0
    wy = w[y][:, None]
    wsum = w.sum()
    inv = 1.0 / float(np.float32(sums[1]))
    t1 = one_m * wy * (p - oh)
    t2 = e_c * (p * wsum - w[None, :])
    ref = (t1 + t2) * inv
    E_p = p * U32 * (CE_P_U + np.abs(z - mx) + C + 2)
    Eb = (one_m * wy * E_p + 3 * U32 * np.abs(t1) + e_c * (E_p * wsum + (C + 4) * U32 * (p * wsum + w[None, :]))
          + U32 * (np.abs(t1) + np.abs(t2))) * abs(inv) + 3 * U32 * np.abs(ref)
    return ref, Eb * (1 + 2.0 ** -10) + 2.0 ** -149


_M64 = (1 << 64) - 1


def mix64(z):
    """head_train_kernels.hip mix64 (the splitmix64 step and finaliser) on uint64 arrays, wrapping arithmetic;
    tests/test_kernel_reference_bounds.py holds it to oracle/head_train_oracle._mix64."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _unxorshift(x: int, s: int) -> int:
    r = x
    for _ in range(64 // s + 1):
        r = x ^ (r >> s)
    return r


def mix64_inverse(h: int) -> int:
    """The z with mix64(z) = h (every step of the hash is a bijection of 64-bit words)."""
    z = _unxorshift(h, 31)
    z = (z * pow(0x94D049BB133111EB, -1, 1 << 64)) & _M64
    z = _unxorshift(z, 27)
    z = (z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & _M64
    z = _unxorshift(z, 30)
    return (z - 0x9E3779B97F4A7C15) & _M64


def dropout_key_hitting(thr: int, i: int, salt: int = 0) -> int:
    """A stream key whose element i hashes to EXACTLY thr in its top 24 bits (thr < 2^24): the one element at which
    `>= thr` and `> thr` differ."""
    h = ((thr & 0xFFFFFF) << 40) | ((0x123456789A + 7919 * salt) & ((1 << 40) - 1))
    return (mix64_inverse(h) - i) & _M64


def dropout_keep_mask(key: int, n: int, thr: int, offset: int = 0) -> np.ndarray:
    """drop_scale's rule: keep element i <=> mix64(key + i) >> 40 >= thr."""
    with np.errstate(over="ignore"):
        idx = (np.uint64(key) + np.arange(offset, n + offset, dtype=np.uint64))
        return (mix64(idx) >> np.uint64(40)).astype(np.int64) >= int(thr)


def gelu_dropout_fwd_ref(z, key, thr, scale):
    """(kept values gelu(z) scale in float64 with exact zeros elsewhere, bound, keep mask).  gelu_erf_lib: GELU_LIB_U u32
    (|z| + |gelu z|) scale, then the product with scale: u32 |ref|."""
    z = np.asarray(z, np.float32).astype(np.float64)
    sc = float(np.float32(scale))
    keep = dropout_keep_mask(key, z.size, thr)
    g = gelu64(z)
    ref = np.where(keep, g * sc, 0.0)
    bound = np.where(keep, GELU_LIB_U * U32 * (np.abs(z) + np.abs(g)) * sc + U32 * np.abs(ref) + 2.0 ** -149, 0.0)
    return ref, bound, keep


def gelu_dropout_bwd_ref(z, d, key, thr, scale):
    """d scale gelu'(z) where kept, exact zero elsewhere: fl(fl(d s) g'), g' off by GELU_GRAD_U u32 (1 + |g'|)."""
    z = np.asarray(z, np.float32).astype(np.float64)
    d = np.asarray(d, np.float32).astype(np.float64)
    sc = float(np.float32(scale))
    keep = dropout_keep_mask(key, z.size, thr)
    gp = gelu_grad64(z)
    ref = np.where(keep, d * sc * gp, 0.0)
    bound = np.where(keep, GELU_GRAD_U * U32 * np.abs(d) * sc * (1.0 + np.abs(gp)) + 2 * U32 * np.abs(ref) + 2.0 ** -149, 0.0)
    return ref, bound, keep


def adam_corrections(lr, step: int):
    """adam_bias_corrections: (float32(lr / (1 - 0.9^step)), float32(1 / sqrt(1 - 0.999^step))), formed in double."""
    return (np.float32(float(np.float32(lr)) / (1.0 - 0.9 ** step)), np.float32(1.0 / math.sqrt(1.0 - 0.999 ** step)))


def adam_decay(n: int, wd, wd_lo: int, wd_hi: int, wd_special) -> np.ndarray:
    """The decay factor of each element: wd_special on [wd_lo, wd_hi), wd elsewhere (the fp32 values, as float64)."""
    i = np.arange(n)
    return np.where((i >= wd_lo) & (i < wd_hi), float(np.float32(wd_special)), float(np.float32(wd)))


def adam_ref_core(p, g, m, v, lr_c1, c2, wdv):
    """torch.optim.Adam (betas 0.9 / 0.999, eps 1e-8 as fp32 constants, L2 decay wdv added to the gradient) in float64, given
    the corrections lr_c1 = lr / (1 - b1^step) and c2 = 1 / sqrt(1 - b2^step) and the per-element decay wdv.  Returns
    ((p, m, v), (Ep, Em, Ev)); each bound follows adam_element, one u32 per fp32 operation:
      g' = g + wd p                        Eg = u32 (|wd p| + |g'|)
      m' = b1 m + (1 - b1) g'              Em = (1 - b1) Eg + u32 (|b1 m| + |(1 - b1) g'| + |m'|)
      v' = b2 v + ((1 - b2) g') g'         Ev = (1 - b2) Eg (2 |g'| + Eg) + u32 (|b2 v| + 2 (1 - b2) g'^2 + |v'|)
      den = sqrtf(v') c2 + eps             Ed = c2 (sqrt(v') - sqrt(v' - Ev) + SQRT_U u32 sqrt(v')) + u32 (c2 sqrt(v') + den)
      upd = (lr_c1 m') / den               Eu = (lr_c1 Em + |upd| Ed) / (den - Ed) + (1 + DIV_U) u32 |upd|
      p' = p - upd                         Ep = Eu + u32 |p'|"""
    f = lambda t: np.asarray(t, np.float32).astype(np.float64)      # noqa: E731
    p, g, m, v = f(p), f(g), f(m), f(v)
    lr_c1, c2 = float(lr_c1), float(c2)
    wdv = np.asarray(wdv, np.float64)
    b1, b2, eps = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-8))
    omb1, omb2 = float(np.float32(1.0) - np.float32(0.9)), float(np.float32(1.0) - np.float32(0.999))
    gi = g + wdv * p
    mi = b1 * m + omb1 * gi
    vi = b2 * v + omb2 * gi * gi
    s = np.sqrt(vi)
    den = s * c2 + eps
    upd = lr_c1 * mi / den
    pn = p - upd
    Eg = U32 * (np.abs(wdv * p) + np.abs(gi))
    Em = omb1 * Eg + U32 * (np.abs(b1 * m) + np.abs(omb1 * gi) + np.abs(mi))
    Ev = omb2 * Eg * (2 * np.abs(gi) + Eg) + U32 * (np.abs(b2 * v) + 2 * omb2 * gi * gi + np.abs(vi))
    Ed = c2 * (s - np.sqrt(np.maximum(vi - Ev, 0.0)) + SQRT_U * U32 * s) + U32 * (c2 * s + den)
    Eu = (lr_c1 * Em + np.abs(upd) * Ed) / (den - Ed) + (1 + DIV_U) * U32 * np.abs(upd)
    Ep = Eu + U32 * np.abs(pn)
    k = 1 + 2.0 ** -10
    return (pn, mi, vi), (Ep * k + 2.0 ** -149, Em * k + 2.0 ** -149, Ev * k + 2.0 ** -149)


def adam_ref(p, g, m, v, lr, wd, wd_lo, wd_hi, wd_special, step):
    """launch_adam_step in float64: adam_ref_core with wd_special on [wd_lo, wd_hi) and the bias corrections
    adam_bias_corrections hands the kernel (fp32 values)."""
    lr_c1, c2 = adam_corrections(lr, step)
    return adam_ref_core(p, g, m, v, lr_c1, c2, adam_decay(np.asarray(p).size, wd, wd_lo, wd_hi, wd_special))


def adam_f32(p, g, m, v, lr, wd, wd_lo, wd_hi, wd_special, step):
    """adam_element in numpy float32, unfused."""
    f = np.float32
    p, g, m, v = (np.asarray(t, f) for t in (p, g, m, v))
    lr_c1, c2 = adam_corrections(lr, step)
    i = np.arange(p.size)
    wdv = np.where((i >= wd_lo) & (i < wd_hi), f(wd_special), f(wd)).astype(f)
    gi = g + wdv * p
    mi = f(0.9) * m + (f(1.0) - f(0.9)) * gi
    vi = f(0.999) * v + (f(1.0) - f(0.999)) * gi * gi
    pn = p - lr_c1 * mi / (np.sqrt(vi) * c2 + f(1e-8))
    return pn.astype(f), mi.astype(f), vi.astype(f)


# Inputs shared by the GPU tests and the CPU validation of the bounds (tests/test_kernel_reference_bounds.py)
def head_gemm_case(M, N, K, seed, *, N_alloc=None, lda=None, ldw=None, bias=True, nan_row=None):
    """A [M][lda], W [N_alloc][ldw] with NaN in what a launch must not use (columns K .. of A, weight rows N .. N_alloc - 1 are
    read into the tile but feed no stored column), bias [N] or None."""
    rng = np.random.default_rng(seed)
    N_alloc, lda, ldw = N_alloc or N, lda or K, ldw or K
    A = np.full((M, lda), np.nan, np.float32)
    A[:, :K] = rng.standard_normal((M, K)).astype(np.float32)
    W = np.full((N_alloc, ldw), np.nan, np.float32)
    W[:N, :K] = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    if nan_row is not None:
        A[nan_row, K // 2] = np.nan
    b = (0.5 * rng.standard_normal(N)).astype(np.float32) if bias else None
    return A, W, b


def ce_case(n, C, seed, with_cw):
    """logits [n][C] (row 0: +-80, row 1: every maximum tied, row 2: two tied maxima at 80, row 3: +-100), labels, class
    weights or None.  expf(80) = 5.5e34 is still an fp32 number, so a kernel that forgot the max subtraction would get rows
    0 and 2 right; expf(100) overflows, and row 3 is where that defect shows."""
    rng = np.random.default_rng(seed)
    z = (3.0 * rng.standard_normal((n, C))).astype(np.float32)
    z[0] = np.where(np.arange(C) % 2 == 0, 80.0, -80.0)
    if n > 1:
        z[1] = np.float32(1.25)
    if n > 2:
        z[2, 0] = z[2, C - 1] = np.float32(80.0)
    if n > 3:
        z[3] = np.where(np.arange(C) % 2 == 0, -100.0, 100.0)
    y = rng.integers(0, C, n).astype(np.int32)
    y[0] = 1                                                         # the -80 logit carries the label
    cw = (0.25 + 2.0 * rng.random(C)).astype(np.float32) if with_cw else None
    return z, y, cw


def colsum_case(rows, cols, seed):
    """src [rows][cols + 3] (NaN in the three unread columns), columns of different magnitudes; returns (src, ld)."""
    rng = np.random.default_rng(seed)
    ld = cols + 3
    src = np.full((rows, ld), np.nan, np.float32)
    src[:, :cols] = (rng.standard_normal((rows, cols)) * rng.uniform(0.1, 10.0, (1, cols)) + 0.5).astype(np.float32)
    return src, ld


def cov_case(n, seed):
    """A raw Rc^T Rc of n + 5 rows, cscale = 1 / (rows - 1), a gscale that is no power of two."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n + 5, n)).astype(np.float32)
    return (x.T @ x).astype(np.float32), np.float32(1.0 / (n + 4)), np.float32(2.0 / 7.0)


def gelu_case(n, thr, which):
    """z spans [-6, 6] (never 0), d is a gradient without zeros; key `which` (0 / 1) puts element n - 1 resp. n // 2 exactly
    AT thr, the one hash value at which `>= thr` and `> thr` differ.  Returns (z, d, key, scale)."""
    rng = np.random.default_rng(n + thr % 1000 + which)
    z = np.linspace(-6.0, 6.0, n) if n > 1 else np.array([0.8])
    z = (z + rng.uniform(0.001, 0.002, n)).astype(np.float32)
    d = rng.standard_normal(n).astype(np.float32)
    d[d == 0] = 1.0
    key = dropout_key_hitting(thr, (n - 1) if which == 0 else n // 2, salt=which)
    scale = np.float32(1.0 / (1.0 - thr / 2.0 ** 24)) if thr < 2 ** 23 else np.float32(1.5)
    return z, d, key, scale


def adam_case(n, seed):
    """Decay is visible: |p| ~ 10, |g| ~ 0.1, m and v as a previous step leaves them (wd p is comparable to g).  Every 7th
    element is quiet (|p| ~ 1e-2, |g| ~ 1e-5, v ~ 1e-10): there sqrt(v) is comparable to sqrt(eps), so eps's place shows."""
    rng = np.random.default_rng(seed)
    sgn = lambda: np.where(rng.random(n) < 0.5, -1.0, 1.0)           # noqa: E731
    p = sgn() * rng.uniform(5.0, 15.0, n)
    g = sgn() * rng.uniform(0.05, 0.15, n)
    m = 0.1 * sgn() * rng.uniform(0.05, 0.15, n)
    v = 0.001 * rng.uniform(0.05, 0.15, n) ** 2 * 10
    q = np.arange(n) % 7 == 3
    p[q] *= 1e-3
    g[q] *= 1e-4
    m[q] *= 1e-4
    v[q] *= 1e-8
    return tuple(t.astype(np.float32) for t in (p, g, m, v))


def ratio(y, ref, bound) -> float:
    """max |y - ref| / bound (inf where y is not finite)."""
    y = np.asarray(y, np.float64)
    d = np.where(np.isfinite(y), np.abs(y - ref), np.inf)
    return float((d / bound).max()) if d.size else 0.0


# ---- classifier head: the sequential kernels (LSTM, BPTT, attention pooling, centre) -----------------------------------------
# Used by tests/test_gpu_head_seq_reference.py through cbas_debug_head_seq_run.  Plain float64 from the kernels' headers and
# classifier_head.py's mathematics; every bound is fixed from where the kernels round, with u1 = 1.01 * 2^-24:
#   a sum of n products (fmaf chain, MFMA chain, lane partials + a butterfly)       n_levels u1 sum |terms|
#   a libm call (expf, tanhf): the project's budget for one, GELU_LIB_U u32 of the result (1 ulp); expf followed by log1pf
#       (softplus) or by logf: CE_LSE_U u32 (1 + |result|); a division, a product, an addition: u1 of the result
#   tanh_bf: the absolute 6e-8 that common.h CLAIMS for it (the header's figure, not a measurement)
# Where the carried state cannot be observed (inference LSTM, BPTT) the error is propagated to first order in float64 beside
# the values (e_c(t) = f_t e_c(t-1) + ..., likewise e_h, e_dh, e_dc) and the result doubled for the second-order terms.
U1 = 1.01 * U32
TANH_BF_ABS = 6e-8            # common.h: "absolute error ~6e-8"
LIBM_U = GELU_LIB_U           # one libm call, u32 of its result
F32_TINY = 2.0 ** -126        # results below the normal range may be flushed


def _wide(x):
    """fp32 images widened to float64; float64 input (the CPU checks against torch.autograd) passes unrounded."""
    x = np.asarray(x)
    return x if x.dtype == np.float64 else x.astype(np.float32).astype(np.float64)


def _sig64(x):
    return 1.0 / (1.0 + np.exp(-x))


def _sig_err(s, E_x):
    """sigmoidf_(x) = 1 / (1 + expf(-x)) given |error of x| <= E_x: expf's share scales with e / (1 + e) = 1 - s, then the
    addition and the division."""
    return s * (1.0 - s) * E_x + U1 * s * (LIBM_U * (1.0 - s) + 2.0)


def _tanh_err(t, kind):
    return TANH_BF_ABS if kind == "infer" else LIBM_U * U1 * np.abs(t)


def lstm_step64(g, W, hp, cp, e_h, e_c, kind, levels=None):
    """One LSTM step of one direction in float64 with its first-order error.  g [w][4h] (gate order i, f, g, o), W [4h][h],
    hp / cp [w][h] the previous state, e_h / e_c [w][h] the bound on the DEVICE's previous state against hp / cp (zeros:
    teacher-forced).  kind "infer" (MFMA chain, tanh_bf) or "train" (fmaf chain, tanhf).  pre = one fp32 addend + H products:
    (H + 1) u1 (|g| + sum |w| |h|); levels = 1 for permutation weights (one exact product and one rounding whatever the order).
    Returns act [w][4h], c, h, E_act, E_c, E_h."""
    H = W.shape[1]
    levels = H + 1 if levels is None else levels
    aW = np.abs(W)
    pre = g + hp @ W.T
    E_pre = levels * U1 * (np.abs(g) + np.abs(hp) @ aW.T) + e_h @ aW.T
    act = _sig64(pre)
    E_act = _sig_err(act, E_pre)
    gg = np.tanh(pre[:, 2 * H:3 * H])
    act[:, 2 * H:3 * H] = gg
    E_act[:, 2 * H:3 * H] = (1.0 - gg * gg) * E_pre[:, 2 * H:3 * H] + _tanh_err(gg, kind)
    i, f, o = act[:, :H], act[:, H:2 * H], act[:, 3 * H:]
    Ei, Ef, Eg, Eo = E_act[:, :H], E_act[:, H:2 * H], E_act[:, 2 * H:3 * H], E_act[:, 3 * H:]
    c = f * cp + i * gg
    E_c = f * e_c + np.abs(cp) * Ef + np.abs(gg) * Ei + i * Eg + 2.0 * U1 * (np.abs(f * cp) + np.abs(i * gg))
    tc = np.tanh(c)
    h = o * tc
    E_h = np.abs(tc) * Eo + o * ((1.0 - tc * tc) * E_c + _tanh_err(tc, kind)) + U1 * np.abs(h)
    return act, c, h, E_act, E_c, E_h


def lstm_fwd_ref(gin, w_hh, kind, levels=None):
    """Free-running bidirectional LSTM forward: gin [w][T][8h], w_hh [2][4h][h] (the fp32 values widened).  Direction 1 runs
    t = T-1 .. 0.  Returns dict act [w][T][8h], c, h [w][T][2h], their propagated bounds E_* (already doubled) and one-step
    bounds S_* (the same step with an exact previous state)."""
    gin = _wide(gin)
    W = _wide(w_hh)
    nw, T, G8 = gin.shape
    H = G8 // 8
    out = {k: np.zeros((nw, T, 8 * H)) for k in ("act", "E_act", "S_act")}
    out.update({k: np.zeros((nw, T, 2 * H)) for k in ("c", "h", "E_c", "E_h", "S_c", "S_h")})
    z = np.zeros((nw, H))
    for d in range(2):
        hp, cp, e_h, e_c = z, z, z, z
        for s in range(T):
            t = T - 1 - s if d else s
            g = gin[:, t, d * 4 * H:(d + 1) * 4 * H]
            act, c, h, Ea, Ec, Eh = lstm_step64(g, W[d], hp, cp, e_h, e_c, kind, levels)
            _, _, _, Sa, Sc, Sh = lstm_step64(g, W[d], hp, cp, z, z, kind, levels)
            for k, v in (("act", act), ("E_act", 2 * Ea), ("S_act", Sa)):
                out[k][:, t, d * 4 * H:(d + 1) * 4 * H] = v
            for k, v in (("c", c), ("h", h), ("E_c", 2 * Ec), ("E_h", 2 * Eh), ("S_c", Sc), ("S_h", Sh)):
                out[k][:, t, d * H:(d + 1) * H] = v
            hp, cp, e_h, e_c = h, c, Eh, Ec
    return out


def lstm_infer_ref(gin, w_hh, lo, hi, levels=None):
    """head_lstm's output [w][hi-lo][2h] and its bound: the forward direction runs steps 0 .. hi-1, the reverse T-1 .. lo, so
    rows [lo, hi) of the full run are what it stores."""
    r = lstm_fwd_ref(gin, w_hh, "infer", levels)
    return r["h"][:, lo:hi], r["E_h"][:, lo:hi], r


def lstm_train_fwd_teacher_ref(gin, w_hh, cst_dev, hout_dev, levels=None):
    """lstm_train_fwd step by step from the DEVICE's own previous c and h (teacher-forced): only the one-step bound applies."""
    gin = _wide(gin)
    W = _wide(w_hh)
    cd = _wide(cst_dev)
    hd = _wide(hout_dev)
    nw, T, G8 = gin.shape
    H = G8 // 8
    out = {k: np.zeros((nw, T, 8 * H)) for k in ("act", "S_act")}
    out.update({k: np.zeros((nw, T, 2 * H)) for k in ("c", "h", "S_c", "S_h")})
    z = np.zeros((nw, H))
    for d in range(2):
        for s in range(T):
            t = T - 1 - s if d else s
            tp = t + 1 if d else t - 1
            hp = hd[:, tp, d * H:(d + 1) * H] if s else z
            cp = cd[:, tp, d * H:(d + 1) * H] if s else z
            act, c, h, Sa, Sc, Sh = lstm_step64(gin[:, t, d * 4 * H:(d + 1) * 4 * H], W[d], hp, cp, z, z, "train", levels)
            out["act"][:, t, d * 4 * H:(d + 1) * 4 * H] = act
            out["S_act"][:, t, d * 4 * H:(d + 1) * 4 * H] = Sa
            for k, v in (("c", c), ("h", h), ("S_c", Sc), ("S_h", Sh)):
                out[k][:, t, d * H:(d + 1) * H] = v
    return out


def lstm_bwd_ref(dhout, act, cst, hout, w_hh):
    """BPTT from the saved images (the very fp32 values handed to the device, widened): returns dgin [w][T][8h], hprev [w][T][2h]
    (hout of the step that fed t, +0 at a direction's first step: exact), the propagated bound E (doubled) and the one-step
    bound S of dgin.  The recurrences: dh = dhout + dh_rec, dc = dc_rec + dh o (1 - tanh^2 c), dc_rec' = dc f,
    dh_rec' = W^T da.  Rounding: 1 - x^2 is absolute u1 (x^2 + |1 - x^2|); a product of k factors k u1; dh_rec' is four fmaf
    chains of H and two levels of additions: (H + 2) u1 sum |w| |da|."""
    dh_in = _wide(dhout)
    A = _wide(act)
    Cc = _wide(cst)
    Hh = _wide(hout)
    W = _wide(w_hh)
    nw, T, G8 = A.shape
    H = G8 // 8
    dgin, E, S = np.zeros_like(A), np.zeros_like(A), np.zeros_like(A)
    hprev = np.zeros_like(Hh)
    z = np.zeros((nw, H))

    def step(a, c, cp, dho, dh_rec, dc_rec, e_dh, e_dc):
        ig, fg, gg, og = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
        tc = np.tanh(c)
        E_tc = LIBM_U * U1 * np.abs(tc)
        dh = dho + dh_rec
        E_dh = e_dh + U1 * np.abs(dh)
        s = 1.0 - tc * tc
        E_s = 2.0 * np.abs(tc) * E_tc + U1 * (tc * tc + np.abs(s))
        term = dh * og * s
        E_term = np.abs(og * s) * E_dh + np.abs(dh * og) * E_s + 2.0 * U1 * np.abs(term)
        dc = dc_rec + term
        E_dc = e_dc + E_term + U1 * np.abs(dc)
        dai = dc * gg * ig * (1.0 - ig)
        daf = dc * cp * fg * (1.0 - fg)
        s2 = 1.0 - gg * gg
        dag = dc * ig * s2
        dao = dh * tc * og * (1.0 - og)
        E_da = np.concatenate([
            np.abs(gg * ig * (1.0 - ig)) * E_dc + 4.0 * U1 * np.abs(dai),
            np.abs(cp * fg * (1.0 - fg)) * E_dc + 4.0 * U1 * np.abs(daf),
            np.abs(ig * s2) * E_dc + np.abs(dc * ig) * U1 * (gg * gg + np.abs(s2)) + 2.0 * U1 * np.abs(dag),
            np.abs(tc * og * (1.0 - og)) * E_dh + np.abs(dh * og * (1.0 - og)) * E_tc + 4.0 * U1 * np.abs(dao)], 1)
        da = np.concatenate([dai, daf, dag, dao], 1)
        return da, E_da, dc * fg, fg * E_dc + U1 * np.abs(dc * fg)

    for d in range(2):
        Wd, aW = W[d], np.abs(W[d])
        dh_rec, dc_rec, e_dh, e_dc = z, z, z, z
        sl4, sl = slice(d * 4 * H, (d + 1) * 4 * H), slice(d * H, (d + 1) * H)
        for st in range(T - 1, -1, -1):
            t = T - 1 - st if d else st
            tp = t + 1 if d else t - 1
            cp = Cc[:, tp, sl] if st else z
            hprev[:, t, sl] = Hh[:, tp, sl] if st else 0.0
            da, E_da, dc_next, e_dc_next = step(A[:, t, sl4], Cc[:, t, sl], cp, dh_in[:, t, sl], dh_rec, dc_rec, e_dh, e_dc)
            _, S_da, _, _ = step(A[:, t, sl4], Cc[:, t, sl], cp, dh_in[:, t, sl], dh_rec, dc_rec, z, z)
            dgin[:, t, sl4], E[:, t, sl4], S[:, t, sl4] = da, 2.0 * E_da, S_da
            dh_rec = da @ Wd
            e_dh = E_da @ aW + (H + 2) * U1 * (np.abs(da) @ aW)
            dc_rec, e_dc = dc_next, e_dc_next
    return dgin, hprev, E + F32_TINY, S + F32_TINY


def softplus_temp_ref(raw):
    """softplus(raw) + 1e-3 with the kernel's switch at raw > 20 (fp32 raw), its derivative, and the bound of the value:
    expf + log1pf CE_LSE_U u32 (1 + |softplus|), the addition u1."""
    raw = float(np.float32(raw))
    k = float(np.float32(1e-3))
    if raw > 20.0:
        return raw + k, 1.0, U1 * (raw + k), 0.0
    sp = math.log1p(math.exp(raw))
    sg = 1.0 / (1.0 + math.exp(-raw))
    return sp + k, sg, CE_LSE_U * U1 * (1.0 + abs(sp)) + U1 * (sp + k), float(_sig_err(sg, 0.0))


def _attention64(hc, w_att, b_att, temp, E_temp, levels):
    """scores, softmax weights and latent of attention pooling over hc [w][nc][H2] with their bounds.  A score is H2 products
    summed in `levels` roundings, + b, / temp; the weight e_t / den: expf's argument carries both scores' errors and one
    subtraction, expf LIBM_U, den nc additions, the division; the latent nc more."""
    nc = hc.shape[1]
    dot = hc @ w_att
    adot = np.abs(hc) @ np.abs(w_att)
    sc = (dot + b_att) / temp
    E_sc = (levels * U1 * adot + U1 * np.abs(dot + b_att)) / abs(temp) + np.abs(sc) * (E_temp / abs(temp) + U1)
    mx = sc.max(1, keepdims=True)
    E_arg = E_sc + E_sc.max(1, keepdims=True) + U1 * np.abs(sc - mx)
    e = np.exp(sc - mx)
    den = e.sum(1, keepdims=True)
    aw = e / den
    R = E_arg + LIBM_U * U1                                    # relative error of e_t
    R_aw = R + R.max(1, keepdims=True) + (nc + 1) * U1         # ... of e_t / den
    lat = (aw[:, :, None] * hc).sum(1)
    E_lat = ((aw * (R_aw + (nc + 2) * U1))[:, :, None] * np.abs(hc)).sum(1) + F32_TINY
    return sc, E_sc, aw, aw * R_aw + F32_TINY, lat, E_lat


def _lerp_bound(lin, lstm, E_lstm, g, E_g):
    """final = lerp(lin, lstm, g) in either of torch.lerp's forms (mathematically one value): the larger of the two forms'
    roundings."""
    d = lstm - lin
    E_d = E_lstm + U1 * np.abs(d)
    fin = lin + g * d
    lo_form = abs(g) * E_d + np.abs(d) * E_g + U1 * np.abs(g * d) + U1 * np.abs(fin)
    hi_form = E_lstm + abs(1.0 - g) * E_d + np.abs(d) * (E_g + U1 * abs(1.0 - g)) + U1 * np.abs(d * (1.0 - g)) + U1 * np.abs(fin)
    return fin, np.maximum(lo_form, hi_form)


def pool_infer_ref(hout, lin_logits, w_att, b_att, att_temp, w_lin2, b_lin2, gate_sigmoid, temperature):
    """head_pool: hout [w][nc][H2] -> latent [w][H2], logits = lerp(lin, latent W2^T + b2, g) [w][C], probs =
    softmax(logits / max(1e-3, temperature)).  A lane holds per = ceil(H2 / 64) columns; wave sums add 6 levels.  Returns
    (probs, logits, latent), (E_probs, E_logits, E_latent)."""
    hc = _wide(hout)
    lin = _wide(lin_logits)
    wa = _wide(w_att)
    W2 = _wide(w_lin2)
    b2 = _wide(b_lin2)
    H2 = hc.shape[2]
    levels = (H2 + 63) // 64 + 7
    _, _, _, _, lat, E_lat = _attention64(hc, wa, float(np.float32(b_att)), float(np.float32(att_temp)), 0.0, levels)
    lstm = lat @ W2.T + b2
    E_lstm = E_lat @ np.abs(W2).T + levels * U1 * (np.abs(lat) @ np.abs(W2).T) + U1 * np.abs(lstm)
    g = float(np.float32(gate_sigmoid))
    fin, E_fin = _lerp_bound(lin, lstm, E_lstm, g, 0.0)
    tdiv = max(float(np.float32(1e-3)), float(np.float32(temperature)))
    zz = fin / tdiv
    E_z = E_fin / tdiv + U1 * np.abs(zz)
    zmax = zz.max(1, keepdims=True)
    e = np.exp(zz - zmax)
    p = e / e.sum(1, keepdims=True)
    Rp = E_z + E_z.max(1, keepdims=True) + U1 * np.abs(zz - zmax) + LIBM_U * U1
    E_p = p * (Rp + Rp.max(1, keepdims=True) + (6 + 1) * U1) + F32_TINY      # the wave sum of the exponentials, the division
    return (p, fin, lat), (E_p, E_fin, E_lat)


def pool_train_fwd_ref(hout, lin_logits, w_att, b_att, raw_temp, w_lin2, b_lin2, raw_gate, lo, hi):
    """pool_train_fwd on hout [w][T][H2], rows [lo, hi): attw, scores [w][nc], latent [w][H2], lstm_logits, final_logits [w][C]
    and their bounds.  block_sum: a product, 6 butterfly levels, up to 4 waves: 11 roundings."""
    hc = _wide(hout)[:, lo:hi]
    lin = _wide(lin_logits)
    wa = _wide(w_att)
    W2 = _wide(w_lin2)
    b2 = _wide(b_lin2)
    H2 = hc.shape[2]
    temp, _, E_temp, _ = softplus_temp_ref(raw_temp)
    sc, E_sc, aw, E_aw, lat, E_lat = _attention64(hc, wa, float(np.float32(b_att)), temp, E_temp, 11)
    lstm = lat @ W2.T + b2
    E_lstm = E_lat @ np.abs(W2).T + (H2 + 1) * U1 * (np.abs(lat) @ np.abs(W2).T + np.abs(b2))
    g = float(_sig64(float(np.float32(raw_gate))))
    fin, E_fin = _lerp_bound(lin, lstm, E_lstm, g, float(_sig_err(g, 0.0)))
    return (aw, sc, lat, lstm, fin), (E_aw, E_sc, E_lat, E_lstm, E_fin)


def pool_train_bwd_ref(hout, lin_logits, w_att, raw_temp, w_lin2, raw_gate, lo, hi, attw, scores, lstm_logits, dfinal, dlat_cov):
    """pool_train_bwd from the saved attw / scores / lstm_logits images (fp32, widened): dhout [w][T][H2] (exactly +0 outside
    [lo, hi)), dlstm_logits, dlin_logits [w][C], part [w][H2 + 12] = [d w_att | d b_att,0,0,0 | d gate,0,0,0 | d att_temp,0,0,0]
    and their bounds (see the derivation beside each line)."""
    f64 = _wide
    hf, lin, wa, W2, aw, sc, lstm, df = (f64(x) for x in (hout, lin_logits, w_att, w_lin2, attw, scores, lstm_logits, dfinal))
    nw, T, H2 = hf.shape
    C = lin.shape[1]
    nc = hi - lo
    hc = hf[:, lo:hi]
    temp, dsp, E_temp, E_dsp = softplus_temp_ref(raw_temp)
    g = float(_sig64(float(np.float32(raw_gate))))
    E_g = float(_sig_err(g, 0.0))
    dl = g * df
    E_dl = np.abs(df) * E_g + U1 * np.abs(dl)
    dlin = (1.0 - g) * df
    E_dlin = np.abs(df) * (E_g + U1 * (1.0 - g)) + U1 * np.abs(dlin)
    P = g * (1.0 - g)                                            # d gate: sum_c df (lstm - lin) g (1 - g), a block sum
    E_P = (1.0 - g) * E_g + g * (E_g + U1 * (1.0 - g)) + U1 * P
    term = df * (lstm - lin) * P
    dgate = term.sum(1)
    E_dgate = (np.abs(df * (lstm - lin)) * E_P + 4.0 * U1 * np.abs(term)).sum(1) + 11 * U1 * np.abs(term).sum(1)
    dlat = dl @ W2 + (f64(dlat_cov) if dlat_cov is not None else 0.0)       # fmaf chain over the classes
    E_dlat = E_dl @ np.abs(W2) + (C + 1) * U1 * (np.abs(dl) @ np.abs(W2) + (np.abs(f64(dlat_cov)) if dlat_cov is not None else 0.0))
    dav = np.einsum("wu,wtu->wt", dlat, hc)                      # block sums
    E_dav = np.einsum("wu,wtu->wt", E_dlat, np.abs(hc)) + 11 * U1 * np.einsum("wu,wtu->wt", np.abs(dlat), np.abs(hc))
    dot = (aw * dav).sum(1, keepdims=True)                       # fmaf chain over the steps
    E_dot = (aw * E_dav).sum(1, keepdims=True) + (nc + 1) * U1 * np.abs(aw * dav).sum(1, keepdims=True)
    ds = aw * (dav - dot)
    E_ds = aw * (E_dav + E_dot + U1 * np.abs(dav - dot)) + U1 * np.abs(ds)
    q = ds / temp
    E_q = E_ds / temp + np.abs(q) * (E_temp / temp + U1)
    dh = np.zeros_like(hf)
    E_dhout = np.zeros_like(hf)
    dh[:, lo:hi] = aw[:, :, None] * dlat[:, None, :] + q[:, :, None] * wa[None, None, :]
    E_dhout[:, lo:hi] = (aw[:, :, None] * E_dlat[:, None, :] + E_q[:, :, None] * np.abs(wa)[None, None, :]
                         + 2.0 * U1 * (np.abs(aw[:, :, None] * dlat[:, None, :]) + np.abs(q[:, :, None] * wa[None, None, :])) + F32_TINY)
    dwatt = np.einsum("wt,wtu->wu", q, hc)
    E_dwatt = np.einsum("wt,wtu->wu", E_q, np.abs(hc)) + (nc + 1) * U1 * np.einsum("wt,wtu->wu", np.abs(q), np.abs(hc))
    dbatt = q.sum(1)
    E_dbatt = E_q.sum(1) + nc * U1 * np.abs(q).sum(1)
    r = ds * sc / temp
    dtemp = -r.sum(1)
    E_dtemp = (np.abs(sc / temp) * E_ds + np.abs(r) * (E_temp / temp + 2.0 * U1)).sum(1) + nc * U1 * np.abs(r).sum(1)
    part = np.zeros((nw, H2 + 12))
    E_part = np.zeros((nw, H2 + 12))
    part[:, :H2], E_part[:, :H2] = dwatt, E_dwatt + F32_TINY
    part[:, H2], E_part[:, H2] = dbatt, E_dbatt + F32_TINY
    part[:, H2 + 4], E_part[:, H2 + 4] = dgate, E_dgate + F32_TINY
    part[:, H2 + 8] = dtemp * dsp
    E_part[:, H2 + 8] = dsp * E_dtemp + np.abs(dtemp) * E_dsp + U1 * np.abs(dtemp * dsp) + F32_TINY
    return (dh, dl, dlin, part), (E_dhout, E_dl + F32_TINY, E_dlin + F32_TINY, E_part)


def centre_ref(xl):
    """head_centre: xl [w][T][L0] minus its time mean; the mean is a sequential sum of T terms and a division, then one
    subtraction: (T + 2) u1 of the magnitudes involved."""
    x = _wide(xl)
    T = x.shape[1]
    m = x.mean(1, keepdims=True)
    am = np.abs(x).mean(1, keepdims=True)
    return x - m, (T + 2) * U1 * (am + np.abs(x - m)) + F32_TINY


def lstm_case(nw, T, h, seed, row_l1=0.5, gin_amp=3.0):
    """gin in +-gin_amp and W_hh whose rows have sum |w| = row_l1: a contraction, so that the propagated bound stays within a
    small multiple of the one-step bound."""
    rng = np.random.default_rng(seed)
    gin = rng.uniform(-gin_amp, gin_amp, (nw, T, 8 * h)).astype(np.float32)
    W = rng.standard_normal((2, 4 * h, h))
    W *= row_l1 * 0.999 / np.abs(W).sum(2, keepdims=True)
    return gin, W.astype(np.float32)


def lstm_perm_weights(h, seed=0):
    """W_hh[dir][g h + u][k] = 2^-s(g, dir) if k = pi_{g,dir}(u) else 0: a different permutation and shift per gate and direction, so
    every pre-activation is one fp32 addend plus one exact product."""
    rng = np.random.default_rng(1000 + h + seed)
    W = np.zeros((2, 4 * h, h), np.float32)
    for d in range(2):
        for g in range(4):
            pi = rng.permutation(h)
            W[d, g * h + np.arange(h), pi] = 2.0 ** -(1 + g + 4 * d)
    return W


LSTM_H = (16, 32, 48, 64, 80, 96, 112, 128)
LSTM_NW_INFER = (1, 15, 16, 17, 33)
LSTM_NW_TRAIN = (1, 3)
LSTM_T = (1, 2, 3, 7, 31)
RANGE_KINDS = ("full", "centre3", "first", "last", "centre1")


def centre_range(kind, T):
    """[lo, hi) of a range kind; centre3 is (T/2 - 1, T/2 + 2) where T holds it, else the full range."""
    if kind == "first":
        return 0, 1
    if kind == "last":
        return T - 1, T
    if kind == "centre1":
        return T // 2, T // 2 + 1
    if kind == "centre3" and T >= 5:
        return T // 2 - 1, T // 2 + 2
    return 0, T


def lstm_suite_cases():
    """The covering set of the LSTM tests: 40 cases (h, nw_infer, nw_train, T, kind, lo, hi) in which every h, window count, T
    and range kind appears with at least two different h (tests/test_kernel_reference_bounds.py asserts the coverage)."""
    cases = []
    for i in range(40):
        r = i // 8
        h = LSTM_H[i % 8]
        T = LSTM_T[(i + r) % 5]
        kind = RANGE_KINDS[(3 * i + 2 * r) % 5]
        lo, hi = centre_range(kind, T)
        cases.append((h, LSTM_NW_INFER[(2 * i + r) % 5], LSTM_NW_TRAIN[(i + r) % 2], T, kind, lo, hi))
    return cases


# pooling shapes of the suite.  Training (H2, C, hi - lo, raw att_temp): H2 = 32, 96, 224 leave dead threads in the last wave,
# hi - lo = 128 fills the score buffer, raw = 25 takes softplus' linear branch.  Inference (H2, C, hi - lo, windows, gate_sigmoid,
# temperature): both lerp forms and g = 0.5 itself, 1e-4 is clamped to 1e-3, four windows per block.
POOL_TRAIN_CASES = [(32, 1, 1, -2.0), (96, 7, 3, 0.5), (128, 64, 128, 25.0), (224, 1, 3, 25.0), (256, 7, 128, -2.0), (32, 64, 3, 0.5),
                    (96, 64, 1, 25.0), (224, 7, 1, 0.5), (256, 1, 128, 0.5), (128, 7, 3, -2.0)]
POOL_INFER_CASES = [(32, 1, 1, 1, 0.3, 1.0), (96, 2, 3, 3, 0.5, 0.5), (128, 7, 31, 4, 0.7, 1e-4), (160, 64, 1, 5, 0.5, 1.0), (224, 2, 31, 1, 0.7, 0.5),
                    (256, 7, 3, 4, 0.3, 1e-4), (32, 64, 31, 5, 0.7, 1.0), (96, 1, 3, 4, 0.3, 0.5), (160, 7, 1, 3, 0.3, 1e-4), (256, 64, 3, 1, 0.5, 0.5),
                    (224, 64, 31, 3, 0.3, 1.0), (128, 2, 1, 5, 0.7, 1.0)]


def pool_case(nw, H2, C, nc, seed, train, temp=0.75, gap=False):
    """Operands of one pooling launch: hout in +-1 like an LSTM's output ([nw][T][H2] with T = nc + 3 and [lo, hi) = [1, nc + 1)
    for training, hout_c = its rows [lo, hi)), w_att scaled by the temperature so that the scores' spread is about one - the
    attention softmax is neither flat nor one-hot.  gap: row 0 of window 0 scores 150 above the rest (expf underflows to 0)."""
    rng = np.random.default_rng(seed)
    T, lo = (nc + 3, 1) if train else (nc, 0)
    hi = lo + nc
    hout = rng.uniform(-1, 1, (nw, T, H2)).astype(np.float32)
    w_att = (rng.standard_normal(H2) * 1.5 * temp / math.sqrt(H2)).astype(np.float32)
    if gap:
        hout[0, lo] = (np.sign(w_att) * 150.0 * temp / np.abs(w_att).sum()).astype(np.float32)
    return dict(hout=hout, hout_c=np.ascontiguousarray(hout[:, lo:hi]), lin=rng.standard_normal((nw, C)).astype(np.float32), w_att=w_att,
                b_att=float(np.float32(0.125)), att_temp=float(np.float32(temp)), gate=0.25,
                w_lin2=(rng.standard_normal((C, H2)) / math.sqrt(H2)).astype(np.float32), b_lin2=rng.standard_normal(C).astype(np.float32),
                lo=lo, hi=hi, T=T)


# ---- classifier head: the expand kernels (head_expand, train_expand_fwd, train_expand_bwd) -----------------------------------
# Used by tests/test_gpu_head_expand_reference.py through cbas_debug_head_expand_run.  Written from classifier_head.py's
# definition on the PROJECTED rows (the bottleneck Linears and lin1 commute with the EMA and the zero-sum stencils): stream k
# of window w is Op_k(P[w][:, k Bn : (k + 1) Bn]) + b_bott, GELU, dropout, LayerNorm(Bn); the linear branch is the mean over
# [lo, hi) of EMA(P[w][:, F : F + C]) + b_lin1.  Bounds are sums of the terms named beside each line, in u1 = 1.01 u32 like the
# section above; the LayerNorm terms are ln_ref's (ln_stats_ref returns its intermediate quantities for the backward).
EXPAND_EPS = 1e-5
EXPAND_T_MAX = 101
EXPAND_SLACK = 1.0 + 2.0 ** -10      # second-order terms of the backward's products of bounds


def expand_temporal_ref(T, alpha, lo, hi):
    """_calculate_robust_deltas as matrices over the window's positions, float64: E (the EMA: x_smooth = E x), D (dx[:, 1:]) and
    A (ddx) on the reflect-padded [s2, s1 | s0, s1, ..], and the centre mean of E's rows [lo, hi).  alpha is the fp32 value."""
    a = float(np.float32(alpha))
    t = np.arange(T)[:, None]
    s = np.arange(T)[None, :]
    E = np.where(s <= t, np.where(s == 0, 1.0, a) * (1.0 - a) ** np.maximum(t - s, 0), 0.0)
    pad = np.concatenate([E[[2, 1]], E], 0)                  # F.pad(.., (2, 0), 'reflect')
    dx = pad[1:] - pad[:-1]
    ddx = dx[1:] - dx[:-1]
    return E, dx[1:], ddx, E[lo:hi].mean(0)


def expand_lds_bytes(T, Bn, NPROJ, fwd, big):
    """head_train_kernels.hip expand_lds."""
    if big:
        return (T * 3 * Bn + 12 * T) * 4
    return (T * NPROJ + 3 * T * T + T * 3 * Bn) * 4 if fwd else (3 * T * T + T * 3 * Bn + 12 * T) * 4


def expand_is_big(T, Bn, NPROJ):
    return max(expand_lds_bytes(T, Bn, NPROJ, True, False), expand_lds_bytes(T, Bn, NPROJ, False, False)) > 160 * 1024


def expand_rows(nw, T, sliding, w0=0, r0=0, n_frames=0):
    """proj row of (w, t): w T + t, or in sliding mode clamp(w0 + w + t - T // 2, 0, n_frames - 1) - r0."""
    if not sliding:
        return np.arange(nw * T, dtype=np.int64).reshape(nw, T)
    f = w0 + np.arange(nw, dtype=np.int64)[:, None] + np.arange(T, dtype=np.int64)[None, :] - T // 2
    return np.clip(f, 0, n_frames - 1) - r0


def _ema64(x, a):
    """s_0 = x_0, s_t = s_{t-1} + a (x_t - s_{t-1}) along axis 1 in float64, and the bound of the fp32 recurrence in EITHER form
    (e0 + a * (x - e0) with the product rounded, or contracted into one fma): the difference and the product round once each
    (2 u1 a |x - s|, the contracted form only the first), the sum once (u1 |s_t|), and the step's incoming error is carried
    through (1 - a); (1 + 4 u1) covers the roundings of the error itself."""
    s = np.empty_like(x)
    E = np.zeros_like(x)
    s[:, 0] = x[:, 0]
    for t in range(1, x.shape[1]):
        d = x[:, t] - s[:, t - 1]
        s[:, t] = s[:, t - 1] + a * d
        E[:, t] = ((1.0 - a) * E[:, t - 1] + U1 * (2.0 * a * np.abs(d) + np.abs(s[:, t]))) * (1.0 + 4.0 * U1)
    return s, E


def expand_infer_ref(X, alpha, b_bott, ln_w, ln_b, b_lin1, Bn, NS, C, lo, hi):
    """head_expand on the gathered rows X [w][T][>= NS Bn + C]: (aug [w][T][NS Bn], lin_logits [w][C]) and their bounds.
      EMA      _ema64 (both lerp forms)
      d1, d2   differences of the rounded EMA values a, b, c = s_t, s_|t-1|, s_|t-2| (the reflect padding): each subtraction
               carries its operands' bounds and rounds once (it is exact only where Sterbenz' lemma applies)
      + bias   u1 |pre|;  gelu_erf: GELU_SLOPE E_pre + ERF_BF_U u32 (|pre| + |g|) + u32 |g| (head_gemm_gelu_ref's terms)
      LN       ln_ref over Bn with that input error (per + 5 <= ln_levels(Bn) additions per value)
      lin      the EMA of the lin1 columns, hi - lo sequential additions, a division, + b_lin1"""
    X = _wide(X)
    a = float(np.float32(alpha))
    nw, T = X.shape[:2]
    F = NS * Bn
    s, Es = _ema64(X[:, :, :F], a)
    i1, i2 = np.abs(np.arange(T) - 1), np.abs(np.arange(T) - 2)
    b, Eb, c, Ec = s[:, i1], Es[:, i1], s[:, i2], Es[:, i2]
    d1 = s - b
    E1 = Es + Eb + U1 * np.abs(d1)
    bc = b - c
    Ebc = Eb + Ec + U1 * np.abs(bc)
    d2 = d1 - bc
    E2 = E1 + Ebc + U1 * np.abs(d2)
    k = (np.arange(F) // Bn)[None, None, :]
    v = np.where(k == 0, s, np.where(k == 1, d1, d2))
    Ev = np.where(k == 0, Es, np.where(k == 1, E1, E2))
    pre = v + _wide(b_bott)
    Epre = Ev * (1.0 + U1) + U1 * np.abs(pre)
    g = gelu64(pre)
    Eg = GELU_SLOPE * Epre + ERF_BF_U * U32 * (np.abs(pre) + Epre + np.abs(g)) + U32 * np.abs(g) + 2.0 ** -149
    aug, Eaug = ln_ref(g.reshape(nw, T, NS, Bn), _wide(ln_w).reshape(NS, Bn), _wide(ln_b).reshape(NS, Bn), EXPAND_EPS, Eg.reshape(nw, T, NS, Bn))
    sl, El = _ema64(X[:, :, F:F + C], a)
    n = hi - lo
    acc = sl[:, lo:hi].sum(1)
    Eacc = El[:, lo:hi].sum(1) + (n - 1) * U1 * (np.abs(sl[:, lo:hi]) + El[:, lo:hi]).sum(1)
    mean = acc / n
    Emean = Eacc / n + U1 * (np.abs(mean) + Eacc / n)
    lin = mean + _wide(b_lin1)
    Elin = Emean + U1 * (np.abs(lin) + Emean) + 2.0 ** -149
    return (aug.reshape(nw, T, F), lin), (Eaug.reshape(nw, T, F), Elin)


def expand_keep_mask(keys, nw, T, Bn, NS, thr):
    """[w][T][NS][Bn]: stream k keeps element (w, t, c) <=> its hash at index (w T + t) Bn + c of the stream's OWN (B, T, Bn)
    tensor under the stream's key reaches thr."""
    return np.stack([dropout_keep_mask(int(keys[k]), nw * T * Bn, thr).reshape(nw, T, Bn) for k in range(NS)], 2)


def _expand_dropped_gelu(y, keep, scale):
    """U = gelu_erf_lib(y) drop_scale and its bound (gelu_dropout_fwd_ref's terms); a dropped element is exactly zero."""
    g = gelu64(y)
    U = np.where(keep, g * scale, 0.0)
    return U, np.where(keep, GELU_LIB_U * U32 * (np.abs(y) + np.abs(g)) * scale + U32 * np.abs(U) + 2.0 ** -149, 0.0)


def expand_train_fwd_ref(proj, tmat, lin_vec, b_bott, ln_w, ln_b, b_lin1, Bn, NS, C, keys, thr, scale):
    """train_expand_fwd on proj [w][T][NPROJ] with the temporal operators as operands.  fp32 operands: Y and lin_logits are the
    kernel's bits (the fmaf chain over s = 0 .. T - 1 from +0, then ONE fp32 addition of the bias), and aug is judged against
    float64 from those Y.  float64 operands (the CPU check against autograd): everything in float64.  Returns a dict: Y, lin
    (fp32 bit for bit, or float64), aug and E_aug (the dropped GELU's bound through ln_ref), U, keep."""
    P = np.asarray(proj)
    exact = P.dtype != np.float64
    nw, T, _ = P.shape
    F = NS * Bn
    tm = np.asarray(tmat).reshape(3, T, T)
    if exact:
        Y = np.empty((nw, T, F), np.float32)
        for k in range(NS):
            cols = np.ascontiguousarray(P[:, :, k * Bn:(k + 1) * Bn].transpose(0, 2, 1)).reshape(nw * Bn, T)
            Y[:, :, k * Bn:(k + 1) * Bn] = fmaf_chain(tm[k], cols).reshape(T, nw, Bn).transpose(1, 0, 2)
        with np.errstate(over="ignore", invalid="ignore"):
            Y = (Y + np.asarray(b_bott, np.float32)).astype(np.float32)
            lc = np.ascontiguousarray(P[:, :, F:F + C].transpose(0, 2, 1)).reshape(nw * C, T)
            lin = (fmaf_chain(np.asarray(lin_vec, np.float32)[None, :], lc).reshape(nw, C) + np.asarray(b_lin1, np.float32)).astype(np.float32)
    else:
        Y = np.einsum("kts,wskc->wtkc", tm[:NS], P[:, :, :F].reshape(nw, T, NS, Bn)).reshape(nw, T, F) + np.asarray(b_bott)
        lin = np.einsum("s,wsc->wc", np.asarray(lin_vec), P[:, :, F:F + C]) + np.asarray(b_lin1)
    keep = expand_keep_mask(keys, nw, T, Bn, NS, thr)
    U, EU = _expand_dropped_gelu(_wide(Y).reshape(nw, T, NS, Bn), keep, float(np.float32(scale)))
    aug, Eaug = ln_ref(U, _wide(ln_w).reshape(NS, Bn), _wide(ln_b).reshape(NS, Bn), EXPAND_EPS, EU)
    return dict(Y=Y, lin=lin, aug=aug.reshape(nw, T, F), E_aug=Eaug.reshape(nw, T, F), U=U, keep=keep)


def ln_stats_ref(x, eps, Ex=None):
    """ln_ref's intermediate quantities (same derivation, same symbols): mean, c = x - mean, rstd, and the bounds K (common
    offset of the centred values), r (each centred value's own error) and rel (relative error of rstd)."""
    x = np.asarray(x, np.float64)
    D = x.shape[-1]
    L = ln_levels(D)
    e = float(np.float32(eps))
    ex = np.zeros_like(x) if Ex is None else np.asarray(Ex, np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        mean = x.mean(-1, keepdims=True)
        K = (L * U32 * (np.abs(x) + ex).sum(-1, keepdims=True) / D + DIV_U * U32 * np.abs(mean)) * (1 + 2 * L * U32) + ex.mean(-1, keepdims=True)
        c = x - mean
        ac = np.abs(c)
        r = U32 * (ac + K + ex) + ex
        var = (c * c).mean(-1, keepdims=True)
        Eq = D * K * K + (r * (2 * ac + 2 * K + r)).sum(-1, keepdims=True) + (L + 1) * U32 * ((ac + K + r) ** 2).sum(-1, keepdims=True)
        t = var + e
        Et = Eq / D + (DIV_U + 1) * U32 * (t + Eq / D)
        lo = np.where(t > Et, t - Et, np.nan)
        rel = np.maximum(np.sqrt(t / lo) - 1.0, 1.0 - np.sqrt(t / (t + Et))) + (SQRT_U + DIV_U) * U32 * (1 + 2.0 ** -20)
        rel = np.where(np.isfinite(rel), rel, np.inf)
    return dict(mean=mean, c=c, rstd=1.0 / np.sqrt(t), K=K, r=r, rel=rel, var=var)


def expand_train_bwd_ref(Y, daug, dlin, tmat, lin_vec, ln_w, Bn, NS, C, NPROJ, keys, thr, scale):
    """train_expand_bwd from a saved Y [w][T][NS Bn]: (dproj [w][T][NPROJ], part [w][3 NS Bn] = [d b_bott | d ln_w | d ln_b]) and
    their bounds.  With L = ln_levels(Bn), per (w, t, k) row and its element c:
      U, xhat   the dropped GELU (bound as in the forward) and (U - mean) rstd with ln_stats_ref's K, r, rel, one product
      dxh       daug ln_w, one rounding; s1 = sum dxh / Bn and s2 = sum dxh xhat / Bn: the terms' errors, L roundings of the
                sum (lane partials and the butterfly), the division
      du        rstd (daug ln_w - s1 - xhat s2): four roundings inside the bracket, rstd's rel, one product
      dyv       fl(fl(du scale) gelu'(y)) where kept (gelu_dropout_bwd_ref's terms), exactly zero where dropped
      part      three sums over t in kernel order: the terms' errors + T u1 sum |terms| (dgam's product adds one more)
      dproj     bottleneck columns: the fmaf chain over t of tmat[k][t][s] dyv_t: sum |tm| E_dyv + T u1 sum |tm dyv|;
                lin1 columns: the ONE product lin_vec[s] dlin[w][c], bit for bit (bound 0); padding columns: +0 (bound 0)."""
    y = np.asarray(Y)
    exact = y.dtype != np.float64
    nw, T, F = y.shape
    y = _wide(y).reshape(nw, T, NS, Bn)
    dy = _wide(daug).reshape(nw, T, NS, Bn)
    gam = _wide(ln_w).reshape(NS, Bn)
    tm = _wide(np.asarray(tmat).reshape(3, T, T))[:NS]
    sc = float(np.float32(scale))
    L = ln_levels(Bn)
    keep = expand_keep_mask(keys, nw, T, Bn, NS, thr)
    U, EU = _expand_dropped_gelu(y, keep, sc)
    st = ln_stats_ref(U, EXPAND_EPS, EU)
    rstd, rel = st["rstd"], st["rel"]
    xhat = st["c"] * rstd
    Ex = rstd * ((1 + rel) * (st["K"] + st["r"]) + np.abs(st["c"]) * rel)
    Ex = Ex + U1 * (np.abs(xhat) + Ex)
    dxh = dy * gam
    Edxh = U1 * np.abs(dxh)
    s1 = dxh.mean(-1, keepdims=True)
    Es1 = (Edxh.sum(-1, keepdims=True) + L * U1 * np.abs(dxh).sum(-1, keepdims=True)) / Bn
    Es1 = Es1 + U1 * (np.abs(s1) + Es1)
    term = dxh * xhat
    Eterm = np.abs(dxh) * Ex + Edxh * (np.abs(xhat) + Ex) + 2 * U1 * np.abs(term)
    s2 = term.mean(-1, keepdims=True)
    Es2 = (Eterm.sum(-1, keepdims=True) + L * U1 * (np.abs(term) + Eterm).sum(-1, keepdims=True)) / Bn
    Es2 = Es2 + U1 * (np.abs(s2) + Es2)
    inner = dxh - s1 - xhat * s2
    Einner = (Es1 + np.abs(xhat) * Es2 + np.abs(s2) * Ex + Ex * Es2
              + U1 * (np.abs(dxh) + np.abs(dxh - s1) + np.abs(xhat * s2) + np.abs(inner))) * EXPAND_SLACK
    du = rstd * inner
    Edu = rstd * (Einner * (1 + rel) + np.abs(inner) * rel)
    Edu = Edu + U1 * (np.abs(du) + Edu)
    gp = gelu_grad64(y)
    dyv = np.where(keep, du * sc * gp, 0.0)
    Edyv = np.where(keep, Edu * sc * np.abs(gp) + GELU_GRAD_U * U32 * (np.abs(du) + Edu) * sc * (1.0 + np.abs(gp)) + 2 * U32 * np.abs(dyv) + 2.0 ** -149, 0.0) * EXPAND_SLACK
    part = np.concatenate([dyv.sum(1).reshape(nw, F), (dy * xhat).sum(1).reshape(nw, F), dy.sum(1).reshape(nw, F)], 1)
    Epart = np.concatenate([(Edyv.sum(1) + T * U1 * (np.abs(dyv) + Edyv).sum(1)).reshape(nw, F),
                            ((np.abs(dy) * Ex).sum(1) + (T + 1) * U1 * (np.abs(dy) * (np.abs(xhat) + Ex)).sum(1)).reshape(nw, F),
                            (T * U1 * np.abs(dy).sum(1)).reshape(nw, F)], 1) * EXPAND_SLACK + F32_TINY
    dproj = np.zeros((nw, T, NPROJ))
    Edproj = np.zeros((nw, T, NPROJ))
    dproj[:, :, :F] = np.einsum("kts,wtkc->wskc", tm, dyv).reshape(nw, T, F)
    Edproj[:, :, :F] = (np.einsum("kts,wtkc->wskc", np.abs(tm), Edyv)
                        + T * U1 * np.einsum("kts,wtkc->wskc", np.abs(tm), np.abs(dyv) + Edyv)).reshape(nw, T, F) * EXPAND_SLACK + F32_TINY
    lp = _wide(lin_vec)[None, :, None] * _wide(dlin)[:, None, :]          # exact in float64: 24 + 24 bits
    with np.errstate(over="ignore", invalid="ignore"):
        dproj[:, :, F:F + C] = lp.astype(np.float32).astype(np.float64) if exact else lp
    return (dproj, part), (Edproj, Epart), dict(keep=keep, rel=rel, var=st["var"], xhat=xhat)


# The suite's shapes, shared by tests/test_gpu_head_expand_reference.py and tests/test_kernel_reference_bounds.py (which checks the
# coverage, the conditioning and every planted defect on exactly these).
EXPAND_BN_NS = ((64, 2), (64, 3), (128, 3), (256, 3))
EXPAND_INFER_T = (3, 4, 15, 31)
EXPAND_TRAIN_T = (3, 15, 31)
EXPAND_INFER_C = (1, 3, 64)
EXPAND_TRAIN_C = (1, 3, 4, 64)
EXPAND_NW = (1, 2, 5)
EXPAND_THR_HALF = 1 << 23            # floor(0.5 * 2^24)


def round_up(n, m):
    return (n + m - 1) // m * m


def expand_big_threshold(Bn, NS, C):
    """(T, T + 1): the longest window whose training forms are resident in LDS and the shortest that takes the big form."""
    NP = round_up(NS * Bn + C, 4)
    T = 3
    while not expand_is_big(T + 1, Bn, NP):
        T += 1
    return T, T + 1


def expand_infer_cases():
    """(Bn, NS, T, C, kind, lo, hi, nw): every value of each list with every (Bn, NS) where the count allows, C = 64 at (64, 2)
    (thread 63 is a linear-branch thread), and the shortest T of the training suite's big form at Bn = 256."""
    cases = []
    for i in range(24):
        r = i // 4
        Bn, NS = EXPAND_BN_NS[i % 4]
        T = EXPAND_INFER_T[(i + r) % 4]
        C = EXPAND_INFER_C[(i + r) % 3]
        kind = RANGE_KINDS[(i + 2 * r) % 5]
        cases.append((Bn, NS, T, C, kind) + centre_range(kind, T) + (EXPAND_NW[(i + r) % 3],))
    cases.append((64, 2, 15, 64, "centre3") + centre_range("centre3", 15) + (2,))
    Tb = expand_big_threshold(256, 3, 4)[1]
    cases.append((256, 3, Tb, 4, "centre3") + centre_range("centre3", Tb) + (1,))
    return cases


def expand_train_cases():
    """(Bn, NS, T, C, thr, nw): the (Bn, NS) set with every T, C and both thresholds, both sides of the big threshold at
    Bn = 256 (NS = 3, C = 4), and the big form at Bn = 64 with the longest window served."""
    cases = []
    for i in range(16):
        r = i // 4
        Bn, NS = EXPAND_BN_NS[i % 4]
        cases.append((Bn, NS, EXPAND_TRAIN_T[(i + r) % 3], EXPAND_TRAIN_C[(i + r) % 4], (0, EXPAND_THR_HALF)[(i + r // 2) % 2], EXPAND_NW[(i + r) % 3]))
    lo_T, hi_T = expand_big_threshold(256, 3, 4)
    cases += [(256, 3, lo_T, 4, EXPAND_THR_HALF, 2), (256, 3, hi_T, 4, EXPAND_THR_HALF, 2), (64, 3, EXPAND_T_MAX, 4, EXPAND_THR_HALF, 1),
              (64, 2, 15, 64, 0, 1), (128, 3, 3, 2, 0, 1)]                   # C = 2: the only class count here that leaves 2 padding columns
    return cases


def expand_case(nw, T, Bn, NS, C, seed, thr=0, amp=2.0):
    """Operands of one expand launch: proj [nw][T][NPROJ] in about +-amp with finite padding columns (the GPU tests poison
    them), biases and LayerNorm parameters away from the trivial 0 / 1, cotangents for the backward, three distinct stream keys
    of which key k makes element 7 + k of its stream hash to exactly thr."""
    rng = np.random.default_rng(seed)
    F = NS * Bn
    NP = round_up(F + C, 4)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(proj=(f(nw, T, NP) * np.float32(amp)), b_bott=f(F) * np.float32(0.5), ln_w=(1 + 0.3 * f(F)).astype(np.float32), ln_b=f(F) * np.float32(0.3),
                b_lin1=f(C), daug=f(nw, T, F), dlin=f(nw, C), NPROJ=NP, keys=[dropout_key_hitting(thr, 7 + k, salt=seed + k) for k in range(3)],
                thr=thr, scale=float(np.float32(1.0 / (1.0 - thr / 2.0 ** 24))))


EXPAND_ALPHA = 0.3
# sliding inference at T = 7 (Bn = 64, NS = 3, C = 3): (n_frames, w0, windows).  With 1, 2 and 5 frames every row is clamped; in the
# clip of 40, w0 = 0 clamps at the first frame, 17 is interior, 35 and 38 end past the last frame
EXPAND_SLIDING = [(1, 0, 3), (2, 0, 2), (2, 1, 1), (5, 0, 5), (5, 3, 4), (40, 0, 2), (40, 17, 5), (40, 35, 5), (40, 38, 2)]


def expand_sliding_layout(n_frames, w0, nw, T):
    """(r0, rows [nw][T], image rows) of a sliding case: the image starts one frame before the first frame the windows read
    (r0 > 0 wherever that frame exists) and ends two rows after the last - rows no window may touch."""
    f = np.clip(w0 + np.arange(nw, dtype=np.int64)[:, None] + np.arange(T, dtype=np.int64)[None, :] - T // 2, 0, n_frames - 1)
    r0 = max(int(f.min()) - 1, 0)
    return r0, f - r0, int(f.max()) - r0 + 3


def expand_seed(Bn, T, C, nw):
    return Bn + 3 * T + C + nw


_expand_cache = {}


def expand_infer_suite_case(case):
    """(operands, (aug, lin), (E_aug, E_lin)) of one expand_infer_cases() entry, computed once per process."""
    if ("i", case) not in _expand_cache:
        Bn, NS, T, C, kind, lo, hi, nw = case
        p = expand_case(nw, T, Bn, NS, C, expand_seed(Bn, T, C, nw))
        ref, E = expand_infer_ref(p["proj"], EXPAND_ALPHA, p["b_bott"], p["ln_w"], p["ln_b"], p["b_lin1"], Bn, NS, C, lo, hi)
        _expand_cache[("i", case)] = (p, ref, E)
    return _expand_cache[("i", case)]


def expand_train_suite_case(case):
    """(operands, tmat, lin_vec, forward reference, Y for the backward, backward reference) of one expand_train_cases() entry,
    computed once per process.  tmat / lin_vec: expand_temporal_ref at the centre3 window, rounded to fp32.  The backward is
    judged on its own: its Y is the float64 forward's (operands widened), rounded to fp32 - not the device's."""
    if ("t", case) not in _expand_cache:
        Bn, NS, T, C, thr, nw = case
        p = expand_case(nw, T, Bn, NS, C, expand_seed(Bn, T, C, nw), thr)
        E, D, A, lv = expand_temporal_ref(T, EXPAND_ALPHA, *centre_range("centre3", T))
        tm, lv = np.stack([E, D, A]).astype(np.float32), lv.astype(np.float32)
        fw = expand_train_fwd_ref(p["proj"], tm, lv, p["b_bott"], p["ln_w"], p["ln_b"], p["b_lin1"], Bn, NS, C, p["keys"], thr, p["scale"])
        w = lambda x: np.asarray(x, np.float64)
        f64 = expand_train_fwd_ref(w(p["proj"]), w(tm), w(lv), w(p["b_bott"]), p["ln_w"], p["ln_b"], w(p["b_lin1"]), Bn, NS, C, p["keys"], thr, p["scale"])
        Yb = f64["Y"].astype(np.float32)
        bw = expand_train_bwd_ref(Yb, p["daug"], p["dlin"], tm, lv, p["ln_w"], Bn, NS, C, p["NPROJ"], p["keys"], thr, p["scale"])
        _expand_cache[("t", case)] = (p, tm, lv, fw, Yb, bw)
    return _expand_cache[("t", case)]


# ---- ViT ingest and the create-time weight packers: exact references -----------------------------------------------------------
# Used by tests/test_gpu_ingest_reference.py through cbas_debug_pack_run.  Written from the contracts in csrc/kernels.h (the slot
# layout of the ingest launchers, the packers' sums and index formulas), not from the kernels; every one has an exact answer, so
# there are no bounds here.  tests/test_kernel_reference_bounds.py ties the slot layout to oracle/vit_oracle.embeddings.
def vit_im2col_ref(green, ps: int):
    """The patch matrix of [n][h][w] planes in the 16 x 16 slot layout: A[b P + py nw + px][16 i + j] = pixel (py ps + i,
    px ps + j) for i, j < ps, in the planes' own dtype; P = nh nw whole patches, the rows and columns past them are not read.
    Returns (A [n P][256], owned [256]): owned marks the slots a launch writes, i < ps (zeros where j >= ps); the slot rows
    i >= ps are never written and hold 0 here."""
    g = np.asarray(green)
    n, h, w = g.shape
    nh, nw = h // ps, w // ps
    A = np.zeros((n, nh, nw, 16, 16), g.dtype)
    for py in range(nh):
        for px in range(nw):
            A[:, py, px, :ps, :ps] = g[:, py * ps:(py + 1) * ps, px * ps:(px + 1) * ps]
    return A.reshape(n * nh * nw, 256), (np.arange(256) // 16) < ps


def u8_to_unit_f32(p) -> np.ndarray:
    """backend/cbas.py:431 on one byte: the float64 quotient p / 255.0, rounded once to float32."""
    return np.float32(np.float64(p) / 255.0)


def f16_pair(v):
    """(hi, lo) fp16 of fp32 values: hi = RNE fp16(v), lo = RNE fp16(v - hi) with the difference taken in fp32 (the K = 512 ingest
    form, launch_convert_f16, launch_pack_patch_weight).  Beyond 65504 hi is an infinity and lo the opposite one."""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def split_operand_bits(x, scale: float) -> np.ndarray:
    """The split image of rows [R][K] fp32 (K % 32 == 0) as uint16 [R][2 K], the inverse of decode_split_operand: K-tile t of a
    row is 64 halves = [hi 32 | lo 32] of x * scale, the value of column 32 t + 16 h + 4 g + e at position 8 g + 4 h + e."""
    x = np.asarray(x, np.float32)
    R, K = x.shape
    hi, lo = f16_pair(x * np.float32(scale))
    k = np.arange(32)
    pos = 8 * ((k % 16) // 4) + 4 * (k // 16) + k % 4
    img = np.zeros((R, K // 32, 2, 32), np.uint16)
    img[:, :, 0, pos] = hi.view(np.uint16).reshape(R, K // 32, 32)
    img[:, :, 1, pos] = lo.view(np.uint16).reshape(R, K // 32, 32)
    return img.reshape(R, 2 * K)


def patch_weight_ref(w, ps: int, wide: bool = False) -> np.ndarray:
    """The patch weight (D, 3, ps, ps) summed over its 3 input channels (the model sees 3 identical ones) as (c0 + c1) + c2, in the
    slot layout [D][16 i + j], zero where i >= ps or j >= ps.  wide = False: the sum in float32 (launch_pack_patch_weight, which
    then splits it with f16_pair); wide = True: in float64, rounded once to float32 (launch_pack_patch_weight_f32)."""
    w = np.asarray(w, np.float32)
    D = w.shape[0]
    c = w.astype(np.float64) if wide else w
    s = ((c[:, 0] + c[:, 1]) + c[:, 2]).astype(np.float32)
    out = np.zeros((D, 16, 16), np.float32)
    out[:, :ps, :ps] = s
    return out.reshape(D, 256)


def interleave_ref(gate, up) -> np.ndarray:
    """launch_interleave_gate_up: out [2 F][K], rows [64 b, 64 b + 32) = gate rows [32 b, 32 b + 32), rows [64 b + 32, 64 b + 64) =
    the up rows of the same outputs; F % 32 == 0."""
    gate, up = np.asarray(gate), np.asarray(up)
    F, K = gate.shape
    out = np.empty((2 * F, K), gate.dtype)
    for b in range(F // 32):
        out[64 * b:64 * b + 32] = gate[32 * b:32 * b + 32]
        out[64 * b + 32:64 * b + 64] = up[32 * b:32 * b + 32]
    return out


def fp8_weight_ref(w, sc_image, n_total: int, n0: int):
    """launch_pack_fp8_weight on w [N][K] (K % 128 == 0): oracle.mx_oracle.mx_quant's e4m3 elements [N][K] (in units of their
    block's scale) and the scale image after the call - a copy of sc_image [K / 128][n_total] dwords with the E8M0 byte of block
    (n, k / 32) placed in dword (k / 128) * n_total + n0 + n, byte (k % 128) / 32 (little endian); every other byte as it was."""
    from oracle.mx_oracle import mx_quant
    w = np.asarray(w, np.float32)
    N, K = w.shape
    _, q, sb = mx_quant(w)
    img = np.array(sc_image, np.uint32).reshape(K // 128, n_total).view(np.uint8).reshape(K // 128, n_total, 4)
    for kb in range(K // 32):
        img[kb // 4, n0:n0 + N, kb % 4] = sb[:, kb]
    return q, img.reshape(K // 128, n_total * 4).view(np.uint32)


def ingest_float_planes(n: int, h: int, w: int, ps: int, seed: int) -> np.ndarray:
    """The float frames of the ingest tests, fp32 [n][h][w]: the pixels past the last whole patch hold NaN (never read); the
    pixels read hold, at random places, 0, -0.0, 1.0, the 256 values k / 255, values below 2^-14 (hi subnormal) and below 2^-24
    (hi zero or the smallest subnormal), and uniforms in [0, 1) everywhere else."""
    rng = np.random.default_rng(seed)
    nh, nw = h // ps, w // ps
    m = n * nh * ps * nw * ps
    tiny = [2.0 ** -14, 1.5 * 2.0 ** -15, 2.0 ** -14 - 2.0 ** -25, 1.3 * 2.0 ** -20, -1.3 * 2.0 ** -20, 2.0 ** -24, 3 * 2.0 ** -25,
            2.0 ** -25, 1.0001 * 2.0 ** -25, 2.0 ** -26, 1.7 * 2.0 ** -30, 2.0 ** -126, 2.0 ** -149]
    special = np.concatenate([[0.0, -0.0, 1.0], np.arange(256) / 255.0, tiny]).astype(np.float32)
    vals = rng.random(m, np.float32)
    assert m >= 2 * len(special)
    vals[rng.permutation(m)[:len(special)]] = special
    g = np.full((n, h, w), np.nan, np.float32)
    g[:, :nh * ps, :nw * ps] = vals.reshape(n, nh * ps, nw * ps)
    return g
