"""Single GEMM and attention launches against float64 references (oracle/kernel_ref.py), element by element.

Each case feeds host operands to ONE library launch through cbas_debug_gemm_run / cbas_debug_attention_run (debug build)
and asserts, for every output element, |kernel - reference| <= the bound derived from where that kernel rounds; the
measured max |error| / bound is printed per case (run with -s to see it).  Besides the bound:
  - precision 3 (fp32 operands): the accumulator equals the k-ordered fmaf chain BIT FOR BIT, and so do the residual and
    q|k|v epilogues written with their rounding points;
  - every output element outside rows < M and columns < N (canaries, and the prefix rows of the patch scatter) is
    untouched byte for byte, and A rows between M and M_alloc hold NaN: they must change nothing;
  - a NaN / inf in one row of A makes that row non-finite and leaves every other row bit-identical;
  - split operands (precision 4) whose scaled high half overflows fp16 give non-finite rows, never finite wrong ones;
    values just inside fp16's range and values whose low halves are fp16 subnormals meet the bound.
Attention sweeps T over every dispatch bucket of launch_attention / launch_attention_f32 and both sides of each boundary,
with a cross-frame leakage trap (the next frame's first keys and the rows past the last frame score huge against this
frame's queries), the largest logit on key T - 1, logits near +-60, uniform keys, and (split kernel) more (frame, head)
items than two per CU so the persistent workgroups walk several."""
import ctypes as C

import numpy as np
import pytest

from cbas_amd import _lib
from oracle import kernel_ref as R

pytestmark = pytest.mark.gpu

c_int, c_int64, c_float, c_void_p = C.c_int, C.c_int64, C.c_float, C.c_void_p


class GemmArgs(C.Structure):            # include/cbas_mi355x_debug.h cbas_debug_gemm_args
    _fields_ = [("struct_bytes", c_int64)] + [(n, c_int) for n in (
        "arith", "epi", "tile", "forms", "group_m", "M", "M_alloc", "N", "K", "lda", "ldo", "D", "sec0",
        "T", "n_prefix", "P", "rope_nh", "rope_nw", "rope_lds", "out_rows")] + [(n, c_float) for n in (
        "in_scale", "a_scale", "w_scale", "out_scale")] + [(n, c_void_p) for n in (
        "A", "W", "bias", "lam", "pos", "rope_cos", "rope_sin", "out")]


class AttnArgs(C.Structure):            # cbas_debug_attention_args
    _fields_ = [("struct_bytes", c_int64)] + [(n, c_int) for n in (
        "arith", "n", "T", "D", "n_heads", "rows_alloc", "out_rows")] + [(n, c_void_p) for n in ("qkv", "q_cls", "out")]


CANARY32 = np.float32(-31337.25)
CANARY16 = np.float16(-1234.0)
ROPE_THETA = 100.0


def _ptr(a):
    return None if a is None else a.ctypes.data


def gemm_run(arith, epi, A, W, bias, *, M, out, tile=0, forms=-1, group_m=0, lam=None, pos=None, cos=None, sin=None,
             D=0, sec0=0, T=0, n_prefix=0, P=0, nh=0, nw=0, rope_lds=0, in_scale=1.0, a_scale=1.0, w_scale=1.0, out_scale=1.0):
    """One launch; `out` (np array [out_rows][ldo], native width) is updated in place.  A is [M_alloc][lda] fp32."""
    lib = _lib.load()
    f32 = lambda x: None if x is None else np.ascontiguousarray(x, np.float32)   # noqa: E731
    A, W, bias, lam, pos, cos, sin = map(f32, (A, W, bias, lam, pos, cos, sin))
    a = GemmArgs()
    a.struct_bytes = C.sizeof(GemmArgs)
    a.arith, a.epi, a.tile, a.forms, a.group_m = arith, epi, tile, forms, group_m
    a.M, a.M_alloc, a.N, a.K, a.lda, a.ldo = M, A.shape[0], W.shape[0], W.shape[1], A.shape[1], out.shape[1]
    a.D, a.sec0, a.T, a.n_prefix, a.P, a.rope_nh, a.rope_nw, a.rope_lds, a.out_rows = D, sec0, T, n_prefix, P, nh, nw, rope_lds, out.shape[0]
    a.in_scale, a.a_scale, a.w_scale, a.out_scale = in_scale, a_scale, w_scale, out_scale
    a.A, a.W, a.bias, a.lam, a.pos, a.rope_cos, a.rope_sin = map(_ptr, (A, W, bias, lam, pos, cos, sin))
    assert out.flags.c_contiguous
    a.out = out.ctypes.data
    _lib.check(lib.cbas_debug_gemm_run(C.byref(a)), f"cbas_debug_gemm_run(arith {arith}, epi {epi}, tile {tile})")
    return out


def attn_run(arith, qkv, n, T, D, out, q_cls=None):
    lib = _lib.load()
    qkv = np.ascontiguousarray(qkv, np.float32)
    q_cls = None if q_cls is None else np.ascontiguousarray(q_cls, np.float32)
    a = AttnArgs()
    a.struct_bytes = C.sizeof(AttnArgs)
    a.arith, a.n, a.T, a.D, a.n_heads, a.rows_alloc, a.out_rows = arith, n, T, D, D // 64, qkv.shape[0], out.shape[0]
    a.qkv, a.q_cls, a.out = _ptr(qkv), _ptr(q_cls), out.ctypes.data
    _lib.check(lib.cbas_debug_attention_run(C.byref(a)), f"cbas_debug_attention_run(arith {arith}, T {T})")
    return out


# ---- GEMM cases -------------------------------------------------------------------------------------------------------
EPI_NAME = {0: "patch", 1: "qkv", 2: "resid", 3: "gelu"}


def native16(arith, epi):
    return arith in (0, 1) and epi in (R.EPI_QKV, R.EPI_GELU)


def make_gemm(rng, epi, M, N, K, *, M_alloc=None, lda=None, ldo=None, D=None, sec0=0, frames_P=(5, 7), n_prefix=5):
    """Random operands and non-zero side data.  A rows M .. M_alloc are NaN (must change nothing)."""
    M_alloc = M_alloc or M + 37
    lda = lda or K
    ldo = ldo or N
    A = np.full((M_alloc, lda), np.nan, np.float32)
    A[:M, :K] = rng.standard_normal((M, K)).astype(np.float32)
    A[:M, K:] = 7.0                                               # columns past K of a strided A: never read
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    d = dict(A=A, W=W, bias=(0.5 * rng.standard_normal(N)).astype(np.float32), M=M, ldo=ldo)
    if epi == R.EPI_RESID:
        d["lam"] = (rng.standard_normal(N) * 0.3).astype(np.float32)
        d["x0"] = rng.standard_normal((M, N)).astype(np.float32)
    nh, nw = frames_P
    P = nh * nw
    if epi == R.EPI_PATCH:
        assert M % P == 0
        d.update(P=P, T=P + n_prefix, n_prefix=n_prefix, pos=rng.standard_normal((P, N)).astype(np.float32), in_scale=1.0)
    if epi == R.EPI_QKV:
        cos, sin = R.rope_cos_sin(nh, nw, 64, ROPE_THETA)
        d.update(D=D or N // 3, sec0=sec0, T=P + n_prefix, n_prefix=n_prefix, P=P, nh=nh, nw=nw, cos=cos, sin=sin)
    return d


def out_buffer(arith, epi, d):
    M, N, ldo = d["M"], d["W"].shape[0], d["ldo"]
    rows = (M // d["P"]) * d["T"] if epi == R.EPI_PATCH else M
    rows_alloc = rows + 19
    if native16(arith, epi):
        out = np.full((rows_alloc, ldo), CANARY16, np.float16)
    else:
        out = np.full((rows_alloc, ldo), CANARY32, np.float32)
    if epi == R.EPI_RESID:
        out[:M, :N] = d["x0"]
    return out


def decode_out(arith, epi, out, d):
    """Output rows/cols the kernel owns -> float64 [rows][N] (split images decoded)."""
    N = d["W"].shape[0]
    if arith == 4 and epi == R.EPI_QKV:
        D, sec0 = d["D"], d["sec0"]
        scales = [{0: R.ATT_QS, 1: R.ATT_KS, 2: R.ATT_VS}[sec0 + i] for i in range(N // D)]
        return R.decode_head_split(out, N, scales)
    if arith == 4 and epi == R.EPI_GELU:
        return R.decode_split_operand(out, N, d.get("out_scale", 4.0))
    return out[:, :N].astype(np.float64)


def gemm_reference(arith, epi, d, a_scale=1.0, w_scale=1.0):
    M = d["M"]
    A = d["A"][:M, :d["W"].shape[1]]
    acc, E, S = R.gemm_acc(arith, A, d["W"], a_scale, w_scale)
    y, Ey, rowmap = R.gemm_epilogue_ref(epi, acc, E, S, bias=d["bias"], lam=d.get("lam"), x0=d.get("x0"), pos=d.get("pos"),
                                        in_scale=d.get("in_scale", 1.0), frames_P=d.get("P"), T=d.get("T"),
                                        n_prefix=d.get("n_prefix", 0), cos=d.get("cos"), sin=d.get("sin"), D=d.get("D"),
                                        sec0=d.get("sec0", 0))
    if epi == R.EPI_GELU:
        v = acc + d["bias"].astype(np.float64)[None, :]
        Ey = Ey + (2e-7 * np.abs(v) + 8 * R.U32 * (np.abs(v) + np.abs(y)) if arith in (0, 1) else
                   4 * R.U32 * (np.abs(v) + np.abs(y)))
    if native16(arith, epi):
        Ey = Ey + R.out_rounding(y, "f16")
    elif arith == 4 and epi in (R.EPI_QKV, R.EPI_GELU):
        sc = d.get("out_scale", 4.0) if epi == R.EPI_GELU else R.ATT_KS
        Ey = Ey + R.out_rounding(y, "split") + R.F16_SUB / sc
    else:
        Ey = Ey + R.out_rounding(y, "f32")
    return y, Ey, rowmap


def check_gemm(arith, epi, d, label, *, a_scale=1.0, w_scale=1.0, **kw):
    """Run, compare with the bound, check canaries; returns (kernel output [rows][N] float64, raw out)."""
    out0 = out_buffer(arith, epi, d)
    out = gemm_run(arith, epi, d["A"], d["W"], d["bias"], M=d["M"], out=out0.copy(), lam=d.get("lam"), pos=d.get("pos"),
                   cos=d.get("cos"), sin=d.get("sin"), D=d.get("D", 0), sec0=d.get("sec0", 0), T=d.get("T", 0),
                   n_prefix=d.get("n_prefix", 0), P=d.get("P", 0), nh=d.get("nh", 0), nw=d.get("nw", 0),
                   in_scale=d.get("in_scale", 1.0), a_scale=a_scale, w_scale=w_scale, out_scale=d.get("out_scale", 4.0), **kw)
    N = d["W"].shape[0]
    y, Ey, rowmap = gemm_reference(arith, epi, d, a_scale, w_scale)
    rows = rowmap if rowmap is not None else np.arange(d["M"])
    got = decode_out(arith, epi, out[rows], d)
    r = R.ratio(got, y, Ey)
    print(f"  gemm arith {arith} {EPI_NAME[epi]:5s} {label:40s} max err / bound = {r:.3g}")
    assert r <= 1.0, (label, r)
    # canaries: every byte outside the rows and columns the launch owns
    own = np.zeros(out.shape, bool)
    own[rows[:, None], np.arange(N)[None, :]] = True
    assert np.array_equal(out.view(np.uint8).reshape(out.shape[0], -1)[~np.repeat(own, out.itemsize, axis=1)],
                          out0.view(np.uint8).reshape(out.shape[0], -1)[~np.repeat(own, out.itemsize, axis=1)]), label
    return got, out


# fp16 operands: every tile form of launch_gemm (gemm_f16.hip launch_epi, gemm_f16_8ph.hip tiles / planner, skinny)
F16_TILES = [0, 1, 2, 3, 4, 7, 13, 14, 15, 16, 17]


@pytest.mark.parametrize("tile", F16_TILES)
@pytest.mark.parametrize("epi", [R.EPI_QKV, R.EPI_RESID, R.EPI_GELU, R.EPI_PATCH])
def test_fp16_gemm_tile_forms_against_float64(tile, epi):
    rng = np.random.default_rng(100 * tile + epi)
    M = 1015 if epi != R.EPI_PATCH else 29 * 35             # 29 frames of 35 patches: the scatter crosses tile rows
    d = make_gemm(rng, epi, M, 768, 256, ldo=768 + (128 if epi == R.EPI_RESID else 0))
    for rope_lds in ((0, 1) if epi == R.EPI_QKV and tile >= 13 else (0,)):
        check_gemm(0, epi, d, f"tile {tile} M {M} N 768 K 256 lds {rope_lds}", tile=tile, rope_lds=rope_lds)


M_EDGES = [1, 37, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383]


@pytest.mark.parametrize("M", M_EDGES)
def test_fp16_gemm_row_edges(M):
    rng = np.random.default_rng(M)
    for epi in (R.EPI_QKV, R.EPI_RESID, R.EPI_GELU):
        d = make_gemm(rng, epi, M, 768, 768)
        for tile in ([0, 1, 8, 9] if M <= 64 else [0, 1, 13]):
            check_gemm(0, epi, d, f"tile {tile} M {M} N 768 K 768", tile=tile)


@pytest.mark.parametrize("M,N,K,epi,tiles", [
    (300, 256, 4096, R.EPI_RESID, [1, 4, 13, 16]),          # long K
    (300, 128, 64, R.EPI_GELU, [1, 2]),                     # N = 128, K = 64: the 128-wide forms at their minimum
    (1000, 256, 128, R.EPI_RESID, [13, 14, 15, 16, 17]),    # ping-pong at its minimum K
    (700, 512, 256, R.EPI_QKV, [1, 13, 17]),                # sec0 = 1: the k | v-only GEMM (N = 2 D)
])
def test_fp16_gemm_k_n_edges(M, N, K, epi, tiles):
    rng = np.random.default_rng(M + N + K)
    kw = dict(D=N // 2, sec0=1) if epi == R.EPI_QKV else {}
    d = make_gemm(rng, epi, M, N, K, **kw)
    for t in tiles:
        check_gemm(0, epi, d, f"tile {t} M {M} N {N} K {K}" + (" sec0 1" if kw else ""), tile=t)


def test_fp16_gemm_strided_cls_rows():
    """The last layer's CLS-row GEMMs: lda = T D (one row per frame), ldo > N."""
    rng = np.random.default_rng(7)
    for epi in (R.EPI_QKV, R.EPI_RESID, R.EPI_GELU):
        d = make_gemm(rng, epi, 40, 768, 256, lda=256 * 5, ldo=768 + 64)
        for t in (0, 1, 8, 9):
            check_gemm(0, epi, d, f"tile {t} M 40 lda {256 * 5} ldo {768 + 64}", tile=t)


def test_fp16_gemm_tall_planner_persistent_raster():
    """More 256-tiles than CUs with a partial last panel: the planner, persistent workgroups and the grouped raster."""
    rng = np.random.default_rng(12865)
    d = make_gemm(rng, R.EPI_QKV, 12865, 2304, 768, frames_P=(14, 14))
    M = 12865
    for gm in (1, 6, 5):
        check_gemm(0, R.EPI_QKV, d, f"tile 17 M {M} N 2304 K 768 group_m {gm}", tile=17, group_m=gm, rope_lds=1)


@pytest.mark.parametrize("epi", [R.EPI_QKV, R.EPI_RESID, R.EPI_GELU, R.EPI_PATCH])
def test_fp16_hi_lo_weight_gemm(epi):
    rng = np.random.default_rng(30 + epi)
    M = 1015 if epi != R.EPI_PATCH else 29 * 35
    d = make_gemm(rng, epi, M, 768, 256)
    for t in (0, 1, 2):
        check_gemm(1, epi, d, f"W hi+lo tile {t} M {M}", tile=t)


# ---- precision 3: bit for bit ------------------------------------------------------------------------------------------
def f32_epilogue_exact(epi, acc32, d):
    """The fp32 epilogues with vit32_epilogue.h's rounding points (contraction off), in numpy float32."""
    f = np.float32
    b = d["bias"].astype(f)[None, :]
    if epi == R.EPI_RESID:
        return (acc32 + b) * d["lam"].astype(f)[None, :] + d["x0"].astype(f)
    if epi == R.EPI_QKV:
        v = acc32 + b
        y = v.copy()
        M, N = v.shape
        t = np.arange(M) % d["T"]
        rows = np.nonzero(t >= d["n_prefix"])[0]
        c, s = d["cos"][t[rows] - d["n_prefix"]], d["sin"][t[rows] - d["n_prefix"]]
        for h0 in range(0, N, 64):
            if h0 // d["D"] + d["sec0"] < 2:
                vh = v[rows, h0:h0 + 64]
                y[rows, h0:h0 + 64] = vh * c + R._rotate_half(vh) * s
        q = np.array([(c_ // d["D"] + d["sec0"]) == 0 for c_ in range(N)])
        y[:, q] = y[:, q] * f(0.125)
        return y
    raise AssertionError(epi)


@pytest.mark.parametrize("M,N,K", [(1, 256, 64), (65, 256, 768), (257, 256, 256), (130, 768, 128)])
def test_precision3_accumulator_is_the_fmaf_chain_bit_for_bit(M, N, K):
    rng = np.random.default_rng(M * 7 + K)
    d = make_gemm(rng, R.EPI_RESID, M, N, K)
    A = d["A"][:M, :K]
    chain = R.fmaf_chain(A, d["W"], R.f32_mfma_k_order(K))
    # x = 0, lambda = 1, bias = 0: the stored value is the accumulator
    z = dict(d, bias=np.zeros(N, np.float32), lam=np.ones(N, np.float32), x0=np.zeros((M, N), np.float32))
    got, _ = check_gemm(3, R.EPI_RESID, z, f"acc M {M} N {N} K {K}")
    got32 = got.astype(np.float32)
    natural = int((R.fmaf_chain(A, d["W"]) != got32).sum()) if M * N * K <= 2e7 else -1
    print(f"    accumulator: {int((chain != got32).sum())} of {M * N} words differ from the MFMA-order fmaf chain "
          f"({natural} from the natural k order)")
    assert np.array_equal(chain.view(np.uint32), got32.view(np.uint32))
    # the residual epilogue with general x, bias, lambda: exact too
    got, _ = check_gemm(3, R.EPI_RESID, d, f"resid M {M} N {N} K {K}")
    assert np.array_equal(f32_epilogue_exact(R.EPI_RESID, chain, d).view(np.uint32), got.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("M,sec0", [(200, 0), (257, 1)])
def test_precision3_qkv_epilogue_bit_for_bit(M, sec0):
    rng = np.random.default_rng(M + sec0)
    N, K = (768, 128) if sec0 == 0 else (512, 128)
    d = make_gemm(rng, R.EPI_QKV, M, N, K, D=256, sec0=sec0)
    got, _ = check_gemm(3, R.EPI_QKV, d, f"qkv M {M} N {N} K {K} sec0 {sec0}")
    chain = R.fmaf_chain(d["A"][:M, :K], d["W"], R.f32_mfma_k_order(K))
    ref = f32_epilogue_exact(R.EPI_QKV, chain, d)
    print(f"    q|k|v epilogue: {int((ref != got.astype(np.float32)).sum())} words differ from the exact restatement")
    assert np.array_equal(ref.view(np.uint32), got.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("epi", [R.EPI_GELU, R.EPI_PATCH])
@pytest.mark.parametrize("M", [1, 65, 1000])
def test_precision3_gemm_bounds(epi, M):
    rng = np.random.default_rng(M + 10 * epi)
    if epi == R.EPI_PATCH:
        M = max(1, M // 35) * 35
    d = make_gemm(rng, epi, M, 768, 256)
    got, _ = check_gemm(3, epi, d, f"M {M} N 768 K 256")
    if epi == R.EPI_GELU:
        acc = R.fmaf_chain(d["A"][:M, :256], d["W"], R.f32_mfma_k_order(256)) if M * 768 * 256 <= 1e8 else None
        if acc is not None:
            v = (acc + d["bias"][None, :]).astype(np.float64)
            y = 0.5 * v * (1.0 + R._erf64(v / np.sqrt(2.0)))
            # near x << 0 the result cancels to ~0: the error is absolute there, so it is stated in ulps of the
            # argument as well as of the result
            ulp_y = np.spacing(np.maximum(np.abs(y), 2.0 ** -126).astype(np.float32)).astype(np.float64)
            ulp_x = np.spacing(np.maximum(np.abs(v), 2.0 ** -126).astype(np.float32)).astype(np.float64)
            big = np.abs(y) >= 0.25 * np.abs(v)
            print(f"    GELU on the exact accumulator: max {np.max(np.abs(got - y)[big] / ulp_y[big]):.2f} fp32 ulps of the "
                  f"result where |gelu(x)| >= |x| / 4, {np.max(np.abs(got - y) / ulp_x):.2f} ulps of x everywhere")


# ---- precision 4 -----------------------------------------------------------------------------------------------------
SPLIT_TILES = [0, 128, 160, 192, 256, -1]


@pytest.mark.parametrize("tile", SPLIT_TILES)
@pytest.mark.parametrize("epi", [R.EPI_QKV, R.EPI_RESID, R.EPI_GELU, R.EPI_PATCH])
def test_split_gemm_forms_against_float64(tile, epi):
    rng = np.random.default_rng(200 + tile + epi)
    shapes = [(1015, 768, 256), (383, 768, 768)] if epi != R.EPI_PATCH else [(29 * 35, 768, 256)]
    if tile == 0:
        shapes += [(65, 768, 256), (200, 768, 64)] if epi != R.EPI_PATCH else []   # the skinny form (M <= 256)
    for M, N, K in shapes:
        d = make_gemm(rng, epi, M, N, K)
        for rope_lds in ((0, 1) if epi == R.EPI_QKV else (0,)):
            check_gemm(4, epi, d, f"tile {tile} M {M} N {N} K {K} lds {rope_lds}", tile=tile, a_scale=2.0, w_scale=4.0,
                       rope_lds=rope_lds)


def test_split_gemm_down_projection_shape():
    rng = np.random.default_rng(3072)
    d = make_gemm(rng, R.EPI_RESID, 700, 256, 3072)
    for t in (0, -1):
        check_gemm(4, R.EPI_RESID, d, f"tile {t} M 700 N 256 K 3072", tile=t, a_scale=4.0, w_scale=8.0)


# ---- operand edge cases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith,tile", [(0, 1), (0, 13), (0, 9), (3, 0), (4, 0), (4, -1)])
def test_nonfinite_row_of_A_stays_in_its_row(arith, tile):
    rng = np.random.default_rng(arith * 10 + abs(tile))
    M = 40 if tile == 9 else 600
    d = make_gemm(rng, R.EPI_RESID, M, 256, 256)
    clean = check_gemm(arith, R.EPI_RESID, d, f"clean tile {tile} M {M}", tile=tile, a_scale=2.0, w_scale=4.0)[1]
    for bad, val in ((3, np.nan), (M - 1, np.inf), (M // 2, -np.inf)):
        A = d["A"].copy()
        A[bad, 17] = val
        out = gemm_run(arith, R.EPI_RESID, A, d["W"], d["bias"], M=M, out=out_buffer(arith, R.EPI_RESID, d), lam=d["lam"],
                       tile=tile, a_scale=2.0, w_scale=4.0)
        others = np.arange(out.shape[0]) != bad
        assert not np.isfinite(out[bad, :256]).any(), (arith, tile, bad)
        assert np.array_equal(out[others].view(np.uint32), clean[others].view(np.uint32)), (arith, tile, bad)


@pytest.mark.parametrize("tile", [0, -1])
def test_split_operand_range_edges(tile):
    """a_scale = 1: |x| >= 65520 overflows the high half (the CBAS_ERANGE fallback relies on a non-finite row);
    65504 <= |x| < 65520 and tiny values whose low halves are fp16 subnormals must meet the bound."""
    rng = np.random.default_rng(65520 + tile)
    M, N, K = 300, 256, 256
    d = make_gemm(rng, R.EPI_RESID, M, N, K)
    A = d["A"]
    A[5, 3] = 65520.0                                                       # rounds to inf in fp16
    A[6, 9] = -70000.0
    A[7, :8] = np.array([65504.0, 65519.0, -65510.0, 65505.5, 65504.0, -65519.9, 65511.0, 65515.0], np.float32)   # inside
    A[8, :] = (rng.standard_normal(K) * 2.0 ** -16).astype(np.float32)      # low halves ~2^-27: fp16 subnormals
    A[9, :] = (rng.standard_normal(K) * 2.0 ** -22).astype(np.float32)      # hi itself subnormal
    d["W"][:, :8] *= 2.0 ** -12                                             # keep row 7's products at a sane size
    out = gemm_run(4, R.EPI_RESID, A, d["W"], d["bias"], M=M, out=out_buffer(4, R.EPI_RESID, d), lam=d["lam"], tile=tile,
                   a_scale=1.0, w_scale=1.0)
    assert not np.isfinite(out[5, :N]).any() and not np.isfinite(out[6, :N]).any()
    keep = np.ones(M, bool)
    keep[[5, 6]] = False
    sub = dict(d, A=A[:M][keep], M=int(keep.sum()), x0=d["x0"][keep])
    y, Ey, _ = gemm_reference(4, R.EPI_RESID, sub)
    r = R.ratio(out[:M][keep, :N], y, Ey)
    print(f"  split range edges tile {tile}: max err / bound = {r:.3g} (rows 7-9: "
          f"{R.ratio(out[7:10, :N], y[5:8], Ey[5:8]):.3g})")
    assert r <= 1.0


# ---- attention -------------------------------------------------------------------------------------------------------
T_SWEEP = [1, 2, 5, 17, 32, 33, 96, 97, 193, 198, 201, 208, 209, 224, 257, 261, 272, 273, 288, 289, 300, 1029, 1205]


def make_qkv(rng, n, T, D, kind="mixed", pad_rows=48):
    """q|k|v rows [n T + pad][3 D] as the q|k|v GEMM leaves them (q x 1/8).  kind:
      mixed    random rows; frame b's queries lean on a per-frame direction u_b; the next frame's first 8 keys and the
               pad rows past the last frame are 15 u_b (huge logits against frame b only if the mask leaks), key T - 1
               of every frame is 5 u_b (the row's largest logit sits in the last, partial key tile)
      large    logits around +-60
      uniform  all keys of a frame equal"""
    H = D // 64
    rows = n * T + pad_rows
    q = rng.standard_normal((rows, H, 64)) * 0.3
    k = rng.standard_normal((rows, H, 64))
    v = rng.standard_normal((rows, H, 64))
    u = rng.standard_normal((n + 1, H, 64))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    fr = np.minimum(np.arange(rows) // T, n)
    if kind == "mixed":
        q += 2.0 * u[fr]
        for b in range(n):
            k[b * T + T - 1] = 5.0 * u[b] + 0.1 * k[b * T + T - 1]
            nxt = slice((b + 1) * T, min((b + 1) * T + 8, rows))
            k[nxt] = 15.0 * u[b]
        k[n * T:] = 15.0 * u[n - 1]
    elif kind == "large":
        q = u[fr] + 0.05 * q
        k = 60.0 * (rng.choice([-1.0, 1.0], size=(rows, H, 1)) * u[fr] + 0.05 * k)
    elif kind == "uniform":
        for b in range(n):
            k[b * T:(b + 1) * T] = k[b * T]
    qkv = np.concatenate([q.reshape(rows, D), k.reshape(rows, D), v.reshape(rows, D)], axis=1).astype(np.float32)
    return qkv


def check_attention(arith, qkv, n, T, D, label, q_cls=None):
    nq = n if q_cls is not None else n * T
    if arith == 0:
        out0 = np.full((nq + 21, D), CANARY16, np.float16)
    else:
        out0 = np.full((nq + 21, D), CANARY32, np.float32)
    out = attn_run(arith, qkv, n, T, D, out0.copy(), q_cls)
    ref, bound = R.attention_ref(arith, qkv, n, T, D, q_cls)
    got = R.decode_split_operand(out[:nq], D, R.ATT_CTX) if arith == 4 else out[:nq].astype(np.float64)
    r = R.ratio(got, ref, bound)
    print(f"  attention arith {arith} {label:42s} max err / bound = {r:.3g}")
    assert r <= 1.0, (label, r)
    assert np.array_equal(out[nq:].view(np.uint8), out0[nq:].view(np.uint8)), label
    return got


@pytest.mark.parametrize("arith", [0, 3, 4])
@pytest.mark.parametrize("T", T_SWEEP)
def test_attention_buckets_against_float64(arith, T):
    rng = np.random.default_rng(T * 3 + arith)
    n = 3 if T <= 300 else 2
    qkv = make_qkv(rng, n, T, 128)
    check_attention(arith, qkv, n, T, 128, f"T {T} D 128 n {n} mixed")
    q_cls = make_qkv(rng, n, 1, 128, kind="mixed", pad_rows=0)[:n, :128]
    check_attention(arith, qkv, n, T, 128, f"T {T} D 128 n {n} CLS-only", q_cls=q_cls)


@pytest.mark.parametrize("arith", [0, 3, 4])
@pytest.mark.parametrize("T,D,kind", [(201, 768, "mixed"), (261, 768, "mixed"), (1029, 1024, "mixed"),
                                      (97, 128, "large"), (1205, 128, "large"), (209, 128, "uniform"), (300, 128, "uniform")])
def test_attention_model_shapes_and_logit_edges(arith, T, D, kind):
    rng = np.random.default_rng(T + D + arith)
    n = 2
    qkv = make_qkv(rng, n, T, D, kind=kind)
    check_attention(arith, qkv, n, T, D, f"T {T} D {D} n {n} {kind}")


def test_split_attention_persistent_walk():
    """n heads > 2 x CUs: the persistent workgroups of attention_split_kernel walk several (frame, head) items."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    T = 33
    n = (2 * cus) // 2 + 37                    # D = 128: two heads per frame
    rng = np.random.default_rng(cus)
    qkv = make_qkv(rng, n, T, 128)
    check_attention(4, qkv, n, T, 128, f"T {T} D 128 n {n} ({2 * n} items, {cus} CUs)")
