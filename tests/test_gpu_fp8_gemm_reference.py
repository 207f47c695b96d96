"""Single MX-fp8 GEMM launches (gemm_f16_8ph.hip, F8 = true) against the float64 product of exactly the e4m3 bytes and E8M0
scale bytes they were given, element by element (oracle/kernel_ref.py: mx_dequant, gemm_acc_mx, the fp16 form's epilogues).

Every case makes ONE launch through cbas_debug_gemm_f8_run (debug build) in the shapes api_enc.hip's vit_qkv / vit_tail use:
M_pad = M up to 128 with a scale image whose row stride is larger (sc_lda = M_alloc + 128), the W window of the k | v launch
(n0, n_total), ldo > N.  It asserts |kernel - reference| <= bound for every owned element (max err / bound is printed: run with
-s) and that every byte of `out` outside rows < M and columns < N is unchanged.  With quantise = 1 the A rows M .. M_alloc hold
NaN and the scale dwords of rows M_alloc .. sc_lda hold 0xff bytes (the E8M0 NaN): whatever reads them shows.
  a. random operands (rows of different scale, every 7th column x 30, one all-zero row) against the bound: every tile form x
     epilogue, row edges, K / N edges and the k | v window, M_alloc variants, the planner's two plans with the grouped raster;
  b. lossless integer operands: the accumulator and the residual epilogue bit for bit; scale bytes at the ends of E8M0's range;
  c. one hot block: names the row and block any misrouted scale or A piece came from;
  d. e4m3 NaN bytes, E8M0 NaN scales, fp32 NaN / inf through the packer: they stay in their row;
  e. all tile forms and the dispatcher give bit-identical outputs."""
import ctypes as C
import functools
import heapq

import numpy as np
import pytest

from cbas_amd import _lib
from oracle import kernel_ref as R

pytestmark = pytest.mark.gpu

c_int, c_int64, c_void_p = C.c_int, C.c_int64, C.c_void_p


class F8Args(C.Structure):              # include/cbas_mi355x_debug.h cbas_debug_gemm_f8_args
    _fields_ = [("struct_bytes", c_int64)] + [(n, c_int) for n in (
        "epi", "tile", "group_m", "quantise", "M", "M_alloc", "N", "K", "sc_lda", "n_total", "n0", "ldo", "out_rows",
        "D", "sec0", "T", "n_prefix", "P", "rope_nh", "rope_nw", "rope_lds")] + [(n, c_void_p) for n in (
        "A", "W", "A8", "A_sc", "W8", "W_sc", "bias", "lam", "rope_cos", "rope_sin", "out")]


CANARY32 = np.float32(-31337.25)
CANARY16 = np.float16(-1234.0)
ROPE_THETA = 100.0
PP_256, PP_192, PP_160, PP_128, PP_AUTO = 13, 14, 15, 16, 17
TILES = [0, PP_256, PP_192, PP_160, PP_128, PP_AUTO]
EPIS = [R.EPI_QKV, R.EPI_RESID, R.EPI_GELU]
EPI_NAME = {1: "qkv", 2: "resid", 3: "gelu"}
SC_FILL = 0xFFFFFFFF                    # scale dwords nobody may use: four E8M0 NaNs


def round_up(n, m):
    return (n + m - 1) // m * m


def f8_run(d, out, *, tile=0, group_m=0, rope_lds=0, quantise=1, epi=None):
    """One launch on case `d`; `out` is updated in place.  quantise = 1 fills d's A8 / A_sc / W8 / W_sc copies and returns them."""
    lib = _lib.load()
    epi = d["epi"] if epi is None else epi
    K = d["K"]
    a = F8Args()
    a.struct_bytes = C.sizeof(F8Args)
    a.epi, a.tile, a.group_m, a.quantise = epi, tile, group_m, quantise
    a.M, a.M_alloc, a.N, a.K, a.sc_lda, a.n_total, a.n0 = d["M"], d["M_alloc"], d["N"], K, d["sc_lda"], d["n_total"], d["n0"]
    a.ldo, a.out_rows = out.shape[1], out.shape[0]
    a.D, a.sec0, a.T, a.n_prefix, a.P = d.get("D", 0), d.get("sec0", 0), d.get("T", 0), d.get("n_prefix", 0), d.get("P", 0)
    a.rope_nh, a.rope_nw, a.rope_lds = d.get("nh", 0), d.get("nw", 0), rope_lds
    if quantise:
        A8 = np.full((d["M_alloc"], K), 0x7F, np.uint8)
        W8 = np.full((d["n_total"], K), 0x7F, np.uint8)
        Asc = np.full((K // 128, d["sc_lda"]), SC_FILL, np.uint32)
        Wsc = np.full((K // 128, d["n_total"]), SC_FILL, np.uint32)
        assert d["A"].shape == A8.shape and d["W"].shape == W8.shape and d["A"].dtype == np.float32 and d["W"].dtype == np.float32
        assert d["A"].flags.c_contiguous and d["W"].flags.c_contiguous
        a.A, a.W = d["A"].ctypes.data, d["W"].ctypes.data
    else:
        A8, W8, Asc, Wsc = (np.ascontiguousarray(d[k]) for k in ("A8", "W8", "A_sc", "W_sc"))
        assert A8.shape == (d["M_alloc"], K) and W8.shape == (d["n_total"], K) and A8.dtype == np.uint8 and W8.dtype == np.uint8
        assert Asc.shape == (K // 128, d["sc_lda"]) and Wsc.shape == (K // 128, d["n_total"]) and Asc.dtype == np.uint32 and Wsc.dtype == np.uint32
    a.A8, a.A_sc, a.W8, a.W_sc = A8.ctypes.data, Asc.ctypes.data, W8.ctypes.data, Wsc.ctypes.data
    keep = [np.ascontiguousarray(d[k], np.float32) if d.get(k) is not None else None for k in ("bias", "lam", "cos", "sin")]
    a.bias, a.lam, a.rope_cos, a.rope_sin = (None if x is None else x.ctypes.data for x in keep)
    assert out.flags.c_contiguous
    a.out = out.ctypes.data
    _lib.check(lib.cbas_debug_gemm_f8_run(C.byref(a)), f"cbas_debug_gemm_f8_run(epi {epi}, tile {tile})")
    return A8, Asc, W8, Wsc


# ---- a. random operands --------------------------------------------------------------------------------------------------
def make_case(epi, M, N, K, seed, *, M_alloc=None, sc_lda=None, n_total=None, n0=0, D=None, sec0=0, ldo=None, frames_P=(5, 7),
              n_prefix=5, acc_only=False):
    """Random operands: rows of very different scale, every 7th column x 30, one all-zero row (scale byte 0); A rows
    M .. M_alloc NaN.  W has n_total rows of which the launch uses n0 .. n0 + N.  acc_only: x = 0, bias 0, lambda 1."""
    rng = np.random.default_rng(seed)
    M_alloc = M_alloc or round_up(M, 128)
    sc_lda = sc_lda or M_alloc + 128
    n_total = n_total or N
    A = np.full((M_alloc, K), np.nan, np.float32)
    A[:M] = (rng.standard_normal((M, K)) * np.exp(rng.standard_normal((M, 1)))).astype(np.float32)
    A[:M, ::7] *= 30.0
    zrow = min(3, M - 1)
    A[zrow] = 0.0
    W = (rng.standard_normal((n_total, K)) * 0.05).astype(np.float32)
    d = dict(epi=epi, M=M, N=N, K=K, M_alloc=M_alloc, sc_lda=sc_lda, n_total=n_total, n0=n0, ldo=ldo or N, A=A, W=W, zrow=zrow,
             bias=(0.5 * rng.standard_normal(N)).astype(np.float32))
    if epi == R.EPI_RESID:
        d["lam"] = (rng.standard_normal(N) * 0.3).astype(np.float32)
        d["x0"] = rng.standard_normal((M, N)).astype(np.float32)
        if acc_only:
            d.update(bias=np.zeros(N, np.float32), lam=np.ones(N, np.float32), x0=np.zeros((M, N), np.float32))
    if epi == R.EPI_QKV:
        nh, nw = frames_P
        cos, sin = R.rope_cos_sin(nh, nw, 64, ROPE_THETA)
        d.update(D=D or N // 3, sec0=sec0, T=nh * nw + n_prefix, n_prefix=n_prefix, P=nh * nw, nh=nh, nw=nw, cos=cos, sin=sin)
    return d


@functools.lru_cache(maxsize=None)
def shared_case(epi, M, N, K, seed, **kw):
    """A case whose reference is computed once (at its first launch) and shared by every test that runs it."""
    return make_case(epi, M, N, K, seed, **dict(kw))


def out_buffer(d):
    M, N = d["M"], d["N"]
    if d["epi"] == R.EPI_RESID:
        out = np.full((M + 19, d["ldo"]), CANARY32, np.float32)
        out[:M, :N] = d["x0"]
    else:
        out = np.full((M + 19, d["ldo"]), CANARY16, np.float16)
    return out


def reference(d, a, w):
    """(y, bound) of case d on the dequantised operands a [M][K], w [N][K]."""
    epi = d["epi"]
    acc, E, S = R.gemm_acc_mx(a, w)
    y, Ey, _ = R.gemm_epilogue_ref(epi, acc, E, S, bias=d["bias"], lam=d.get("lam"), x0=d.get("x0"), T=d.get("T"),
                                   n_prefix=d.get("n_prefix", 0), cos=d.get("cos"), sin=d.get("sin"), D=d.get("D"), sec0=d.get("sec0", 0))
    if epi == R.EPI_GELU:                   # the implementation term gemm_reference adds for arith 0 (gelu_fast4)
        v = acc + d["bias"].astype(np.float64)[None, :]
        Ey = Ey + 2e-7 * np.abs(v) + 8 * R.U32 * (np.abs(v) + np.abs(y))
    Ey = Ey + R.out_rounding(y, "f32" if epi == R.EPI_RESID else "f16")
    return y, Ey, acc, S


def dequant(d, q):
    A8, Asc, W8, Wsc = q
    M, N, n0 = d["M"], d["N"], d["n0"]
    return R.mx_dequant(A8[:M], Asc, M, d["sc_lda"]), R.mx_dequant(W8[n0:n0 + N], Wsc[:, n0:n0 + N], N, N)


def assert_canaries(out, out0, M, N, label):
    own = np.zeros(out.shape, bool)
    own[:M, :N] = True
    mask = ~np.repeat(own, out.itemsize, axis=1)
    assert np.array_equal(out.view(np.uint8).reshape(out.shape[0], -1)[mask], out0.view(np.uint8).reshape(out.shape[0], -1)[mask]), label


def check(d, label, **kw):
    """One quantise = 1 launch of case d against the bound; returns the raw output."""
    out0 = out_buffer(d)
    out = out0.copy()
    q = f8_run(d, out, **kw)
    M, N = d["M"], d["N"]
    if "ref" not in d:
        # the packer's part of the contract this file leans on: NaN rows past M get scale byte 0, the dwords past M_alloc keep their fill
        assert np.all(q[1][:, d["M_alloc"]:] == SC_FILL), label
        d["q"] = q
        d["ref"] = reference(d, *dequant(d, q))
    else:
        assert all(np.array_equal(x, y) for x, y in zip(q, d["q"])), label       # same operands every time
    y, Ey, _, S = d["ref"]
    r = R.ratio(out[:M, :N], y, Ey)
    print(f"  mx-fp8 {EPI_NAME[d['epi']]:5s} {label:58s} max err / bound = {r:.3g}")
    assert r <= 1.0, (label, r)
    assert_canaries(out, out0, M, N, label)
    return out


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("epi", EPIS)
def test_mx_gemm_tile_forms_against_float64(tile, epi):
    d = shared_case(epi, 1015, 768, 256, 100 + epi, ldo=768 + (128 if epi == R.EPI_RESID else 0))
    for rope_lds in ((0, 1) if epi == R.EPI_QKV else (0,)):
        check(d, f"tile {tile} M 1015 N 768 K 256 lds {rope_lds}", tile=tile, rope_lds=rope_lds)


M_EDGES = [1, 37, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383]
EDGE_TILES = [0, PP_128, PP_256]


@pytest.mark.parametrize("M", M_EDGES)
def test_mx_gemm_row_edges(M):
    for epi in EPIS:
        d = shared_case(epi, M, 768, 768, 1000 * epi + M)
        for tile in EDGE_TILES:
            check(d, f"tile {tile} M {M} N 768 K 768", tile=tile)


# (M, N, K, epi, extra): the minimum; the down projection; the k | v launch of the pruned last layer (W_sc points at column D of a
# 3 D-wide scale image) and the same shape with a scale image of its own
KN_EDGES = [
    (300, 256, 256, R.EPI_RESID, ()),
    (300, 256, 3072, R.EPI_RESID, ()),
    (700, 512, 256, R.EPI_QKV, (("D", 256), ("n0", 256), ("n_total", 768), ("sec0", 1))),
    (700, 512, 256, R.EPI_QKV, (("D", 256), ("sec0", 1))),
]
KN_TILES = [0, PP_256, PP_160, PP_128]


@pytest.mark.parametrize("M,N,K,epi,extra", KN_EDGES)
def test_mx_gemm_k_n_edges_and_the_kv_window(M, N, K, epi, extra):
    d = shared_case(epi, M, N, K, M + N + K + len(extra), **dict(extra))
    for tile in KN_TILES:
        check(d, f"tile {tile} M {M} N {N} K {K} " + " ".join(f"{k} {v}" for k, v in extra), tile=tile, rope_lds=1 if epi == R.EPI_QKV else 0)


# M_alloc = M: a 256-row tile clamps rows 300 .. 511 (A rows and scale dwords) at row 299; 384 = M up to 128 (the product's M_pad);
# 512 = M up to 256.  (M_alloc, sc_lda): the stride of the scale image larger than M_alloc, and equal to it
M_ALLOCS = [(300, 428), (384, 512), (512, 640), (300, 300), (384, 384), (512, 512)]


@pytest.mark.parametrize("M_alloc,sc_lda", M_ALLOCS)
def test_mx_gemm_m_alloc_and_scale_stride(M_alloc, sc_lda):
    for epi in EPIS:
        d = shared_case(epi, 300, 768, 512, 7 * M_alloc + sc_lda + epi, M_alloc=M_alloc, sc_lda=sc_lda)
        check(d, f"tile {PP_256} M 300 M_alloc {M_alloc} sc_lda {sc_lda}", tile=PP_256)


# ---- planner and raster: a port of pp_plan (gemm_f16_8ph.hip) picks the M ------------------------------------------------------
PP_COST = {256: 1.0, 192: 0.86, 160: 0.79, 128: 0.63}


def _makespan(n_main, c_main, n_tail, c_tail, slots):
    free, end = [0.0] * slots, 0.0
    for n, c in ((n_main, c_main), (n_tail, c_tail)):
        for _ in range(n):
            t = heapq.heappop(free) + c
            heapq.heappush(free, t)
            end = max(end, t)
    return end


def pp_plan(M, N, cus):
    """(tile rows, main panels) as pp_plan returns them."""
    tn, best, bt = N // 256, (256, 0), 1e30
    for bm in (256, 192, 160):
        t = _makespan(-(-M // bm) * tn, PP_COST[bm], 0, 0.0, cus)
        if t < bt - 1e-9:
            best, bt = (bm, 0), t
    for mp in range(1, -(-M // 256)):
        t = _makespan(mp * tn, 1.0, -(-(M - mp * 256) // 128) * tn, PP_COST[128], cus)
        if t < bt - 0.02:
            best, bt = (256, mp), t
    return best


@functools.lru_cache(maxsize=None)
def planner_Ms(N=2304):
    """The smallest M (N = 2304: nine column tiles) at which launch_gemm hands an MX-fp8 problem to the planner - 120 tiles of 256
    rows: M = 3329 - and the planner takes a uniform 160- or 192-row plan, and the smallest at which it takes main panels with a
    128-row tail.  On 256 CUs: M = 3329 is 21 x 9 = 189 tiles of 160 rows, ONE round at 0.79 of a 256-row tile's time, where 14 x 9
    = 126 tiles of 256 rows cost 1.0; every M up to 8960 fits a uniform plan at least as well as a tail (one or two full rounds);
    M = 8961 is 36 panels = 324 tiles of 256 rows (two rounds, 2.0) or 57 x 9 = 513 of 160 (three rounds, 2.37), but 15 main panels
    (135 tiles) + 41 x 9 = 369 tail tiles of 128 rows at 0.63 finish at 1.63: main panels with a tail.  Other CU counts move the two
    values; they are searched, not assumed."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    uniform = tail = None
    for M in range(1, 20000, 32):           # every tile height is a multiple of 32: the tile counts change at 32 k + 1 only
        if -(-M // 256) * (N // 256) < 120:
            continue
        bm, mp = pp_plan(M, N, cus)
        if uniform is None and mp == 0 and bm in (160, 192):
            uniform = M
        if tail is None and mp > 0:
            tail = M
        if uniform and tail:
            return cus, uniform, tail
    raise AssertionError(f"no M below 20000 reaches both plans on {cus} CUs")


@pytest.mark.parametrize("which", ["uniform", "tail"])
def test_mx_gemm_planner_plans_and_grouped_raster(which):
    cus, m_uniform, m_tail = planner_Ms()
    M = m_uniform if which == "uniform" else m_tail
    bm, mp = pp_plan(M, 2304, cus)
    print(f"  {cus} CUs: M {M} -> {bm}-row tiles, {mp} main panels" + (" + 128-row tail" if mp else ""))
    d = make_case(R.EPI_QKV, M, 2304, 768, M, frames_P=(14, 14))
    for gm in (1, 5, 6):
        check(d, f"planner M {M} N 2304 K 768 group_m {gm}", tile=0, group_m=gm, rope_lds=1)


def test_mx_gemm_all_zero_row_is_the_epilogue_of_a_zero_accumulator():
    """S = 0 on the all-zero row (scale byte 0, bytes 0), so its bound is the epilogue's own: bias (+ RoPE, x 1/8) / x + b lambda /
    gelu(b), and their output rounding."""
    for epi in EPIS:
        d = shared_case(epi, 1015, 768, 256, 100 + epi, ldo=768 + (128 if epi == R.EPI_RESID else 0))
        out = check(d, "all-zero row, tile 0", tile=0)
        y, Ey, acc, S = d["ref"]
        z = d["zrow"]
        assert np.all(S[z] == 0.0) and np.all(acc[z] == 0.0)
        zero = dict(d, M=1)
        yz, Ez, _, _ = reference(dict(zero, x0=d["x0"][z:z + 1]) if epi == R.EPI_RESID else dict(zero, T=10 ** 9, n_prefix=0, cos=None),
                                 np.zeros((1, d["K"])), np.zeros((d["N"], d["K"])))
        if epi != R.EPI_QKV:                # (q|k|v: row z = 3 is a prefix row: no RoPE, as with cos = None)
            assert np.array_equal(yz[0], y[z])
        r = R.ratio(out[z:z + 1, :d["N"]], yz, Ez)
        print(f"    zero row {z}: max err / the epilogue's own bound = {r:.3g}")
        assert r <= 1.0


def mx_random_cases():
    """The operands of every random-operand case of this file (A and W are drawn first from a case's seed, whatever its epilogue)
    as (label, make_case kwargs, tiles): what MX_ACC_U was measured over (kernel_ref.py), through measure_acc."""
    out = [(f"tile forms {EPI_NAME[e]}", dict(M=1015, N=768, K=256, seed=100 + e), TILES) for e in EPIS]
    out += [(f"row edge M {M} {EPI_NAME[e]}", dict(M=M, N=768, K=768, seed=1000 * e + M), EDGE_TILES) for M in M_EDGES for e in EPIS]
    out += [(f"k/n edge {M}x{N}x{K} {dict(extra)}", dict(M=M, N=N, K=K, seed=M + N + K + len(extra),
                                                         **{k: v for k, v in extra if k in ("n0", "n_total")}), KN_TILES)
            for M, N, K, _, extra in KN_EDGES]
    out += [(f"M_alloc {ma} sc_lda {ld} {EPI_NAME[e]}", dict(M=300, N=768, K=512, seed=7 * ma + ld + e, M_alloc=ma, sc_lda=ld), [PP_256])
            for ma, ld in M_ALLOCS for e in EPIS]
    out += [(f"tile forms agree {EPI_NAME[e]}", dict(M=1000, N=768, K=768, seed=5 + e), TILES) for e in EPIS]
    out += [("fp32 non-finite, clean launch", dict(M=300, N=512, K=256, seed=11), [PP_256])]
    _, m_uniform, m_tail = planner_Ms()
    out += [(f"planner M {M}", dict(M=M, N=2304, K=768, seed=M), [0]) for M in (m_uniform, m_tail)]
    return out


def measure_acc(d, tile, group_m=0):
    """The accumulator-only launch of case d (RESID, x = 0, bias 0, lambda 1): (max |kernel - acc| / S, its position)."""
    out = out_buffer(d)
    q = f8_run(d, out, tile=tile, group_m=group_m)
    if "ref" not in d:
        a, w = dequant(d, q)
        d["ref"] = R.gemm_acc_mx(a, w)
    acc, _, S = d["ref"]
    got = out[:d["M"], :d["N"]].astype(np.float64)
    assert np.all(got[S == 0.0] == 0.0)
    rel = np.abs(got - acc) / np.where(S > 0.0, S, 1.0)
    i = np.unravel_index(np.argmax(rel), rel.shape)
    return float(rel[i]), i


# ---- b. lossless integer operands ------------------------------------------------------------------------------------------
def lossless_case(K, seed, *, M=300, N=512, n_total=768, n0=256, **kw):
    M_alloc = round_up(M, 128)
    sc_lda = M_alloc + 128
    L = R.mx_lossless_case(M_alloc, n_total, K, seed, sc_lda, **kw)
    d = dict(epi=R.EPI_RESID, M=M, N=N, K=K, M_alloc=M_alloc, sc_lda=sc_lda, n_total=n_total, n0=n0, ldo=N + 64, **L)
    d.update(bias=np.zeros(N, np.float32), lam=np.ones(N, np.float32), x0=np.zeros((M, N), np.float32))
    a = R.mx_lossless_values(L["ai"][:M], L["sa"][:M])
    w = R.mx_lossless_values(L["wi"][n0:n0 + N], L["sw"][n0:n0 + N])
    d["acc"] = a @ w.T                      # integers x a power of two, far below 2^53: exact in float64 in any order
    d["S"] = np.abs(a) @ np.abs(w).T
    return d


def same_bits(got32, ref64):
    """Words of got (fp32) that differ from the exact float64 value (a zero's sign aside)."""
    ref32 = ref64.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref64)                   # the reference itself is an fp32 number
    return int(((got32 + np.float32(0.0)).view(np.uint32) != (ref32 + np.float32(0.0)).view(np.uint32)).sum())


def run_lossless(d, tile, label):
    out0 = out_buffer(d)
    out = out0.copy()
    f8_run(d, out, tile=tile, quantise=0)
    assert_canaries(out, out0, d["M"], d["N"], label)
    return out[:d["M"], :d["N"]]


@pytest.mark.parametrize("K", [256, 768])
def test_mx_gemm_lossless_operands_bit_for_bit(K):
    d = lossless_case(K, 40 + K)
    rng = np.random.default_rng(K)
    # residual epilogue with every step exact: integer bias and residual, lambda a power of two
    e = dict(d, bias=rng.integers(-8, 9, d["N"]).astype(np.float32), lam=rng.choice([-2.0, -0.5, 0.5, 1.0, 2.0], d["N"]).astype(np.float32),
             x0=rng.integers(-64, 65, (d["M"], d["N"])).astype(np.float32))
    y = e["x0"].astype(np.float64) + (d["acc"] + e["bias"][None, :]) * e["lam"][None, :]
    for tile in TILES:
        n_acc = same_bits(run_lossless(d, tile, f"lossless acc tile {tile}"), d["acc"])
        n_res = same_bits(run_lossless(e, tile, f"lossless resid tile {tile}"), y)
        print(f"  lossless K {K} tile {tile}: {n_acc} accumulator words and {n_res} residual-epilogue words of {d['M'] * d['N']} differ")
        assert n_acc == 0 and n_res == 0, (tile, n_acc, n_res)


@pytest.mark.parametrize("sb_a,sb_w", [(254, 1), (1, 254)])
def test_mx_gemm_scale_bytes_at_the_ends_of_e8m0(sb_a, sb_w):
    """2^127 x 2^-126: the product scale is 2^1; the exponents must add without an intermediate overflow or flush."""
    d = lossless_case(256, sb_a, sb_lo=sb_a, sb_hi=sb_a)
    w = R.mx_lossless_case(d["M_alloc"], d["n_total"], 256, sb_a, d["sc_lda"], sb_lo=sb_w, sb_hi=sb_w)
    d.update(W_sc=w["W_sc"], sw=w["sw"], wi=w["wi"], W8=w["W8"])
    acc = 2.0 * (d["ai"][:d["M"]].astype(np.float64) @ d["wi"][d["n0"]:d["n0"] + d["N"]].astype(np.float64).T)
    assert np.array_equal(acc, R.mx_dequant(d["A8"][:d["M"]], d["A_sc"], d["M"], d["sc_lda"]) @
                          R.mx_dequant(d["W8"][d["n0"]:d["n0"] + d["N"]], d["W_sc"][:, d["n0"]:d["n0"] + d["N"]], d["N"], d["N"]).T)
    for tile in (PP_256, PP_128):
        n = same_bits(run_lossless(d, tile, f"scales {sb_a} x {sb_w} tile {tile}"), acc)
        print(f"  A scale byte {sb_a} x W scale byte {sb_w}, tile {tile}: {n} words differ")
        assert n == 0, (tile, n)


# ---- c. one hot block --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [PP_160, PP_256])
def test_mx_gemm_one_hot_block_names_its_row_and_block(tile):
    """All of A is zero but block b of row r: ones with scale byte 127 + b.  Row r of the output is 2^b x the sum of W's block b,
    every other row 0, exactly; a wrong row or a wrong power of two names where a misrouted A piece or scale byte came from."""
    M, N, K = 261, 256, 768
    d = lossless_case(K, 77, M=M, N=N, n_total=N, n0=0)
    w = R.mx_lossless_values(d["wi"], d["sw"])                              # [N][K]
    wsum = w.reshape(N, K // 32, 32).sum(-1)                                 # [N][block]
    for r in (0, 63, 64, 159, 160, 255, M - 1):
        for b in range(K // 32):
            ai = np.zeros((d["M_alloc"], K), np.int64)
            ai[r, 32 * b:32 * b + 32] = 1
            sa = np.full((d["M_alloc"], K // 32), 127, np.uint8)
            sa[r, b] = 127 + b
            h = dict(d, A8=R.mx_int_bytes(ai), A_sc=R.mx_scale_image(sa, d["sc_lda"]))
            got = run_lossless(h, tile, f"one hot row {r} block {b} tile {tile}").astype(np.float64)
            want = np.zeros((M, N))
            want[r] = 2.0 ** b * wsum[:, b]
            if not np.array_equal(got, want):
                rows = np.nonzero(np.any(got != 0.0, axis=1))[0]
                fits = [(int(rr), int(bb), int(ee)) for rr in rows for bb in range(K // 32) for ee in range(-2, 26)
                        if np.any(wsum[:, bb] != 0) and np.array_equal(got[rr], 2.0 ** ee * wsum[:, bb])]
                raise AssertionError(f"tile {tile}: hot (row {r}, block {b}, 2^{b}) gave non-zero rows {rows.tolist()}; "
                                     f"(row, W block, power of two) that explain a row exactly: {fits}")


# ---- d. non-finite operands ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [PP_128, PP_256])
def test_mx_gemm_nonfinite_bytes_and_scales_stay_in_their_row(tile):
    M, N = 300, 512
    d = lossless_case(256, 9, M=M, N=N)
    A8, A_sc = d["A8"].copy(), d["A_sc"].copy()
    A8[M:] = 0x7F                                                            # rows M .. M_alloc: e4m3 NaN bytes, E8M0 NaN scales
    A_sc[:, M:] = SC_FILL
    rng = np.random.default_rng(tile)
    e = dict(d, A8=A8, A_sc=A_sc, bias=rng.integers(-8, 9, N).astype(np.float32), lam=np.ones(N, np.float32),
             x0=rng.integers(-64, 65, (M, N)).astype(np.float32))
    clean = run_lossless(e, tile, f"clean tile {tile}")
    assert np.isfinite(clean).all()
    for bad in (3, M // 2, M - 1):
        nan_byte = A8.copy()
        nan_byte[bad, 17] = 0x7F
        nan_scale = A_sc.copy()
        nan_scale.view(np.uint8).reshape(A_sc.shape[0], A_sc.shape[1], 4)[1, bad, 2] = 0xFF      # block 6 of the row
        for what, h in (("e4m3 NaN byte", dict(e, A8=nan_byte)), ("E8M0 NaN scale", dict(e, A_sc=nan_scale))):
            out = run_lossless(h, tile, f"{what} row {bad} tile {tile}")
            others = np.arange(M) != bad
            n_fin = int(np.isfinite(out[bad]).sum())
            print(f"  {what} in row {bad}, tile {tile}: {n_fin} of {N} outputs of the row finite")
            assert np.array_equal(out[others].view(np.uint32), clean[others].view(np.uint32)), (what, tile, bad)
            assert n_fin == 0, (what, tile, bad, n_fin)


def test_mx_gemm_nonfinite_fp32_through_the_packer_stays_in_its_row():
    """quantise = 1: what the block quantiser makes of a NaN / inf is the row kernels' business (printed); the other rows are not."""
    M, N, K = 300, 512, 256
    d = make_case(R.EPI_RESID, M, N, K, 11)
    out0 = out_buffer(d)
    clean = out0.copy()
    f8_run(d, clean, tile=PP_256)
    for bad, vals in ((3, (np.nan, np.inf)), (M // 2, (np.nan, -np.inf)), (M - 1, (np.inf, np.nan))):
        A = d["A"].copy()
        A[bad, 17], A[bad, 200] = vals
        out = out0.copy()
        A8, Asc, _, _ = f8_run(dict(d, A=A), out, tile=PP_256)
        sb = Asc.view(np.uint8).reshape(K // 128, -1, 4)[:, bad].reshape(-1)
        print(f"  fp32 {vals} in row {bad}: bytes at the two places {A8[bad, 17]:#04x} {A8[bad, 200]:#04x}, scale bytes {sb.tolist()}, "
              f"{int(np.isfinite(out[bad, :N]).sum())} of {N} outputs of the row finite")
        others = np.arange(out.shape[0]) != bad
        assert np.array_equal(out[others].view(np.uint32), clean[others].view(np.uint32)), bad


# ---- e. tile forms agree -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", EPIS)
def test_mx_gemm_tile_forms_and_the_dispatcher_agree_bit_for_bit(epi):
    """launch_gemm promises that a row does not depend on how many rows shared its batch: small batches take the 128-row tile,
    large ones the planner's, so every tile form must give the same bits (test_gpu_gemm_variants.py asserts it for fp16)."""
    d = shared_case(epi, 1000, 768, 768, 5 + epi)
    outs = {tile: check(d, f"agree tile {tile} M 1000 N 768 K 768", tile=tile, rope_lds=1 if epi == R.EPI_QKV else 0) for tile in TILES}
    for tile in TILES[1:]:
        n = int((outs[tile].view(np.uint8) != outs[0].view(np.uint8)).any(axis=1).sum())
        print(f"    tile {tile} vs the dispatcher: {n} rows differ")
        assert n == 0, (tile, n)
