"""Single launches of the row-wise encoder kernels against float64 references (oracle/kernel_ref.py), element by element.

Each harness call (cbas_debug_rows_run, debug build) feeds host operands to ONE launcher: the ViT LayerNorms (fp16, fp32,
split, MX-fp8 output, the CLS-row final norm) and the ConvNeXt producers (stem gather, in-place LayerNorm, 2 x 2 window
LayerNorm, depthwise 7 x 7 + LayerNorm, pool + LayerNorm).  For every output element |kernel - reference| <= the bound
derived from where the kernel rounds (validated on the CPU by tests/test_kernel_reference_bounds.py); the largest
max |error| / bound of a test is printed (run with -s).  Besides the bound:
  - everything outside the rows and columns a launch owns is unchanged byte for byte (canary rows past M, columns C .. ld of
    the in-place stream, canary dwords of the scale image);
  - the split image decodes to exactly split_value(plain fp32 output), cls_f16 is the RNE rounding of cls_f32, the stem
    gather is exact;
  - depthwise frames equal the same frame run alone bit for bit, with neighbours of magnitude 1e6; the unread last row /
    column of an odd downsample grid holds NaN;
  - the MX scale bytes sit at out_sc[(col / 128) * sc_ld + row], byte (col % 128) / 32, and equal mx_scale_exp of the
    reference block maximum (either neighbour where that maximum is within the bound of a scale boundary: <= 1 % of blocks);
  - the non-finite counters count exactly the frames with a NaN / inf / variance-overflowing value, other frames' rows
    are bit-identical to the clean run, and a NULL counter changes nothing;
  - the harness refuses, by return code and without launching, every shape a launcher would mis-handle.
Every shape is a handful of rows (1023 at most): widths cover NV = ceil(D / 256) = 1 .. 6 and partial last vectors."""
import ctypes as C

import numpy as np
import pytest

from cbas_amd import _lib
from oracle import kernel_ref as R

pytestmark = pytest.mark.gpu

c_int, c_int64, c_float, c_void_p = C.c_int, C.c_int64, C.c_float, C.c_void_p
(LN_F16, LN_F32, LN_SPLIT, LN_F8, FINAL_CLS, CNX_STEM_U8, CNX_STEM_F32, CNX_LN_ROWS, CNX_DOWNSAMPLE, CNX_DWCONV_LN,
 CNX_POOL_LN) = range(11)
EINVAL = -1


class RowsArgs(C.Structure):            # include/cbas_mi355x_debug.h cbas_debug_rows_args
    _fields_ = ([("struct_bytes", c_int64)] + [(n, c_int) for n in ("op", "split", "M", "n", "D", "T", "h", "w", "sc_ld")] +
                [("eps", c_float), ("ld", c_int64), ("frame_stride", c_int64), ("row_stride", c_int64), ("pixel_stride", c_int64),
                 ("x", c_void_p), ("x_bytes", c_int64), ("gamma", c_void_p), ("beta", c_void_p), ("wt", c_void_p), ("bias", c_void_p),
                 ("out", c_void_p), ("out_bytes", c_int64), ("out2", c_void_p), ("out2_bytes", c_int64), ("counter", c_void_p)])


CANARY32 = np.float32(-31337.25)
CANARY16 = np.float16(-1234.0)
VIT_D = [128, 256, 384, 768, 1024, 1280]
VIT_M = [1, 3, 4, 5, 1023]
CNX_C = [32, 96, 192, 384, 768, 800, 1536]


def rows_call(op, *, x=None, x_addr=None, x_bytes=None, out=None, out2=None, counter=None, gamma=None, beta=None, wt=None, bias=None,
              **kw):
    """One harness call; returns its code.  out / out2 / counter are updated in place."""
    lib = _lib.load()
    a = RowsArgs()
    a.struct_bytes = C.sizeof(RowsArgs)
    a.op = op
    for k, v in kw.items():
        setattr(a, k, v)
    keep = [np.ascontiguousarray(t, np.float32) if t is not None else None for t in (gamma, beta, wt, bias)]
    a.gamma, a.beta, a.wt, a.bias = [None if t is None else t.ctypes.data for t in keep]
    if x is not None:
        assert x.flags.c_contiguous
        a.x, a.x_bytes = x.ctypes.data, x.nbytes
    if x_addr is not None:
        a.x, a.x_bytes = x_addr, x_bytes
    for name, buf in (("out", out), ("out2", out2)):
        if buf is not None:
            assert buf.flags.c_contiguous
            setattr(a, name, buf.ctypes.data)
            setattr(a, name + "_bytes", buf.nbytes)
    if counter is not None:
        a.counter = counter.ctypes.data
    return lib.cbas_debug_rows_run(C.byref(a))


def run(op, **kw):
    _lib.check(rows_call(op, **kw), f"cbas_debug_rows_run(op {op})")


def eps_of(i):
    return 1e-5 if i % 2 else 1e-6


def f16_rne(x32):
    return np.asarray(x32, np.float32).astype(np.float16)


# ---- ViT LayerNorms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", VIT_D)
@pytest.mark.parametrize("op", [LN_F16, LN_F32, LN_SPLIT], ids=["f16", "f32", "split"])
def test_vit_layernorm(op, D):
    worst = 0.0
    for M in VIT_M:
        for ld in (D, 5 * D):
            eps = eps_of(M + ld // D)
            x, gamma, beta = R.rows_case(M, D, 100 + D + M, ld=ld)
            ref, E = R.ln_ref(x[:, :D], gamma, beta, eps)
            if op == LN_F16:
                out = np.full((M + 3, D), CANARY16, np.float16)
            else:
                out = np.full((M + 3, D), CANARY32, np.float32)
            run(op, x=x, out=out, gamma=gamma, beta=beta, M=M, D=D, ld=ld, eps=eps)
            assert (out[M:] == out.dtype.type(CANARY16 if op == LN_F16 else CANARY32)).all(), "canary rows past M changed"
            if op == LN_SPLIT:
                plain = np.full((M, D), CANARY32, np.float32)
                run(LN_F32, x=x, out=plain, gamma=gamma, beta=beta, M=M, D=D, ld=ld, eps=eps)
                y = R.decode_split_operand(out[:M], D, 1.0)
                assert np.array_equal(y, R.split_value(plain, 1.0)), "split image != split_value(plain fp32 output)"
                bound = R.stored_bound(ref, E, "split")
            else:
                y = out[:M].astype(np.float64)
                bound = R.stored_bound(ref, E, "f16" if op == LN_F16 else "f32")
            r = R.ratio(y, ref, bound)
            worst = max(worst, r)
            assert r <= 1.0, (M, ld, eps, r)
    print(f"[rows ln op {op} D {D}] max err / bound {worst:.3f}")


@pytest.mark.parametrize("D", [256, 384, 768, 1024])
def test_layernorm_mx_fp8(D):
    worst, tolerated, total = 0.0, 0, 0
    for M in VIT_M:
        x0, gamma, beta = R.rows_case(M, D, R.mx_row_seed(D, M))
        eps = 1e-5 if M % 2 else 1e-6
        ref, E = R.ln_ref(x0, gamma, beta, eps)
        want, lo, hi = R.mx_scale_window(ref, E)
        case_tol = int((lo != hi).sum())
        assert case_tol <= 0.01 * lo.size
        for ld in (D, 5 * D):
            x = np.full((M, ld), 7.0, np.float32)
            x[:, :D] = x0
            sc_ld = M + 5
            out8 = np.full((M + 3, D), 0x5A, np.uint8)
            sc = np.full((D // 128, sc_ld), 0xA5A5A5A5, np.uint32)
            run(LN_F8, x=x, out=out8, out2=sc, gamma=gamma, beta=beta, M=M, D=D, ld=ld, sc_ld=sc_ld, eps=eps)
            assert (out8[M:] == 0x5A).all() and (sc[:, M:] == 0xA5A5A5A5).all(), "canaries changed"
            val, sb = R.mx_row_decode(out8, sc, M, D)
            assert ((sb >= lo) & (sb <= hi)).all(), "a scale byte is not mx_scale_exp of its block's maximum"
            assert (sb[lo == hi] == want[lo == hi]).all()
            r = R.ratio(val, ref, R.mx_row_bound(ref, E, sb))
            worst = max(worst, r)
            assert r <= 1.0, (M, ld, r)
        tolerated += case_tol
        total += lo.size
    print(f"[rows ln f8 D {D}] max err / bound {worst:.3f}; blocks at a scale boundary {tolerated} of {total}")


@pytest.mark.parametrize("D", VIT_D)
def test_final_norm_cls(D):
    worst = 0.0
    for n in VIT_M:
        for T in (1, 5):
            eps = eps_of(n + T)
            x, gamma, beta = R.rows_case(n, D, 200 + D + n, ld=T * D)
            x[:, D:] = np.nan                                    # the other tokens of a frame: never read
            ref, E = R.ln_ref(x[:, :D], gamma, beta, eps)
            c32 = np.full((n + 2, D), CANARY32, np.float32)
            c16 = np.full((n + 2, D), CANARY16, np.float16)
            cnt = np.array([11], np.uint32)
            run(FINAL_CLS, x=x, out=c32, out2=c16, counter=cnt, gamma=gamma, beta=beta, n=n, T=T, D=D, eps=eps)
            assert (c32[n:] == CANARY32).all() and (c16[n:] == CANARY16).all() and cnt[0] == 11
            assert np.array_equal(c16[:n].view(np.uint16), f16_rne(c32[:n]).view(np.uint16)), "cls_f16 != RNE(cls_f32)"
            r = R.ratio(c32[:n], ref, R.stored_bound(ref, E, "f32"))
            worst = max(worst, r)
            assert r <= 1.0, (n, T, r)
    print(f"[rows final_norm_cls D {D}] max err / bound {worst:.3f}")


def _plant(rows, D):
    """NaN, +inf and a finite value whose square overflows the variance, in rows 1, 3, 4 (row-major views of the CLS rows)."""
    rows[1, D // 3] = np.nan
    rows[3, 0] = np.inf
    rows[4, D - 1] = 1.0e20
    return [1, 3, 4]


@pytest.mark.parametrize("D", [384, 1280])
def test_final_norm_cls_counts_nonfinite_frames(D):
    n, T = 6, 3
    x, gamma, beta = R.rows_case(n, D, 300 + D, ld=T * D)
    x[0, D:] = np.nan                                            # NaN in frame 0's other tokens: not the CLS row's business

    def go(xx, counter):
        c32 = np.full((n, D), CANARY32, np.float32)
        c16 = np.full((n, D), CANARY16, np.float16)
        run(FINAL_CLS, x=xx, out=c32, out2=c16, counter=counter, gamma=gamma, beta=beta, n=n, T=T, D=D, eps=1e-5)
        return c32, c16

    cnt = np.array([7], np.uint32)
    clean32, clean16 = go(x, cnt)
    assert cnt[0] == 7 and np.isfinite(clean32).all()
    bad = x.copy()
    frames = _plant(bad, D)
    b32, b16 = go(bad, cnt)
    assert cnt[0] == 7 + len(frames), f"counter rose by {cnt[0] - 7}, {len(frames)} frames are out of range"
    others = [b for b in range(n) if b not in frames]
    assert np.array_equal(b32[others].view(np.uint32), clean32[others].view(np.uint32))
    assert np.array_equal(b16[others].view(np.uint16), clean16[others].view(np.uint16))
    n32, n16 = go(bad, None)                                     # nonfinite = NULL: same rows
    assert np.array_equal(n32.view(np.uint32), b32.view(np.uint32)) and np.array_equal(n16.view(np.uint16), b16.view(np.uint16))


# ---- ConvNeXt producers ------------------------------------------------------------------------------------------------
def _cnx_params(C, seed):
    rng = np.random.default_rng(seed)
    gamma = (1.0 + 0.5 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(C)).astype(np.float32)
    wt = (rng.standard_normal((49, C)) / 7.0).astype(np.float32)
    bias = (0.2 * rng.standard_normal(C)).astype(np.float32)
    return rng, gamma, beta, wt, bias


def _lds(C):
    return (C, (C + 127) // 128 * 128)


def test_cnx_stem_gather_is_exact():
    rng = np.random.default_rng(5)
    n, h, w = 3, 9, 14                                           # neither a multiple of 4: the remainder is never read
    ho, wo = h // 4, w // 4
    row_stride, ps = 3 * w + 5, 3
    rgb = rng.integers(0, 255, (n, h, row_stride), dtype=np.uint8)
    green = rgb[:, :, 1:1 + 3 * w:3]                             # the green plane inside RGB rows with 5 bytes of padding
    green[:, 4 * ho:], green[:, :, 4 * wo:] = 255, 255
    want = R.cnx_stem_ref(np.ascontiguousarray(green), True)
    plain = None
    for split in (0, 1):
        A = np.full((n * ho * wo + 2, 32), CANARY32, np.float32)
        run(CNX_STEM_U8, x_addr=rgb.ctypes.data + 1, x_bytes=rgb.nbytes - 1, out=A, n=n, h=h, w=w, split=split,
            frame_stride=h * row_stride, row_stride=row_stride, pixel_stride=ps)
        assert (A[-2:] == CANARY32).all()
        if not split:
            plain = A[:-2].copy()
            assert np.array_equal(plain.view(np.uint32), want.view(np.uint32)) and not plain[:, 16:].any()
        else:
            assert np.array_equal(R.decode_split_operand(A[:-2], 32, 1.0), R.split_value(plain, 1.0))
    f = rng.standard_normal((n, h, w)).astype(np.float32)
    f[:, 4 * ho:], f[:, :, 4 * wo:] = np.nan, np.nan
    want = R.cnx_stem_ref(f, False)
    for split in (0, 1):
        A = np.full((n * ho * wo + 2, 32), CANARY32, np.float32)
        run(CNX_STEM_F32, x=f, out=A, n=n, h=h, w=w, split=split)
        assert (A[-2:] == CANARY32).all()
        if not split:
            assert np.array_equal(A[:-2].view(np.uint32), want.view(np.uint32))
        else:
            assert np.array_equal(R.decode_split_operand(A[:-2], 32, 1.0), R.split_value(want, 1.0))


@pytest.mark.parametrize("C", CNX_C)
def test_cnx_ln_rows_in_place(C):
    worst = 0.0
    for M in VIT_M:
        for ld in _lds(C):
            eps = eps_of(M + ld)
            x, gamma, beta = R.rows_case(M, C, 400 + C + M, ld=ld)
            ref, E = R.ln_ref(x[:, :C], gamma, beta, eps)
            img = np.full((M + 3, ld), CANARY32, np.float32)
            img[:M] = x
            run(CNX_LN_ROWS, out=img, gamma=gamma, beta=beta, M=M, D=C, ld=ld, eps=eps)
            assert (img[M:] == CANARY32).all() and (img[:M, C:] == np.float32(7.0)).all(), "bytes outside [M][C] changed"
            r = R.ratio(img[:M, :C], ref, R.stored_bound(ref, E, "f32"))
            worst = max(worst, r)
            assert r <= 1.0, (M, ld, r)
    print(f"[rows cnx_ln_rows C {C}] max err / bound {worst:.3f}")


@pytest.mark.parametrize("C", CNX_C)
def test_cnx_downsample(C):
    worst = 0.0
    rng, gamma, beta, _, _ = _cnx_params(C, 500 + C)
    n = 3
    for gi, (h, w) in enumerate(((5, 7), (2, 2))):
        for ld in _lds(C):
            eps = eps_of(gi + ld)
            x = np.full((n, h, w, ld), 7.0, np.float32)
            x[..., :C] = (rng.standard_normal((n, h, w, C)) * 1.5 + rng.standard_normal((n, h, w, 1))).astype(np.float32)
            x[0, 0, 0, :C] = (1e3 + rng.standard_normal(C)).astype(np.float32)
            x[1, 1, 1, :C] = np.float32(-0.75)
            x[2, 0, 1, C // 2] = np.float32(1.0e4)
            ho, wo = h // 2, w // 2
            x[:, 2 * ho:], x[:, :, 2 * wo:] = np.nan, np.nan     # the odd grid's last row / column: never read
            ref, E = R.cnx_downsample_ref(x[..., :C], gamma, beta, eps)
            m = n * ho * wo
            outs = []
            for split in (0, 1):
                A = np.full((m + 2, 4 * C), CANARY32, np.float32)
                run(CNX_DOWNSAMPLE, x=x, out=A, gamma=gamma, beta=beta, n=n, h=h, w=w, D=C, ld=ld, eps=eps, split=split)
                assert (A[m:] == CANARY32).all()
                outs.append(A[:m])
            assert np.isfinite(outs[0]).all(), "a NaN of the unread last row / column reached the output"
            assert np.array_equal(R.decode_split_operand(outs[1], 4 * C, 1.0), R.split_value(outs[0], 1.0))
            r = R.ratio(outs[0], ref, R.stored_bound(ref, E, "f32"))
            worst = max(worst, r)
            assert r <= 1.0, (h, w, ld, r)
    print(f"[rows cnx_downsample C {C}] max err / bound {worst:.3f}")


@pytest.mark.parametrize("C", CNX_C)
def test_cnx_dwconv_ln(C):
    worst = 0.0
    rng, gamma, beta, wt, bias = _cnx_params(C, 600 + C)
    n = 3
    for fi, (h, w) in enumerate(((1, 1), (2, 3), (3, 3), (7, 7), (8, 5), (14, 14))):
        ld = _lds(C)[fi % 2]
        eps = eps_of(fi // 2)
        x = np.full((n, h, w, ld), 7.0, np.float32)
        x[..., :C] = (rng.standard_normal((n, h, w, C)) * 1.5 + 0.3).astype(np.float32)
        x[0, ..., :C] *= np.float32(1.0e6)                       # the neighbours: a leak across frames is unmistakable
        x[2, ..., :C] *= np.float32(-1.0e6)
        ref, E = R.cnx_dwconv_ln_ref(x[..., :C], wt, bias, gamma, beta, eps)
        m = n * h * w
        outs = []
        for split in (0, 1):
            A = np.full((m + 2, C), CANARY32, np.float32)
            run(CNX_DWCONV_LN, x=x, out=A, gamma=gamma, beta=beta, wt=wt, bias=bias, n=n, h=h, w=w, D=C, ld=ld, eps=eps, split=split)
            assert (A[m:] == CANARY32).all()
            outs.append(A[:m])
        assert np.array_equal(R.decode_split_operand(outs[1], C, 1.0), R.split_value(outs[0], 1.0))
        for b in range(n):                                       # each frame alone: bit-identical
            A1 = np.full((h * w, C), CANARY32, np.float32)
            run(CNX_DWCONV_LN, x=np.ascontiguousarray(x[b:b + 1]), out=A1, gamma=gamma, beta=beta, wt=wt, bias=bias, n=1, h=h, w=w,
                D=C, ld=ld, eps=eps)
            assert np.array_equal(A1.view(np.uint32), outs[0][b * h * w:(b + 1) * h * w].view(np.uint32)), (h, w, b)
        r = R.ratio(outs[0], ref, R.stored_bound(ref, E, "f32"))
        worst = max(worst, r)
        assert r <= 1.0, (h, w, ld, r)
    print(f"[rows cnx_dwconv_ln C {C}] max err / bound {worst:.3f}")


@pytest.mark.parametrize("C", CNX_C)
def test_cnx_pool_ln(C):
    worst = 0.0
    rng, gamma, beta, _, _ = _cnx_params(C, 700 + C)
    n = 3
    for hi, hw in enumerate((1, 3, 4, 5, 49, 196)):
        ld = _lds(C)[hi % 2]
        eps = eps_of(hi // 2)
        x = np.full((n, hw, ld), 7.0, np.float32)
        x[..., :C] = (rng.standard_normal((n, hw, C)) * 1.5 + rng.standard_normal((n, 1, 1))).astype(np.float32)
        x[1, :, :C] += np.float32(1.0e3)                         # a large pooled mean with a small spread
        x[2, :, C // 3] = np.float32(1.0e4)                      # one massive channel
        ref, E = R.cnx_pool_ln_ref(x[..., :C], gamma, beta, eps)
        c32 = np.full((n + 2, C), CANARY32, np.float32)
        c16 = np.full((n + 2, C), CANARY16, np.float16)
        cnt = np.array([3], np.uint32)
        run(CNX_POOL_LN, x=x, out=c32, out2=c16, counter=cnt, gamma=gamma, beta=beta, n=n, h=1, w=hw, D=C, ld=ld, eps=eps)
        assert (c32[n:] == CANARY32).all() and (c16[n:] == CANARY16).all() and cnt[0] == 3
        assert np.array_equal(c16[:n].view(np.uint16), f16_rne(c32[:n]).view(np.uint16)), "cls_f16 != RNE(cls_f32)"
        r = R.ratio(c32[:n], ref, R.stored_bound(ref, E, "f32"))
        worst = max(worst, r)
        assert r <= 1.0, (hw, ld, r)
    print(f"[rows cnx_pool_ln C {C}] max err / bound {worst:.3f}")


@pytest.mark.parametrize("C", [96, 1536])
def test_cnx_pool_ln_counts_nonfinite_frames(C):
    n, hw = 6, 5
    rng, gamma, beta, _, _ = _cnx_params(C, 800 + C)
    x = (rng.standard_normal((n, hw, C)) * 1.5).astype(np.float32)

    def go(xx, counter):
        c32 = np.full((n, C), CANARY32, np.float32)
        c16 = np.full((n, C), CANARY16, np.float16)
        run(CNX_POOL_LN, x=xx, out=c32, out2=c16, counter=counter, gamma=gamma, beta=beta, n=n, h=1, w=hw, D=C, ld=C, eps=1e-6)
        return c32, c16

    cnt = np.array([7], np.uint32)
    clean32, clean16 = go(x, cnt)
    assert cnt[0] == 7 and np.isfinite(clean32).all()
    bad = x.copy()
    frames = _plant(bad[:, hw - 1], C)                           # one pixel (the last: a partial round of four) per bad frame
    b32, b16 = go(bad, cnt)
    assert cnt[0] == 7 + len(frames), f"counter rose by {cnt[0] - 7}, {len(frames)} frames are out of range"
    others = [b for b in range(n) if b not in frames]
    assert np.array_equal(b32[others].view(np.uint32), clean32[others].view(np.uint32))
    assert np.array_equal(b16[others].view(np.uint16), clean16[others].view(np.uint16))
    n32, n16 = go(bad, None)
    assert np.array_equal(n32.view(np.uint32), b32.view(np.uint32)) and np.array_equal(n16.view(np.uint16), b16.view(np.uint16))


# ---- refusals: by the harness's return code, nothing is launched ----------------------------------------------------------
def test_the_harness_refuses_what_a_launcher_would_mishandle():
    D, M = 256, 4
    x, gamma, beta = R.rows_case(M, D, 1)
    out16 = np.zeros((M, D), np.float16)
    out32 = np.zeros((M, D), np.float32)
    sc = np.zeros((D // 128, M), np.uint32)
    out8 = np.zeros((M, D), np.uint8)
    ok = dict(x=x, out=out16, gamma=gamma, beta=beta, M=M, D=D, ld=D, eps=1e-5)
    assert rows_call(LN_F16, **ok) == 0
    bad = lambda op=LN_F16, **kw: rows_call(op, **{**ok, **kw})          # noqa: E731
    assert bad(M=0) == EINVAL and bad(M=-3) == EINVAL
    assert bad(D=130) == EINVAL and bad(D=0) == EINVAL                   # D % 4
    assert bad(ld=D - 4) == EINVAL                                       # ld < D
    assert bad(M=M + 1) == EINVAL                                        # the rows leave x and out
    assert bad(x=None) == EINVAL and bad(gamma=None) == EINVAL and bad(out=None) == EINVAL
    assert bad(ld=2 * D) == EINVAL                                       # a row stride that leaves the input image
    big = np.zeros((1, 1284), np.float32)
    for op in (LN_F16, LN_F32, FINAL_CLS):                               # beyond the launcher's switch
        assert rows_call(op, x=big, out=np.zeros((1, 1284), np.float32), gamma=big[0], beta=big[0], M=1, n=1, T=1, D=1284, ld=1284,
                         eps=1e-5) == EINVAL
    assert bad(LN_SPLIT, out=out32, D=48, ld=48) == EINVAL               # split: whole 32-column tiles
    f8 = dict(out=out8, out2=sc, sc_ld=M)
    assert bad(LN_F8, **f8) == 0
    assert bad(LN_F8, **{**f8, "sc_ld": M - 1}) == EINVAL
    assert bad(LN_F8, **{**f8, "out2": None}) == EINVAL
    for Dbad in (128, 1280, 320):
        xb, gb, bb = R.rows_case(M, Dbad, 2)
        assert rows_call(LN_F8, x=xb, out=np.zeros((M, Dbad), np.uint8), out2=np.zeros((Dbad // 128 + 1, M), np.uint32), gamma=gb, beta=bb,
                         M=M, D=Dbad, ld=Dbad, sc_ld=M, eps=1e-5) == EINVAL, Dbad
    # ConvNeXt: widths, grids, strides
    Cw = 96
    xc = np.zeros((2, 3, 3, Cw), np.float32)
    g = np.ones(Cw, np.float32)
    A = np.zeros((2 * 9, 4 * Cw), np.float32)
    cn = dict(x=xc, out=A, gamma=g, beta=g, wt=np.zeros((49, Cw), np.float32), bias=g, n=2, h=3, w=3, D=Cw, ld=Cw, eps=1e-6)
    assert rows_call(CNX_DWCONV_LN, **cn) == 0 and rows_call(CNX_DOWNSAMPLE, **cn) == 0
    assert rows_call(CNX_DWCONV_LN, **{**cn, "n": 0}) == EINVAL
    assert rows_call(CNX_DWCONV_LN, **{**cn, "n": 3}) == EINVAL          # a third frame leaves the input image
    assert rows_call(CNX_DWCONV_LN, **{**cn, "wt": None}) == EINVAL
    assert rows_call(CNX_DWCONV_LN, **{**cn, "D": 80}) == EINVAL         # C % 32
    assert rows_call(CNX_DWCONV_LN, **{**cn, "ld": Cw - 32}) == EINVAL
    assert rows_call(CNX_DOWNSAMPLE, **{**cn, "h": 1}) == EINVAL
    assert rows_call(CNX_POOL_LN, **{**cn, "out": None}) == EINVAL       # cls_f32 and cls_f16 both NULL
    wide = np.zeros((1, 1568), np.float32)
    assert rows_call(CNX_LN_ROWS, out=wide, gamma=wide[0], beta=wide[0], M=1, D=1568, ld=1568, eps=1e-6) == EINVAL
    frames = np.zeros((2, 8, 8), np.uint8)
    As = np.zeros((2 * 4, 32), np.float32)
    st = dict(x=frames, out=As, n=2, h=8, w=8, frame_stride=64, row_stride=8, pixel_stride=1)
    assert rows_call(CNX_STEM_U8, **st) == 0
    assert rows_call(CNX_STEM_U8, **{**st, "h": 3}) == EINVAL and rows_call(CNX_STEM_U8, **{**st, "w": 3}) == EINVAL
    assert rows_call(CNX_STEM_U8, **{**st, "frame_stride": 65}) == EINVAL      # the last frame's last patch leaves the image
    assert rows_call(CNX_STEM_U8, **{**st, "pixel_stride": 3}) == EINVAL
    assert rows_call(CNX_STEM_U8, **{**st, "row_stride": 0}) == EINVAL
    assert rows_call(CNX_STEM_F32, x=np.zeros((2, 3, 8), np.float32), out=As, n=2, h=3, w=8) == EINVAL
    a = RowsArgs()
    a.struct_bytes = C.sizeof(RowsArgs) - 8                                     # the handshake
    assert _lib.load().cbas_debug_rows_run(C.byref(a)) == EINVAL
