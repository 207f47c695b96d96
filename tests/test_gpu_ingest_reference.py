"""Single launches of the ViT ingest kernels and the create-time weight packers against exact references, bit for bit.

Each harness call (cbas_debug_pack_run, debug build) feeds host operands to ONE launcher: the four im2col launchers (each of
which also launches its prefix-row writer) and the packers launch_pack_patch_weight, launch_pack_patch_weight_f32,
launch_pack_split_weight, launch_convert_f16, launch_interleave_gate_up and launch_pack_fp8_weight.  Every one of them has an
exact answer (oracle/kernel_ref.py, written from the contracts in csrc/kernels.h and tied to the model definition on the CPU by
tests/test_kernel_reference_bounds.py), so every comparison here is np.array_equal on bit views: there is no tolerance in this
file.  The output images are pre-filled, uploaded and copied back whole, so whatever a launch does not own is a canary:
  - ingest: a non-square patch grid (2 x 3, a py / px swap is another matrix), a remainder that is never read (255 / NaN), 252 or
    288 threads; slots with j >= ps are zero, slot rows i >= ps and the rows past n P keep the canary; the K = 512 form holds hi in
    columns 0 .. 255 and lo in 256 .. 511; the split images decode to split_value(plain, 1.0); a planar byte layout gives the bytes
    of the interleaved one; of x exactly the prefix rows are written, NaN payloads included;
  - packers: the rows past the last one keep the canary; the lo == NULL forms leave hi as it was; three launch_pack_fp8_weight calls
    into one scale image (the q | k | v routing) leave each other's bytes and the unused columns alone;
  - the harness refuses, by return code and without launching, every argument the launchers would mis-handle.
Shapes run: ingest n = 3, ps 14 -> 31 x 47 pixels, ps 16 -> 35 x 53, n_prefix 5, D 132 (prefix rows: n_prefix 1 / 5, D 4 / 132 / 768);
PATCH_W* D 1 / 5 / 8; SPLIT_W (1, 32), (5, 96), (3, 256); CONVERT_F16 1 / 255 / 257; INTERLEAVE (32, 1), (32, 5), (96, 40); FP8_W
(3, 128), (5, 384)."""
import ctypes as C

import numpy as np
import pytest

from cbas_amd import _lib
from oracle import kernel_ref as R
from oracle.mx_oracle import e4m3_decode, mx_quant

pytestmark = pytest.mark.gpu

c_int, c_int64, c_float, c_void_p = C.c_int, C.c_int64, C.c_float, C.c_void_p
(IM2COL_U8, IM2COL_F32, IM2COL_U8_F32, IM2COL_F32_F32, PATCH_W, PATCH_W_F32, SPLIT_W, CONVERT_F16, INTERLEAVE, FP8_W) = range(10)
EINVAL = -1
F32, U16, U32 = np.float32, np.uint16, np.uint32


class PackArgs(C.Structure):            # include/cbas_mi355x_debug.h cbas_debug_pack_args
    _fields_ = ([("struct_bytes", c_int64)] +
                [(n, c_int) for n in ("op", "split", "n", "h", "w", "ps", "n_prefix", "D", "K", "n_total", "n0")] +
                [("scale", c_float), ("N", c_int64), ("F", c_int64), ("frame_stride", c_int64), ("row_stride", c_int64),
                 ("pixel_stride", c_int64), ("in_", c_void_p * 2), ("in_bytes", c_int64 * 2), ("out", c_void_p * 4),
                 ("out_bytes", c_int64 * 4)])


CAN16 = U16(0xE4D2)                     # fp16 -1234.0; an fp32 image of it reads 0xE4D2E4D2
CAN8 = np.uint8(0x5A)
CAN_SC = U32(0xA5A5A5A5)


def make_args(op, ins, outs, **kw):
    """The argument block of one harness call.  ins / outs: arrays (C-contiguous), (address, bytes) pairs, or None."""
    a = PackArgs()
    a.struct_bytes = C.sizeof(PackArgs)
    a.op = op
    for k, v in kw.items():
        setattr(a, k, v)
    for field, count, items in (("in_", "in_bytes", ins), ("out", "out_bytes", outs)):
        for i, t in enumerate(items):
            if t is None:
                continue
            if isinstance(t, tuple):
                addr, nbytes = t
            else:
                assert t.flags.c_contiguous
                addr, nbytes = t.ctypes.data, t.nbytes
            getattr(a, field)[i] = addr
            getattr(a, count)[i] = nbytes
    return a


def pack_call(op, ins, outs, **kw):
    """One harness call; returns its code.  The out arrays are updated in place."""
    _lib.require_debug("cbas_debug_pack_run")
    return _lib.load().cbas_debug_pack_run(C.byref(make_args(op, ins, outs, **kw)))


def run(op, ins, outs, **kw):
    _lib.check(pack_call(op, ins, outs, **kw), f"cbas_debug_pack_run(op {op})")


# ---- ingest --------------------------------------------------------------------------------------------------------------------
def ingest_shape(ps):
    return 3, 2 * ps + 3, 3 * ps + 5            # a 2 x 3 patch grid, 3 rows and 5 columns never read


_u8_cache = {}


def u8_frames(ps):
    """(green [n][h][w], interleaved buffer, its strides, planar buffer, its strides).  The pixels read are random bytes with all
    256 values in every frame; the green pixels past the last whole patch hold 255.  Interleaved: RGB pixels, 5 bytes of padding
    after each row, frames h * row_stride + 7 bytes apart, red / blue / padding random - the caller passes buffer + 1."""
    if ps not in _u8_cache:
        n, h, w = ingest_shape(ps)
        rng = np.random.default_rng(900 + ps)
        green = np.full((n, h, w), 255, np.uint8)
        valid = rng.integers(0, 256, (n, 2 * ps, 3 * ps), dtype=np.uint8)
        for b in range(n):
            valid[b].reshape(-1)[rng.permutation(valid[b].size)[:256]] = np.arange(256, dtype=np.uint8)
            assert len(np.unique(valid[b])) == 256
        green[:, :2 * ps, :3 * ps] = valid
        rs = 3 * w + 5
        fs = h * rs + 7
        rgb = rng.integers(0, 256, n * fs + 3, dtype=np.uint8)
        for b in range(n):
            for y in range(h):
                o = 1 + b * fs + y * rs
                rgb[o:o + 3 * w:3] = green[b, y]
        _u8_cache[ps] = (green, rgb, (fs, rs, 3), np.ascontiguousarray(green).reshape(-1).copy(), (h * w, w, 1))
    return _u8_cache[ps]


def prefix_rows(NP, D, seed):
    p = np.random.default_rng(seed).standard_normal((NP, D)).astype(F32)
    pb = p.view(U32)
    pb[0, 0], pb[NP - 1, D - 1] = 0x7FC12345, 0xFFA00001      # a quiet and a signalling NaN with payloads
    pb[0, 1], pb[0, 2] = 0x80000000, 0x00000001               # -0.0, the smallest subnormal
    return p


def run_ingest(op, split, ps, NP, D, layout="rgb", seed=0):
    """One ingest launch on the suite's frames.  Returns (A as uint16 [n P + 2][halves], x [n T + 2][D] fp32, prefix)."""
    n, h, w = ingest_shape(ps)
    P = 6
    T = P + NP
    halves = 256 if op == IM2COL_U8 else 512                  # 256 fp16; 512 fp16; 256 fp32 slots
    A = np.full((n * P + 2, halves), CAN16, U16)
    x = np.full((n * T + 2, 2 * D), CAN16, U16).view(F32)
    prefix = prefix_rows(NP, D, 40 + NP + D + seed)
    kw = dict(n=n, h=h, w=w, ps=ps, n_prefix=NP, D=D, split=split)
    if op in (IM2COL_U8, IM2COL_U8_F32):
        _, rgb, st_rgb, planar, st_pl = u8_frames(ps)
        buf, st, off = (rgb, st_rgb, 1) if layout == "rgb" else (planar, st_pl, 0)
        frames = (buf.ctypes.data + off, buf.nbytes - off)
        kw.update(frame_stride=st[0], row_stride=st[1], pixel_stride=st[2])
    else:
        frames = R.ingest_float_planes(n, h, w, ps, 700 + ps)
    run(op, (frames, prefix), (A, x), **kw)
    return A, x, prefix


def check_x(x, prefix, n, T):
    """Rows b T + r, r < n_prefix, hold prefix[r] bit for bit; every patch row and every row past n T keeps the canary."""
    NP = prefix.shape[0]
    want = np.full(x.shape, 0, U32)
    want[:] = U32(0xE4D2E4D2)
    for b in range(n):
        want[b * T:b * T + NP] = prefix.view(U32)
    got = x.view(U32)
    for b in range(n):
        assert np.array_equal(got[b * T:b * T + NP], want[b * T:b * T + NP]), f"prefix rows of frame {b}"
        assert np.array_equal(got[b * T + NP:(b + 1) * T], want[b * T + NP:(b + 1) * T]), f"a patch row of frame {b} was written"
    assert np.array_equal(got[n * T:], want[n * T:]), "a row past n T was written (the prefix writer ran too far)"


def ingest_values(op, ps):
    """(values [n P][256] in the slot layout as the op stores them before any split, owned [256])."""
    n, h, w = ingest_shape(ps)
    if op in (IM2COL_U8, IM2COL_U8_F32):
        v, owned = R.vit_im2col_ref(u8_frames(ps)[0], ps)
        return (v.astype(F32) if op == IM2COL_U8 else R.u8_to_unit_f32(v)), owned
    v, owned = R.vit_im2col_ref(R.ingest_float_planes(n, h, w, ps, 700 + ps), ps)
    assert np.isfinite(v).all()
    return v, owned


def ingest_want(op, split, ps, rows):
    """The whole A image a launch must leave, as uint16 [rows][halves], and the mask of the halves the launch owns."""
    v, owned = ingest_values(op, ps)
    nP = v.shape[0]
    if op == IM2COL_U8:
        img, own = v.astype(np.float16).view(U16), owned
    elif op == IM2COL_F32:
        hi, lo = R.f16_pair(v)
        img, own = np.concatenate([hi.view(U16), lo.view(U16)], axis=1), np.concatenate([owned, owned])
    elif not split:
        img, own = v.view(U16).reshape(nP, 512), np.repeat(owned, 2)
    else:
        img = R.split_operand_bits(v, 1.0)
        own = np.arange(512) < 32 * ps                        # K-tile t = slot rows 2 t, 2 t + 1: ps / 2 whole 128-byte tiles
    want = np.full((rows, img.shape[1]), CAN16, U16)
    want[:nP, own] = img[:, own]
    return want, own


INGEST = [(IM2COL_U8, 0), (IM2COL_F32, 0), (IM2COL_U8_F32, 0), (IM2COL_U8_F32, 1), (IM2COL_F32_F32, 0), (IM2COL_F32_F32, 1)]
INGEST_IDS = ["u8", "f32", "u8_f32", "u8_f32_split", "f32_f32", "f32_f32_split"]


@pytest.mark.parametrize("ps", [14, 16])
@pytest.mark.parametrize("op,split", INGEST, ids=INGEST_IDS)
def test_ingest_is_exact(op, split, ps):
    n, NP, D, P = 3, 5, 132, 6
    A, x, prefix = run_ingest(op, split, ps, NP, D)
    want, own = ingest_want(op, split, ps, A.shape[0])
    nP = n * P
    assert np.array_equal(A[:nP, own], want[:nP, own]), "an owned slot differs from the reference"
    assert np.array_equal(A[nP:], want[nP:]), "canary rows past n P changed"
    assert np.array_equal(A[:nP, ~own], want[:nP, ~own]), "a slot row i >= ps was written"
    v, owned = ingest_values(op, ps)
    zero = owned & (np.arange(256) % 16 >= ps)
    if ps == 14:
        assert zero.sum() == 28 and (~owned).sum() == 32
    if not split:                                             # slots j >= ps of the rows i < ps: written, as zeros
        cols = {IM2COL_U8: zero, IM2COL_F32: np.concatenate([zero, zero])}.get(op, np.repeat(zero, 2))
        assert not A[:nP, cols].any()
    else:
        plain, _, _ = run_ingest(op, 0, ps, NP, D)
        got = R.decode_split_operand(A[:nP].view(F32), 16 * ps, 1.0)
        assert np.array_equal(got, R.split_value(plain[:nP].view(F32)[:, :16 * ps], 1.0)), "split image != split_value(plain)"
        assert np.array_equal(got, R.split_value(v[:, :16 * ps], 1.0))
        assert not got[:, np.arange(16 * ps) % 16 >= ps].any()
    if op == IM2COL_F32:                                      # hi in columns 0 .. 255, lo in 256 .. 511
        hi, lo = R.f16_pair(v)
        assert np.array_equal(A[:nP, :256][:, owned], hi.view(U16)[:, owned])
        assert np.array_equal(A[:nP, 256:][:, owned], lo.view(U16)[:, owned])
        assert (lo[:, owned] != 0).any()
    check_x(x, prefix, n, P + NP)
    if op in (IM2COL_U8, IM2COL_U8_F32):                      # tight planar rows, pixel_stride 1: the same bytes
        A2, x2, _ = run_ingest(op, split, ps, NP, D, layout="planar")
        assert np.array_equal(A2, A) and np.array_equal(x2.view(U32), x.view(U32))


@pytest.mark.parametrize("D", [4, 132, 768])
@pytest.mark.parametrize("NP", [1, 5])
def test_prefix_rows_are_exact(NP, D):
    """Each of the four launchers runs its own prefix writer; n (n_prefix D / 4) threads: 3 (one partial block) to 2880."""
    for op, split in ((IM2COL_U8, 0), (IM2COL_F32, 0), (IM2COL_U8_F32, 1), (IM2COL_F32_F32, 0)):
        A, x, prefix = run_ingest(op, split, 14, NP, D, seed=op)
        check_x(x, prefix, 3, 6 + NP)
        want, _ = ingest_want(op, split, 14, A.shape[0])
        assert np.array_equal(A, want)


# ---- packers ---------------------------------------------------------------------------------------------------------------------
def patch_weights(D, ps):
    rng = np.random.default_rng(300 + 10 * D + ps)
    w = rng.standard_normal((D, 3, ps, ps)).astype(F32) * np.array([1.0, 0.37, -2.1], F32).reshape(1, 3, 1, 1)
    w[0, :, 0, 0] = [1.0, 2.0 ** -30, -1.0]                    # float32 sum 0, float64 sum 2^-30
    w[0, :, 0, 1] = [16777216.0, 1.0, 1.0]                     # float32 2^24 (beyond fp16: hi = inf, recorded), float64 2^24 + 2
    w[D - 1, :, ps - 1, ps - 1] = [0.1, -0.1, 3.0e-9]
    w[D - 1, :, ps - 1, 0] = [1.0, 2.0 ** -24, 2.0 ** -24]     # (1 + 2^-24) -> 1 (tie), + 2^-24 -> 1 in float32; 1 + 2^-23 in float64
    return w


@pytest.mark.parametrize("ps", [14, 16])
@pytest.mark.parametrize("D", [1, 5, 8])
def test_pack_patch_weight_is_exact(D, ps):
    w = patch_weights(D, ps)
    ref = R.patch_weight_ref(w, ps, False)
    assert not np.array_equal(ref, R.patch_weight_ref(w, ps, True)), "the inputs would not tell the two summations apart"
    h, l = R.f16_pair(ref)
    hi, lo = np.full((D + 1, 256), CAN16, U16), np.full((D + 1, 256), CAN16, U16)
    hi2, lo2 = np.full((D + 1, 512), CAN16, U16), np.full((D + 1, 512), CAN16, U16)
    run(PATCH_W, (w, None), (hi, lo, hi2, lo2), D=D, ps=ps)
    assert np.array_equal(hi[:D], h.view(U16)) and np.array_equal(lo[:D], l.view(U16)), "hi / lo differ from the reference"
    assert np.array_equal(hi2[:D], np.concatenate([h, h], 1).view(U16)) and np.array_equal(lo2[:D], np.concatenate([l, l], 1).view(U16))
    for img in (hi, lo, hi2, lo2):
        assert (img[D] == CAN16).all(), "row D changed"
    assert (l != 0).any()
    hi_b, hi2_b = np.full((D + 1, 256), CAN16, U16), np.full((D + 1, 512), CAN16, U16)
    run(PATCH_W, (w, None), (hi_b, None, hi2_b, None), D=D, ps=ps)
    assert np.array_equal(hi_b, hi) and np.array_equal(hi2_b, hi2), "lo = lo2 = NULL changed hi / hi2"


@pytest.mark.parametrize("ps", [14, 16])
@pytest.mark.parametrize("D", [1, 5, 8])
def test_pack_patch_weight_f32_is_exact(D, ps):
    w = patch_weights(D, ps)
    out = np.full((D + 1, 512), CAN16, U16)
    run(PATCH_W_F32, (w, None), (out, None, None, None), D=D, ps=ps)
    assert np.array_equal(out[:D].view(U32), R.patch_weight_ref(w, ps, True).view(U32))
    assert (out[D] == CAN16).all(), "row D changed"


@pytest.mark.parametrize("scale", [1.0, 2.0 ** 10, 2.0 ** -3], ids=["s1", "s2^10", "s2^-3"])
@pytest.mark.parametrize("N,K", [(1, 32), (5, 96), (3, 256)])
def test_pack_split_weight_is_exact(N, K, scale):
    rng = np.random.default_rng(500 + N + K)
    w = (rng.standard_normal((N, K)) * 10.0 ** rng.uniform(-3, 0.5, (N, K))).astype(F32)
    w[0, :6] = [0.0, -0.0, 1.0, 2.0 ** -8 * 1.2345, -3.0, 1.0 + 2.0 ** -11]
    if scale == 1.0:                                          # low halves in fp16's subnormal range at scale 1
        _, lo = R.f16_pair(w)
        assert ((np.abs(lo) < 2.0 ** -14) & (lo != 0)).any()
    out = np.full((N + 1, 2 * K), CAN16, U16)
    run(SPLIT_W, (w, None), (out, None, None, None), N=N, K=K, scale=scale)
    # Finding (kernels.h, launch_pack_split_weight): for x = -0.0 the packer stores lo = -0.0 (0x8000) where fp16(x - hi) is +0.0 -
    # the compiler fuses the scale, the rounding and the subtraction into mixed-precision FMAs (v_fma_mixlo_f16 / v_fma_mix_f32) and
    # the zero keeps the product's sign; the ingest kernels (no scale multiply to fuse) store +0.0.  hi + lo is -0.0 either way.  So
    # the low half of a zero is held to be A zero, every other half to the reference's bits.
    k = np.arange(32)
    zero_lo = np.zeros((N, K // 32, 2, 32), bool)
    zero_lo[:, :, 1, 8 * ((k % 16) // 4) + 4 * (k // 16) + k % 4] = (w == 0).reshape(N, K // 32, 32)
    zero_lo = zero_lo.reshape(N, 2 * K)
    want = R.split_operand_bits(w, scale)
    assert zero_lo.sum() == 2
    assert np.array_equal(out[:N][~zero_lo], want[~zero_lo]), "the split image differs from the reference"
    assert ((out[:N][zero_lo] & 0x7FFF) == 0).all(), "the low half of a zero is not a zero"
    assert np.array_equal(R.decode_split_operand(out[:N].view(F32), K, scale), R.split_value(w, scale))
    assert (out[N] == CAN16).all(), "the row past N changed"


CONVERT_EDGES = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2049.0, 2051.0, -2049.0, 65504.0, 65505.0, 65519.996, 65520.0, 65536.0,
                          1.0e6, -65520.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 1.0001 * 2.0 ** -25, -(2.0 ** -25), 1.1 * 2.0 ** -15,
                          2.0 ** -14 - 2.0 ** -25, 0.0, -0.0, 2.0 ** -149, 1.0 / 3.0, -1.0 / 255.0], F32)


@pytest.mark.parametrize("with_lo", [True, False], ids=["lo", "nolo"])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_convert_f16_is_exact(n, with_lo):
    rng = np.random.default_rng(600 + n)
    v = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 4, n)).astype(F32)
    m = min(n, len(CONVERT_EDGES))
    v[n - m:] = CONVERT_EDGES[:m]                             # n = 1: the tie 1 + 2^-11; the last elements of the partial block otherwise
    h, l = R.f16_pair(v)
    if n > 1:
        assert np.isinf(h).any() and np.isinf(l).any(), "the overflow to infinity is part of the record"
    hi, lo = np.full(n + 1, CAN16, U16), np.full(n + 1, CAN16, U16)
    run(CONVERT_F16, (v, None), (hi, lo if with_lo else None, None, None), N=n)
    assert np.array_equal(hi[:n], h.view(U16)), "hi differs from numpy's round-to-nearest-even"
    assert hi[n] == CAN16 and lo[n] == CAN16
    if with_lo:
        assert np.array_equal(lo[:n], l.view(U16)), "lo differs from fp16(v - hi)"
    else:
        assert (lo == CAN16).all()


@pytest.mark.parametrize("F,K", [(32, 1), (32, 5), (96, 40)])
def test_interleave_gate_up_is_exact(F, K):
    gate = np.arange(F * K, dtype=np.int64).reshape(F, K).astype(F32)
    up = gate + F32(F * K)
    out = np.full((2 * F + 1, 2 * K), CAN16, U16)
    run(INTERLEAVE, (gate, up), (out, None, None, None), F=F, K=K)
    got = out[:2 * F].view(F32)
    want = R.interleave_ref(gate, up)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), f"out rows {bad[:8]} hold source rows {(got[bad[:8], 0] // K).astype(int)} (gate 0 .. {F - 1}, up {F} ..)"
    assert np.array_equal(got.view(U32), want.view(U32)) and (out[2 * F] == CAN16).all()


FP8_E = {128: (-3, 0, 5), 384: (-9, -3, 0, 5, 7)}


def fp8_weights(N, K, seed):
    """[N][K] fp32 by blocks of 32: random blocks over six decades, one all-zero block, one whose maximum 440 s rounds up to 448
    after scaling, and maxima exactly at 448 * 2^e, one fp32 ulp above and one below, for several e."""
    rng = np.random.default_rng(seed)
    nb = N * K // 32
    w = (rng.standard_normal((nb, 32)) * 10.0 ** rng.uniform(-3, 3, (nb, 1))).astype(F32)
    tops = [None, F32(440.0 * 4.0)]
    for e in FP8_E[K]:
        t = F32(448.0 * 2.0 ** e)
        tops += [t, np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(0.0))]
    assert len(tops) <= nb
    for blk, t in zip(rng.permutation(nb)[:len(tops)], tops):
        if t is None:
            w[blk] = 0.0
            continue
        w[blk] = (rng.uniform(-0.5, 0.5, 32) * float(t)).astype(F32)
        w[blk, rng.integers(32)] = t if rng.integers(2) else -t
    w[w == 0] = np.abs(w[w == 0])                               # +0.0 only: mx_quant has no sign for a zero
    return w.reshape(N, K)


def check_fp8(w8, N, w):
    q = mx_quant(w)[1]
    assert not ((w8[:N] & 0x7F) == 0x7F).any(), "an e4m3 NaN code"
    assert np.array_equal(e4m3_decode(w8[:N]).view(U32), q.view(U32)), "the bytes do not decode to mx_quant's elements"
    assert (w8[N] == CAN8).all(), "the row past N changed"


@pytest.mark.parametrize("route", [0, 1, 2], ids=["n0=0", "n0=N", "n0=2N+4"])
@pytest.mark.parametrize("N,K", [(3, 128), (5, 384)])
def test_pack_fp8_weight_is_exact(N, K, route):
    n_total, n0 = ((N, 0), (3 * N + 4, N), (3 * N + 4, 2 * N + 4))[route]
    w = fp8_weights(N, K, 800 + N + route)
    sb = mx_quant(w)[2]
    assert (sb == 0).any() and len(np.unique(sb)) > 6
    w8 = np.full((N + 1, K), CAN8, np.uint8)
    sc = np.full((K // 128 + 1, n_total), CAN_SC, U32)         # one canary row of dwords past the image
    run(FP8_W, (w, None), (w8, sc, None, None), N=N, K=K, n_total=n_total, n0=n0)
    check_fp8(w8, N, w)
    _, want = R.fp8_weight_ref(w, sc[:-1] * 0 + CAN_SC, n_total, n0)
    assert np.array_equal(sc[:-1], want), "a scale byte is misplaced or wrong"
    assert (sc[-1] == CAN_SC).all()


@pytest.mark.parametrize("N,K", [(3, 128), (5, 384)])
def test_pack_fp8_weight_routes_q_k_v_into_one_scale_image(N, K):
    n_total = 3 * N + 4
    sc = np.full((K // 128 + 1, n_total), CAN_SC, U32)
    want = sc[:-1].copy()
    for i, n0 in enumerate((2 * N + 4, 0, N)):
        w = fp8_weights(N, K, 850 + N + i)
        w8 = np.full((N + 1, K), CAN8, np.uint8)
        run(FP8_W, (w, None), (w8, sc, None, None), N=N, K=K, n_total=n_total, n0=n0)
        check_fp8(w8, N, w)
        _, want = R.fp8_weight_ref(w, want, n_total, n0)
        assert np.array_equal(sc[:-1], want), f"call {i} (n0 = {n0}) touched another call's columns or misplaced its own"
    assert (sc[:-1, 2 * N:2 * N + 4] == CAN_SC).all() and (sc[-1] == CAN_SC).all(), "canary dwords changed"


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_harness_refuses_what_the_launchers_would_mishandle():
    """One bad field at a time on otherwise valid arguments: CBAS_EINVAL, and the output images unchanged byte for byte."""
    lib = _lib.load()
    _lib.require_debug("cbas_debug_pack_run")
    ps = 14
    n, h, w = ingest_shape(ps)
    NP, D, P = 2, 8, 6
    _, rgb, st, _, _ = u8_frames(ps)
    fplanes = R.ingest_float_planes(n, h, w, ps, 1)
    prefix = prefix_rows(NP, D, 1)
    u8_need = (n - 1) * st[0] + (2 * ps - 1) * st[1] + (3 * ps - 1) * st[2] + 1

    def outs_for(*shapes):
        return [None if s is None else np.full(s, CAN16, U16) for s in shapes] + [None] * (4 - len(shapes))

    def base(op):
        """(ins, outs, kw) of a valid call of op."""
        if op in (IM2COL_U8, IM2COL_U8_F32):
            return ([(rgb.ctypes.data + 1, u8_need), prefix], outs_for((n * P, 256 if op == IM2COL_U8 else 512), (n * (P + NP), 2 * D)),
                    dict(n=n, h=h, w=w, ps=ps, n_prefix=NP, D=D, frame_stride=st[0], row_stride=st[1], pixel_stride=st[2]))
        if op in (IM2COL_F32, IM2COL_F32_F32):
            return [fplanes, prefix], outs_for((n * P, 512), (n * (P + NP), 2 * D)), dict(n=n, h=h, w=w, ps=ps, n_prefix=NP, D=D)
        if op == PATCH_W:
            return [patch_weights(2, ps), None], outs_for((2, 256), (2, 256), (2, 512), (2, 512)), dict(D=2, ps=ps)
        if op == PATCH_W_F32:
            return [patch_weights(2, ps), None], outs_for((2, 512)), dict(D=2, ps=ps)
        if op == SPLIT_W:
            return [np.ones((2, 96), F32), None], outs_for((2, 192)), dict(N=2, K=96, scale=1.0)
        if op == CONVERT_F16:
            return [np.ones(96, F32), None], outs_for((96,), (96,)), dict(N=96)
        if op == INTERLEAVE:
            return [np.ones((96, 4), F32), np.ones((96, 4), F32)], outs_for((192, 8)), dict(F=96, K=4)
        return [np.ones((2, 384), F32), None], outs_for((2, 192), (3, 2 * 8)), dict(N=2, K=384, n_total=8, n0=3)

    checked = []

    def refused(op, what, mutate=None, **over):
        ins, outs, kw = base(op)
        kw.update(over)
        a = make_args(op, ins, outs, **kw)
        if mutate:
            mutate(a)
        rc = lib.cbas_debug_pack_run(C.byref(a))
        assert rc == EINVAL, f"op {op}: {what} was accepted (code {rc})"
        for o in outs:
            assert o is None or (o == CAN16).all(), f"op {op}: {what} was refused after an output image changed"
        checked.append((op, what))

    def null_in(i):
        return lambda a: a.in_.__setitem__(i, None)

    def null_out(i):
        return lambda a: a.out.__setitem__(i, None)

    def short_in(i):
        return lambda a: a.in_bytes.__setitem__(i, a.in_bytes[i] - 1)

    def short_out(i):
        return lambda a: a.out_bytes.__setitem__(i, a.out_bytes[i] - 1)

    assert lib.cbas_debug_pack_run(None) == EINVAL
    for op in range(10):                                       # every baseline is valid; then the struct size and the op
        ins, outs, kw = base(op)
        run(op, ins, outs, **kw)
        refused(op, "struct_bytes", lambda a: setattr(a, "struct_bytes", a.struct_bytes - 8))
    refused(IM2COL_U8, "op -1", lambda a: setattr(a, "op", -1))
    refused(IM2COL_U8, "op 10", lambda a: setattr(a, "op", 10))
    for op in (IM2COL_U8, IM2COL_F32, IM2COL_U8_F32, IM2COL_F32_F32):
        for i in (0, 1):
            refused(op, f"in[{i}] NULL", null_in(i))
            refused(op, f"out[{i}] NULL", null_out(i))
            refused(op, f"in[{i}] one byte short", short_in(i))
            refused(op, f"out[{i}] one byte short", short_out(i))
        for bad in (0, -1):
            refused(op, f"n = {bad}", n=bad)
            refused(op, f"D = {bad}", D=bad)
        for bad in (0, 8, 15, 32):
            refused(op, f"ps = {bad}", ps=bad)
        refused(op, "h < ps", h=ps - 1)
        refused(op, "w < ps", w=ps - 1)
        refused(op, "n_prefix = 0", n_prefix=0)
        refused(op, "n_prefix = -1", n_prefix=-1)
        refused(op, "D % 4", D=6)
        refused(op, "one frame more than the images hold", n=n + 1)
        refused(op, "one prefix row more than the images hold", n_prefix=NP + 1)
        refused(op, "a patch row more than the images hold", h=3 * ps)
    for op in (IM2COL_U8, IM2COL_U8_F32):
        for name, good in (("frame_stride", st[0]), ("row_stride", st[1]), ("pixel_stride", st[2])):
            for bad in (0, -1, -good):
                refused(op, f"{name} = {bad}", **{name: bad})
            refused(op, f"{name} + 1: the last read leaves in_bytes", **{name: good + 1})
            refused(op, f"{name} = 2^62", **{name: 1 << 62})
    for op in (PATCH_W, PATCH_W_F32):
        refused(op, "w NULL", null_in(0))
        refused(op, "out[0] NULL", null_out(0))
        refused(op, "w one byte short", short_in(0))
        refused(op, "out[0] one byte short", short_out(0))
        for bad in (0, -1):
            refused(op, f"D = {bad}", D=bad)
        refused(op, "D = 3: more rows than the images hold", D=3)
        for bad in (0, 8, 15, 32):
            refused(op, f"ps = {bad}", ps=bad)
    refused(PATCH_W, "hi2 NULL", null_out(2))
    refused(PATCH_W, "lo NULL alone", null_out(1))
    refused(PATCH_W, "lo2 NULL alone", null_out(3))
    for i in (1, 2, 3):
        refused(PATCH_W, f"out[{i}] one byte short", short_out(i))
    for op in (SPLIT_W, CONVERT_F16, FP8_W):
        refused(op, "in[0] NULL", null_in(0))
        refused(op, "out[0] NULL", null_out(0))
        refused(op, "in[0] one byte short", short_in(0))
        refused(op, "out[0] one byte short", short_out(0))
        for bad in (0, -1):
            refused(op, f"N = {bad}", N=bad)
    refused(SPLIT_W, "N = 3", N=3)
    refused(CONVERT_F16, "N = 97", N=97)
    refused(CONVERT_F16, "lo one byte short", short_out(1))
    for bad in (0, -32, 48, 16, 33):
        refused(SPLIT_W, f"K = {bad}", K=bad)
    for bad in (0, -128, 64, 192, 129, 32):
        refused(FP8_W, f"K = {bad}", K=bad)
    refused(FP8_W, "scales NULL", null_out(1))
    refused(FP8_W, "scales one byte short", short_out(1))
    refused(FP8_W, "n0 = -1", n0=-1)
    refused(FP8_W, "n0 + N > n_total", n0=7)
    refused(FP8_W, "n_total = 4 < n0 + N", n_total=4)
    refused(FP8_W, "n_total = 9: a column more than the scale image holds", n_total=9)
    refused(FP8_W, "N = 3", N=3)
    for i in (0, 1):
        refused(INTERLEAVE, f"in[{i}] NULL", null_in(i))
        refused(INTERLEAVE, f"in[{i}] one byte short", short_in(i))
    refused(INTERLEAVE, "out NULL", null_out(0))
    refused(INTERLEAVE, "out one byte short", short_out(0))
    for bad in (0, -32, 48, 16, 97):
        refused(INTERLEAVE, f"F = {bad}", F=bad)
    for bad in (0, -1, 5):
        refused(INTERLEAVE, f"K = {bad}", K=bad)
    refused(INTERLEAVE, "F = 128: more rows than the images hold", F=128)
    assert len(checked) > 200
