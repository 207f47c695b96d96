"""CLS attention maps on the GPU: the kernel of cls_attention.hip one launch at a time against float64 with a derived error bar,
then DinoEncoder.cls_attention against rows recorded from transformers' own models (tests/golden/make_goldens_attention.py),
and the promises around it: nothing else in the forward moves, a frame's map does not depend on its batch, the two ingest forms
agree, refusals, workspace growth, frame_maps / compare_encoders.

The kernel's error bar (u = 2^-24; everything the kernel does is fp32):

  scores.  s = sum of 64 products, summed as an 8-term fmaf chain per lane and a 3-level tree: for any order
      |s^ - s| <= gamma_64 sum_j |q_j k_j|,   gamma_n = n u / (1 - n u).
  Operands: arith 0 gets fp16-representable values and arith 3 fp32 ones, so they enter exactly.  Arith 4 packs x' = x * scale
  (q: 16, K: 4) as hi = fp16(x'), lo = fp16(x' - hi): |x' - hi| <= 2^-11 |x'|, the second rounding leaves 2^-22 |x'| (2^-25
  absolute where lo is subnormal), and the kernel's float(hi) + float(lo) rounds once more: |dx'| <= (2^-22 + 2^-24) |x'| + 2^-25,
  which adds sum_j (|q_j| dk_j + |k_j| dq_j + dq_j dk_j) to the score's bar.  The power-of-two score scale is exact.
  The subtraction s^ - max rounds once: u |s - max| more in the exponent.  E = the largest such total over a row.

  softmax.  The exact softmax of scores that are off by at most E lies within p (exp(2 E) - 1) of p.  On top, relative to p: expf
  (1 ulp <= 2 u) in the numerator; in the denominator the same 2 u and the sum's rounding - every term passes through at most
  d = ceil(T / 1024) + 12 additions (its lane's chain, two 6-level trees): gamma_d; the division: u.  Together
      |p^ - p| <= p (expm1(2 E) + (6 + d) u).

  map.  The head mean adds gamma_NH on the sum and 2 u for 1 / NH and the product: mean_h(bar_h) + (NH + 2) u mean_h(p).
"""
import math
import os

import numpy as np
import pytest
import torch

from cbas_amd import config as C, weights as W, synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ENC_SEED = 1234
CLS_TOL = 1e-3              # precision 0: tests/test_gpu_parity.py's gate
CLS_TOL_F32 = 5e-6          # precisions 3 / 4: tests/test_gpu_fp32.py's gate
MAP_TOL_F32 = 2e-5          # max |d| / max |ref| of heads and map in precisions 3 / 4: the bar of the fp32 stage taps
# precision 0: twice the largest max |d| / max |ref| measured over every fixture on an MI355X (2.33e-3: the heads of ViT-B/16 at
# 224^2; the tiny fixtures measure 2e-4 .. 3.5e-4), rounded up to one digit; may not exceed 1e-2
MAP_TOL_F16 = 5e-3


def _lib():
    from cbas_amd import _lib as L
    L.require_debug("cbas_debug_cls_attention")
    return L.load()


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- the kernel against float64 ---------------------------------------------------------------------------------------------
# (n, T, NH, NP, strided): strided = the queries sit in row b*T of a q|k|v image (row stride T*3*D), else compact rows (stride D)
CASES = [(1, 1, 1, 1, False), (3, 21, 2, 5, False), (1, 63, 2, 1, False), (3, 64, 1, 5, True), (1, 65, 12, 5, False),
         (3, 201, 12, 5, True), (1, 1029, 2, 1, False), (3, 1374, 2, 5, False), (1, 26, 20, 1, True), (3, 201, 20, 5, False),
         (2, 8100, 1, 1, False)]      # the largest T the kernel's 64 KiB of LDS takes is 8160 with NP = 1: eight tokens per thread
EQUAL = (3, 65, 2, 5, False)


def operands(case, fp16, equal=False):
    """q (n, ldq) and K (n T, 3 D) float32 images; scores reach |s| ~ 20 (peaky softmaxes)."""
    n, T, NH, NP, strided = case
    D = 64 * NH
    q = W.synth_normal(91, f"q{case}", (n, D), 1.0)
    K = W.synth_normal(92, f"K{case}", (n * T, 3 * D), 0.75)
    if equal:
        K = np.repeat(K.reshape(n, T, 3 * D)[:, :1], T, axis=1).reshape(n * T, 3 * D)
    if fp16:
        q, K = q.astype(np.float16).astype(np.float32), K.astype(np.float16).astype(np.float32)
    if strided:
        img = W.synth_normal(93, f"img{case}", (n, T * 3 * D), 1.0)
        img[:, :D] = q
        return np.ascontiguousarray(img), np.ascontiguousarray(K), T * 3 * D
    return np.ascontiguousarray(q), np.ascontiguousarray(K), D


def run_kernel(arith, case, q, K, ldq, want_heads=True, want_map=True):
    n, T, NH, NP, _ = case
    heads = np.full((n, NH, T), 7.0, np.float32) if want_heads else None
    mp = np.full((n, T - NP), 7.0, np.float32) if want_map else None
    lib = _lib()
    rc = lib.cbas_debug_cls_attention(arith, q.ctypes.data, K.ctypes.data, n, T, NH, NP, ldq, K.shape[1],
                                      heads.ctypes.data if want_heads else None, mp.ctypes.data if want_map else None)
    assert rc == 0, lib.cbas_last_error()
    return heads, mp


_REF = {}


def reference(arith, case, q, K, key):
    """float64 heads / map and their bars for the values the kernel multiplies."""
    k = (arith if arith == 4 else 0, key, case)
    if k in _REF:
        return _REF[k]
    n, T, NH, NP, _ = case
    D = 64 * NH
    qh = q[:, :D].astype(np.float64).reshape(n, NH, 1, 64)
    kh = K[:, :D].astype(np.float64).reshape(n, T, NH, 64).transpose(0, 2, 1, 3)
    s = (qh * kh).sum(-1)                                            # (n, NH, T)
    sabs = (np.abs(qh) * np.abs(kh)).sum(-1)
    Es = gamma(64) * sabs
    if arith == 4:
        dq = ((2.0 ** -22 + 2.0 ** -24) * np.abs(qh) * 16.0 + 2.0 ** -25) / 16.0
        dk = ((2.0 ** -22 + 2.0 ** -24) * np.abs(kh) * 4.0 + 2.0 ** -25) / 4.0
        Es = Es + (np.abs(qh) * dk + np.abs(kh) * dq + dq * dk).sum(-1)
    m = s.max(-1, keepdims=True)
    E = (Es + U * np.abs(s - m)).max(-1, keepdims=True)
    e = np.exp(s - m)
    p = e / e.sum(-1, keepdims=True)
    d = math.ceil(T / 1024) + 12
    bar = p * (np.expm1(2.0 * E) + (6 + d) * U)
    mp = p[:, :, NP:].mean(1)
    mbar = bar[:, :, NP:].mean(1) + (NH + 2) * U * mp
    _REF[k] = (p, bar, mp, mbar, float(np.abs(s).max()))
    return _REF[k]


def check_against_reference(arith, case, equal=False):
    n, T, NH, NP, _ = case
    q, K, ldq = operands(case, arith == 0, equal)
    p, bar, mp, mbar, smax = reference(arith, case, q, K, ("eq" if equal else "rand", arith == 0))
    heads, got_map = run_kernel(arith, case, q, K, ldq)
    rh = float((np.abs(heads.astype(np.float64) - p) / bar).max())
    rm = float((np.abs(got_map.astype(np.float64) - mp) / mbar).max()) if T > NP else 0.0
    print(f"[cls attention arith {arith} case {case}{' equal scores' if equal else ''}] max |s| {smax:.1f}; error / bound: heads {rh:.3f}, map {rm:.3f}")
    assert np.isfinite(heads).all() and rh <= 1.0 and rm <= 1.0
    # rows sum to 1 within T u
    dev = float(np.abs(heads.astype(np.float64).sum(-1) - 1.0).max())
    assert dev <= T * U, (dev, T * U)
    # the map is the head mean of the patch columns, in fp32, heads ascending, bit for bit
    acc = heads[:, 0, NP:].copy()
    for h in range(1, NH):
        acc = acc + heads[:, h, NP:]
    want = acc * (np.float32(1.0) / np.float32(NH))
    np.testing.assert_array_equal(got_map.view(np.uint32), want.astype(np.float32).view(np.uint32))
    # either output alone gives the same bits
    only_map = run_kernel(arith, case, q, K, ldq, want_heads=False)[1]
    only_heads = run_kernel(arith, case, q, K, ldq, want_map=False)[0]
    np.testing.assert_array_equal(only_map.view(np.uint32), got_map.view(np.uint32))
    np.testing.assert_array_equal(only_heads.view(np.uint32), heads.view(np.uint32))
    return heads, got_map


@pytest.mark.parametrize("arith", (0, 3, 4))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_T%d_NH%d_NP%d_%s" % (c[0], c[1], c[2], c[3], "strided" if c[4] else "compact"))
def test_kernel_against_float64(arith, case):
    check_against_reference(arith, case)


@pytest.mark.parametrize("arith", (0, 3, 4))
def test_kernel_equal_scores(arith):
    heads, _ = check_against_reference(arith, EQUAL, equal=True)
    assert np.abs(heads.astype(np.float64) * EQUAL[1] - 1.0).max() <= 4 * U


@pytest.mark.parametrize("arith", (0, 3, 4))
def test_kernel_nonfinite_row_stays_in_its_frame(arith):
    case = (3, 201, 12, 5, False)
    n, T, NH, NP, _ = case
    q, K, ldq = operands(case, arith == 0)
    good_h, good_m = run_kernel(arith, case, q, K, ldq)
    bad = K.copy()
    bad[1 * T + 77, :] = np.nan
    bad[1 * T + 5, 3] = np.inf
    h, m = run_kernel(arith, case, q, bad, ldq)
    for b in (0, 2):
        np.testing.assert_array_equal(h[b].view(np.uint32), good_h[b].view(np.uint32))
        np.testing.assert_array_equal(m[b].view(np.uint32), good_m[b].view(np.uint32))
    assert not np.isfinite(h[1]).all()


def test_kernel_refusals():
    lib = _lib()
    q = np.zeros((1, 64), np.float32)
    K = np.zeros((4, 64), np.float32)
    out = np.zeros((1, 1, 4), np.float32)
    assert lib.cbas_debug_cls_attention(3, q.ctypes.data, K.ctypes.data, 1, 4, 1, 1, 64, 64, None, None) == -1
    assert lib.cbas_debug_cls_attention(3, q.ctypes.data, K.ctypes.data, 1, 4, 1, 5, 64, 64, out.ctypes.data, None) == -1
    assert lib.cbas_debug_cls_attention(3, q.ctypes.data, K.ctypes.data, 1, 4, 1, 1, 60, 64, out.ctypes.data, None) == -1
    assert lib.cbas_debug_cls_attention(1, q.ctypes.data, K.ctypes.data, 1, 4, 1, 1, 64, 64, out.ctypes.data, None) == -1
    # a token row beyond the kernel's LDS (2 T - NP floats in 64 KiB - 256 bytes: T <= 8160 at NP = 1) is refused, not launched
    T = 8161
    K = np.zeros((T, 64), np.float32)
    out = np.full((1, 1, T), 7.0, np.float32)
    assert lib.cbas_debug_cls_attention(3, q.ctypes.data, K.ctypes.data, 1, T, 1, 1, 64, 64, out.ctypes.data, None) == -1
    assert (out == 7.0).all()
    assert lib.cbas_debug_cls_attention(3, q.ctypes.data, K.ctypes.data, 1, T - 1, 1, 1, 64, 64, out.ctypes.data, None) == 0
    assert np.abs(out[0, 0, :T - 1].astype(np.float64) * (T - 1) - 1.0).max() <= 4 * U and out[0, 0, T - 1] == 7.0


# ---- the encoder against transformers' attentions ----------------------------------------------------------------------------
# fixture -> (config, precisions its family allows, max_frame)
FIXTURES = {"vit_tiny": (C.VIT_TINY, (0, 3, 4)), "gated_tiny": (C.VIT_TINY_GATED, (0, 3, 4)),
            "dinov2reg_tiny": (C.DINOV2_REG_TINY, (0, 3, 4)), "dinov2_tiny": (C.DINOV2_TINY, (0, 3, 4)),
            "vitb16": (C.VIT_B16, (0, 3, 4))}


_WEIGHTS = {}


def make_enc(cfg, hw, max_batch, precision, **kw):
    from cbas_amd.encoder import DinoEncoder
    if cfg not in _WEIGHTS:                     # generated once per configuration and never changed
        _WEIGHTS[cfg] = W.synth_encoder_weights(cfg, ENC_SEED)
    return DinoEncoder.from_weights(cfg, _WEIGHTS[cfg], "cuda", max_batch=max_batch, max_frame=hw, precision=precision, **kw)


def rel_rows(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


def rel_max(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / np.abs(b).max())


@pytest.mark.parametrize("precision", (0, 3, 4))
@pytest.mark.parametrize("name", list(FIXTURES))
def test_encoder_against_goldens(golden_dir, name, precision):
    cfg, precisions = FIXTURES[name]
    assert precision in precisions
    g = np.load(os.path.join(golden_dir, f"cls_attention_{name}.npz"))
    tags = [str(t) for t in g["tags"]]
    hw = (max(int(g[f"{t}_height"]) for t in tags), max(int(g[f"{t}_width"]) for t in tags))
    enc = make_enc(cfg, hw, 4, precision)
    NP = 1 + cfg.num_register_tokens
    try:
        for t in tags:
            n, H, Wd, seed = (int(g[f"{t}_{k}"]) for k in ("n", "height", "width", "seed"))
            dev = torch.from_numpy(synth.cage_frames(seed, n, H, Wd)).cuda()
            c16, c32, maps, heads = enc.cls_attention(dev, per_head=True)
            nh, nw = H // cfg.patch_size, Wd // cfg.patch_size
            assert maps.shape == (n, nh, nw) and heads.shape == (n, cfg.num_attention_heads, NP + nh * nw)
            eh = rel_max(heads.cpu().numpy(), g[f"{t}_heads"])
            em = rel_max(maps.cpu().numpy().reshape(n, -1), g[f"{t}_map"])
            ec = float(rel_rows(c32.cpu().numpy(), g[f"{t}_cls"]).max())
            print(f"[cls attention {name} {t} {H}x{Wd} p{precision}] max |d| / max |ref|: heads {eh:.3e}, map {em:.3e}; CLS rel {ec:.2e}")
            tol = MAP_TOL_F16 if precision == 0 else MAP_TOL_F32
            assert eh < tol and em < tol
            assert ec < (CLS_TOL if precision == 0 else CLS_TOL_F32)
            np.testing.assert_array_equal(enc.cls_attention(dev)[2].cpu().numpy(), maps.cpu().numpy())       # the map-only form
    finally:
        enc.close()


def _bits(t):
    return t.cpu().numpy().view(np.uint16 if t.dtype == torch.float16 else np.uint32)


def _same_as_encode(enc, dev):
    a16, a32 = enc.encode_u8(dev)
    a16, a32 = _bits(a16), _bits(a32)
    b16, b32, maps, heads = enc.cls_attention(dev, per_head=True)
    np.testing.assert_array_equal(_bits(b16), a16)
    np.testing.assert_array_equal(_bits(b32), a32)
    c16, c32 = enc.encode_u8(dev)                       # and a following plain call
    np.testing.assert_array_equal(_bits(c16), a16)
    np.testing.assert_array_equal(_bits(c32), a32)
    assert torch.isfinite(maps).all() and torch.isfinite(heads).all()
    assert float((heads.double().sum(-1) - 1.0).abs().max()) <= heads.shape[-1] * U
    return maps, heads


# (config, frame size, frames, max_batch, precisions)
# precision 2 needs widths that are multiples of 256: ViT-B carries it, the tiny configurations (D = 128) cannot be built in it
MOVES = [("vitb16", C.VIT_B16, (224, 224), 7, 8, (0, 2, 3, 4)), ("vit_tiny", C.VIT_TINY, (72, 88), 7, 8, (0, 3, 4)),
         ("gated_tiny", C.VIT_TINY_GATED, (64, 64), 7, 8, (0, 3, 4)), ("dinov2reg_tiny", C.DINOV2_REG_TINY, (70, 70), 7, 8, (0, 3, 4)),
         ("dinov2_tiny", C.DINOV2_TINY, (70, 70), 7, 8, (0, 3, 4))]
MOVE_CASES = [(name, cfg, hw, n, mb, p) for (name, cfg, hw, n, mb, ps) in MOVES for p in ps]


@pytest.mark.parametrize("lanes", ("default", "1"))
@pytest.mark.parametrize("name,cfg,hw,n,max_batch,precision", MOVE_CASES, ids=[f"{m[0]}_p{m[5]}" for m in MOVE_CASES])
def test_nothing_else_moves(monkeypatch, name, cfg, hw, n, max_batch, precision, lanes):
    """cls_attention's CLS rows are encode_u8's, f16 and f32, and so are those of a plain call after it.  With the last layer
    unpruned the queries come from row b*T of q|k|v instead of the compact rows: the same GEMM rows, so the same map bits -
    except in precision 2, whose full q|k|v GEMM is MX-fp8 where the compact CLS query is fp16."""
    if lanes == "1":
        monkeypatch.setenv("CBAS_LANES", "1")
    else:
        monkeypatch.delenv("CBAS_LANES", raising=False)
    dev = torch.from_numpy(synth.cage_frames(81, n, *hw)).cuda()
    enc = make_enc(cfg, hw, max_batch, precision)
    try:
        maps, heads = _same_as_encode(enc, dev)
        enc.set_prune_last_layer(False)
        maps2, heads2 = _same_as_encode(enc, dev)
        enc.set_prune_last_layer(True)
        if precision != 2:
            np.testing.assert_array_equal(_bits(heads2), _bits(heads), err_msg=f"{name} p{precision}: unpruned heads")
            np.testing.assert_array_equal(_bits(maps2), _bits(maps), err_msg=f"{name} p{precision}: unpruned map")
    finally:
        enc.close()


@pytest.mark.parametrize("precision", (0, 3, 4))
def test_batch_invariance(precision):
    """A frame's map and heads are the same bits alone, at position 5 of 7 and in a batch of max_batch."""
    for cfg, hw, max_batch in ((C.VIT_B16, (224, 224), 16), (C.VIT_TINY, (72, 88), 16)):
        enc = make_enc(cfg, hw, max_batch, precision)
        try:
            frames = synth.cage_frames(83, max_batch, *hw)
            dev = torch.from_numpy(frames).cuda()
            _, _, m1, h1 = enc.cls_attention(dev[5:6], per_head=True)
            _, _, m7, h7 = enc.cls_attention(dev[:7], per_head=True)
            _, _, mf, hf = enc.cls_attention(dev, per_head=True)
            for m, h in ((m7, h7), (mf, hf)):
                np.testing.assert_array_equal(_bits(m[5]), _bits(m1[0]))
                np.testing.assert_array_equal(_bits(h[5]), _bits(h1[0]))
            # more frames than max_batch: the method walks them in pieces
            more = torch.cat([dev, dev[:3]])
            _, _, mm, _ = enc.cls_attention(more, per_head=True)
            np.testing.assert_array_equal(_bits(mm[:max_batch]), _bits(mf))
            np.testing.assert_array_equal(_bits(mm[max_batch:]), _bits(mf[:3]))
        finally:
            enc.close()


@pytest.mark.parametrize("precision", (3, 4))
def test_ingest_forms_agree(precision):
    for cfg, hw in ((C.VIT_TINY, (72, 88)), (C.DINOV2_REG_TINY, (70, 70))):
        enc = make_enc(cfg, hw, 4, precision)
        try:
            frames = synth.cage_frames(85, 3, *hw)
            u8 = enc.cls_attention(torch.from_numpy(frames).cuda(), per_head=True)
            x = torch.from_numpy(frames[:, :, :, 1] / 255.0).float().cuda().unsqueeze(1)
            f32 = enc.cls_attention(x, per_head=True)
            for a, b in zip(u8, f32):
                np.testing.assert_array_equal(_bits(a), _bits(b))
            planes = enc.cls_attention(torch.from_numpy(np.ascontiguousarray(frames[:, :, :, 1])).cuda(), per_head=True)
            for a, b in zip(u8, planes):
                np.testing.assert_array_equal(_bits(a), _bits(b))
        finally:
            enc.close()


def test_refusals_and_growth():
    from cbas_amd.encoder import DinoEncoder
    cnx = DinoEncoder.from_weights(C.CONVNEXT_TINY, W.synth_convnext_weights(C.CONVNEXT_TINY, ENC_SEED), "cuda", max_batch=2,
                                   max_frame=(64, 64), precision=4)
    try:
        dev = torch.from_numpy(synth.cage_frames(87, 2, 64, 64)).cuda()
        with pytest.raises(ValueError, match="ConvNeXt"):
            cnx.cls_attention(dev)
        out = torch.empty((2, 256), dtype=torch.float32, device="cuda")
        mp = torch.empty((2, 16), dtype=torch.float32, device="cuda")
        lib = cnx._lib
        st = torch.cuda.current_stream().cuda_stream
        assert lib.cbas_enc_forward_u8_attn(cnx._h, dev.data_ptr() + 1, 2, 64, 64, 64 * 64 * 3, 64 * 3, 3, out.data_ptr(), None, st,
                                            None, mp.data_ptr()) == -1
        assert b"ConvNeXt" in lib.cbas_last_error()
        x = torch.zeros((2, 1, 64, 64), dtype=torch.float32, device="cuda")
        assert lib.cbas_enc_forward_f32_attn(cnx._h, x.data_ptr(), 2, 64, 64, out.data_ptr(), None, st, None, mp.data_ptr()) == -1
        assert b"ConvNeXt" in lib.cbas_last_error()
    finally:
        cnx.close()
    enc = make_enc(C.VIT_TINY, (32, 32), 4, 0)
    try:
        lib = enc._lib
        st = torch.cuda.current_stream().cuda_stream
        dev = torch.from_numpy(synth.cage_frames(87, 2, 32, 32)).cuda()
        out = torch.empty((2, 128), dtype=torch.float32, device="cuda")
        assert lib.cbas_enc_forward_u8_attn(enc._h, dev.data_ptr() + 1, 2, 32, 32, 32 * 32 * 3, 32 * 3, 3, out.data_ptr(), None, st,
                                            None, None) == -1
        assert b"both NULL" in lib.cbas_last_error()
        x = torch.zeros((2, 1, 32, 32), dtype=torch.float32, device="cuda")
        assert lib.cbas_enc_forward_f32_attn(enc._h, x.data_ptr(), 2, 32, 32, out.data_ptr(), None, st, None, None) == -1
        assert b"both NULL" in lib.cbas_last_error()
        # a frame larger than the workspace grows it, as encode_u8 does
        big = torch.from_numpy(synth.cage_frames(88, 2, 64, 80)).cuda()
        c16, c32, maps = enc.cls_attention(big)
        assert enc.max_frame == (64, 80) and maps.shape == (2, 4, 5)
        np.testing.assert_array_equal(_bits(enc.encode_u8(big)[1]), _bits(c32))
    finally:
        enc.close()
    # 91 x 91 patches + 5 prefix tokens = 8286 > the 8162 the map kernel's LDS holds at NP = 5: refused before anything is queued
    enc = make_enc(C.VIT_TINY, (1456, 1456), 1, 3)
    try:
        lib = enc._lib
        st = torch.cuda.current_stream().cuda_stream
        dev = torch.from_numpy(np.ascontiguousarray(synth.cage_frames(90, 1, 1456, 1456)[:, :, :, 1])).cuda()
        out = torch.empty((1, 128), dtype=torch.float32, device="cuda")
        mp = torch.full((1, 91 * 91), 7.0, dtype=torch.float32, device="cuda")
        assert lib.cbas_enc_forward_u8_attn(enc._h, dev.data_ptr(), 1, 1456, 1456, 1456 * 1456, 1456, 1, out.data_ptr(), None, st,
                                            None, mp.data_ptr()) == -1
        assert b"8286 tokens" in lib.cbas_last_error()
        with pytest.raises(RuntimeError, match="tokens"):
            enc.cls_attention(dev)
        torch.cuda.synchronize()
        assert bool((mp == 7.0).all())
    finally:
        enc.close()


def test_frame_maps(tmp_path):
    from cbas_amd import attention_maps as A
    frames = synth.cage_frames(89, 40, 64, 64)
    vid = str(tmp_path / "clip.npy")
    np.save(vid, frames)
    enc = make_enc(C.VIT_TINY, (64, 64), 16, 4)
    try:
        idx = list(range(40))
        maps, green = A.frame_maps(enc, vid, idx)
        np.testing.assert_array_equal(green, frames[:, :, :, 1])
        want = enc.cls_attention(torch.from_numpy(frames).cuda())[2].cpu().numpy()
        np.testing.assert_array_equal(maps.view(np.uint32), want.view(np.uint32))
        pick = [33, 2, 17]
        maps2, green2 = A.frame_maps(enc, vid, pick)
        np.testing.assert_array_equal(maps2.view(np.uint32), want[pick].view(np.uint32))
        np.testing.assert_array_equal(green2, frames[pick, :, :, 1])
        with pytest.raises(IndexError):
            A.frame_maps(enc, vid, [40])
    finally:
        enc.close()


def test_compare_encoders_writes_a_figure(tmp_path):
    pytest.importorskip("PIL", reason="compare_encoders renders its maps with Pillow")
    pytest.importorskip("matplotlib", reason="compare_encoders draws its figure with matplotlib")
    from cbas_amd import attention_maps as A
    vid = str(tmp_path / "clip.npy")
    np.save(vid, synth.cage_frames(89, 40, 64, 64))
    enc = make_enc(C.VIT_TINY, (64, 64), 16, 4)
    enc2 = make_enc(C.VIT_TINY_GATED, (64, 64), 16, 0)
    try:
        out = A.compare_encoders(vid, 7, {"tiny (precision 4)": enc, "tiny gated (precision 0)": enc2}, str(tmp_path / "cmp.png"))
        assert os.path.getsize(out) > 0
        assert enc._h is not None and enc2._h is not None          # encoders handed in ready stay open
    finally:
        enc.close(); enc2.close()
