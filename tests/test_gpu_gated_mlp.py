"""Gated-MLP DINOv3 encoders on the GPU: the fused gate | up GEMM (EPI_SWIGLU) one launch at a time against float64 in every
arithmetic and form, the bit identity of the forms, and whole encoders (tiny_gated stage by stage, ViT-S+/16, a one-layer model at
the ViT-H+ width) against transformers' DINOv3ViTModel rows recorded by tests/golden/make_goldens_gated.py."""
import ctypes
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

from cbas_amd import config as C, weights as W, synth

pytestmark = pytest.mark.gpu

CLS_TOL = 1e-3              # precision 0: tests/test_gpu_parity.py's gate
CLS_TOL_F32 = 5e-6          # precisions 3 / 4: tests/test_gpu_fp32.py's gate
ENC_SEED = 1234
U32, U16, F16_SUB = 2.0 ** -24, 2.0 ** -11, 2.0 ** -25
SILU_SLOPE = 1.1            # max |d silu / dx| (1.0998 at x = 2.3994)
# Implementation term of silu(g) * u relative to |y|, from the operations and number formats (not from measurements):
#   precision 3 / 4: expf (<= 1 ulp), 1 + e, the division, the product - each rounded once: 5 u32 suffices, 6 taken
#   precision 0: exp2's argument -g log2(e) is rounded to fp32, which moves exp(-g) by |g| log2(e) ln(2) 2^-24 = |g| u32 relative,
#                then v_exp_f32 and v_rcp_f32 (1 ulp each = 2 u32), the add and two products: (|g| + 8) u32
IMPL = {0: lambda g: (np.abs(g) + 8.0) * U32, 3: lambda g: 6.0 * U32, 4: lambda g: 6.0 * U32}
A_SCALE, W_SCALE, OUT_SCALE = 1.0, 8.0, 4.0      # arith 4: the encoder's own LayerNorm-row and MLP-output scales, a typical weight scale


def rel_rows(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


def _lib():
    from cbas_amd import _lib as L
    L.require_debug("cbas_debug_gemm_swiglu")
    return L.load()


def run_swiglu(arith, tile, forms, A, Wg, Wu, bg, bu, M=None, lda=None):
    """One launch; returns h [M][F] float64 as stored (decoded for arith 4) with canary rows untouched checked by the caller."""
    from oracle import kernel_ref as KR
    lib = _lib()
    M_alloc, K = A.shape[0], Wg.shape[1]
    lda = lda or A.shape[1]
    M = M or M_alloc
    F = Wg.shape[0]
    A = np.ascontiguousarray(A, np.float32)
    out = np.full((M, F), 7.0, np.float16 if arith == 0 else np.float32)
    rc = lib.cbas_debug_gemm_swiglu(arith, tile, forms, M, M_alloc, F, K, lda, A.ctypes.data, Wg.ctypes.data, Wu.ctypes.data,
                                    bg.ctypes.data, bu.ctypes.data, A_SCALE, W_SCALE, OUT_SCALE, out.ctypes.data)
    assert rc == 0, lib.cbas_last_error()
    if arith == 4:
        return KR.decode_split_operand(out, F, OUT_SCALE), out
    return out.astype(np.float64), out


_REF = {}


def swiglu_ref(arith, key, A, Wg, Wu, bg, bu):
    """float64 reference and bound on the operands the kernel multiplies; computed once per (arith, problem)."""
    from oracle import kernel_ref as KR
    if (arith, key) not in _REF:
        ag, Eg, _ = KR.gemm_acc(arith, A, Wg, A_SCALE, W_SCALE)
        au, Eu, _ = KR.gemm_acc(arith, A, Wu, A_SCALE, W_SCALE)
        vg, vu = ag + bg[None, :].astype(np.float64), au + bu[None, :].astype(np.float64)
        with np.errstate(over="ignore"):
            s = vg / (1.0 + np.exp(-vg))
        y = s * vu
        E = SILU_SLOPE * (Eg + U32 * np.abs(vg)) * np.abs(vu) + np.abs(s) * (Eu + U32 * np.abs(vu)) + 2 * U32 * np.abs(y)
        E = E + IMPL[arith](vg) * np.abs(y)
        E = E + KR.out_rounding(y, {0: "f16", 3: "f32", 4: "split"}[arith]) + (F16_SUB / OUT_SCALE if arith == 4 else 0.0)
        _REF[(arith, key)] = (y, E)
    return _REF[(arith, key)]


def problem(F, K, M=300, seed=5, a_std=1.0, w_std=None):
    w_std = w_std or 1.0 / np.sqrt(K)
    A = W.synth_normal(seed, f"A{F}x{K}", (M, K), a_std)
    Wg = W.synth_normal(seed, f"Wg{F}x{K}", (F, K), w_std)
    Wu = W.synth_normal(seed, f"Wu{F}x{K}", (F, K), w_std)
    bg = W.synth_uniform(seed, f"bg{F}", (F,), -0.5, 0.5)
    bu = W.synth_uniform(seed, f"bu{F}", (F,), -0.5, 0.5)
    return A, Wg, Wu, bg, bu


SHAPES = ((128, 128), (384, 192), (640, 1280))
# (arith, tile, forms, row counts): every form api_enc.hip can send the gate | up GEMM to
FORMS = [(0, 1, 0, (37, 129, 257, 300)),      # 16-wave 128 x 128
         (0, 4, 0, (37, 129, 257, 300)),      # 16-wave 256 x 256
         (0, 16, 0, (37, 129, 257, 300)),     # ping-pong, 128-row tiles
         (0, 13, 0, (129, 257, 300)),         # ping-pong, 256-row tiles
         (0, 17, 0, (257, 300)),              # ping-pong planner (256-row tiles + 128-row tail)
         (0, 9, 0, (1, 37)),                  # fp16 skinny
         (0, 0, 0, (1, 37, 300)),             # the planner's own choice
         (3, 0, 0, (1, 37, 129, 257, 300)),   # fp32
         (4, 0, 0, (1, 37, 129, 257, 300)),   # split, 128 x 128 kernels (M <= 256) / 8-wave split kernel
         (4, 0, 1, (257, 300)),               # split ping-pong
         (4, 128, 1, (300,)),                 # split ping-pong, 128-row tiles
         (4, 0, 2, (1, 37, 129))]             # split skinny


PP_TILES = (13, 16, 17)
# the fp16 ping-pong kernel walks K in 128-wide steps; at K = 192 launch_gemm answers a forced ping-pong tile with the 128 x 128
# kernel, which the other rows cover - those combinations are left out, not run under the wrong name.  (384, 256) takes the
# (384, 192) case's place for them: three 256-column tiles again, two K steps.
CASES = [(a, t, f, Ms, F, K) for (a, t, f, Ms) in FORMS for (F, K) in SHAPES if not (a == 0 and t in PP_TILES and K % 128)]
CASES += [(0, t, 0, Ms, 384, 256) for (a, t, f, Ms) in FORMS if a == 0 and t in PP_TILES]


@pytest.mark.parametrize("arith,tile,forms,Ms,F,K", CASES)
def test_swiglu_gemm_against_float64(arith, tile, forms, Ms, F, K):
    from oracle import kernel_ref as KR
    A, Wg, Wu, bg, bu = problem(F, K)
    ref, E = swiglu_ref(arith, (F, K), A, Wg, Wu, bg, bu)
    for M in Ms:
        y, _ = run_swiglu(arith, tile, forms, A[:M], Wg, Wu, bg, bu)
        r = KR.ratio(y, ref[:M], E[:M])
        print(f"[swiglu arith {arith} tile {tile} forms {forms} F {F} K {K} M {M}] ratio {r:.3f}")
        assert r <= 1.0, (M, r)


@pytest.mark.parametrize("arith", (0, 3, 4))
def test_swiglu_strided_cls_rows(arith):
    """lda = T * D: one row per frame, the pruned last layer's CLS rows (skinny forms for arith 0 / 4)."""
    from oracle import kernel_ref as KR
    T, D, F, n = 5, 128, 128, 9
    A, Wg, Wu, bg, bu = problem(F, D, M=n * T, seed=9)
    cls = np.ascontiguousarray(A.reshape(n, T * D)[:, :D])
    ref, E = swiglu_ref(arith, ("cls", F, D), cls, Wg, Wu, bg, bu)
    y, _ = run_swiglu(arith, 0, 2 if arith == 4 else 0, A.reshape(n, T * D), Wg, Wu, bg, bu, lda=T * D)
    assert KR.ratio(y, ref, E) <= 1.0


@pytest.mark.parametrize("arith", (0, 3, 4))
def test_swiglu_large_gate_gives_no_nan(arith):
    """|g| up to 60 (exp(-g) spans 1e-26 .. 1e26) and beyond fp32's exp range through the bias: finite in, finite out."""
    from oracle import kernel_ref as KR
    F, K, M = 128, 128, 37
    A, Wg, Wu, bg, bu = problem(F, K, M=M, seed=13, w_std=4.0 / np.sqrt(K))
    bg = bg.copy()
    bg[:8] = (-200.0, 200.0, -95.0, 95.0, -60.0, 60.0, -88.5, 88.5)
    ref, E = swiglu_ref(arith, ("big", F, K), A, Wg, Wu, bg, bu)
    assert np.abs(ref).max() * OUT_SCALE < 6.0e4
    y, _ = run_swiglu(arith, 0, -1, A, Wg, Wu, bg, bu)
    assert np.isfinite(y).all()
    assert KR.ratio(y, ref, E) <= 1.0


@pytest.mark.parametrize("arith,tile,forms", ((0, 1, 0), (0, 16, 0), (3, 0, 0), (4, 0, 0), (4, 0, 1)))
def test_swiglu_nonfinite_row_stays_in_its_row(arith, tile, forms):
    F, K, M = 128, 128, 300
    A, Wg, Wu, bg, bu = problem(F, K, M=M, seed=17)
    good, _ = run_swiglu(arith, tile, forms, A, Wg, Wu, bg, bu)
    bad = A.copy()
    bad[131, 5] = np.inf
    bad[7, :] = np.nan
    y, _ = run_swiglu(arith, tile, forms, bad, Wg, Wu, bg, bu)
    keep = np.ones(M, bool)
    keep[[7, 131]] = False
    np.testing.assert_array_equal(y[keep], good[keep])
    assert not np.isfinite(y[7]).any() and not np.isfinite(y[131]).all()


def test_swiglu_forms_are_bit_identical():
    F, K = 384, 256
    A, Wg, Wu, bg, bu = problem(F, K, M=300, seed=21)
    base0 = run_swiglu(0, 1, 0, A, Wg, Wu, bg, bu)[1]
    for tile in (4, 13, 16, 17, 0):
        np.testing.assert_array_equal(run_swiglu(0, tile, 0, A, Wg, Wu, bg, bu)[1].view(np.uint16), base0.view(np.uint16), err_msg=f"tile {tile}")
    np.testing.assert_array_equal(run_swiglu(0, 9, 0, A[:37], Wg, Wu, bg, bu)[1].view(np.uint16), base0[:37].view(np.uint16))
    base4 = run_swiglu(4, -1, 0, A, Wg, Wu, bg, bu)[1]
    for tile in (0, 128, 160, 192, 256):
        np.testing.assert_array_equal(run_swiglu(4, tile, 1, A, Wg, Wu, bg, bu)[1].view(np.uint32), base4.view(np.uint32), err_msg=f"split tile {tile}")
    np.testing.assert_array_equal(run_swiglu(4, 0, 2, A[:129], Wg, Wu, bg, bu)[1].view(np.uint32),
                                  run_swiglu(4, 0, 0, A[:129], Wg, Wu, bg, bu)[1].view(np.uint32))
    np.testing.assert_array_equal(run_swiglu(4, 0, 2, A[:129], Wg, Wu, bg, bu)[1].view(np.uint32), base4[:129].view(np.uint32))


def test_swiglu_persistent_ping_pong_matches_the_16_wave_kernel():
    """The ViT-S+ up projection at batch 64 (M = 12 864, K = 384, N = 3072: 612 tiles, more than the CUs, so the ping-pong kernel
    walks tiles persistently) stores the same bits as the 16-wave kernel."""
    F, K, M = 1536, 384, 64 * 201
    A, Wg, Wu, bg, bu = problem(F, K, M=M, seed=23)
    a = run_swiglu(0, 17, 0, A, Wg, Wu, bg, bu)[1]
    b = run_swiglu(0, 4, 0, A, Wg, Wu, bg, bu)[1]
    np.testing.assert_array_equal(a.view(np.uint16), b.view(np.uint16))


# ---- whole encoders ---------------------------------------------------------------------------------------------------------
def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def make_enc(cfg, hw, max_batch, precision):
    from cbas_amd.encoder import DinoEncoder
    return DinoEncoder.from_weights(cfg, W.synth_encoder_weights(cfg, ENC_SEED), "cuda", max_batch=max_batch, max_frame=hw,
                                    precision=precision)


def _tol(precision):
    return CLS_TOL if precision == 0 else CLS_TOL_F32


def split_tap(enc, dev, layer, T):
    """Precision 4: the buffer after the up GEMM of `layer`, read raw and decoded from the split image (one K-tile of the down
    projection per 32 columns, values x 4) -> float64 (n T, F)."""
    from cbas_amd import _lib as L
    from oracle import kernel_ref as KR
    L.require_debug("cbas_enc_debug_forward_u8")
    n, H, Wd, Cn = dev.shape
    F = enc.config.intermediate_size
    torch.cuda.synchronize()
    L.check(enc._lib.cbas_enc_debug_forward_u8(enc._h, dev.data_ptr() + 1, n, H, Wd, H * Wd * Cn, Wd * Cn, Cn, layer, 6),
            "cbas_enc_debug_forward_u8")
    raw = np.empty((n * T, F), np.float32)
    L.check(enc._lib.cbas_enc_debug_read(enc._h, 3, raw.ctypes.data, raw.nbytes), "cbas_enc_debug_read")
    return KR.decode_split_operand(raw, F, 4.0)


@pytest.mark.parametrize("precision", (0, 3, 4))
def test_tiny_gated_stagewise_and_cls(golden_dir, precision):
    g = load(golden_dir, "gated_tiny")
    cfg = C.VIT_TINY_GATED
    enc = make_enc(cfg, (64, 80), 16, precision)
    try:
        mlp = ctypes.c_int32(-1)
        assert enc._lib.cbas_enc_get_mlp(enc._h, ctypes.byref(mlp)) == 0 and mlp.value == 1
        for tag in ("a", "b"):
            H, Wd, seed = int(g[f"{tag}_height"]), int(g[f"{tag}_width"]), int(g[f"{tag}_seed"])
            frames = synth.cage_frames(seed, 2, H, Wd)
            dev = torch.from_numpy(frames).cuda()
            T = cfg.num_tokens(H, Wd)
            for l in range(cfg.num_hidden_layers):
                # the up GEMM's output; precision 4 stores it as the down projection's split hi | lo image (scale 4)
                act = (split_tap(enc, dev, l, T) if precision == 4 else enc.debug_tap(dev, l, 6, 3).astype(np.float64)).reshape(2, T, -1)
                ref = g[f"{tag}_act{l}"].astype(np.float64)
                err = np.abs(act - ref).max() / np.abs(ref).max()
                print(f"[tiny_gated p{precision} {tag} layer {l}] silu(gate) * up: max err / max |ref| {err:.2e}")
                assert err < (2e-3 if precision == 0 else 2e-6)
                x = enc.debug_tap(dev, l, 7, 0).reshape(2, T, -1)
                r = rel_rows(x.reshape(2 * T, -1), g[f"{tag}_layer{l}"].reshape(2 * T, -1))
                print(f"[tiny_gated p{precision} {tag} layer {l}] residual stream rel {r.max():.2e}")
                assert r.max() < _tol(precision)
            ref = g[f"{tag}_cls"]
            c16, c32 = enc.encode_u8(dev)
            r1 = rel_rows(c32.cpu().numpy(), ref)
            print(f"[tiny_gated p{precision} {tag}] CLS rel {r1.max():.2e}")
            assert r1.max() < _tol(precision)
            # batches of 1, 3 and 13 (13 x 21 = 273 rows: the ping-pong kernels with a 128-row tail): a frame's row is its own
            one = enc.encode_u8(dev[:1])[1].cpu().numpy()
            np.testing.assert_array_equal(one[0], c32.cpu().numpy()[0])
            for nb in (3, 13):
                rep = dev[[i % 2 for i in range(nb)]].contiguous()
                out = enc.encode_u8(rep)[1].cpu().numpy()
                for i in range(nb):
                    np.testing.assert_array_equal(out[i], c32.cpu().numpy()[i % 2], err_msg=f"batch {nb} row {i}")
            # forward_f32 on green / 255 agrees with forward_u8; the full last layer gives the pruned one's bits
            x = torch.from_numpy(frames[:, :, :, 1] / 255.0).float().cuda().unsqueeze(1)
            f32 = enc(x).squeeze(1).cpu().numpy()
            assert rel_rows(f32, ref).max() < _tol(precision)
            if precision >= 3:              # the fp32 modes read the same green / 255 either way (tests/test_gpu_fp32.py)
                np.testing.assert_array_equal(f32, c32.cpu().numpy())
            # the slot API, from the host and from the device, gives forward_u8's bits
            enc.submit_host(0, frames)
            o16 = torch.empty((2, cfg.hidden_size), dtype=torch.float16, device="cuda")
            o32 = torch.empty((2, cfg.hidden_size), dtype=torch.float32, device="cuda")
            enc.submit_dev(1, dev, o16, o32)
            h16, h32 = enc.wait(0, want_f32=True)
            enc.wait_stream(1)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(h32, c32.cpu().numpy())
            np.testing.assert_array_equal(h16, c16.cpu().numpy())
            assert torch.equal(o32, c32) and torch.equal(o16, c16)
            assert enc._lib.cbas_enc_set_prune_last_layer(enc._h, 0) == 0
            full = enc.encode_u8(dev)[1].cpu().numpy()
            assert enc._lib.cbas_enc_set_prune_last_layer(enc._h, 1) == 0
            np.testing.assert_array_equal(full, c32.cpu().numpy())
    finally:
        enc.close()


@pytest.mark.parametrize("precision", (0, 3, 4))
def test_vits16plus_cls(golden_dir, precision):
    g = load(golden_dir, "gated_vits16plus")
    enc = make_enc(C.VIT_S16PLUS, (224, 224), 2, precision)
    try:
        frames = synth.cage_frames(int(g["frame_seed"]), int(g["n"]), 224, 224)
        c32 = enc.encode_u8(torch.from_numpy(frames).cuda())[1].cpu().numpy()
        r = rel_rows(c32, g["cls"])
        print(f"[vits16plus p{precision}] CLS rel {r.max():.2e}")
        assert r.max() < _tol(precision)
    finally:
        enc.close()


@pytest.mark.parametrize("precision", (0, 3, 4))
def test_width_1280_cls(golden_dir, precision):
    g = load(golden_dir, "gated_w1280")
    cfg = replace(C.VIT_H16PLUS, num_hidden_layers=1, image_size=32)
    enc = make_enc(cfg, (32, 32), 2, precision)
    try:
        frames = synth.cage_frames(int(g["frame_seed"]), int(g["n"]), 32, 32)
        c32 = enc.encode_u8(torch.from_numpy(frames).cuda())[1].cpu().numpy()
        r = rel_rows(c32, g["cls"])
        print(f"[w1280 p{precision}] CLS rel {r.max():.2e}")
        assert r.max() < _tol(precision)
    finally:
        enc.close()


def test_width_1280_gelu_handle_layernorm():
    """mlp = 0 at D = 1280 (the new LayerNorm instantiation for non-gated callers): the LayerNorm-1 tap of a precision-3 handle and
    the final norm of its CLS rows against float64 restatements on the handle's own residual stream."""
    cfg = C.ViTConfig(hidden_size=1280, intermediate_size=1280, num_hidden_layers=1, num_attention_heads=20, image_size=32)
    w = W.synth_encoder_weights(cfg, ENC_SEED)
    from cbas_amd.encoder import DinoEncoder
    enc = DinoEncoder.from_weights(cfg, w, "cuda", max_batch=2, max_frame=(32, 32), precision=3)
    try:
        dev = torch.from_numpy(synth.cage_frames(3, 2, 32, 32)).cuda()

        def ln(x, gw, gb):
            x = x.astype(np.float64)
            mu = x.mean(-1, keepdims=True)
            var = ((x - mu) ** 2).mean(-1, keepdims=True)
            return (x - mu) / np.sqrt(var + cfg.layer_norm_eps) * gw.astype(np.float64) + gb.astype(np.float64)

        x0 = enc.debug_tap(dev, 0, 0, 0)
        h1 = enc.debug_tap(dev, 0, 1, 1)
        ref = ln(x0, w["model.layer.0.norm1.weight"], w["model.layer.0.norm1.bias"])
        assert np.abs(h1 - ref).max() <= 8 * U32 * np.abs(ref).max()
        assert enc._lib.cbas_enc_set_prune_last_layer(enc._h, 0) == 0
        x1 = enc.debug_tap(dev, 0, 7, 0)
        c32 = enc.encode_u8(dev)[1].cpu().numpy()
        T = cfg.num_tokens(32, 32)
        ref = ln(x1.reshape(2, T, -1)[:, 0], w["norm.weight"], w["norm.bias"])
        assert np.abs(c32 - ref).max() <= 8 * U32 * np.abs(ref).max()
    finally:
        enc.close()


def test_lifecycle_refusals_and_gelu_create_unchanged(golden_dir):
    from cbas_amd import _lib as L
    from cbas_amd.encoder import DinoEncoder, pack_encoder_weights
    lib = L.load()
    cfg = C.VIT_TINY_GATED
    blob = pack_encoder_weights(cfg, W.synth_encoder_weights(cfg, ENC_SEED))

    def cc(c, precision):
        return L.EncConfig(c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads, c.num_register_tokens,
                           c.patch_size, c.layer_norm_eps, c.rope_theta, 4, 64, 64, precision, 1, 0)

    for precision, mlp in ((2, 1), (1, 1), (0, 2)):
        h = ctypes.c_void_p()
        rc = lib.cbas_enc_create_mlp(ctypes.byref(cc(cfg, precision)), mlp, blob.ctypes.data, blob.shape[0], 0, ctypes.byref(h))
        assert rc == -1                                                     # CBAS_EINVAL
        assert not h.value and lib.cbas_last_error()
    # _fit_frame and range_fallback keep the kind
    enc = make_enc(cfg, (32, 32), 4, 4)
    try:
        frames = torch.from_numpy(synth.cage_frames(61, 2, 64, 64)).cuda()
        c32 = enc.encode_u8(frames)[1].cpu().numpy()                      # rebuilds the handle for 64 x 64
        g = load(golden_dir, "gated_tiny")
        assert rel_rows(c32, g["a_cls"]).max() < CLS_TOL_F32
        mlp = ctypes.c_int32(-1)
        assert lib.cbas_enc_get_mlp(enc._h, ctypes.byref(mlp)) == 0 and mlp.value == 1
        twin = enc.range_fallback()
        assert lib.cbas_enc_get_mlp(twin._h, ctypes.byref(mlp)) == 0 and mlp.value == 1 and twin.precision == 3
        assert rel_rows(twin.encode_u8(frames)[1].cpu().numpy(), g["a_cls"]).max() < CLS_TOL_F32
    finally:
        enc.close()
    # a GELU model through both create calls: the same bits
    gv = load(golden_dir, "vit_tiny")
    tcfg = C.VIT_TINY
    tw = W.synth_encoder_weights(tcfg, ENC_SEED)
    a = DinoEncoder.from_weights(tcfg, tw, "cuda", max_batch=4, max_frame=(64, 64), precision=0)
    try:
        fr = torch.from_numpy(synth.cage_frames(7, 2, 64, 64)).cuda()       # the first frames of tests/golden/vit_tiny.npz
        ra = a.encode_u8(fr)[1].cpu().numpy()
        tb = pack_encoder_weights(tcfg, tw)
        h = ctypes.c_void_p()
        assert lib.cbas_enc_create(ctypes.byref(cc(tcfg, 0)), tb.ctypes.data, tb.shape[0], 0, ctypes.byref(h)) == 0
        out = torch.empty((2, tcfg.hidden_size), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert lib.cbas_enc_forward_u8(h, fr.data_ptr() + 1, 2, 64, 64, 64 * 64 * 3, 64 * 3, 3, out.data_ptr(), None,
                                       torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        mlp = ctypes.c_int32(-1)
        assert lib.cbas_enc_get_mlp(h, ctypes.byref(mlp)) == 0 and mlp.value == 0
        lib.cbas_enc_destroy(h)
        np.testing.assert_array_equal(out.cpu().numpy(), ra)
        assert rel_rows(ra, gv["last_hidden"][:2, 0]).max() < CLS_TOL         # and they are the recorded rows
    finally:
        a.close()


def _overflowing_weights(cfg):
    """|silu(gate) * up| x 4 beyond fp16's range in one column of the down projection's input, the way tests/test_gpu_fp32.py
    forces it for GELU: silu(~4) x 40 000 x 4 > 65 504, while the fp32 result stays moderate."""
    w = {k: v.copy() for k, v in W.synth_encoder_weights(cfg, ENC_SEED).items()}
    w["model.layer.0.mlp.gate_proj.bias"][3] = 4.0
    w["model.layer.0.mlp.gate_proj.weight"][3] = 0.0
    w["model.layer.0.mlp.up_proj.bias"][3] = 40000.0
    w["model.layer.0.mlp.down_proj.weight"][:, 3] *= 1e-4
    return w


def _rows(path):
    from cbas_amd import h5io
    with h5io.ClsReader(path) as r:
        return r.read(0, r.shape[0])


def test_precision4_overflow_is_erange_and_the_file_path_gives_the_precision3_rows(tmp_path, capsys):
    """A precision-4 gated handle whose activations leave the range answers CBAS_ERANGE; encode_file then re-encodes the clip
    through the twin, and the rows it writes are, bit for bit, the rows a separately built precision-3 gated encoder writes - which
    are the float64 restatement's (tests/gated_ref.py) to the fp32 gate before the fp16 store."""
    from cbas_amd import pipeline as P
    from cbas_amd.encoder import DinoEncoder
    import gated_ref as G
    cfg = C.VIT_TINY_GATED
    w = _overflowing_weights(cfg)
    frames = synth.cage_frames(61, 40, 64, 64)
    ref = G.forward(frames, w, cfg)[:, 0]
    assert np.isfinite(ref).all()
    for sub in ("a", "b"):
        (tmp_path / sub).mkdir()
        np.save(str(tmp_path / sub / "vid.npy"), frames)
    enc = DinoEncoder.from_weights(cfg, w, "cuda", max_batch=16, max_frame=(64, 64), precision=4)
    enc3 = DinoEncoder.from_weights(cfg, w, "cuda", max_batch=16, max_frame=(64, 64), precision=3)
    try:
        enc.submit_host(0, frames[:8])
        with pytest.raises(RuntimeError, match="non-finite CLS row.*precision 4"):
            enc.wait(0, want_f32=True)
        out = P.encode_file(enc, str(tmp_path / "a" / "vid.npy"))
        assert "re-encoded in precision 3" in capsys.readouterr().out
        got = _rows(out)
        want = _rows(P.encode_file(enc3, str(tmp_path / "b" / "vid.npy")))
        assert "re-encoded" not in capsys.readouterr().out
        assert got.shape == (40, cfg.hidden_size) and got.dtype == np.float16
        np.testing.assert_array_equal(got.view(np.uint16), want.view(np.uint16))
        c32 = enc3.encode_u8(torch.from_numpy(frames).cuda())[1].cpu().numpy()
        r = rel_rows(c32, ref)
        print(f"[tiny_gated overflow] precision-3 rows against the float64 restatement: rel {r.max():.2e}")
        assert r.max() < CLS_TOL_F32
        np.testing.assert_array_equal(got.view(np.uint16), c32.astype(np.float16).view(np.uint16))
        mlp = ctypes.c_int32(-1)
        twin = enc.range_fallback()
        assert enc._lib.cbas_enc_get_mlp(twin._h, ctypes.byref(mlp)) == 0 and mlp.value == 1 and twin.precision == 3
    finally:
        enc.close(); enc3.close()


def test_encode_file_writes_forward_rounded_to_fp16_from_a_checkpoint_directory(tmp_path):
    """A tiny_gated checkpoint directory written by save_encoder_checkpoint loads through DinoEncoder(path) (the reference's
    constructor form, precision 4 by default) and encode_file on a 40-frame .npy clip writes DinoEncoder.forward's rows rounded
    to fp16."""
    from cbas_amd import pipeline as P
    from cbas_amd.encoder import DinoEncoder
    cfg = C.VIT_TINY_GATED
    ck = str(tmp_path / "ckpt")
    W.save_encoder_checkpoint(ck, cfg, W.synth_encoder_weights(cfg, ENC_SEED))
    enc = DinoEncoder(ck, device="cuda", max_batch=16, max_frame=(64, 64))
    try:
        assert enc.config == cfg and enc.precision == 4
        mlp = ctypes.c_int32(-1)
        assert enc._lib.cbas_enc_get_mlp(enc._h, ctypes.byref(mlp)) == 0 and mlp.value == 1
        frames = synth.cage_frames(61, 40, 64, 64)
        np.save(str(tmp_path / "vid.npy"), frames)
        out = P.encode_file(enc, str(tmp_path / "vid.npy"))
        assert out == str(tmp_path / "vid_cls.h5")
        got = _rows(out)
        x = torch.from_numpy(frames[:, :, :, 1] / 255.0).float().cuda().unsqueeze(0)       # (1, 40, H, W), as cbas.py feeds it
        fwd = enc(x).squeeze(0)
        np.testing.assert_array_equal(got.view(np.uint16), fwd.half().cpu().numpy().view(np.uint16))
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gated_tiny.npz"))
        assert rel_rows(fwd[:2].cpu().numpy(), g["a_cls"]).max() < CLS_TOL_F32              # the fixture's two frames lead the clip
    finally:
        enc.close()


def test_swiglu_split_weight_scale_with_unequal_gate_and_up_magnitudes():
    """Precision 4 scales the fused gate | up weight by ONE power of two, taken from the larger of the two maxima.  With
    |W_up| = 64 |W_gate| the gate rows sit 6 bits lower in their fp16 halves; hi + lo still carries 22 bits, so the launch stays
    inside the float64 bound computed on the operands as split."""
    from oracle import kernel_ref as KR
    F, K, M = 128, 128, 129
    A, Wg, Wu, bg, bu = problem(F, K, M=M, seed=29)
    Wg, Wu = (Wg / 8.0).astype(np.float32), (Wu * 8.0).astype(np.float32)
    ref, E = swiglu_ref(4, ("ratio64", F, K), A, Wg, Wu, bg, bu)
    for forms in (0, 2):
        y, _ = run_swiglu(4, 0, forms, A, Wg, Wu, bg, bu)
        r = KR.ratio(y, ref, E)
        print(f"[swiglu arith 4 forms {forms}, |Wu| = 64 |Wg|] ratio {r:.3f}")
        assert r <= 1.0
