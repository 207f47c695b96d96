"""Per-layer hidden states, per-layer CLS attention and attention rollout on the GPU: the two kernels of attention_rollout.hip one
launch at a time against float64, then DinoEncoder.hidden_states / cls_attention(layer=) / attention_rollout against rows recorded
from transformers' own models (tests/golden/make_goldens_layers.py), and the promises around them.

Bar of the head-mean attention kernel (u = 2^-24; everything is fp32): the bar tests/test_gpu_cls_attention.py derives for the CLS
kernel, row by row - the score bound gamma_64 sum |q_j k_j| holds for any summation order (here ONE 64-term fmaf chain), the
split operands of arith 4 add the same terms - with the one difference of this kernel's softmax sum: a wave per query row, so a
term passes through at most d = ceil(T / 64) + 6 additions (a lane's chain, one 6-level tree) instead of ceil(T / 1024) + 12:
    |p^ - p| <= p (expm1(2 E) + (6 + d) u),      mean over heads: mean_h(bar_h) + (NH + 2) u mean_h(p).
Bar of the chain step: every entry is a length-T fmaf chain of non-negative terms whose exact sum is at most the row sum 1 of a
row-stochastic product: T u.  The largest error / bar of each test is printed (run with -s)."""
import ctypes as C_
import math
import os

import numpy as np
import pytest
import torch

from cbas_amd import config as C, weights as W, synth, _lib as L_
from cbas_amd.encoder import token_grid

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ENC_SEED = 1234
TOL_F16, TOL_F32 = 1e-3, 5e-6                 # per-row ||d|| / ||ref||: tests/test_gpu_hidden_state.py
MAP_TOL_F16, MAP_TOL_F32 = 5e-3, 2e-5         # max |d| / max |ref|: tests/test_gpu_cls_attention.py
# rollout, max |d| / max |ref|: the smaller of L x MAP_TOL (row-stochastic products are non-expansive: at most the sum of the
# per-layer errors) and 4 x the largest value measured over every fixture on an MI355X - 2.70e-4 in precision 0 (ViT-B/16 at 224^2;
# the tiny fixtures 0.9e-4 .. 1.1e-4) and 1.01e-6 in precisions 3 / 4 (ViT-B/16; tiny 2.3e-7 .. 3.6e-7)
ROLL_GATE_F16, ROLL_GATE_F32 = 1.1e-3, 4.1e-6
TINY = {"vit_tiny": C.VIT_TINY, "gated_tiny": C.VIT_TINY_GATED, "dinov2reg_tiny": C.DINOV2_REG_TINY, "dinov2_tiny": C.DINOV2_TINY}
_WEIGHTS = {}


def lib():
    L_.require_debug("cbas_debug_attention_mean")
    return L_.load()


def gamma(n):
    return n * U / (1.0 - n * U)


def bits(a):
    a = a.detach().contiguous().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- a. the head-mean attention kernel against float64 --------------------------------------------------------------------------
MEAN_CASES = [(2, 25, 2), (2, 65, 1), (2, 201, 12), (2, 261, 6), (1, 1029, 1)]      # (n, T, NH); NP does not enter this kernel
_OPS, _REF = {}, {}


def operands(case, fp16, equal=False):
    k = (case, fp16, equal)
    if k not in _OPS:
        n, T, NH = case
        D = 64 * NH
        q = W.synth_normal(191, f"q{case}", (n * T, D), 1.0)
        K = W.synth_normal(192, f"K{case}", (n * T, D), 0.75)
        if equal:
            K = np.repeat(K.reshape(n, T, D)[:, :1], T, axis=1).reshape(n * T, D)
        if fp16:
            q, K = q.astype(np.float16).astype(np.float32), K.astype(np.float16).astype(np.float32)
        _OPS[k] = (np.ascontiguousarray(q), np.ascontiguousarray(K))
    return _OPS[k]


def reference(arith, case, q, K, key):
    k = (arith == 4, key, case)
    if k in _REF:
        return _REF[k]
    n, T, NH = case
    qh = q.astype(np.float64).reshape(n, T, NH, 64).transpose(0, 2, 1, 3)       # (n, NH, T, 64)
    kh = K.astype(np.float64).reshape(n, T, NH, 64).transpose(0, 2, 1, 3)
    s = qh @ kh.transpose(0, 1, 3, 2)                                           # (n, NH, Tq, Tk)
    aq, ak = np.abs(qh), np.abs(kh)
    Es = gamma(64) * (aq @ ak.transpose(0, 1, 3, 2))
    if arith == 4:
        dq = ((2.0 ** -22 + 2.0 ** -24) * aq * 16.0 + 2.0 ** -25) / 16.0
        dk = ((2.0 ** -22 + 2.0 ** -24) * ak * 4.0 + 2.0 ** -25) / 4.0
        Es = Es + aq @ dk.transpose(0, 1, 3, 2) + dq @ ak.transpose(0, 1, 3, 2) + dq @ dk.transpose(0, 1, 3, 2)
    m = s.max(-1, keepdims=True)
    E = (Es + U * np.abs(s - m)).max(-1, keepdims=True)
    e = np.exp(s - m)
    p = e / e.sum(-1, keepdims=True)
    d = math.ceil(T / 64) + 6
    bar = p * (np.expm1(2.0 * E) + (6 + d) * U)
    mp = p.mean(1)
    _REF[k] = (mp, bar.mean(1) + (NH + 2) * U * mp, float(np.abs(s).max()))
    return _REF[k]


def run_mean(arith, case, q, K, blend=0):
    n, T, NH = case
    out = np.full((n, T, T), 7.0, np.float32)
    rc = lib().cbas_debug_attention_mean(arith, q.ctypes.data, K.ctypes.data, n, T, NH, q.shape[1], K.shape[1], blend, out.ctypes.data)
    assert rc == 0, lib().cbas_last_error()
    return out


@pytest.mark.parametrize("arith", (0, 3, 4))
@pytest.mark.parametrize("case", MEAN_CASES, ids=lambda c: "n%d_T%d_NH%d" % c)
def test_mean_kernel_against_float64(arith, case):
    n, T, NH = case
    q, K = operands(case, arith == 0)
    mp, mbar, smax = reference(arith, case, q, K, ("rand", arith == 0))
    got = run_mean(arith, case, q, K)
    r = float((np.abs(got.astype(np.float64) - mp) / mbar).max())
    dev = float(np.abs(got.astype(np.float64).sum(-1) - 1.0).max())
    print(f"[attention mean arith {arith} case {case}] max |s| {smax:.1f}; error / bound {r:.3f}; row sums off by {dev:.2e} (bound {T * float(mbar.max()):.2e})")
    assert smax >= 15.0 and np.isfinite(got).all() and r <= 1.0
    assert dev <= T * float(mbar.max())


@pytest.mark.parametrize("arith", (0, 3, 4))
def test_mean_kernel_equal_scores_and_blend(arith):
    case = (2, 65, 2)
    q, K = operands(case, arith == 0, equal=True)
    got = run_mean(arith, case, q, K)
    # exact: every e is 1, the sum is 65, p = fl(1 / 65) for each head; NH = 2 is a power of two, so p + p and x (1 / NH) round nothing
    assert same(got, np.full_like(got, np.float32(1.0) / np.float32(65)))
    q, K = operands(case, arith == 0)
    a, b = run_mean(arith, case, q, K), run_mean(arith, case, q, K, blend=1)
    assert same(b, np.float32(0.5) * a + np.float32(0.5) * np.eye(65, dtype=np.float32)[None])


@pytest.mark.parametrize("arith", (0, 3, 4))
def test_mean_kernel_nonfinite_row_stays_in_its_rows(arith):
    case = (2, 201, 12)
    n, T, NH = case
    q, K = operands(case, arith == 0)
    good = run_mean(arith, case, q, K)
    bad = q.copy()
    bad[1 * T + 77, :] = np.nan
    got = run_mean(arith, case, bad, K)
    assert same(got[0], good[0])
    keep = np.arange(T) != 77
    assert same(got[1][keep], good[1][keep]) and not np.isfinite(got[1][77]).any()


# ---- b. the chain step against float64 --------------------------------------------------------------------------------------------
def stochastic(seed, tag, n, T):
    a = np.abs(W.synth_normal(seed, tag, (n, T, T), 1.0)).astype(np.float64) ** 3 + 1e-3
    return np.ascontiguousarray((a / a.sum(-1, keepdims=True)).astype(np.float32))


@pytest.mark.parametrize("T", (25, 201, 261))
def test_rollout_step_against_float64(T):
    n = 2
    A, R = stochastic(193, f"A{T}", n, T), stochastic(194, f"R{T}", n, T)
    out = np.full((n, T, T), 7.0, np.float32)
    assert lib().cbas_debug_rollout_step(A.ctypes.data, R.ctypes.data, n, T, out.ctypes.data) == 0, lib().cbas_last_error()
    ref = A.astype(np.float64) @ R.astype(np.float64)
    bar = T * U * ref.sum(-1, keepdims=True)
    r = float((np.abs(out.astype(np.float64) - ref) / bar).max())
    print(f"[rollout step T {T}] error / bound {r:.3f}")
    assert r <= 1.0
    again = np.empty_like(out)
    assert lib().cbas_debug_rollout_step(A.ctypes.data, R.ctypes.data, n, T, again.ctypes.data) == 0 and same(out, again)


def test_debug_entry_refusals():
    l = lib()
    q = np.zeros((4, 64), np.float32)
    out = np.full((1, 4, 4), 7.0, np.float32)
    ok = [3, q.ctypes.data, q.ctypes.data, 1, 4, 1, 64, 64, 0, out.ctypes.data]
    assert l.cbas_debug_attention_mean(*ok) == 0 and np.abs(out - 0.25).max() < 1e-6
    out[:] = 7.0
    for i, v in ((0, 1), (1, None), (2, None), (9, None), (3, 0), (4, 0), (5, 0), (6, 60), (7, 60), (6, 32), (4, 8200)):
        bad = list(ok)
        bad[i] = v
        assert l.cbas_debug_attention_mean(*bad) == -1 and l.cbas_last_error(), (i, v)      # T = 8200: one row does not fit LDS
    assert (out == 7.0).all()
    A = np.eye(4, dtype=np.float32)[None].copy()
    assert l.cbas_debug_rollout_step(A.ctypes.data, A.ctypes.data, 1, 4, out.ctypes.data) == 0 and same(out, A)
    out[:] = 7.0
    for bad in ((None, A.ctypes.data, 1, 4, out.ctypes.data), (A.ctypes.data, None, 1, 4, out.ctypes.data), (A.ctypes.data, A.ctypes.data, 0, 4, out.ctypes.data),
                (A.ctypes.data, A.ctypes.data, 1, 0, out.ctypes.data), (A.ctypes.data, A.ctypes.data, 1, 4, None)):
        assert l.cbas_debug_rollout_step(*bad) == -1 and l.cbas_last_error(), bad
    assert (out == 7.0).all()


# ---- c. the encoder ---------------------------------------------------------------------------------------------------------------
def make_enc(cfg, hw, max_batch, precision):
    from cbas_amd.encoder import DinoEncoder
    if cfg not in _WEIGHTS:
        _WEIGHTS[cfg] = (W.synth_convnext_weights if C.is_convnext(cfg) else W.synth_encoder_weights)(cfg, ENC_SEED)
    return DinoEncoder.from_weights(cfg, _WEIGHTS[cfg], "cuda", max_batch=max_batch, max_frame=hw, precision=precision)


def rel_rows(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float((np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)).max())


def rel_max(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(np.asarray(b, np.float64)).max())


def ln64(x, w, b, eps):
    x = np.asarray(x, np.float64)
    c = x - x.mean(-1, keepdims=True)
    return c / np.sqrt((c * c).mean(-1, keepdims=True) + eps) * w.astype(np.float64) + b.astype(np.float64)


def fixture(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "encoder_layers.npz"))
    n, H, Wd, seed = (int(g[f"{name}_{k}"]) for k in ("n", "height", "width", "seed"))
    return g, n, H, Wd, torch.from_numpy(synth.cage_frames(seed, n, H, Wd)).cuda()


GOLDEN_CASES = [(name, p) for name in TINY for p in (0, 3, 4)] + [("vitb16", 0), ("vitb16", 4)]


@pytest.mark.parametrize("name,precision", GOLDEN_CASES, ids=[f"{n}_p{p}" for n, p in GOLDEN_CASES])
def test_encoder_against_goldens(golden_dir, name, precision):
    """Hidden states raw and normed, per-layer CLS heads and maps, rollout.  Measured on an MI355X: see DESIGN.md section 17."""
    cfg = TINY.get(name, C.VIT_B16)
    g, n, H, Wd, dev = fixture(golden_dir, name)
    Lc, NP = cfg.num_hidden_layers, cfg.num_prefix_tokens
    nh, nw, _ = token_grid(cfg, H, Wd)
    rows, lay, ref = g[f"{name}_rows"], [int(v) for v in g[f"{name}_hs_layers"]], g[f"{name}_hidden"]
    wts = dict(W.canonical_encoder_weights(cfg, _WEIGHTS.get(cfg) or W.synth_encoder_weights(cfg, ENC_SEED)))
    tol, mtol = (TOL_F16, MAP_TOL_F16) if precision == 0 else (TOL_F32, MAP_TOL_F32)
    enc = make_enc(cfg, (H, Wd), 4, precision)
    try:
        raw = enc.hidden_states(dev, layers=lay).cpu().numpy()
        nrm = enc.hidden_states(dev, layers=lay, norm=True).cpu().numpy()
        assert raw.shape == (len(lay), n, NP + nh * nw, cfg.hidden_size)
        e_raw = [rel_rows(raw[j][:, rows], ref[j]) for j in range(len(lay))]
        e_nrm = [rel_rows(nrm[j][:, rows], ln64(ref[j], wts["norm.weight"], wts["norm.bias"], cfg.layer_norm_eps)) for j in range(len(lay))]
        print(f"[layers {name} p{precision}] hidden per-row rel by layer {lay}: raw {['%.2e' % e for e in e_raw]}, normed {['%.2e' % e for e in e_nrm]}")
        _, _, maps, heads = enc.cls_attention(dev, per_head=True, layer="all")
        assert maps.shape == (n, Lc, nh, nw) and heads.shape == (n, Lc, cfg.num_attention_heads, NP + nh * nw)
        e_map = [rel_max(maps[:, l].reshape(n, -1).cpu().numpy(), g[f"{name}_cls_map"][l]) for l in range(Lc)]
        print(f"[layers {name} p{precision}] CLS map max|d|/max|ref| by layer: {['%.2e' % e for e in e_map]}")
        e_heads = []
        if f"{name}_cls_heads" in g:
            e_heads = [rel_max(heads[:, l].cpu().numpy(), g[f"{name}_cls_heads"][l]) for l in range(Lc)]
            print(f"[layers {name} p{precision}] CLS heads by layer: {['%.2e' % e for e in e_heads]}")
        roll = enc.attention_rollout(dev)
        assert roll.shape == (n, nh, nw) and roll.dtype == torch.float32
        e_roll = [rel_max(roll.reshape(n, -1).cpu().numpy(), g[f"{name}_rollout_cls"])]
        if f"{name}_rollout_patch" in g:
            rp = enc.attention_rollout(dev, query=tuple(int(v) for v in g[f"{name}_patch_pixel"]))
            e_roll.append(rel_max(rp.reshape(n, -1).cpu().numpy(), g[f"{name}_rollout_patch"]))
        gate = min(Lc * mtol, ROLL_GATE_F16 if precision == 0 else ROLL_GATE_F32)
        print(f"[layers {name} p{precision}] rollout max|d|/max|ref| (CLS, patch query): {['%.2e' % e for e in e_roll]}; gate {gate:.1e}")
        enc.check_finite()
        assert max(e_raw) < tol and max(e_nrm) < tol
        assert max(e_map + e_heads) < mtol
        assert max(e_roll) < gate
    finally:
        enc.close()


@pytest.mark.parametrize("name,precision", [("vit_tiny", 0), ("vit_tiny", 4), ("vitb16", 0), ("vitb16", 4)])
def test_bit_identities(golden_dir, name, precision):
    cfg = TINY.get(name, C.VIT_B16)
    g, n, H, Wd, dev = fixture(golden_dir, name)
    Lc = cfg.num_hidden_layers
    enc = make_enc(cfg, (H, Wd), 16, precision)
    try:
        allh = enc.hidden_states(dev)
        assert allh.shape[0] == Lc + 1
        assert same(enc.hidden_states(dev, layers=[Lc], norm=True)[0], enc.hidden_state(dev))
        assert same(enc.hidden_states(dev, layers=[-1], norm=True, dtype=torch.float16)[0], enc.hidden_state(dev, dtype=torch.float16))
        assert same(enc.hidden_states(dev, layers=[0, 1]), allh[:2]) and same(enc.hidden_states(dev, layers=[1, 0]), allh[[1, 0]])
        assert same(enc.hidden_states(dev, dtype=torch.float16), allh.half())                      # fp16 = RNE(fp32)
        assert same(enc.hidden_states(dev), allh)                                                  # two calls agree
        p_old, x_old = enc.patch_tokens(dev)
        hs = enc.hidden_state(dev)
        P0 = cfg.num_prefix_tokens
        assert same(p_old.reshape(n, -1, cfg.hidden_size), hs[:, P0:]) and same(x_old, hs[:, :P0])
        p_l, x_l = enc.patch_tokens(dev, layer=1, norm=False)
        assert same(p_l.reshape(n, -1, cfg.hidden_size), allh[1][:, P0:]) and same(x_l, allh[1][:, :P0])
        c16, c32, maps, heads = enc.cls_attention(dev, per_head=True, layer="all")
        e16, e32 = enc.encode_u8(dev)
        assert same(c16, e16) and same(c32, e32)
        for l in (1, Lc):
            _, _, m1, h1 = enc.cls_attention(dev, per_head=True, layer=l)
            assert same(m1, maps[:, l - 1]) and same(h1, heads[:, l - 1])
        assert same(enc.cls_attention(dev, layer=-1)[2], maps[:, Lc - 1])
        # layer L against the pruned path's map: within the bar; bit-identity is recorded, not required
        _, _, m0 = enc.cls_attention(dev)
        mtol = MAP_TOL_F16 if precision == 0 else MAP_TOL_F32
        e = rel_max(maps[:, Lc - 1].cpu().numpy(), m0.cpu().numpy())
        print(f"[layers {name} p{precision}] cls_attention(layer=L) vs cls_attention(): max|d|/max|ref| {e:.2e}, bit-identical: {same(maps[:, Lc - 1], m0)}")
        assert e < mtol
        # the debug tap of the residual stream after block l (which = 0: the fp32 stream)
        for l in range(Lc + 1):
            tap = enc.debug_tap(dev, 0 if l == 0 else l - 1, 0 if l == 0 else 7, 0)
            assert same(allh[l].reshape(tap.shape), tap), l
        # a frame alone, at position 5 of 7, in a batch of 16: identical bits for all three outputs
        one = dev[:1]
        def three(fr, i):
            return (enc.hidden_states(fr, layers=[0, Lc])[:, i], enc.cls_attention(fr, layer="all")[2][i], enc.attention_rollout(fr)[i],
                    enc.attention_rollout(fr, start_layer=Lc)[i])
        base = three(one, 0)
        for total, pos in ((7, 5), (16, 0), (16, 15)):
            batch = dev[torch.arange(total) % n].clone()
            batch[pos] = one[0]
            for a, b in zip(three(batch, pos), base):
                assert same(a, b), (total, pos)
        assert all(same(a, b) for a, b in zip(three(one, 0), base))
        enc.check_finite()
    finally:
        enc.close()


@pytest.mark.parametrize("lanes", (1, 2))
def test_nothing_else_moves(golden_dir, lanes):
    cfg = C.VIT_TINY
    g, n, H, Wd, dev = fixture(golden_dir, "vit_tiny")
    enc, fresh = make_enc(cfg, (H, Wd), 4, 0), make_enc(cfg, (H, Wd), 4, 0)
    try:
        enc.set_lanes(lanes)
        before = enc.encode_u8(dev)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()                          # both readings without blocks torch merely caches (`before` stays alive)
        free0 = torch.cuda.mem_get_info()[0]
        hs = enc.hidden_states(dev)
        roll = enc.attention_rollout(dev)
        maps = enc.cls_attention(dev, layer="all")[2]
        torch.cuda.synchronize()
        enc.check_finite()
        del hs, roll, maps
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        assert torch.cuda.mem_get_info()[0] >= free0      # the call's own tensors freed: the handle holds nothing more
        after, other = enc.encode_u8(dev), fresh.encode_u8(dev)
        for a, b, c in zip(before, after, other):
            assert same(a, b) and same(a, c)
        enc.check_finite()
    finally:
        enc.close()
        fresh.close()


@pytest.mark.parametrize("precision", (0, 3, 4))
def test_ingest_forms_agree(golden_dir, precision):
    """The u8 forms and the float (B,1,H,W) form, as tests/test_gpu_cls_attention.py::test_ingest_forms_agree requires of the maps:
    the same bits in precisions 3 and 4 (one forward behind both).  Precision 0 feeds float pixels as an fp16 hi + lo pair where the
    u8 form feeds the byte, so there the float form is held to the bars against the u8 form."""
    cfg = C.VIT_TINY
    g, n, H, Wd, dev = fixture(golden_dir, "vit_tiny")
    x = torch.from_numpy(dev[:, :, :, 1].cpu().numpy() / 255.0).float().cuda().unsqueeze(1)
    enc = make_enc(cfg, (H, Wd), 4, precision)
    try:
        a, b = enc.hidden_states(dev), enc.hidden_states(x)
        ra, rb = enc.attention_rollout(dev), enc.attention_rollout(x)
        ca, cb = enc.cls_attention(dev, per_head=True, layer="all"), enc.cls_attention(x, per_head=True, layer="all")
        green = dev[:, :, :, 1].contiguous()
        assert same(a, enc.hidden_states(green)) and same(ra, enc.attention_rollout(green))
        if precision >= 3:
            assert same(a, b) and same(ra, rb)
            for u, v in zip(ca, cb):
                assert same(u, v)
        else:
            e, er = rel_rows(b.cpu().numpy(), a.cpu().numpy()), rel_max(rb.cpu().numpy(), ra.cpu().numpy())
            em = max(rel_max(v.cpu().numpy(), u.cpu().numpy()) for u, v in zip(ca[2:], cb[2:]))
            print(f"[layers ingest p0] float form vs u8 form: hidden {e:.2e}, rollout {er:.2e}, CLS maps / heads {em:.2e}")
            assert e < TOL_F16 and er < min(cfg.num_hidden_layers * MAP_TOL_F16, ROLL_GATE_F16) and em < MAP_TOL_F16
            assert rel_rows(cb[1].cpu().numpy(), ca[1].cpu().numpy()) < TOL_F16
    finally:
        enc.close()


def test_rollout_properties(golden_dir):
    cfg = C.VIT_TINY
    g, n, H, Wd, dev = fixture(golden_dir, "vit_tiny")
    Lc, NP, T = cfg.num_hidden_layers, cfg.num_prefix_tokens, cfg.num_tokens(H, Wd)
    enc = make_enc(cfg, (H, Wd), 4, 4)
    try:
        r = enc._layers_call(dev, 1, "attention_rollout", rollout=(1, None))
        sc = r["scratch"].view(torch.float32).reshape(3, n, T, T)
        full = sc[1 + ((Lc - 1) & 1)].cpu().numpy().astype(np.float64)              # the product of all layers
        assert same(torch.from_numpy(full[:, 0, NP:].astype(np.float32)), r["rollout"].reshape(n, -1))
        dev_sum = float(np.abs(full.sum(-1) - 1.0).max())
        print(f"[rollout] full rows sum to 1 within {dev_sum:.2e} (bound {Lc * T * 2.0 ** -23:.2e})")
        assert dev_sum <= Lc * T * 2.0 ** -23
        last = enc.attention_rollout(dev, start_layer=Lc)
        m = enc.cls_attention(dev, layer=Lc)[2]
        e = rel_max(last.cpu().numpy(), 0.5 * m.cpu().numpy())
        print(f"[rollout] start_layer = L vs 0.5 x cls_attention(layer=L): {e:.2e}")
        assert e < MAP_TOL_F32 and same(enc.attention_rollout(dev, start_layer=-1), last)
    finally:
        enc.close()


def layers_args(**kw):
    a = L_.LayersArgs()
    a.struct_bytes = C_.sizeof(L_.LayersArgs)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_product_entry_refusals(golden_dir):
    l = L_.load()
    cfg = C.VIT_TINY
    g, n, H, Wd, dev = fixture(golden_dir, "vit_tiny")
    Lc, T, D = cfg.num_hidden_layers, cfg.num_tokens(H, Wd), cfg.hidden_size
    x = (dev[:, :, :, 1].float() / 255.0).unsqueeze(1).contiguous()
    green = dev[:, :, :, 1].contiguous()
    enc = make_enc(cfg, (H, Wd), 4, 4)
    cnx = make_enc(C.CONVNEXT_TINY, (H, Wd), 4, 4)
    p2 = make_enc(C.VIT_B16, (32, 32), 1, 2)
    wide = make_enc(cfg, (16, 16 * 8200), 1, 4)
    try:
        hs = torch.full((2, n, T, D), 7.0, device="cuda")
        roll = torch.full((n, T - cfg.num_prefix_tokens), 7.0, device="cuda")
        need = int(l.cbas_enc_layers_scratch_bytes(enc._h, n, H, Wd))
        assert need == 3 * n * T * T * 4
        scratch = torch.empty((need + 16,), dtype=torch.uint8, device="cuda")
        lay = (C_.c_int32 * 2)(0, Lc)
        lp = C_.cast(lay, C_.c_void_p)
        good = dict(hidden_layers=lp, n_hidden_layers=2, hidden_f32_dev=hs.data_ptr(), ld_hidden=D, hidden_layer_stride=n * T * D,
                    rollout_dev=roll.data_ptr(), rollout_start_layer=1, scratch_dev=scratch.data_ptr(), scratch_bytes=need)

        def call(h, a, u8=True):
            if u8:
                return l.cbas_enc_forward_u8_layers(h, green.data_ptr(), n, H, Wd, H * Wd, Wd, 1, C_.byref(a) if a is not None else None, None)
            return l.cbas_enc_forward_f32_layers(h, x.data_ptr(), n, H, Wd, C_.byref(a) if a is not None else None, None)

        bad_layer = (C_.c_int32 * 2)(0, Lc + 1)
        at_bad = (C_.c_int32 * 1)(Lc + 1)
        cases = {"null handle": (None, layers_args(**good)), "ConvNeXt handle": (cnx._h, layers_args(**good)),
                 "precision 2": (p2._h, layers_args(**good)), "all destinations NULL": (enc._h, layers_args()),
                 "null args": (enc._h, None),
                 "layer L + 1": (enc._h, layers_args(**{**good, "hidden_layers": C_.cast(bad_layer, C_.c_void_p)})),
                 "attention layer L + 1": (enc._h, layers_args(attn_layers=C_.cast(at_bad, C_.c_void_p), n_attn_layers=1, attn_map_dev=roll.data_ptr())),
                 "start layer 0": (enc._h, layers_args(**{**good, "rollout_start_layer": 0})),
                 "scratch one byte short": (enc._h, layers_args(**{**good, "scratch_bytes": need - 1})),
                 "misaligned hidden": (enc._h, layers_args(**{**good, "hidden_f32_dev": hs.data_ptr() + 4})),
                 "misaligned scratch": (enc._h, layers_args(**{**good, "scratch_dev": scratch.data_ptr() + 4})),
                 "ld too small": (enc._h, layers_args(**{**good, "ld_hidden": D - 4}))}
        for what, (h, a) in cases.items():
            for u8 in (True, False):
                assert call(h, a, u8) == -1 and l.cbas_last_error(), what
        # a token row that does not fit the kernels' LDS: refused before anything is queued
        Hw, Ww = 16, 16 * 8200
        big = torch.zeros((1, Hw, Ww), dtype=torch.uint8, device="cuda")
        for a in (layers_args(rollout_dev=roll.data_ptr(), rollout_start_layer=1, scratch_dev=scratch.data_ptr(), scratch_bytes=1 << 60),
                  layers_args(attn_layers=C_.cast((C_.c_int32 * 1)(1), C_.c_void_p), n_attn_layers=1, attn_map_dev=roll.data_ptr())):
            assert l.cbas_enc_forward_u8_layers(wide._h, big.data_ptr(), 1, Hw, Ww, Hw * Ww, Ww, 1, C_.byref(a), None) == -1
            assert b"LDS" in l.cbas_last_error() or b"tokens" in l.cbas_last_error()
        assert l.cbas_enc_layers_scratch_bytes(None, n, H, Wd) == -1 and l.cbas_enc_layers_scratch_bytes(cnx._h, n, H, Wd) == -1
        torch.cuda.synchronize()
        assert (hs == 7.0).all() and (roll == 7.0).all()                           # nothing was launched
        assert call(enc._h, layers_args(**good)) == 0
        torch.cuda.synchronize()
        assert not (hs == 7.0).any() and not (roll == 7.0).any()
        # the Python refusals
        with pytest.raises(ValueError):
            cnx.hidden_states(dev)
        with pytest.raises(ValueError):
            cnx.attention_rollout(dev)
        with pytest.raises(ValueError, match="precision 2"):
            p2.hidden_states(dev[:1, :32, :32])
        with pytest.raises(ValueError):
            enc.hidden_states(dev, layers=[Lc + 1])
        with pytest.raises(ValueError, match="normalised"):
            enc.patch_tokens(dev, norm=False)
    finally:
        for e in (enc, cnx, p2, wide):
            e.close()


def test_attention_maps_cli(golden_dir, tmp_path):
    from cbas_amd import attention_maps as A
    cfg = C.VIT_TINY
    ck = tmp_path / "ckpt"
    ck.mkdir()
    W.save_encoder_checkpoint(str(ck), cfg, W.synth_encoder_weights(cfg, ENC_SEED))
    clip = tmp_path / "clip.npy"
    np.save(clip, synth.cage_frames(7, 3, 72, 88))
    for extra, out in ((["--kind", "attention", "--layer", "all"], "all.png"), (["--kind", "rollout"], "roll.png"),
                       (["--kind", "rollout", "--query", "20,40"], "rollq.png")):
        png = tmp_path / out
        assert A.main(["--video", str(clip), "--frame", "1", "--encoder", str(ck), "--out", str(png), "--precision", "4"] + extra) == 0
        assert png.stat().st_size > 1000
