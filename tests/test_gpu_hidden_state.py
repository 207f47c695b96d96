"""Every token's final hidden state on the GPU: the kernels of tokens_out.hip one launch at a time against float64 (through
cbas_debug_rows_run, ops TOKEN_ROWS / TOKEN_SIM), then DinoEncoder.hidden_state against rows recorded from transformers' own
models (tests/golden/make_goldens_hidden_state.py), and the promises around it: encode_u8 keeps its bits, a frame's block does
not depend on its batch, refusals, similarity_map.

Bars of the single launches (u = 2^-24):
  rows        the LayerNorm bound of oracle/kernel_ref.py ln_ref - derived from where ln_row / cnx_ln round, as
              tests/test_gpu_rows_reference.py uses it for LN_F32 - plus the stored format's rounding (fp16: one fp16 rounding of a
              value within the bound); the ConvNeXt row 0 through cnx_pool_ln_ref (the pooled mean's own summation error).
  similarity  three fp32 sums of D terms, each a lane's fmaf chain of c = 4 ceil(D / 256) terms then a 6-level tree:
              |sum^ - sum| <= g sum |terms|, g = gamma(c + 6).  q.q and p.p have positive terms, so they are off by g relatively,
              their square roots by g / 2 + 2 u (sqrtf: 1 ulp budgeted), the product of the roots by one more u, the division by
              one more:  |cos^ - cos| <= g sum |q_i p_i| / (|q| |p|) + |cos| (g + 6 u), times 1.01 for the second-order terms.
The largest error / bar of each test is printed (run with -s)."""
import ctypes as C_
import math
import os

import numpy as np
import pytest
import torch

from cbas_amd import config as C, weights as W, synth
from cbas_amd.encoder import query_token_index, token_grid
from oracle import kernel_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ENC_SEED = 1234
TOL_F32 = 5e-6              # precisions 3 / 4, per-row ||d|| / ||ref||: tests/test_gpu_fp32.py's gate
# precision 0: tests/test_gpu_parity.py's gate for the CLS row.  The patch and register rows had never been measured; on an MI355X
# their largest per-row error is 2.2e-4 (vit_tiny), 1.9e-4 (gated_tiny, dinov2reg_tiny, dinov2_tiny) and 6.7e-4 (vitb16, whose CLS
# row measures 5.4e-4): every family is inside the project's 1e-3, so all rows share the CLS row's gate
TOL_F16 = 1e-3
TOKEN_ROWS, TOKEN_SIM, FINAL_CLS, CNX_POOL_LN = 11, 12, 4, 10
CANARY32, CANARY16 = np.float32(-31337.25), np.float16(-1234.0)
c_int, c_int64, c_float, c_void_p = C_.c_int, C_.c_int64, C_.c_float, C_.c_void_p


class RowsArgs(C_.Structure):            # include/cbas_mi355x_debug.h cbas_debug_rows_args
    _fields_ = ([("struct_bytes", c_int64)] + [(n, c_int) for n in ("op", "split", "M", "n", "D", "T", "h", "w", "sc_ld")] +
                [("eps", c_float), ("ld", c_int64), ("frame_stride", c_int64), ("row_stride", c_int64), ("pixel_stride", c_int64),
                 ("x", c_void_p), ("x_bytes", c_int64), ("gamma", c_void_p), ("beta", c_void_p), ("wt", c_void_p), ("bias", c_void_p),
                 ("out", c_void_p), ("out_bytes", c_int64), ("out2", c_void_p), ("out2_bytes", c_int64), ("counter", c_void_p)])


def rows_call(op, *, x, out=None, out2=None, counter=None, gamma=None, beta=None, query=None, **kw):
    """One harness call; returns its code.  out / out2 / counter are updated in place."""
    from cbas_amd import _lib
    _lib.require_debug("cbas_debug_rows_run")
    a = RowsArgs()
    a.struct_bytes, a.op = C_.sizeof(RowsArgs), op
    for k, v in kw.items():
        setattr(a, k, v)
    keep = [np.ascontiguousarray(t, np.float32) if t is not None else None for t in (gamma, beta)]
    a.gamma, a.beta = [None if t is None else t.ctypes.data for t in keep]
    q = None if query is None else np.ascontiguousarray(query, np.int32)
    a.wt = None if q is None else q.ctypes.data
    assert x.flags.c_contiguous
    a.x, a.x_bytes = x.ctypes.data, x.nbytes
    for name, buf in (("out", out), ("out2", out2)):
        if buf is not None:
            assert buf.flags.c_contiguous
            setattr(a, name, buf.ctypes.data)
            setattr(a, name + "_bytes", buf.nbytes)
    if counter is not None:
        a.counter = counter.ctypes.data
    return _lib.load().cbas_debug_rows_run(C_.byref(a))


def run(op, **kw):
    from cbas_amd import _lib
    _lib.check(rows_call(op, **kw), f"cbas_debug_rows_run(op {op})")


def ln64(x, gamma, beta, eps):
    """LayerNorm over the last axis, biased variance, float64; eps the fp32 value the kernel receives."""
    x = np.asarray(x, np.float64)
    c = x - x.mean(-1, keepdims=True)
    return c / np.sqrt((c * c).mean(-1, keepdims=True) + float(np.float32(eps))) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def images(rows, ld_out, want32, want16):
    return (np.full((rows + 2, ld_out), CANARY32, np.float32) if want32 else None,
            np.full((rows + 2, ld_out), CANARY16, np.float16) if want16 else None)


def check_rows(o32, o16, rows, D, ref, E, tag):
    """Bound, canaries (rows past the last one, columns D .. ld_out) and fp16 = RNE(fp32) of one launch's images."""
    worst = 0.0
    for o, kind, canary in ((o32, "f32", CANARY32), (o16, "f16", CANARY16)):
        if o is None:
            continue
        assert (o[rows:] == canary).all() and (o[:rows, D:] == canary).all(), f"{tag}: {kind} canaries changed"
        r = R.ratio(o[:rows, :D].astype(np.float64), ref, R.stored_bound(ref, E, kind))
        assert r <= 1.0, (tag, kind, r)
        worst = max(worst, r)
    if o32 is not None and o16 is not None:
        assert np.array_equal(bits(o16[:rows, :D]), bits(o32[:rows, :D].astype(np.float16))), f"{tag}: fp16 != RNE(fp32)"
    return worst


# ---- a. one launch of each kernel against float64 ----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 384, 768, 1280])
def test_final_norm_rows(D):
    worst = 0.0
    for M in (1, 3, 65):                 # rows_case plants a large-mean row, a CONSTANT row (M > 1) and a massive channel (M > 2)
        for ld, ld_out in ((D, D), (D + 12, D + 8)):
            eps = 1e-5 if M % 2 else 1e-6
            x, gamma, beta = R.rows_case(M, D, 400 + D + M, ld=ld)
            ref = ln64(x[:, :D], gamma, beta, eps)
            ref_o, E = R.ln_ref(x[:, :D], gamma, beta, eps)
            assert np.abs(ref - ref_o).max() <= 1e-12 * max(1.0, np.abs(ref).max())
            both = None
            for want32, want16 in ((True, True), (True, False), (False, True)):
                o32, o16 = images(M, ld_out, want32, want16)
                cnt = np.array([11], np.uint32)
                run(TOKEN_ROWS, x=x, out=o32, out2=o16, counter=cnt, gamma=gamma, beta=beta, M=M, D=D, ld=ld, sc_ld=ld_out, eps=eps)
                assert cnt[0] == 11
                worst = max(worst, check_rows(o32, o16, M, D, ref, E, f"M {M} ld {ld}"))
                if both is None:
                    both = (o32, o16)
                else:                    # one image alone holds the bits it holds beside the other
                    for o, b in zip((o32, o16), both):
                        assert o is None or np.array_equal(bits(o), bits(b))
            # row r is the CLS kernel's row: launch_final_norm_cls on the same rows (T = 1 when ld == D) gives the same bits
            if ld == D:
                c32, c16 = np.zeros((M, D), np.float32), np.zeros((M, D), np.float16)
                run(FINAL_CLS, x=x, out=c32, out2=c16, gamma=gamma, beta=beta, n=M, T=1, D=D, eps=eps)
                assert np.array_equal(bits(c32), bits(both[0][:M, :D])) and np.array_equal(bits(c16), bits(both[1][:M, :D]))
    print(f"[token rows D {D}] max err / bound {worst:.3f}")


@pytest.mark.parametrize("D", [384, 1280])
def test_final_norm_rows_nan_stays_in_its_row(D):
    M = 6
    x, gamma, beta = R.rows_case(M, D, 500 + D)

    def go(xx, counter):
        o32, o16 = images(M, D, True, True)
        run(TOKEN_ROWS, x=xx, out=o32, out2=o16, counter=counter, gamma=gamma, beta=beta, M=M, D=D, ld=D, sc_ld=D, eps=1e-5)
        return o32[:M], o16[:M]

    cnt = np.array([7], np.uint32)
    clean32, clean16 = go(x, cnt)
    assert cnt[0] == 7 and np.isfinite(clean32).all()
    bad = x.copy()
    bad[4, D // 3] = np.nan
    b32, b16 = go(bad, cnt)
    assert cnt[0] == 8, f"one row holds a NaN, the counter rose by {cnt[0] - 7}"
    assert np.isnan(b32[4]).all() and np.isnan(b16[4]).all()
    others = [r for r in range(M) if r != 4]
    assert np.array_equal(bits(b32[others]), bits(clean32[others])) and np.array_equal(bits(b16[others]), bits(clean16[others]))
    bad[1, 0], bad[5, D - 1] = np.inf, 1.0e20            # + infinity, and a finite value whose square overflows the variance
    go(bad, cnt)
    assert cnt[0] == 8 + 3
    n32, _ = go(bad, None)                               # nonfinite = NULL: same rows
    assert np.array_equal(bits(n32[[0, 2, 3]]), bits(clean32[[0, 2, 3]]))


@pytest.mark.parametrize("Cw", [32, 96, 256])
def test_convnext_token_rows(Cw):
    ld = (Cw + 127) // 128 * 128
    worst = 0.0
    for n, (h, w) in ((1, (1, 5)), (3, (1, 5)), (1, (10, 20)), (3, (10, 20))):          # T = 6 and 201
        hw, T = h * w, h * w + 1
        eps = 1e-6
        x, gamma, beta = R.rows_case(n * hw, Cw, 600 + Cw + n + hw, ld=ld)
        x[:, Cw:] = np.nan                                                             # the stream's padding columns: never read
        xs = x[:, :Cw].reshape(n, hw, Cw)
        ref = np.empty((n, T, Cw))
        E = np.empty((n, T, Cw))
        ref[:, 0], E[:, 0] = R.cnx_pool_ln_ref(xs, gamma, beta, eps)
        y, e = R.ln_ref(x[:, :Cw], gamma, beta, eps)
        ref[:, 1:], E[:, 1:] = y.reshape(n, hw, Cw), e.reshape(n, hw, Cw)
        assert np.abs(ref[:, 1:] - ln64(xs, gamma, beta, eps)).max() <= 1e-12 * np.abs(ref).max()
        assert np.abs(ref[:, 0] - ln64(xs.astype(np.float64).mean(1), gamma, beta, eps)).max() <= 1e-12 * np.abs(ref).max()
        for ld_out, (want32, want16) in ((Cw, (True, True)), (Cw + 8, (True, False)), (Cw + 8, (False, True))):
            o32, o16 = images(n * T, ld_out, want32, want16)
            cnt = np.array([3], np.uint32)
            run(TOKEN_ROWS, x=x, out=o32, out2=o16, counter=cnt, gamma=gamma, beta=beta, n=n, h=h, w=w, D=Cw, ld=ld, sc_ld=ld_out, eps=eps)
            assert cnt[0] == 3
            worst = max(worst, check_rows(o32, o16, n * T, Cw, ref.reshape(n * T, Cw), E.reshape(n * T, Cw), f"C {Cw} n {n} hw {hw}"))
            if want32 and want16:        # row 0 is launch_cnx_pool_ln's row, bit for bit
                c32, c16 = np.zeros((n, Cw), np.float32), np.zeros((n, Cw), np.float16)
                run(CNX_POOL_LN, x=x, out=c32, out2=c16, gamma=gamma, beta=beta, n=n, h=h, w=w, D=Cw, ld=ld, eps=eps)
                assert np.array_equal(bits(c32), bits(o32[:n * T:T, :Cw])) and np.array_equal(bits(c16), bits(o16[:n * T:T, :Cw]))
    # a NaN in one pixel: its own row and the pooled row of its frame, nothing else; both are counted
    n, h, w = 2, 2, 3
    x, gamma, beta = R.rows_case(n * h * w, Cw, 700 + Cw, ld=ld)
    clean, _ = images(n * 7, Cw, True, False)
    run(TOKEN_ROWS, x=x, out=clean, gamma=gamma, beta=beta, n=n, h=h, w=w, D=Cw, ld=ld, sc_ld=Cw, eps=1e-6)
    x[6 + 2, 5] = np.nan                 # frame 1, pixel 2 -> output rows 7 (pooled) and 7 + 1 + 2
    o32, _ = images(n * 7, Cw, True, False)
    cnt = np.array([0], np.uint32)
    run(TOKEN_ROWS, x=x, out=o32, counter=cnt, gamma=gamma, beta=beta, n=n, h=h, w=w, D=Cw, ld=ld, sc_ld=Cw, eps=1e-6)
    nan_rows = np.isnan(o32[:14]).all(1)
    assert cnt[0] == 2 and sorted(np.flatnonzero(nan_rows)) == [7, 10]
    assert np.array_equal(bits(o32[:14][~nan_rows]), bits(clean[:14][~nan_rows]))
    print(f"[convnext token rows C {Cw}] max err / bound {worst:.3f}")


def sim_ref(tok, P0, q):
    """float64 cosines (n, T - P0) of row q[b] against the patch rows and the bar of the module docstring."""
    D = tok.shape[2]
    t = tok.astype(np.float64)
    qr = t[np.arange(len(t)), q][:, None, :]
    pr = t[:, P0:]
    den = np.linalg.norm(qr, axis=2) * np.linalg.norm(pr, axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = np.where(den > 0, (qr * pr).sum(2) / den, 0.0)
        c = 4 * math.ceil(D / 256) + 6
        g = c * U / (1 - c * U)
        bar = np.where(den > 0, 1.01 * (g * (np.abs(qr) * np.abs(pr)).sum(2) / den + np.abs(cos) * (g + 6 * U)), 0.0)
    return cos, bar


@pytest.mark.parametrize("D", [64, 384, 768, 1280])
def test_token_similarity(D):
    worst = 0.0
    for n, T, P0 in ((1, 6, 1), (3, 6, 2), (3, 201, 5), (1, 201, 1)):
        for ld in (D, D + 8):
            tok = np.full((n, T, ld), np.nan, np.float32)
            tok[:, :, :D] = W.synth_normal(95, f"tok{n}{T}{D}", (n, T, D), 1.0) + W.synth_normal(96, f"m{n}{T}{D}", (n, 1, D), 0.7)
            tok[n - 1, P0 + (T - P0) // 2, :D] = 0.0                               # a zero patch row: 0, not NaN
            for fp16 in (0, 1):
                tk = tok.astype(np.float16).astype(np.float32) if fp16 else tok    # the fp16 form reads RNE(tokens): hand it exact values
                for query in (None, np.zeros(n, np.int32), np.full(n, T - 1, np.int32), np.arange(n, dtype=np.int32) % T):
                    mp = np.full((n + 1, T - P0), CANARY32, np.float32)
                    run(TOKEN_SIM, x=tk, out=mp, query=query, n=n, T=T, D=D, M=P0, ld=ld, split=fp16)
                    cos, bar = sim_ref(tk[:, :, :D], P0, np.zeros(n, np.int64) if query is None else query.astype(np.int64))
                    assert (mp[n:] == CANARY32).all() and np.isfinite(mp[:n]).all()
                    assert mp[n - 1, (T - P0) // 2] == 0.0
                    if query is not None and query[0] == T - 1:
                        assert np.abs(mp[:n, -1] - 1.0).max() <= 6 * U                 # a row against itself: two roots, a product, a division
                    r = float((np.abs(mp[:n] - cos) / np.maximum(bar, 1e-300))[bar > 0].max())
                    assert r <= 1.0, (n, T, P0, ld, fp16, r)
                    worst = max(worst, r)
    # a zero QUERY row: the whole map is 0; an index outside the frame is clamped, never read
    tok = W.synth_normal(97, f"z{D}", (2, 6, D), 1.0)
    tok[1, 0] = 0.0
    mp = np.full((2, 5), CANARY32, np.float32)
    run(TOKEN_SIM, x=tok, out=mp, n=2, T=6, D=D, M=1, ld=D)
    assert (mp[1] == 0.0).all() and (mp[0] != 0.0).all()
    a, b = np.empty((2, 5), np.float32), np.empty((2, 5), np.float32)
    run(TOKEN_SIM, x=tok, out=a, query=np.array([99, -3], np.int32), n=2, T=6, D=D, M=1, ld=D)
    run(TOKEN_SIM, x=tok, out=b, query=np.array([5, 0], np.int32), n=2, T=6, D=D, M=1, ld=D)
    assert np.array_equal(bits(a), bits(b))
    print(f"[token similarity D {D}] max err / bound {worst:.3f}")


def test_harness_refusals():
    D, M = 64, 3
    x, gamma, beta = R.rows_case(M, D, 1)
    out = np.zeros((M, D), np.float32)
    ok = dict(x=x, out=out, gamma=gamma, beta=beta, M=M, D=D, ld=D, sc_ld=D, eps=1e-5)
    assert rows_call(TOKEN_ROWS, **ok) == 0
    for bad in ({"M": 0}, {"M": M + 1}, {"sc_ld": D - 4}, {"sc_ld": D + 4}, {"sc_ld": D + 2}, {"ld": D + 4}, {"D": 62}, {"out": None},
                {"gamma": None}):
        assert rows_call(TOKEN_ROWS, **{**ok, **bad}) == -1, bad
    big = np.zeros((1, 1284), np.float32)
    assert rows_call(TOKEN_ROWS, x=big, out=big.copy(), gamma=big[0], beta=big[0], M=1, D=1284, ld=1284, sc_ld=1284, eps=1e-5) == -1
    cn = dict(x=np.zeros((2 * 6, 128), np.float32), out=np.zeros((2 * 7, 96), np.float32), gamma=np.ones(96), beta=np.ones(96), n=2, h=2, w=3,
              D=96, ld=128, sc_ld=96, eps=1e-6)
    assert rows_call(TOKEN_ROWS, **cn) == 0
    for bad in ({"n": 3}, {"D": 80}, {"h": 0}, {"w": 4}, {"n": 0}):
        assert rows_call(TOKEN_ROWS, **{**cn, **bad}) == -1, bad
    tok = np.zeros((2, 6, D), np.float32)
    sm = dict(x=tok, out=np.zeros((2, 5), np.float32), n=2, T=6, D=D, M=1, ld=D)
    assert rows_call(TOKEN_SIM, **sm) == 0
    for bad in ({"M": 6}, {"M": -1}, {"T": 7}, {"n": 3}, {"ld": D - 4}, {"out": None}, {"M": 0}):
        assert rows_call(TOKEN_SIM, **{**sm, **bad}) == -1, bad


# ---- b. hidden_state against transformers' rows --------------------------------------------------------------------------------
FIXTURES = {"vit_tiny": (C.VIT_TINY, (0, 3, 4)), "gated_tiny": (C.VIT_TINY_GATED, (0, 3, 4)), "dinov2reg_tiny": (C.DINOV2_REG_TINY, (0, 3, 4)),
            "dinov2_tiny": (C.DINOV2_TINY, (0, 3, 4)), "vitb16": (C.VIT_B16, (0, 3, 4)), "convnext_tiny": (C.CONVNEXT_TINY, (3, 4)),
            "convnext_t": (C.CONVNEXT_T, (3, 4))}
GOLDEN_CASES = [(name, p) for name, (_, ps) in FIXTURES.items() for p in ps]
_WEIGHTS = {}


def make_enc(cfg, hw, max_batch, precision):
    from cbas_amd.encoder import DinoEncoder
    if cfg not in _WEIGHTS:                     # generated once per configuration and never changed
        _WEIGHTS[cfg] = (W.synth_convnext_weights if C.is_convnext(cfg) else W.synth_encoder_weights)(cfg, ENC_SEED)
    return DinoEncoder.from_weights(cfg, _WEIGHTS[cfg], "cuda", max_batch=max_batch, max_frame=hw, precision=precision)


def rel_rows(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


@pytest.mark.parametrize("name,precision", GOLDEN_CASES, ids=[f"{n}_p{p}" for n, p in GOLDEN_CASES])
def test_hidden_state_against_goldens(golden_dir, name, precision):
    cfg = FIXTURES[name][0]
    g = np.load(os.path.join(golden_dir, "hidden_state.npz"))
    n, H, Wd, seed = (int(g[f"{name}_{k}"]) for k in ("n", "height", "width", "seed"))
    rows, ref = g[f"{name}_rows"], g[f"{name}_hidden"]
    nh, nw, P0 = token_grid(cfg, H, Wd)
    enc = make_enc(cfg, (H, Wd), 4, precision)
    try:
        dev = torch.from_numpy(synth.cage_frames(seed, n, H, Wd)).cuda()
        hs = enc.hidden_state(dev)
        assert hs.shape == (n, P0 + nh * nw, cfg.hidden_size) and hs.dtype == torch.float32
        err = rel_rows(hs.cpu().numpy()[:, rows], ref)                     # (n, kept rows)
        e_cls, e_rest = float(err[:, 0].max()), float(err[:, 1:].max())
        c16, c32 = enc.encode_u8(dev)
        e_enc = float(rel_rows(hs[:, 0].cpu().numpy(), c32.cpu().numpy()).max())
        print(f"[hidden_state {name} {H}x{Wd} p{precision}] per-row rel: CLS {e_cls:.3e}, other rows {e_rest:.3e} "
              f"(prefix {float(err[:, :P0].max()):.3e}); row 0 vs encode_u8 {e_enc:.3e}")
        tol = TOL_F16 if precision == 0 else TOL_F32
        assert e_cls < tol and e_enc < tol
        assert e_rest < tol
        # row 0 is, bit for bit, the CLS row of the same forward: encode_u8 with the last layer unpruned (ConvNeXt: any encode_u8)
        if not C.is_convnext(cfg):
            enc.set_prune_last_layer(False)
            c16, c32 = enc.encode_u8(dev)
            enc.set_prune_last_layer(True)
        h16 = enc.hidden_state(dev, dtype=torch.float16)
        assert np.array_equal(bits(hs[:, 0].contiguous()), bits(c32)) and np.array_equal(bits(h16[:, 0].contiguous()), bits(c16))
        assert np.array_equal(bits(h16), bits(hs.half()))                  # the fp16 image is RNE of the fp32 one
        patches, prefix = enc.patch_tokens(dev)
        assert patches.shape == (n, nh, nw, cfg.hidden_size) and prefix.shape == (n, P0, cfg.hidden_size)
        assert np.array_equal(bits(patches.reshape(n, nh * nw, -1).contiguous()), bits(hs[:, P0:].contiguous()))
        assert np.array_equal(bits(prefix.contiguous()), bits(hs[:, :P0].contiguous()))
    finally:
        enc.close()


# ---- c. encode_u8 is unchanged ------------------------------------------------------------------------------------------------
MOVES = [("vitb16", C.VIT_B16, (224, 224), (0, 1, 4)), ("vit_tiny", C.VIT_TINY, (72, 88), (0, 3, 4)), ("gated_tiny", C.VIT_TINY_GATED, (72, 88), (0, 3)),
         ("dinov2reg_tiny", C.DINOV2_REG_TINY, (72, 88), (0, 4)), ("convnext_tiny", C.CONVNEXT_TINY, (72, 88), (3, 4))]
MOVE_CASES = [(name, cfg, hw, p) for (name, cfg, hw, ps) in MOVES for p in ps]


@pytest.mark.parametrize("name,cfg,hw,precision", MOVE_CASES, ids=[f"{m[0]}_p{m[3]}" for m in MOVE_CASES])
def test_encode_u8_is_unchanged(name, cfg, hw, precision):
    dev = torch.from_numpy(synth.cage_frames(181, 5, *hw)).cuda()
    enc, fresh = make_enc(cfg, hw, 8, precision), make_enc(cfg, hw, 8, precision)
    try:
        a16, a32 = enc.encode_u8(dev)
        hs = enc.hidden_state(dev)
        sim = enc.similarity_map(dev)
        b16, b32 = enc.encode_u8(dev)
        f16, f32 = fresh.encode_u8(dev)                 # a handle that never served a token call
        for x16, x32 in ((b16, b32), (f16, f32)):
            assert np.array_equal(bits(x16), bits(a16)) and np.array_equal(bits(x32), bits(a32))
        assert torch.isfinite(hs).all() and torch.isfinite(sim).all()
        assert np.array_equal(bits(enc.hidden_state(dev)), bits(hs))        # and the token call repeats itself
    finally:
        enc.close()
        fresh.close()


# ---- d. batch invariance and refusals ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", (0, 3, 4))
def test_batch_invariance_and_refusals(precision):
    for cfg, hw in ((C.VIT_TINY, (72, 88)), (C.DINOV2_TINY, (72, 88)), (C.CONVNEXT_TINY, (72, 88))):
        if C.is_convnext(cfg) and precision == 0:
            continue
        max_batch = 4
        enc = make_enc(cfg, hw, max_batch, precision)
        try:
            dev = torch.from_numpy(synth.cage_frames(183, max_batch + 1, *hw)).cuda()
            one, three, full = enc.hidden_state(dev[2:3]), enc.hidden_state(dev[:3]), enc.hidden_state(dev[:max_batch])      # n == max_batch works
            assert np.array_equal(bits(three[2]), bits(one[0])) and np.array_equal(bits(full[2]), bits(one[0]))
            s1, s3 = enc.similarity_map(dev[2:3], query=(40, 40)), enc.similarity_map(dev[:3], query=(40, 40))
            assert np.array_equal(bits(s3[2]), bits(s1[0]))
            with pytest.raises(RuntimeError, match=r"n=5 outside \(0, max_batch=4\]"):
                enc.hidden_state(dev)
            with pytest.raises(ValueError, match="float32 or torch.float16"):
                enc.hidden_state(dev[:1], dtype=torch.float64)
            with pytest.raises(ValueError, match="outside"):
                enc.similarity_map(dev[:1], query=(71, 0))
            x = torch.from_numpy(synth.cage_frames(183, 3, *hw)[:, :, :, 1] / 255.0).float().cuda().unsqueeze(1)
            if precision != 0:          # the float32 ingest is the same forward: precision 0 feeds it hi + lo pixels, the others exactly
                assert np.array_equal(bits(enc.hidden_state(x)), bits(three))
            else:
                assert float(rel_rows(enc.hidden_state(x).cpu().numpy(), three.cpu().numpy()).max()) < TOL_F16
        finally:
            enc.close()


def test_precision_2_is_refused():
    from cbas_amd import _lib
    enc = make_enc(C.VIT_B16, (64, 64), 2, 2)
    try:
        dev = torch.from_numpy(synth.cage_frames(185, 1, 64, 64)).cuda()
        for call in (enc.hidden_state, enc.patch_tokens, enc.similarity_map):
            with pytest.raises(ValueError, match="a different encoder"):
                call(dev)
        out = torch.empty((1, 21, 768), dtype=torch.float32, device="cuda")     # the library says so itself
        rc = _lib.load().cbas_enc_forward_u8_tokens(enc._h, dev.data_ptr() + 1, 1, 64, 64, 64 * 64 * 3, 64 * 3, 3, out.data_ptr(), None, 768, None,
                                                    None, None)
        assert rc == -1 and b"a different encoder" in _lib.load().cbas_last_error()
        assert enc.encode_u8(dev)[0].shape == (1, 768)
    finally:
        enc.close()


def test_library_refuses_bad_token_arguments():
    from cbas_amd import _lib
    enc = make_enc(C.VIT_TINY, (64, 64), 2, 3)
    try:
        lib = _lib.load()
        dev = torch.from_numpy(synth.cage_frames(185, 1, 64, 64)).cuda()
        out = torch.empty((1, 21, 136), dtype=torch.float32, device="cuda")
        args = lambda p32, p16, ld: (enc._h, dev.data_ptr() + 1, 1, 64, 64, 64 * 64 * 3, 64 * 3, 3, p32, p16, ld, None, None, None)   # noqa: E731
        assert lib.cbas_enc_forward_u8_tokens(*args(None, None, 128)) == -1 and b"both NULL" in lib.cbas_last_error()
        for ld in (124, 130):
            assert lib.cbas_enc_forward_u8_tokens(*args(out.data_ptr(), None, ld)) == -1 and b"ld_tokens" in lib.cbas_last_error()
        out.fill_(-7.0)                     # a row stride of the caller's: columns D .. ld are not touched
        assert lib.cbas_enc_forward_u8_tokens(*args(out.data_ptr(), None, 136)) == 0, lib.cbas_last_error()
        torch.cuda.synchronize()
        assert (out[:, :, 128:] == -7.0).all() and np.array_equal(bits(out[:, :, :128].contiguous()), bits(enc.hidden_state(dev)))
    finally:
        enc.close()


# ---- e. similarity_map ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", (0, 4))
def test_similarity_map(precision):
    for cfg, hw in ((C.VIT_TINY, (72, 88)), (C.DINOV2_REG_TINY, (72, 88)), (C.CONVNEXT_TINY, (72, 88))):
        if C.is_convnext(cfg) and precision == 0:
            continue
        enc = make_enc(cfg, hw, 4, precision)
        try:
            n = 3
            dev = torch.from_numpy(synth.cage_frames(187, n, *hw)).cuda()
            nh, nw, P0 = token_grid(cfg, *hw)
            hs = enc.hidden_state(dev).cpu().numpy().astype(np.float64)
            for query in (None, (0, 0), (40, 50)):
                sim = enc.similarity_map(dev, query=query)
                assert sim.shape == (n, nh, nw) and sim.dtype == torch.float32 and torch.isfinite(sim).all()
                q = hs[:, query_token_index(cfg, *hw, query)][:, None, :]
                p = hs[:, P0:]
                cos = (q * p).sum(2) / (np.linalg.norm(q, axis=2) * np.linalg.norm(p, axis=2))
                d = float(np.abs(sim.cpu().numpy().reshape(n, -1) - cos).max())
                print(f"[similarity_map {cfg.model_type} p{precision} query {query}] max |d| {d:.2e}; range {float(sim.min()):.3f} .. {float(sim.max()):.3f}")
                assert d <= 1e-5
                if query is not None:       # the query's own patch
                    qi = query_token_index(cfg, *hw, query) - P0
                    assert np.abs(sim.cpu().numpy().reshape(n, -1)[:, qi] - 1.0).max() <= 1e-6
        finally:
            enc.close()
