"""Single launches of the head's sequential kernels - the recurrent LSTM of inference and of training, BPTT, the attention
pooling of both, head_centre - against the float64 references of oracle/kernel_ref.py, element by element.

Each harness call (cbas_debug_head_seq_run, debug build) feeds host operands to ONE launcher.  The references and every bound
were fixed on the CPU first (tests/test_kernel_reference_bounds.py: torch.autograd in float64, planted defects, conditioning):
  - permutation weights make every pre-activation one addend plus one exact product: only the gate functions' bound is left,
    which isolates indexing and fragment-layout mistakes of each of the eight instantiations;
  - random contraction weights: inference free-running within the propagated bound, training forward teacher-forced within
    the one-step bound, BPTT free-running from float64-forward images, hprev bit for bit;
  - a window's bits do not depend on its position in the 16-row MFMA tile nor on its neighbours; a NaN stays in its window.
Every output image carries the canary in rows a launch does not own and TAIL floats past its end; NaN sits in every operand
element a launch must not read.  Each test prints its largest error / bound (run with -s)."""
import ctypes as C

import numpy as np
import pytest

from cbas_amd import _lib
from oracle import kernel_ref as R

pytestmark = pytest.mark.gpu

(LSTM_INFER, LSTM_TRAIN_FWD, LSTM_TRAIN_BWD, POOL_INFER, POOL_TRAIN_FWD, POOL_TRAIN_BWD, CENTRE) = range(7)
EINVAL = -1
CANARY = np.float32(-31337.25)
TAIL = 5
F32 = np.float32
NI, NO = 10, 5


class SeqArgs(C.Structure):               # include/cbas_mi355x_debug.h cbas_debug_head_seq_args
    _fields_ = ([("struct_bytes", C.c_int64)] + [(n, C.c_int) for n in ("op", "h", "H2", "T", "lo", "hi", "C", "L0")] +
                [("n_windows", C.c_int64)] + [(n, C.c_float) for n in ("b_att", "att_temp", "gate", "temperature")] +
                [("in_", C.c_void_p * NI), ("in_bytes", C.c_int64 * NI), ("out", C.c_void_p * NO), ("out_bytes", C.c_int64 * NO)])


def seq_call(op, ins, outs, *, in_bytes=None, out_bytes=None, struct_bytes=None, **kw):
    """One harness call; returns its code.  ins / outs: arrays or None (an absent image); outs are updated in place."""
    _lib.require_debug("cbas_debug_head_seq_run")
    a = SeqArgs()
    a.struct_bytes = C.sizeof(SeqArgs) if struct_bytes is None else struct_bytes
    a.op = op
    for k, v in kw.items():
        setattr(a, k, v)
    keep = []
    for i, t in enumerate(ins):
        if t is None:
            continue
        t = np.ascontiguousarray(t, F32)
        keep.append(t)
        a.in_[i] = t.ctypes.data
        a.in_bytes[i] = (in_bytes or {}).get(i, t.nbytes)
    for i, t in enumerate(outs):
        if t is None:
            continue
        assert t.flags.c_contiguous and t.dtype == F32
        a.out[i] = t.ctypes.data
        a.out_bytes[i] = (out_bytes or {}).get(i, t.nbytes)
    return _lib.load().cbas_debug_head_seq_run(C.byref(a))


def run(op, ins, outs, **kw):
    _lib.check(seq_call(op, ins, outs, **kw), f"cbas_debug_head_seq_run(op {op})")


def image(n):
    return np.full(int(n) + TAIL, CANARY, F32)


def body(img, shape):
    n = int(np.prod(shape))
    assert (img[n:] == CANARY).all(), "canary past the image changed"
    return img[:n].reshape(shape)


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- launches ---------------------------------------------------------------------------------------------------------------
def lstm_infer(gin, W, lo, hi, poison=True):
    """head_lstm on gin [w][T][8h]; with poison, NaN sits where the launch must not read: the forward direction's columns at
    t >= hi and the reverse direction's at t < lo."""
    nw, T, G8 = gin.shape
    h = G8 // 8
    g = gin.copy()
    if poison:
        g[:, hi:, :4 * h] = np.nan
        g[:, :lo, 4 * h:] = np.nan
    out = image(nw * (hi - lo) * 2 * h)
    run(LSTM_INFER, [g, W], [out], h=h, T=T, lo=lo, hi=hi, n_windows=nw)
    return body(out, (nw, hi - lo, 2 * h))


def lstm_train_fwd(gin, W):
    nw, T, G8 = gin.shape
    h = G8 // 8
    act, cst, hout = image(nw * T * 8 * h), image(nw * T * 2 * h), image(nw * T * 2 * h)
    run(LSTM_TRAIN_FWD, [gin, W], [act, cst, hout], h=h, T=T, n_windows=nw)
    return body(act, (nw, T, 8 * h)), body(cst, (nw, T, 2 * h)), body(hout, (nw, T, 2 * h))


def lstm_train_bwd(dh, act, cst, hout, W):
    nw, T, G8 = act.shape
    h = G8 // 8
    dgin, hprev = image(nw * T * 8 * h), image(nw * T * 2 * h)
    run(LSTM_TRAIN_BWD, [dh, act, cst, hout, W], [dgin, hprev], h=h, T=T, n_windows=nw)
    return body(dgin, (nw, T, 8 * h)), body(hprev, (nw, T, 2 * h))


CASES = R.lstm_suite_cases()
CASE_IDS = [f"h{c[0]}-w{c[1]}-{c[2]}-T{c[3]}-{c[4]}" for c in CASES]


# ---- a. permutation weights: the gate functions' bound alone ------------------------------------------------------------------
@pytest.mark.parametrize("h", R.LSTM_H)
def test_lstm_permutation_weights_leave_only_the_gate_functions(h):
    """W_hh[dir][g h + u][k] = 2^-s(g, dir) at k = pi_{g,dir}(u): any summation order gives the same pre-activation bits, so both
    forward kernels must meet the float64 reference within the bound of sigmoid / tanh alone (levels = 1: the one rounding of
    the addend + product).  W_hh = 0: the outputs depend on gin element by element."""
    W = R.lstm_perm_weights(h)
    worst = 0.0
    for (nw, T, lo, hi) in ((17, 7, 2, 5), (1, 31, 0, 31), (3, 2, 1, 2)):
        gin, _ = R.lstm_case(nw, T, h, 31 * h + T)
        ref, E, full = R.lstm_infer_ref(gin, W, lo, hi, levels=1)
        got = lstm_infer(gin, W, lo, hi)
        r = R.ratio(got, ref, E)
        worst = max(worst, r)
        assert r <= 1.0, ("inference", h, nw, T, lo, hi, r)
        if nw <= 3:
            act, cst, hout = lstm_train_fwd(gin, W)
            tf = R.lstm_train_fwd_teacher_ref(gin, W, cst, hout, levels=1)
            for name, y, k in (("act", act, "act"), ("cst", cst, "c"), ("hout", hout, "h")):
                r = R.ratio(y, tf[k], tf["S_" + k])
                worst = max(worst, r)
                assert r <= 1.0, ("training forward", name, h, nw, T, r)
    # W_hh = 0: the two directions are one function of their own gin columns.  Window 1 holds window 0 reversed in time with the
    # directions' columns exchanged, so each of its directions sees what the other saw in window 0
    Z = np.zeros_like(W)
    gin, _ = R.lstm_case(2, 3, h, h)
    rev = gin[0][::-1]
    gin[1] = np.concatenate([rev[:, 4 * h:], rev[:, :4 * h]], 1)
    swap = lambda y: np.concatenate([y[::-1][:, y.shape[1] // 2:], y[::-1][:, :y.shape[1] // 2]], 1)
    got = lstm_infer(gin, Z, 0, 3, poison=False)
    act, cst, hout = lstm_train_fwd(gin, Z)
    assert same_bits(got[1], swap(got[0])), ("W_hh = 0, inference: an output depends on more than its own gin column", h)
    assert same_bits(hout[1], swap(hout[0])) and same_bits(cst[1], swap(cst[0])) and same_bits(act[1], swap(act[0])), ("W_hh = 0, training forward", h)
    print(f"[lstm permutation h {h}] max err / bound {worst:.3f}")


# ---- b, e. random weights within the propagated / one-step bounds; inference against training forward -----------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_lstm_random_weights_within_the_bounds(case):
    h, nwi, nwt, T, kind, lo, hi = case
    gall, W = R.lstm_case(max(nwi, nwt), T, h, 7 * h + T + nwi)
    gin = np.ascontiguousarray(gall[:nwi])
    ref, E, _ = R.lstm_infer_ref(gin, W, lo, hi)
    got = lstm_infer(gin, W, lo, hi)
    r_inf = R.ratio(got, ref, E)
    assert r_inf <= 1.0, ("inference, free-running", case, r_inf)
    # training forward on the first nwt windows of the same operands, teacher-forced
    gt = np.ascontiguousarray(gall[:nwt])
    nb = min(nwi, nwt)
    act, cst, hout = lstm_train_fwd(gt, W)
    tf = R.lstm_train_fwd_teacher_ref(gt, W, cst, hout)
    r_tf = max(R.ratio(act, tf["act"], tf["S_act"]), R.ratio(cst, tf["c"], tf["S_c"]), R.ratio(hout, tf["h"], tf["S_h"]))
    assert r_tf <= 1.0, ("training forward, teacher-forced", case, r_tf)
    # e. the product trains with one kernel and serves with the other: rows [lo, hi) differ by at most the sum of the two bounds
    fr = R.lstm_fwd_ref(gt, W, "train")
    r_e = R.ratio(got[:nb], hout[:nb, lo:hi].astype(np.float64), E[:nb] + fr["E_h"][:nb, lo:hi])
    assert r_e <= 1.0, ("inference against training forward", case, r_e)
    # BPTT, free-running, from the float64 forward's images rounded to fp32; dhout non-zero at every t
    a32, c32, h32 = (fr[k].astype(F32) for k in ("act", "c", "h"))
    dh = np.random.default_rng(h * T + 1).standard_normal(h32.shape).astype(F32)
    dh[dh == 0] = 1
    dgin, hprev, Eb, _ = R.lstm_bwd_ref(dh, a32, c32, h32, W)
    g, hp = lstm_train_bwd(dh, a32, c32, h32, W)
    r_b = R.ratio(g, dgin, Eb)
    assert r_b <= 1.0, ("BPTT", case, r_b)
    assert same_bits(hp, hprev.astype(F32)), ("hprev is hout at the feeding step, +0 at the first", case)
    print(f"[lstm {CASE_IDS[CASES.index(case)]}] err / bound: inference {r_inf:.3f}, training forward {r_tf:.3f}, infer vs train {r_e:.3f}, BPTT {r_b:.3f}")


# ---- c. a window is alone in its tile ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [16, 80, 128])
def test_a_windows_bits_do_not_depend_on_its_place_or_its_neighbours(h):
    T, lo, hi = 7, 2, 5
    gin, W = R.lstm_case(33, T, h, 3 * h)
    one = gin[5:6].copy()
    alone = lstm_infer(one, W, lo, hi)
    for pos in (0, 7, 15, 16):
        for amp in (1.0, 40.0):                           # ... whatever the neighbours hold
            g = (gin * F32(amp)).astype(F32)
            g[pos] = one[0]
            got = lstm_infer(g, W, lo, hi)
            assert same_bits(got[pos], alone[0]), ("inference", h, pos, amp)
    g3 = gin[:3].copy()
    g3[2] = one[0]
    a1, c1, h1 = lstm_train_fwd(one, W)
    a3, c3, h3 = lstm_train_fwd(g3, W)
    assert same_bits(a3[2], a1[0]) and same_bits(c3[2], c1[0]) and same_bits(h3[2], h1[0]), ("training forward", h)
    dh = np.random.default_rng(h).standard_normal((3, T, 2 * h)).astype(F32)
    d1, p1 = lstm_train_bwd(dh[2:3], a1, c1, h1, W)
    d3, p3 = lstm_train_bwd(dh, a3, c3, h3, W)
    assert same_bits(d3[2], d1[0]) and same_bits(p3[2], p1[0]), ("BPTT", h)
    print(f"[lstm window isolation h {h}] bit for bit at positions 0, 7, 15, 16 of 33 and in both training kernels")


# ---- d. a non-finite input stays in its window and shows ----------------------------------------------------------------------------
@pytest.mark.parametrize("h", [32, 112])
def test_nan_stays_in_its_window_and_shows(h):
    """NaN in all four gates' columns of one window at one t: the other windows of the tile keep their bits, and that window's
    h is NaN from that step on in each direction.  Then NaN in the g-gate column only: tanh must hand it on (tanh_bf once began
    with fmaxf(-2|x|, -100), which drops a NaN and returned +-1: the inference kernel wrote finite h where lstm_train_fwd, on
    tanhf, writes NaN)."""
    nw, T, t0, bad = 16, 7, 3, 6
    gin, W = R.lstm_case(nw, T, h, 5 * h)
    clean = lstm_infer(gin, W, 0, T, poison=False)
    for cols, tag in ((slice(None), "all gates"), (np.r_[2 * h:3 * h, 6 * h:7 * h], "g gate only")):
        g = gin.copy()
        g[bad, t0, cols] = np.nan
        got = lstm_infer(g, W, 0, T, poison=False)
        others = np.arange(nw) != bad
        assert same_bits(got[others], clean[others]), ("NaN left its window", tag, h)
        assert np.isnan(got[bad, t0:, :h]).all() and np.isnan(got[bad, :t0 + 1, h:]).all(), ("NaN did not show from its step on", tag, h)
        assert same_bits(got[bad, :t0, :h], clean[bad, :t0, :h]) and same_bits(got[bad, t0 + 1:, h:], clean[bad, t0 + 1:, h:]), ("steps before the NaN", tag, h)
        _, _, ht = lstm_train_fwd(np.ascontiguousarray(g[bad:bad + 1]), W)
        assert np.array_equal(np.isnan(ht[0]), np.isnan(got[bad])), ("inference and training forward disagree on where NaN is", tag, h)
    print(f"[lstm NaN h {h}] stays in its window, shows from its step on, g-gate NaN included")


# ---- f. pooling, inference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.POOL_INFER_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_pool_inference(case):
    H2, Cc, nc, nw, g, temperature = case
    worst = 0.0
    for gap in (False, True) if (H2, Cc) == (128, 7) else (False,):
        c = R.pool_case(nw, H2, Cc, nc, H2 + Cc + nc + nw, train=False, gap=gap)
        ref, E = R.pool_infer_ref(c["hout_c"], c["lin"], c["w_att"], c["b_att"], c["att_temp"], c["w_lin2"], c["b_lin2"], g, temperature)
        ins = [c["hout_c"], c["lin"], c["w_att"], c["w_lin2"], c["b_lin2"]]
        kw = dict(H2=H2, T=nc, lo=0, hi=nc, C=Cc, n_windows=nw, b_att=c["b_att"], att_temp=c["att_temp"], gate=g, temperature=temperature)
        shapes = ((nw, Cc), (nw, Cc), (nw, H2))
        outs = [image(np.prod(s)) for s in shapes]
        run(POOL_INFER, ins, outs, **kw)
        full = [body(o, s) for o, s in zip(outs, shapes)]
        for name, y, r_, e_ in zip(("probs", "logits", "latent"), full, ref, E):
            r = R.ratio(y, r_, e_)
            worst = max(worst, r)
            assert r <= 1.0, (name, case, gap, r)
        assert np.abs(full[0].astype(np.float64).sum(1) - 1.0).max() <= Cc * R.U1, ("probs do not sum to 1 within C u1", case)
        aw = R._attention64(c["hout_c"].astype(np.float64), c["w_att"].astype(np.float64), c["b_att"], c["att_temp"], 0.0, 1)[2]
        if nc > 1 and not gap:
            assert 1.0 / nc + 1e-3 < aw.max(1).min() and aw.max(1).max() < 1.0 - 1e-6, ("the attention softmax is flat or one-hot", case)
        if gap:
            assert (aw[0] < 2.0 ** -150).any(), "no weight underflows"
        for missing in range(3):                           # each of probs, logits, latent NULL in turn: the others keep their bits
            o2 = [None if i == missing else image(np.prod(s)) for i, s in enumerate(shapes)]
            run(POOL_INFER, ins, o2, **kw)
            for i, s in enumerate(shapes):
                if i != missing:
                    assert same_bits(body(o2[i], s), full[i]), ("an output changed when another was NULL", case, missing, i)
    print(f"[pool inference {case}] max err / bound {worst:.3f}")


# ---- g. pooling, training forward and backward ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.POOL_TRAIN_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_pool_training_forward_and_backward(case):
    H2, Cc, nc, raw = case
    nw = 3
    c = R.pool_case(nw, H2, Cc, nc, H2 + Cc + nc, train=True, temp=R.softplus_temp_ref(raw)[0])
    T, lo, hi = c["T"], c["lo"], c["hi"]
    hout = c["hout"].copy()
    hout[:, :lo] = np.nan                                  # rows outside [lo, hi) must not be read
    hout[:, hi:] = np.nan
    ins = [hout, c["lin"], c["w_att"], c["w_lin2"], c["b_lin2"]]
    kw = dict(H2=H2, T=T, lo=lo, hi=hi, C=Cc, n_windows=nw, b_att=c["b_att"], att_temp=raw, gate=c["gate"])
    ref, E = R.pool_train_fwd_ref(c["hout"], c["lin"], c["w_att"], c["b_att"], raw, c["w_lin2"], c["b_lin2"], c["gate"], lo, hi)
    shapes = ((nw, nc), (nw, nc), (nw, H2), (nw, Cc), (nw, Cc))
    outs = [image(np.prod(s)) for s in shapes]
    run(POOL_TRAIN_FWD, ins, outs, **kw)
    got = [body(o, s) for o, s in zip(outs, shapes)]
    worst_f = 0.0
    for name, y, r_, e_ in zip(("attw", "scores", "latent", "lstm_logits", "final_logits"), got, ref, E):
        r = R.ratio(y, r_, e_)
        worst_f = max(worst_f, r)
        assert r <= 1.0, ("forward", name, case, r)
    assert np.abs(got[0].astype(np.float64).sum(1) - 1.0).max() <= (nc + 1) * R.U1, ("attw does not sum to 1", case)
    # backward from the float64 forward's images rounded to fp32
    aw, sc, _, lstm, _ = (x.astype(F32) for x in ref)
    df = np.random.default_rng(H2 + Cc).standard_normal((nw, Cc)).astype(F32)
    worst_b = 0.0
    for dcov in (None, np.random.default_rng(nc).standard_normal((nw, H2)).astype(F32)):
        bref, bE = R.pool_train_bwd_ref(c["hout"], c["lin"], c["w_att"], raw, c["w_lin2"], c["gate"], lo, hi, aw, sc, lstm, df, dcov)
        bshapes = ((nw, T, H2), (nw, Cc), (nw, Cc), (nw, H2 + 12))
        bouts = [image(np.prod(s)) for s in bshapes]
        run(POOL_TRAIN_BWD, ins + [aw, sc, lstm, df, dcov], bouts, **kw)
        bgot = [body(o, s) for o, s in zip(bouts, bshapes)]
        for name, y, r_, e_ in zip(("dhout", "dlstm_logits", "dlin_logits", "part"), bgot, bref, bE):
            m = e_ > 0                                     # bound 0: dhout outside [lo, hi) and part's unnamed slots, exact zeros (below)
            r = R.ratio(y[m], r_[m], e_[m])
            worst_b = max(worst_b, r)
            assert r <= 1.0, ("backward", name, case, dcov is not None, r)
        dh, part = bgot[0], bgot[3]
        assert same_bits(dh[:, :lo], np.zeros_like(dh[:, :lo])) and same_bits(dh[:, hi:], np.zeros_like(dh[:, hi:])), ("dhout outside [lo, hi) is not +0", case)
        zero_slots = [H2 + i for i in (1, 2, 3, 5, 6, 7, 9, 10, 11)]
        assert same_bits(part[:, zero_slots], np.zeros((nw, 9), F32)), ("part's unnamed tail slots are not +0", case)
    print(f"[pool training {case}] max err / bound: forward {worst_f:.3f}, backward {worst_b:.3f}")


# ---- h. centre ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3, 31])
def test_centre(T):
    worst = 0.0
    for L0 in (4, 256, 260):
        nw = 3
        x = (np.random.default_rng(T + L0).standard_normal((nw, T, L0)) + 2.0).astype(F32)
        x[2] = x[0]                                        # equal data in two windows: equal bits
        ref, E = R.centre_ref(x)
        img = image(nw * T * L0)
        img[:nw * T * L0] = x.ravel()
        run(CENTRE, [], [img], T=T, L0=L0, n_windows=nw)
        got = body(img, (nw, T, L0))
        r = R.ratio(got, ref, E)
        worst = max(worst, r)
        assert r <= 1.0, (T, L0, r)
        assert same_bits(got[2], got[0]), ("equal columns in two windows differ", T, L0)
    print(f"[centre T {T}] max err / bound {worst:.3f}")


# ---- i. refusals -------------------------------------------------------------------------------------------------------------------
def _refused(word, op, ins, outs, **kw):
    before = [None if o is None else o.copy() for o in outs]
    rc = seq_call(op, ins, outs, **kw)
    msg = (_lib.load().cbas_last_error() or b"").decode(errors="replace")
    assert rc == EINVAL, (op, kw, rc)
    assert word in msg, (word, msg)
    for o, b in zip(outs, before):
        assert o is None or same_bits(o, b), "a refused call touched an output"


def test_harness_refuses_what_the_launchers_would_mishandle():
    h, T, nw = 16, 3, 2
    gin, W = R.lstm_case(nw, T, h, 1)
    out = image(nw * T * 2 * h)
    ok = dict(h=h, T=T, lo=0, hi=T, n_windows=nw)
    for bad_h in (0, 8, 24, 144):
        _refused("h =", LSTM_INFER, [gin, W], [out], **dict(ok, h=bad_h))
    _refused("n_windows", LSTM_INFER, [gin, W], [out], **dict(ok, n_windows=0))
    _refused("T =", LSTM_INFER, [gin, W], [out], **dict(ok, T=0, hi=0))
    for lo, hi in ((-1, 2), (2, 2), (2, 1), (0, T + 1)):
        _refused("lo", LSTM_INFER, [gin, W], [out], **dict(ok, lo=lo, hi=hi))
    _refused("too small", LSTM_INFER, [gin, W], [out], in_bytes={0: gin.nbytes - 4}, **ok)
    _refused("too small", LSTM_INFER, [gin, W], [out], in_bytes={1: W.nbytes - 4}, **ok)
    _refused("too small", LSTM_INFER, [gin, W], [out], out_bytes={0: nw * T * 2 * h * 4 - 4}, **ok)
    _refused("NULL", LSTM_INFER, [gin, None], [out], **ok)
    _refused("NULL", LSTM_INFER, [gin, W], [None], **ok)
    _refused("struct_bytes", LSTM_INFER, [gin, W], [out], struct_bytes=8, **ok)
    _refused("op", 7, [gin, W], [out], **ok)
    a8, s2 = image(nw * T * 8 * h), image(nw * T * 2 * h)
    _refused("too small", LSTM_TRAIN_FWD, [gin, W], [a8, s2, s2.copy()], out_bytes={1: 8}, h=h, T=T, n_windows=nw)
    _refused("NULL", LSTM_TRAIN_BWD, [s2, a8, s2, s2, None], [a8.copy(), s2.copy()], h=h, T=T, n_windows=nw)
    _refused("too small", LSTM_TRAIN_BWD, [s2, a8, s2, s2, W], [a8.copy(), s2.copy()], in_bytes={2: 16}, h=h, T=T, n_windows=nw)
    # pooling
    H2, Cc, nc = 32, 2, 3
    c = R.pool_case(nw, H2, Cc, nc, 1, train=True)
    ins = [c["hout"], c["lin"], c["w_att"], c["w_lin2"], c["b_lin2"]]
    pk = dict(H2=H2, T=c["T"], lo=c["lo"], hi=c["hi"], C=Cc, n_windows=nw, b_att=0.0, att_temp=0.5, gate=0.25, temperature=1.0)
    fo = [image(nw * nc), image(nw * nc), image(nw * H2), image(nw * Cc), image(nw * Cc)]
    for op in (POOL_INFER, POOL_TRAIN_FWD):
        _refused("C =", op, ins, fo, **dict(pk, C=0))
        _refused("C =", op, ins, fo, **dict(pk, C=65))
        _refused("H2 =", op, ins, fo, **dict(pk, H2=258))
        _refused("lo", op, ins, fo, **dict(pk, lo=2, hi=2))
    _refused("H2 =", POOL_TRAIN_FWD, ins, fo, **dict(pk, H2=48))
    _refused("hi - lo", POOL_TRAIN_FWD, ins, fo, **dict(pk, T=140, lo=0, hi=129))
    _refused("too small", POOL_TRAIN_FWD, ins, fo, in_bytes={0: c["hout"].nbytes - 4}, **pk)
    _refused("NULL", POOL_TRAIN_FWD, ins[:4] + [None], fo, **pk)
    _refused("NULL", POOL_TRAIN_FWD, ins, fo[:4] + [None], **pk)
    _refused("all NULL", POOL_INFER, ins, [None, None, None], **pk)
    bo = [image(nw * c["T"] * H2), image(nw * Cc), image(nw * Cc), image(nw * (H2 + 12))]
    bi = ins + [fo[0][:nw * nc], fo[1][:nw * nc], fo[3][:nw * Cc], fo[4][:nw * Cc]]
    _refused("NULL", POOL_TRAIN_BWD, bi[:8], bo, **pk)                  # dfinal is not optional (dlat_cov is)
    _refused("too small", POOL_TRAIN_BWD, bi, bo, out_bytes={3: nw * (H2 + 12) * 4 - 4}, **pk)
    x = image(nw * T * 4)
    _refused("L0", CENTRE, [], [x], T=T, L0=0, n_windows=nw)
    _refused("too small", CENTRE, [], [x], T=T, L0=8, n_windows=nw)
    _refused("NULL", CENTRE, [], [None], T=T, L0=4, n_windows=nw)
    assert _lib.load().cbas_debug_head_seq_run(None) == EINVAL


def test_the_served_neighbours_of_the_refusals_pass():
    """nc = 128, C = 64 (training pooling), h = 128 with T = 1 and lo = hi - 1 (inference LSTM): the limits themselves are served."""
    c = R.pool_case(1, 256, 64, 128, 9, train=True, temp=R.softplus_temp_ref(0.5)[0])
    ref, E = R.pool_train_fwd_ref(c["hout"], c["lin"], c["w_att"], c["b_att"], 0.5, c["w_lin2"], c["b_lin2"], c["gate"], c["lo"], c["hi"])
    shapes = ((1, 128), (1, 128), (1, 256), (1, 64), (1, 64))
    outs = [image(np.prod(s)) for s in shapes]
    run(POOL_TRAIN_FWD, [c["hout"], c["lin"], c["w_att"], c["w_lin2"], c["b_lin2"]], outs, H2=256, T=c["T"], lo=c["lo"], hi=c["hi"], C=64,
        n_windows=1, b_att=c["b_att"], att_temp=0.5, gate=c["gate"])
    worst = max(R.ratio(body(o, s), r_, e_) for o, s, r_, e_ in zip(outs, shapes, ref, E))
    gin, W = R.lstm_case(1, 1, 128, 2)
    ref, E, _ = R.lstm_infer_ref(gin, W, 0, 1)
    worst = max(worst, R.ratio(lstm_infer(gin, W, 0, 1), ref, E))
    assert worst <= 1.0, worst
    print(f"[served limits] max err / bound {worst:.3f}")
