"""Single launches of the head's three expand kernels - head_expand (inference, fixed and sliding windows), train_expand_fwd and
train_expand_bwd (resident and big storage forms) - against the float64 references of oracle/kernel_ref.py, element by element.

Each harness call (cbas_debug_head_expand_run, debug build) feeds host operands to ONE launcher.  The references, the bounds and
the cases were fixed on the CPU first (tests/test_kernel_reference_bounds.py: torch.autograd in float64 on a transcription of the
model, fp32 emulations accepted, planted defects rejected on these very shapes, conditioning):
  - training forward Y and lin_logits, the backward's lin1 and padding columns of dproj: bit for bit (the kernel spells the order);
  - aug of all three kernels, inference lin_logits, dproj's bottleneck columns, part: within the propagated bound;
  - the temporal operators build_temporal hands the training kernels equal the float64 reference rounded to fp32;
  - sliding and fixed-window launches on the same rows return the same bits; a window's bits do not depend on its neighbours; a NaN
    stays in its window and shows.
Every output image carries the canary in TAIL floats past its end; NaN sits in every operand element a launch must not read.  Each
test prints its largest error / bound (run with -s)."""
import ctypes as C

import numpy as np
import pytest

from cbas_amd import _lib
from oracle import kernel_ref as R

pytestmark = pytest.mark.gpu

INFER, TRAIN_FWD, TRAIN_BWD = range(3)
EINVAL = -1
CANARY = np.float32(-31337.25)
TAIL = 5
F32 = np.float32
NI, NO = 9, 3
ALPHA = R.EXPAND_ALPHA


class ExpandArgs(C.Structure):            # include/cbas_mi355x_debug.h cbas_debug_head_expand_args
    _fields_ = ([("struct_bytes", C.c_int64)] + [(n, C.c_int) for n in ("op", "T", "Bn", "NS", "C", "NPROJ", "lo", "hi", "sliding")] +
                [("alpha", C.c_float), ("scale", C.c_float), ("thr", C.c_uint32)] +
                [(n, C.c_int64) for n in ("n_windows", "w0", "r0", "n_frames")] + [("key", C.c_uint64 * 3)] +
                [("in_", C.c_void_p * NI), ("in_bytes", C.c_int64 * NI), ("out", C.c_void_p * NO), ("out_bytes", C.c_int64 * NO)])


def expand_call(op, ins, outs, *, in_bytes=None, out_bytes=None, struct_bytes=None, keys=None, **kw):
    """One harness call; returns its code.  ins: {index: array}; outs: arrays or None, updated in place."""
    _lib.require_debug("cbas_debug_head_expand_run")
    a = ExpandArgs()
    a.struct_bytes = C.sizeof(ExpandArgs) if struct_bytes is None else struct_bytes
    a.op = op
    for k, v in kw.items():
        setattr(a, k, v)
    for k, v in enumerate(keys or ()):
        a.key[k] = v
    keep = []
    for i, t in ins.items():
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
    return _lib.load().cbas_debug_head_expand_run(C.byref(a))


def run(op, ins, outs, **kw):
    _lib.check(expand_call(op, ins, outs, **kw), f"cbas_debug_head_expand_run(op {op})")


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
def params(p):
    return {1: p["b_bott"], 2: p["ln_w"], 3: p["ln_b"], 4: p["b_lin1"]}


def infer(img, p, Bn, NS, Cc, lo, hi, nw, T, sliding=None):
    """head_expand on the proj image [rows][NPROJ]; sliding = (w0, r0, n_frames)."""
    F_ = NS * Bn
    aug, lin = image(nw * T * F_), image(nw * Cc)
    kw = dict(sliding=1, w0=sliding[0], r0=sliding[1], n_frames=sliding[2]) if sliding else {}
    run(INFER, {**params(p), 0: img}, [aug, lin], T=T, Bn=Bn, NS=NS, C=Cc, NPROJ=img.shape[-1], lo=lo, hi=hi, alpha=ALPHA, n_windows=nw, **kw)
    return body(aug, (nw, T, F_)), body(lin, (nw, Cc))


def poisoned(proj, F_, Cc, hi=None):
    """NaN where a launch must not read: the padding columns, and (inference, fixed windows) the lin1 columns at t >= hi."""
    x = proj.copy()
    x[..., F_ + Cc:] = np.nan
    if hi is not None:
        x[:, hi:, F_:F_ + Cc] = np.nan
    return x


def train_kw(p, Bn, NS, Cc, nw, T):
    return dict(T=T, Bn=Bn, NS=NS, C=Cc, NPROJ=p["NPROJ"], n_windows=nw, thr=p["thr"], scale=p["scale"], keys=p["keys"])


def train_fwd(proj, p, tm, lv, Bn, NS, Cc):
    nw, T, _ = proj.shape
    F_ = NS * Bn
    Y, aug, lin = image(nw * T * F_), image(nw * T * F_), image(nw * Cc)
    run(TRAIN_FWD, {**params(p), 0: proj, 5: tm, 6: lv}, [Y, aug, lin], **train_kw(p, Bn, NS, Cc, nw, T))
    return body(Y, (nw, T, F_)), body(aug, (nw, T, F_)), body(lin, (nw, Cc))


def train_bwd(Yb, daug, dlin, p, tm, lv, Bn, NS, Cc):
    nw, T, F_ = Yb.shape
    dproj, part = image(nw * T * p["NPROJ"]), image(nw * 3 * F_)
    run(TRAIN_BWD, {0: Yb, 2: p["ln_w"], 5: tm, 6: lv, 7: daug, 8: dlin}, [dproj, part], **train_kw(p, Bn, NS, Cc, nw, T))
    return body(dproj, (nw, T, p["NPROJ"])), body(part, (nw, 3 * F_))


def ident(case):
    return "-".join(str(v) for v in case)


# ---- a. inference, fixed windows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.expand_infer_cases(), ids=ident)
def test_inference_fixed_windows(case):
    Bn, NS, T, Cc, kind, lo, hi, nw = case
    p, ref, E = R.expand_infer_suite_case(case)
    aug, lin = infer(poisoned(p["proj"], NS * Bn, Cc, hi).reshape(nw * T, -1), p, Bn, NS, Cc, lo, hi, nw, T)
    ra, rl = R.ratio(aug, ref[0], E[0]), R.ratio(lin, ref[1], E[1])
    print(f"[expand inference {ident(case)}] err / bound: aug {ra:.3f}, lin_logits {rl:.3f}")
    assert ra <= 1.0 and rl <= 1.0, (case, ra, rl)


# ---- b. inference, sliding windows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sl", R.EXPAND_SLIDING, ids=ident)
def test_inference_sliding_windows(sl):
    """The row map with its clamps at both ends of a clip: against the reference fed the gathered rows, and bit for bit against a
    fixed-window launch on the gathered rows.  Rows of the image no window may read hold NaN."""
    nf, w0, nw = sl
    T, Bn, NS, Cc = 7, 64, 3, 3
    r0, rows, n_img = R.expand_sliding_layout(nf, w0, nw, T)
    p = R.expand_case(1, n_img, Bn, NS, Cc, 40 + nf + w0)
    img = poisoned(p["proj"][0], NS * Bn, Cc)
    lo, hi = R.centre_range("centre3", T)
    ref, E = R.expand_infer_ref(img[rows], ALPHA, p["b_bott"], p["ln_w"], p["ln_b"], p["b_lin1"], Bn, NS, Cc, lo, hi)
    gathered = np.ascontiguousarray(img[rows]).reshape(nw * T, -1)
    unread = np.setdiff1d(np.arange(n_img), rows)
    assert unread.size >= 2
    img[unread] = np.nan
    aug, lin = infer(img, p, Bn, NS, Cc, lo, hi, nw, T, sliding=(w0, r0, nf))
    ra, rl = R.ratio(aug, ref[0], E[0]), R.ratio(lin, ref[1], E[1])
    print(f"[expand sliding {ident(sl)} r0 {r0}] err / bound: aug {ra:.3f}, lin_logits {rl:.3f}")
    assert ra <= 1.0 and rl <= 1.0, (sl, ra, rl)
    aug_f, lin_f = infer(gathered, p, Bn, NS, Cc, lo, hi, nw, T)
    assert same_bits(aug, aug_f) and same_bits(lin, lin_f), ("sliding and fixed-window launches differ on the same rows", sl)


# ---- c. training forward and backward, both storage forms ------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.expand_train_cases(), ids=ident)
def test_training_forward_and_backward(case):
    """Forward: Y and lin_logits bit for bit, aug within the bound.  Backward, fed Y of the float64 forward rounded to fp32 (the two
    launches are judged separately): the lin1 and padding columns of dproj bit for bit, the bottleneck columns and part within
    their bounds.  The resident and the big storage form (both sides of the threshold at Bn = 256, the long window at Bn = 64)
    cannot share a shape, so they meet only through the reference: the bit-for-bit Y and lin_logits checks in both forms are what
    establishes the kernel's "same fma order: same bits" promise for everything it spells as fmaf."""
    Bn, NS, T, Cc, thr, nw = case
    F_ = NS * Bn
    p, tm, lv, fw, Yb, ((dp, part), (Edp, Epart), _) = R.expand_train_suite_case(case)
    Y, aug, lin = train_fwd(poisoned(p["proj"], F_, Cc), p, tm, lv, Bn, NS, Cc)
    assert same_bits(Y, fw["Y"]), ("Y is not the fmaf chain over s, then + bias", case, int((bits(Y) != bits(fw["Y"])).sum()))
    assert same_bits(lin, fw["lin"]), ("lin_logits is not the fmaf chain over lin_vec, then + b_lin1", case)
    rf = R.ratio(aug, fw["aug"], fw["E_aug"])
    dropped = ~fw["keep"].reshape(nw, T, F_)
    g, pt = train_bwd(Yb, p["daug"], p["dlin"], p, tm, lv, Bn, NS, Cc)
    m = Edp > 0
    rb, rp = R.ratio(g[m], dp[m], Edp[m]), R.ratio(pt, part, Epart)
    big = R.expand_is_big(T, Bn, p["NPROJ"])
    print(f"[expand training {ident(case)} {'big' if big else 'resident'}] err / bound: aug {rf:.3f}, dproj {rb:.3f}, part {rp:.3f}; dropped {dropped.mean():.2f}")
    assert rf <= 1.0, ("aug", case, rf)
    assert rb <= 1.0 and rp <= 1.0, ("backward", case, rb, rp)
    assert same_bits(g[:, :, F_:F_ + Cc], dp[:, :, F_:F_ + Cc].astype(F32)), ("dproj's lin1 columns are not the one product lin_vec[s] dlin[w][c]", case)
    assert same_bits(g[:, :, F_ + Cc:], np.zeros((nw, T, p["NPROJ"] - F_ - Cc), F32)), ("dproj's padding columns are not +0", case)


# ---- d. the temporal operators the training kernels are handed ------------------------------------------------------------------
@pytest.mark.parametrize("T", [3, 15, 31, 101])
def test_build_temporal_is_the_reference_rounded_to_fp32(T):
    _lib.require_debug("cbas_debug_build_temporal")
    for alpha in (0.1, 0.3, 0.49):
        for kind in R.RANGE_KINDS:
            lo, hi = R.centre_range(kind, T)
            tm, lv = image(3 * T * T), image(T)
            _lib.check(_lib.load().cbas_debug_build_temporal(T, alpha, lo, hi, tm.ctypes.data, lv.ctypes.data), "cbas_debug_build_temporal")
            E, D, A, l = R.expand_temporal_ref(T, alpha, lo, hi)
            assert same_bits(body(tm, (3, T, T)), np.stack([E, D, A]).astype(F32)), (T, alpha, kind)
            assert same_bits(body(lv, (T,)), l.astype(F32)), (T, alpha, kind)
    lib = _lib.load()
    tm, lv = image(3 * T * T), image(T)
    for bad in ((2, 0, 1), (102, 0, 1), (T, -1, 1), (T, 1, 1), (T, 0, T + 1)):
        assert lib.cbas_debug_build_temporal(bad[0], 0.3, bad[1], bad[2], tm.ctypes.data, lv.ctypes.data) == EINVAL
    assert lib.cbas_debug_build_temporal(T, 0.3, 0, T, None, lv.ctypes.data) == EINVAL and (tm == CANARY).all() and (lv == CANARY).all()


# ---- e. a window is alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bn,NS", [(64, 2), (256, 3)])
def test_a_windows_bits_do_not_depend_on_its_neighbours_and_a_nan_stays_in_its_window(Bn, NS):
    """thr = 0: the dropout index holds the window number, so only then is a window alone the same launch.  NaN in one stream-0
    element of window `bad` at t0: that window's rows of stream 0 from t0 on are NaN (the EMA carries it, LayerNorm spreads it
    over the row), every other row of the launch keeps its bits; likewise a NaN in Y through the backward."""
    T, Cc, nw, one, bad, t0 = 7, 3, 5, 3, 1, 3
    F_ = NS * Bn
    p = R.expand_case(nw, T, Bn, NS, Cc, 77 + Bn)
    lo, hi = R.centre_range("centre3", T)
    E, D, A, l = R.expand_temporal_ref(T, ALPHA, lo, hi)
    tm, lv = np.stack([E, D, A]).astype(F32), l.astype(F32)
    flat = lambda x: x.reshape(-1, x.shape[-1])
    aug, lin = infer(flat(p["proj"]), p, Bn, NS, Cc, lo, hi, nw, T)
    Y, taug, tlin = train_fwd(p["proj"], p, tm, lv, Bn, NS, Cc)
    dproj, part = train_bwd(Y, p["daug"], p["dlin"], p, tm, lv, Bn, NS, Cc)
    for amp in (1.0, 40.0):                                # ... whatever the neighbours hold
        q = (p["proj"] * F32(amp)).astype(F32)
        q[one] = p["proj"][one]
        a5, l5 = infer(flat(q), p, Bn, NS, Cc, lo, hi, nw, T)
        assert same_bits(a5[one], aug[one]) and same_bits(l5[one], lin[one]), ("inference", amp)
        y5, t5, tl5 = train_fwd(q, p, tm, lv, Bn, NS, Cc)
        assert same_bits(y5[one], Y[one]) and same_bits(t5[one], taug[one]) and same_bits(tl5[one], tlin[one]), ("training forward", amp)
    a1, l1 = infer(flat(p["proj"][one:one + 1]), p, Bn, NS, Cc, lo, hi, 1, T)
    y1, t1, tl1 = train_fwd(p["proj"][one:one + 1], p, tm, lv, Bn, NS, Cc)
    d1, p1 = train_bwd(Y[one:one + 1], p["daug"][one:one + 1], p["dlin"][one:one + 1], p, tm, lv, Bn, NS, Cc)
    assert same_bits(a1[0], aug[one]) and same_bits(l1[0], lin[one]), "inference: a window alone"
    assert same_bits(y1[0], Y[one]) and same_bits(t1[0], taug[one]) and same_bits(tl1[0], tlin[one]), "training forward: a window alone"
    assert same_bits(d1[0], dproj[one]) and same_bits(p1[0], part[one]), "training backward: a window alone"
    # NaN
    q = p["proj"].copy()
    q[bad, t0, 5] = np.nan
    others = np.arange(nw) != bad
    for name, got, clean in (("inference", infer(flat(q), p, Bn, NS, Cc, lo, hi, nw, T)[0], aug), ("training forward", train_fwd(q, p, tm, lv, Bn, NS, Cc)[1], taug)):
        assert same_bits(got[others], clean[others]), ("NaN left its window", name)
        hit = np.zeros((T, F_), bool)                      # inference carries the NaN forward from t0; training's matrix form multiplies
        hit[t0 if name == "inference" else 0:, :Bn] = True   # it into every position (0 x NaN), so stream 0's rows are NaN at every t
        assert np.isnan(got[bad][hit]).all(), ("NaN did not show in its rows", name)
        assert same_bits(got[bad][~hit], clean[bad][~hit]), ("NaN spread past its rows", name)
    yq = Y.copy()
    yq[bad, t0, 5] = np.nan
    dq, pq = train_bwd(yq, p["daug"], p["dlin"], p, tm, lv, Bn, NS, Cc)
    assert same_bits(dq[others], dproj[others]) and same_bits(pq[others], part[others]), "backward: NaN left its window"
    assert np.isnan(dq[bad, :, :Bn]).all() and np.isnan(pq[bad, :Bn]).all(), "backward: NaN did not show in its stream's columns"
    assert same_bits(dq[bad, :, Bn:], dproj[bad, :, Bn:]), "backward: NaN spread to other streams' columns"
    print(f"[expand window isolation Bn {Bn} NS {NS}] bit for bit alone, beside scaled neighbours, and beside a NaN window")


# ---- f. refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(word, op, ins, outs, **kw):
    before = [None if o is None else o.copy() for o in outs]
    rc = expand_call(op, ins, outs, **kw)
    msg = (_lib.load().cbas_last_error() or b"").decode(errors="replace")
    assert rc == EINVAL, (op, kw, rc)
    assert word in msg, (word, msg)
    for o, b in zip(outs, before):
        assert o is None or same_bits(o, b), "a refused call touched an output"


def _small(op, Bn=64, NS=2, T=3, Cc=3, nw=2, NP=None):
    """Images and arguments of a served launch of `op`, sized for (Bn, NS, T, C, nw, NPROJ)."""
    F_ = NS * Bn
    NP = R.round_up(F_ + Cc, 4) if NP is None else NP
    z = lambda *s: np.ones(s, F32)
    if op == INFER:
        return {0: z(nw * T, NP), 1: z(F_), 2: z(F_), 3: z(F_), 4: z(Cc)}, [image(nw * T * F_), image(nw * Cc)], \
            dict(T=T, Bn=Bn, NS=NS, C=Cc, NPROJ=NP, lo=0, hi=T, alpha=ALPHA, n_windows=nw)
    kw = dict(T=T, Bn=Bn, NS=NS, C=Cc, NPROJ=NP, n_windows=nw, thr=0, scale=1.0, keys=[1, 2, 3])
    if op == TRAIN_FWD:
        return {0: z(nw, T, NP), 1: z(F_), 2: z(F_), 3: z(F_), 4: z(Cc), 5: z(3, T, T), 6: z(T)}, [image(nw * T * F_), image(nw * T * F_), image(nw * Cc)], kw
    return {0: z(nw, T, F_), 2: z(F_), 5: z(3, T, T), 6: z(T), 7: z(nw, T, F_), 8: z(nw, Cc)}, [image(nw * T * NP), image(nw * 3 * F_)], kw


def test_harness_refuses_what_the_launchers_would_mishandle():
    for op in (INFER, TRAIN_FWD, TRAIN_BWD):
        ins, outs, ok = _small(op)
        for T in (2, 0, 102):
            _refused("T =", op, ins, outs, **dict(ok, T=T, hi=min(T, 3)) if op == INFER else dict(ok, T=T))
        for nw in (0, -1):
            _refused("n_windows", op, ins, outs, **dict(ok, n_windows=nw))
        for Bn in (0, 32, 96, 320):
            _refused("Bn =", op, ins, outs, **dict(ok, Bn=Bn))
        for NS in (1, 4):
            _refused("NS =", op, ins, outs, **dict(ok, NS=NS))
        for Cc in (0, 65):
            _refused("C =", op, ins, outs, **dict(ok, C=Cc))
        for NP in (128, 130, 133, 134):                    # below NS Bn + C = 131; not a multiple of 4
            _refused("NPROJ", op, ins, outs, **dict(ok, NPROJ=NP))
        for i in ins:
            _refused("NULL", op, {**ins, i: None}, outs, **ok)
            _refused("too small", op, ins, outs, in_bytes={i: ins[i].nbytes - 4}, **ok)
        for i in range(len(outs)):
            _refused("NULL", op, ins, [None if j == i else o for j, o in enumerate(outs)], **ok)
            _refused("too small", op, ins, outs, out_bytes={i: outs[i].nbytes - 4 * TAIL - 4}, **ok)
        _refused("struct_bytes", op, ins, outs, struct_bytes=8, **ok)
        if op != INFER:
            _refused("thr", op, ins, outs, **dict(ok, thr=1 << 24))
            i2, o2, k2 = _small(op, Bn=256, NS=3, T=53, Cc=4, nw=1)          # the big form itself: 53 x (3 x 256 + 12) floats
            _refused("LDS", op, i2, o2, **k2)
    ins, outs, ok = _small(INFER)
    _refused("op", 3, ins, outs, **ok)
    _refused("op", -1, ins, outs, **ok)
    for lo, hi in ((-1, 2), (2, 2), (2, 1), (0, 4)):
        _refused("lo", INFER, ins, outs, **dict(ok, lo=lo, hi=hi))
    i2, o2, k2 = _small(INFER, Bn=256, NS=3, T=54, Cc=4, nw=1)
    _refused("LDS", INFER, i2, o2, **k2)
    i2, o2, k2 = _small(TRAIN_BWD, NP=264)                 # 136 columns past NS Bn = 128 for a block of 128 threads
    _refused("NPROJ", TRAIN_BWD, i2, o2, **k2)
    # sliding: the image holds rows 0 .. 5; four windows of T = 7 from w0 read frames w0 - 3 .. w0 + 6
    sl = dict(ok, sliding=1, T=7, lo=0, hi=7, n_windows=4)
    outs7 = [image(4 * 7 * 128), image(4 * 3)]
    _refused("n_frames", INFER, ins, outs7, **dict(sl, w0=0, r0=0, n_frames=0))
    _refused("sliding", INFER, ins, outs7, **dict(sl, w0=0, r0=0, n_frames=7))           # the last window reads row 6
    _refused("sliding", INFER, ins, outs7, **dict(sl, w0=10, r0=8, n_frames=40))         # rows -1 .. 7
    _refused("sliding", INFER, ins, outs7, **dict(sl, w0=10, r0=2, n_frames=40))         # rows 5 .. 13
    _refused("sliding", INFER, ins, outs7, **dict(sl, w0=0, r0=1, n_frames=6))           # row -1
    _refused("sliding", INFER, {**ins, 0: None}, outs7, **dict(sl, w0=0, r0=0, n_frames=6))
    _refused("sliding", INFER, ins, outs7, in_bytes={0: ins[0].nbytes - 4}, **dict(sl, w0=0, r0=0, n_frames=6))
    assert _lib.load().cbas_debug_head_expand_run(None) == EINVAL


def test_the_served_neighbours_of_the_refusals_pass():
    """The limits themselves are served: T = 3 and T = 101, C = 64, Bn = 256 at the longest windows whose LDS fits (inference
    T = 53, training's big form T = 52), NPROJ - NS Bn equal to the backward's block, the sliding image that ends exactly at
    the last row read, and thr = 2^24 - 1 (nothing is kept here: every aug row is ln_b, bit for bit)."""
    worst = 0.0
    for (Bn, NS, T, Cc, nw) in ((64, 2, 3, 64, 1), (64, 3, 101, 1, 1), (256, 3, 53, 4, 1)):
        p = R.expand_case(nw, T, Bn, NS, Cc, T + Cc)
        ref, E = R.expand_infer_ref(p["proj"], ALPHA, p["b_bott"], p["ln_w"], p["ln_b"], p["b_lin1"], Bn, NS, Cc, T - 1, T)
        aug, lin = infer(poisoned(p["proj"], NS * Bn, Cc).reshape(nw * T, -1), p, Bn, NS, Cc, T - 1, T, nw, T)
        worst = max(worst, R.ratio(aug, ref[0], E[0]), R.ratio(lin, ref[1], E[1]))
    # sliding, the image ending at the last row read: n_frames 6, rows 0 .. 5
    p = R.expand_case(1, 6, 64, 2, 3, 5)
    rows = R.expand_rows(3, 7, True, 0, 0, 6)
    ref, E = R.expand_infer_ref(p["proj"][0][rows], ALPHA, p["b_bott"], p["ln_w"], p["ln_b"], p["b_lin1"], 64, 2, 3, 0, 7)
    aug, lin = infer(p["proj"][0], p, 64, 2, 3, 0, 7, 3, 7, sliding=(0, 0, 6))
    worst = max(worst, R.ratio(aug, ref[0], E[0]), R.ratio(lin, ref[1], E[1]))
    # training: the longest big-form window at Bn = 256, thr = 2^24 - 1
    Bn, NS, T, Cc, nw = 256, 3, 52, 4, 1
    assert R.expand_lds_bytes(T, Bn, 772, True, True) <= 160 * 1024 < R.expand_lds_bytes(T + 1, Bn, 772, True, True)
    p = R.expand_case(nw, T, Bn, NS, Cc, 52, (1 << 24) - 1)
    p["scale"] = 2.0
    lo, hi = R.centre_range("centre3", T)
    E_, D, A, l = R.expand_temporal_ref(T, ALPHA, lo, hi)
    tm, lv = np.stack([E_, D, A]).astype(F32), l.astype(F32)
    fw = R.expand_train_fwd_ref(p["proj"], tm, lv, p["b_bott"], p["ln_w"], p["ln_b"], p["b_lin1"], Bn, NS, Cc, p["keys"], p["thr"], p["scale"])
    Y, aug, lin = train_fwd(poisoned(p["proj"], NS * Bn, Cc), p, tm, lv, Bn, NS, Cc)
    assert same_bits(Y, fw["Y"]) and same_bits(lin, fw["lin"])
    gone = ~fw["keep"].reshape(nw, T, NS, Bn).any(-1)
    assert gone.sum() >= gone.size - NS                    # all but the three threshold elements' rows
    assert same_bits(aug.reshape(nw, T, NS, Bn)[gone], np.broadcast_to(p["ln_b"].reshape(NS, Bn), (nw, T, NS, Bn))[gone]), "a row with nothing kept is not ln_b"
    # backward: NPROJ - NS Bn equal to the block (128 threads write 128 columns past the bottleneck's)
    Bn, NS, T, Cc, nw, NP = 64, 2, 3, 64, 1, 256
    p = R.expand_case(nw, T, Bn, NS, Cc, 9)
    p["NPROJ"] = NP
    E_, D, A, l = R.expand_temporal_ref(T, ALPHA, 0, T)
    tm, lv = np.stack([E_, D, A]).astype(F32), l.astype(F32)
    Yb = (p["daug"] * F32(0.5)).astype(F32)
    (dp, part), (Edp, Epart), _ = R.expand_train_bwd_ref(Yb, p["daug"], p["dlin"], tm, lv, p["ln_w"], Bn, NS, Cc, NP, p["keys"], 0, 1.0)
    g, pt = train_bwd(Yb, p["daug"], p["dlin"], p, tm, lv, Bn, NS, Cc)
    m = Edp > 0
    worst = max(worst, R.ratio(g[m], dp[m], Edp[m]), R.ratio(pt, part, Epart))
    assert same_bits(g[~m], dp[~m].astype(F32))
    assert worst <= 1.0, worst
    print(f"[expand served limits] max err / bound {worst:.3f}")
