"""Inputs for the Viterbi decode (csrc/seq_viterbi.hip) and the forward-backward pass (csrc/seq_hmm.hip) that sit on the seams
the fixtures of test_gpu_bouts.py and test_gpu_hmm.py leave unrun - the register widths 4, 8 and 32, clips of 17, 18 and 34
pieces, clip scores beyond 2^32, more than 2048 x 256 scores, 300 clips in one table - each with the result it must give.

Every input is built from tests/viterbi_ref.py, tests/hmm_ref.py and numpy alone, seeded per case, and is read-only; the
expectation is the serial numpy definition of those two files, computed once per case (``lru_cache``).  The float32 restatement
of a forward-backward case (``restatement``), which the device's bars are measured with, is ``bouts.posteriors_host``.
tests/test_seq_seams_host.py pins cases and references to the package's numpy routines without a GPU;
tests/test_gpu_seq_seams.py holds the kernels to them.

The many-clips table has 300 entries.  Its first and its last entry are clips of no frame, so the clips of more than one piece
stand at entries 3, 63, 64, 65, 255, 256, 257 and 298: entry 299 cannot be both."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_ref as H  # noqa: E402
import viterbi_ref as V  # noqa: E402

from cbas_amd import bouts  # noqa: E402

assert bouts.CHUNK == bouts.HMM_CHUNK
P = bouts.CHUNK

# scores (N, C) int32, table (n_clips, 2) int64, A (C, C) int32, prior (C,) int32; labels / clip_score: V.viterbi_ref of them
ViterbiCase = namedtuple("ViterbiCase", "name scores table A prior labels clip_score")
# probs (N, C) float32, A (C, C) float32, prior (C,) float32; ref: H.posteriors_ref of them = (gamma, Xi, Pi, loglik) in float64
HmmCase = namedtuple("HmmCase", "name probs table A prior ref")

WIDTH_CLASSES = [3, 4, 5, 8, 16, 17, 32]              # register widths 4, 4, 8, 8, 16, 32, 32: C == CP and C == CP / 2 + 1
REGIMES = ["random", "ties"]
WIDTH_HMM = [("softmax", "sticky"), ("one_hot", "forbidden"), ("uniform", "positive")]
LONG_FRAMES = [16 * P + 1, 17 * P + 1, 33 * P + 1]    # 17, 18 and 34 pieces: pieces - 1 = 16 (L = 1, no empty segment), L = 2, L = 3
LONG_HMM = [("uniform", "sticky"), ("softmax", "forbidden"), ("one_hot", "positive")]
LONG_SHAPES = [(3, "three"), (9, "three"), (64, "eighteen")]      # the 18-piece clip alone at C = 64: 64 KB of back-pointers a piece
RANGE_VARIANTS = ["low", "high", "mixed"]
RANGE_FRAMES, RANGE_CLASSES = 5 * P + 1, 3
STRIDE_FRAMES, STRIDE_CLASSES = 8197, 64
STRIDE_GRID = 2048 * 256                               # threads of one trip of vt_scores_kernel / vt_check_kernel
assert STRIDE_FRAMES * STRIDE_CLASSES == 524608 and STRIDE_FRAMES * STRIDE_CLASSES > STRIDE_GRID
STRIDE_PLANTED = 300                                   # the last elements of the probabilities are exact powers of two
MANY_ENTRIES, MANY_CLASSES = 300, 5
MANY_LONG = {3: 2 * P + 3, 63: P + 1, 64: 2 * P + 3, 65: P + 1, 255: 2 * P + 3, 256: P + 1, 257: 2 * P + 3, 298: P + 1}
MANY_HMM = [("softmax", "sticky"), ("one_hot", "forbidden")]


def frozen(*arrays):
    for x in arrays:
        if x is not None:
            x.setflags(write=False)


# ---- tables -----------------------------------------------------------------------------------------------------------------------
def width_layout():
    """The layout of test_gpu_bouts.py / test_gpu_hmm.py: clips of 1, 2, P-1, P, P+1 and 2P+3 frames back to back, a clip of no
    frame and a gap of 5 unowned frames behind the second, 3 unowned frames at the end."""
    table, at = [], 0
    for i, n in enumerate([1, 2, P - 1, P, P + 1, 2 * P + 3]):
        table.append((at, n))
        at += n
        if i == 1:
            table.append((at, 0))
            at += 5
    return np.array(table, np.int64), at + 3


def long_layout(shape):
    """"three": the clips of 17, 18 and 34 pieces back to back with a gap of 5 frames between the first two; "eighteen": the
    clip of 18 pieces alone."""
    if shape == "eighteen":
        return np.array([(0, LONG_FRAMES[1])], np.int64), LONG_FRAMES[1]
    a, b, c = LONG_FRAMES
    return np.array([(0, a), (a + 5, b), (a + 5 + b, c)], np.int64), a + 5 + b + c


def stride_layout():
    """A clip of 2P frames, then clips of 1 .. 40 frames back to back up to frame 8193, and 3 frames owned by no clip: flat
    element 2048 * 256 is column 0 of frame 8192, inside the last short clip; the last element lies in the tail."""
    table, at, i = [(0, 2 * P)], 2 * P, 0
    end = STRIDE_FRAMES - 3
    while at < end:
        n = min(1 + (i * 7) % 40, end - at)
        table.append((at, n))
        at += n
        i += 1
    table = np.array(table, np.int64)
    assert table[-1].sum() == end and table[-1, 0] <= STRIDE_GRID // STRIDE_CLASSES < end
    return table, STRIDE_FRAMES


@functools.lru_cache(maxsize=None)
def many_layout():
    """300 entries: clips of no frame (the first entry, the last, and runs of two to four in a row), clips of 1 .. 40 frames, gaps
    of 1 .. 6 unowned frames, and MANY_LONG."""
    rng = np.random.default_rng(300)
    kind = rng.random(MANY_ENTRIES)
    run = 0
    table, at = [], 0
    for i in range(MANY_ENTRIES):
        if i in MANY_LONG:
            n, run = MANY_LONG[i], 0
        elif i in (0, MANY_ENTRIES - 1) or run > 0 or kind[i] < 0.12:
            n = 0
            run = run - 1 if run > 0 else (int(rng.integers(1, 4)) if kind[i] < 0.06 else 0)
        else:
            n = int(rng.integers(1, 41))
        table.append((at, n))
        at += n
        if kind[i] > 0.8:
            at += int(rng.integers(1, 7))
    table = np.array(table, np.int64)
    table.setflags(write=False)
    return table, at + 2


def owned_rows(table, N):
    owned = np.zeros(N, bool)
    for first, n in table:
        owned[first:first + n] = True
    return owned


def pieces_of(n):
    return -(-int(n) // P)


# ---- Viterbi ------------------------------------------------------------------------------------------------------------------------
def _viterbi_case(name, table, N, C, regime, seed):
    rng = np.random.default_rng(seed)
    if regime == "random":
        scores, A, prior = rng.integers(-8192, 1, size=(N, C)), rng.integers(-3000, 1, size=(C, C)), rng.integers(-3000, 1, size=C)
    else:
        assert regime == "ties"
        scores, A, prior = rng.integers(-2, 1, size=(N, C)), rng.integers(-2, 1, size=(C, C)), rng.integers(-2, 1, size=C)
    scores, A, prior = scores.astype(np.int32), A.astype(np.int32), prior.astype(np.int32)
    labels, clip_score = V.viterbi_ref(scores, table, A, prior)
    frozen(scores, table, A, prior, labels, clip_score)
    return ViterbiCase(name, scores, table, A, prior, labels, clip_score)


@functools.lru_cache(maxsize=None)
def viterbi_width(C, regime):
    table, N = width_layout()
    return _viterbi_case(f"width C={C} {regime}", table, N, C, regime, 7000 + 10 * C + REGIMES.index(regime))


@functools.lru_cache(maxsize=None)
def viterbi_long(C, shape, regime):
    table, N = long_layout(shape)
    return _viterbi_case(f"long C={C} {shape} {regime}", table, N, C, regime, 8000 + 10 * C + REGIMES.index(regime))


@functools.lru_cache(maxsize=None)
def viterbi_many(regime):
    table, N = many_layout()
    return _viterbi_case(f"many clips {regime}", table, N, MANY_CLASSES, regime, 9000 + REGIMES.index(regime))


@functools.lru_cache(maxsize=None)
def viterbi_range(variant):
    """One clip of 5P + 1 frames whose transitions and prior lie at the documented limits: every step costs or earns about 2^20,
    so the clip score leaves 32 bits."""
    rng = np.random.default_rng(9100 + RANGE_VARIANTS.index(variant))
    C, N, top = RANGE_CLASSES, RANGE_FRAMES, V.TRANS_LIMIT
    low = lambda size: rng.integers(-top, -top + 3001, size=size)          # noqa: E731
    high = lambda size: rng.integers(top - 3000, top + 1, size=size)       # noqa: E731
    if variant == "low":
        A, prior = low((C, C)), low(C)
    elif variant == "high":
        A, prior = high((C, C)), high(C)
    else:
        # i -> i + 1 (mod C) earns about 2^20, staying and every other move cost as much: the best path changes its state at
        # every frame, so its score is positive and beyond 2^32 while most candidates of every step lie far below zero
        pick = (np.arange(C)[None, :] - np.arange(C)[:, None]) % C == 1
        A, prior = np.where(pick, high((C, C)), low((C, C))), np.where([True, False, True], high(C), low(C))
    scores = rng.integers(-8192, 1, size=(N, C)).astype(np.int32)
    A, prior = A.astype(np.int32), prior.astype(np.int32)
    table = np.array([(0, N)], np.int64)
    labels, clip_score = V.viterbi_ref(scores, table, A, prior)
    assert abs(int(clip_score[0])) > 1 << 32, (variant, clip_score)
    assert variant == "mixed" or (clip_score[0] < 0) == (variant == "low")
    assert A.min() >= -top and A.max() <= top and (variant != "mixed" or (A.min() < 0 < A.max()))
    frozen(scores, table, A, prior, labels, clip_score)
    return ViterbiCase(f"score range {variant}", scores, table, A, prior, labels, clip_score)


StrideCase = namedtuple("StrideCase", "probs planted decode")          # planted: the flat indices that hold exact powers of two


@functools.lru_cache(maxsize=None)
def viterbi_stride():
    """524 608 probabilities for ``cbasx_viterbi_scores`` - softmax rows, the last 300 elements overwritten with 2^0 .. 2^-40 -
    and their float64 scores as the input of the decode."""
    rng = np.random.default_rng(9200)
    N, C = STRIDE_FRAMES, STRIDE_CLASSES
    table, _ = stride_layout()
    probs = H.make_probs("softmax", N, C, rng)
    planted = np.arange(N * C - STRIDE_PLANTED, N * C)
    probs.reshape(-1)[planted] = np.exp2(-(np.arange(STRIDE_PLANTED) % 41).astype(np.float64)).astype(np.float32)
    scores = V.scores_ref(probs)
    assert scores.reshape(-1)[planted].tolist() == [max(-256 * (k % 41), -8192) for k in range(STRIDE_PLANTED)]
    A, prior = rng.integers(-3000, 1, size=(C, C)).astype(np.int32), rng.integers(-3000, 1, size=C).astype(np.int32)
    labels, clip_score = V.viterbi_ref(scores, table, A, prior)
    frozen(probs, planted, scores, table, A, prior, labels, clip_score)
    return StrideCase(probs, planted, ViterbiCase("grid stride", scores, table, A, prior, labels, clip_score))


def viterbi_cases():
    """Every Viterbi case, for the host test."""
    out = [viterbi_width(C, r) for C in WIDTH_CLASSES for r in REGIMES]
    out += [viterbi_long(C, shape, r) for C, shape in LONG_SHAPES for r in REGIMES]
    out += [viterbi_range(v) for v in RANGE_VARIANTS] + [viterbi_stride().decode] + [viterbi_many(r) for r in REGIMES]
    return out


# ---- forward-backward ---------------------------------------------------------------------------------------------------------------
def _hmm_case(name, table, N, C, inputs, kind, seed):
    rng = np.random.default_rng(seed)
    probs, A = H.make_probs(inputs, N, C, rng), H.make_transitions(kind, C, rng)
    prior = rng.dirichlet(np.ones(C)).astype(np.float32)
    prior = (prior / prior.sum()).astype(np.float32)
    ref = H.posteriors_ref(probs, table, A, prior)
    frozen(probs, table, A, prior, *ref)
    return HmmCase(name, probs, table, A, prior, ref)


def _seed(base, C, inputs, kind):
    return base + 100 * C + 10 * H.INPUTS.index(inputs) + H.TRANSITIONS.index(kind)


@functools.lru_cache(maxsize=None)
def hmm_width(C, inputs, kind):
    table, N = width_layout()
    return _hmm_case(f"width C={C} {inputs} {kind}", table, N, C, inputs, kind, _seed(10000, C, inputs, kind))


@functools.lru_cache(maxsize=None)
def hmm_long(C, shape, inputs, kind):
    table, N = long_layout(shape)
    return _hmm_case(f"long C={C} {shape} {inputs} {kind}", table, N, C, inputs, kind, _seed(20000, C, inputs, kind))


@functools.lru_cache(maxsize=None)
def hmm_many(inputs, kind):
    table, N = many_layout()
    return _hmm_case(f"many clips {inputs} {kind}", table, N, MANY_CLASSES, inputs, kind, _seed(30000, MANY_CLASSES, inputs, kind))


HMM_KEYS = ([("width", C, i, k) for C in WIDTH_CLASSES for i, k in WIDTH_HMM]
            + [("long", C, shape, i, k) for C, shape in LONG_SHAPES for i, k in LONG_HMM] + [("many", i, k) for i, k in MANY_HMM])


def hmm_case(key):
    return {"width": hmm_width, "long": hmm_long, "many": hmm_many}[key[0]](*key[1:])


@functools.lru_cache(maxsize=None)
def restatement(key):
    """``bouts.posteriors_host(dtype=np.float32)`` of a case: ``(gamma, Xi, Pi, loglik, flags)``."""
    case = hmm_case(key)
    out = bouts.posteriors_host(case.probs, case.table, case.A, case.prior, dtype=np.float32)
    frozen(*out[:4])
    return out


@functools.lru_cache(maxsize=None)
def posterior_flag_case():
    """C = 2 under ``A = eye(2)``: an ordinary clip of 40 frames, the clip ``[[1, 0], [inf, inf]]`` - its second frame has no
    finite alpha, so neither frame has a posterior - and an ordinary clip of P + 9 frames.  ``(probs, table, A, prior, the same
    without the middle clip: probs, table)``.  Under the identity a clip never leaves its state, so alpha_t is the likelihood
    ratio of the frames before t and beta_t that of the frames after: the ordinary rows stay within 0.45 .. 0.55, where neither
    ratio leaves float32 over P + 9 frames and every frame keeps a posterior."""
    rng = np.random.default_rng(9300)

    def rows(n):
        x = rng.uniform(0.45, 0.55, size=(n, 1))
        return np.concatenate([x, 1.0 - x], axis=1).astype(np.float32)

    first, last = rows(40), rows(P + 9)
    middle = np.array([[1.0, 0.0], [np.inf, np.inf]], np.float32)
    probs, clean = np.concatenate([first, middle, last]), np.concatenate([first, last])
    table, clean_table = np.array([(0, 40), (40, 2), (42, P + 9)], np.int64), np.array([(0, 40), (40, P + 9)], np.int64)
    A, prior = np.eye(2, dtype=np.float32), np.array([0.5, 0.5], np.float32)
    frozen(probs, clean, table, clean_table, A, prior)
    return probs, table, A, prior, clean, clean_table
