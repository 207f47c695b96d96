"""The cases of tests/seq_seam_cases.py against the package's numpy routines, without a GPU: ``bouts.viterbi_host`` equals
``viterbi_ref`` bit for bit and ``bouts.posteriors_host`` in float64 agrees with ``posteriors_ref`` within the bars of
tests/test_hmm_host.py, so two independent statements of each definition stand behind every expectation before
tests/test_gpu_seq_seams.py holds a kernel to it.  Also the conditions that keep the device's bars meaningful: the float32
restatement's error ``e32`` is at most 1e-5 on every case, so the bar ``4 e32 + 2^-23`` stays three orders below the 1e-2 of a
wrong seam; its flags are 0; the many-clips table has the ties the offset searches must step over; the score-range cases leave
32 bits."""
import numpy as np
import pytest

import seq_seam_cases as S
from cbas_amd import bouts

VITERBI_CASES = S.viterbi_cases
P = S.P


def viterbi_ids():
    ids = [f"width-{C}-{r}" for C in S.WIDTH_CLASSES for r in S.REGIMES]
    ids += [f"long-{C}-{shape}-{r}" for C, shape in S.LONG_SHAPES for r in S.REGIMES]
    return ids + [f"range-{v}" for v in S.RANGE_VARIANTS] + ["stride"] + [f"many-{r}" for r in S.REGIMES]


@pytest.mark.parametrize("i", range(len(viterbi_ids())), ids=viterbi_ids())
def test_viterbi_host_equals_the_reference(i):
    case = VITERBI_CASES()[i]
    labels, clip_score = bouts.viterbi_host(case.scores, case.table, case.A, case.prior)
    assert labels.dtype == np.int32 and clip_score.dtype == np.int64
    assert np.array_equal(labels, case.labels), (case.name, np.flatnonzero(labels != case.labels)[:8])
    assert np.array_equal(clip_score, case.clip_score), case.name
    owned = S.owned_rows(case.table, case.scores.shape[0])
    assert (case.labels[~owned] == -1).all() and (case.labels[owned] >= 0).all()
    assert (case.clip_score[case.table[:, 1] == 0] == 0).all()


def test_the_score_range_cases_leave_32_bits():
    got = {v: int(S.viterbi_range(v).clip_score[0]) for v in S.RANGE_VARIANTS}
    print("score range:", got)
    assert got["low"] < -(1 << 32) and got["high"] > 1 << 32 and abs(got["mixed"]) > 1 << 32
    for v in S.RANGE_VARIANTS:
        case = S.viterbi_range(v)
        assert case.scores.shape == (5 * P + 1, 3) and np.abs(case.A).max() <= 1 << 20 and np.abs(case.prior).max() <= 1 << 20
        assert np.abs(case.A).min() >= (1 << 20) - 3000 and case.scores.min() >= -8192 and case.scores.max() <= 0
    mixed = S.viterbi_range("mixed")
    assert (mixed.A < 0).any() and (mixed.A > 0).any() and (mixed.prior < 0).any() and (mixed.prior > 0).any()


def test_the_grid_stride_case_takes_a_second_trip():
    stride = S.viterbi_stride()
    case = stride.decode
    N, C = stride.probs.shape
    assert N * C == 524608 > S.STRIDE_GRID and case.scores.shape == (N, C)
    assert np.array_equal(bouts.scores_host(stride.probs), case.scores)
    owned = S.owned_rows(case.table, N)
    assert case.table[0, 1] == 2 * P and len(case.table) > 100 and not owned[-3:].any() and owned[:-3].all()
    assert owned[S.STRIDE_GRID // C]                                               # element 2048 * 256 lies in a clip
    assert stride.planted.size == 300 and stride.planted[-1] == N * C - 1
    mant = np.frexp(stride.probs.reshape(-1)[stride.planted].astype(np.float64))[0]
    assert (mant == 0.5).all()                                                     # exact powers of two


def test_the_many_clips_table_has_its_ties():
    table, N = S.many_layout()
    pieces = np.array([S.pieces_of(n) for n in table[:, 1]])
    empty = table[:, 1] == 0
    print(f"many clips: {len(table)} entries, {int(empty.sum())} of no frame, {int((pieces > 1).sum())} of more than one piece, "
          f"{int(table[:, 1].sum())} owned of {N} frames")
    assert len(table) == 300 and empty.sum() >= 60 and (pieces > 1).sum() >= 8 and empty[0] and empty[-1]
    assert sorted(np.flatnonzero(pieces > 1).tolist()) == sorted(S.MANY_LONG)
    runs = np.flatnonzero(empty[:-2] & empty[1:-1] & empty[2:])
    assert runs.size >= 1                                                          # three clips of no frame in a row
    assert (table[1:, 0] >= table[:-1].sum(axis=1)).all() and (table[1:, 0] > table[:-1].sum(axis=1)).any()      # in order, with gaps
    short = table[(pieces == 1), 1]
    assert short.min() == 1 and short.max() == 40 and table[-1].sum() < N


@pytest.mark.parametrize("key", S.HMM_KEYS, ids=lambda k: "-".join(str(x) for x in k))
def test_posteriors_host_equals_the_reference_and_the_restatement_is_close(key):
    case = S.hmm_case(key)
    want = case.ref
    gamma, Xi, Pi, loglik, flags = bouts.posteriors_host(case.probs, case.table, case.A, case.prior)
    assert flags == 0 and gamma.dtype == np.float64
    assert np.abs(gamma - want[0]).max() <= 1e-11
    assert np.abs(Xi - want[1]).max() <= 1e-10 * max(1.0, want[1].max()) and np.abs(Pi - want[2]).max() <= 1e-11
    assert np.abs(loglik - want[3]).max() <= 1e-10 * max(1.0, np.abs(want[3]).max())
    assert (loglik[case.table[:, 1] == 0] == 0.0).all() and (gamma[~S.owned_rows(case.table, len(gamma))] == 0).all()
    # the float32 restatement: what the device's bars are measured with
    g32, x32, _, l32, f32 = S.restatement(key)
    mag = np.abs(want[3])
    e32 = {"gamma": np.abs(g32.astype(np.float64) - want[0]).max(), "xi": np.abs(x32 - want[1]).max() / want[1].max(),
           "loglik": (np.abs(l32 - want[3])[mag > 0] / mag[mag > 0]).max()}
    print(f"hmm {case.name}: " + " ".join(f"{k} e32={v:.3g}" for k, v in e32.items()))
    assert f32 == 0 and g32.dtype == np.float32 and (l32[mag == 0] == 0).all()
    for k, v in e32.items():
        assert v <= 1e-5, (k, v)


def test_the_posterior_flag_case_on_the_host():
    probs, table, A, prior, clean, clean_table = S.posterior_flag_case()
    gamma, Xi, Pi, loglik, flags = bouts.posteriors_host(probs, table, A, prior)
    want = bouts.posteriors_host(clean, clean_table, A, prior)
    assert flags == bouts.FLAG_POSTERIOR and want[4] == 0
    assert np.flatnonzero(np.isnan(gamma).any(axis=1)).tolist() == [40, 41] and np.isnan(gamma[40:42]).all()
    assert np.array_equal(gamma[:40], want[0][:40]) and np.array_equal(gamma[42:], want[0][40:])
    assert np.array_equal(loglik[[0, 2]], want[3])
    # a step without a posterior counts nothing
    assert np.isfinite(Xi).all() and np.array_equal(Xi, want[1])
