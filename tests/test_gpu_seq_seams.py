"""cbasx_viterbi_scores / cbasx_viterbi_decode (csrc/seq_viterbi.hip) and cbasx_hmm_posteriors (csrc/seq_hmm.hip) at their
seams: every case of tests/seq_seam_cases.py through the raw entry points.  The Viterbi results are integers and must equal the
serial numpy definition bit for bit; forward-backward is held to the per-case bars of test_gpu_hmm.py - with e32 the error of
``bouts.posteriors_host(dtype=np.float32)`` against float64 on the case, ``4 e32 + 2^-23`` for gamma in absolute terms, for Xi
relative to its largest entry and for loglik relative to its magnitude - and never to a figure taken from the device.
tests/test_seq_seams_host.py pins the same cases to the package's numpy routines without a GPU.

What each test reaches that the fixtures of test_gpu_bouts.py and test_gpu_hmm.py (C = 1, 2, 9, 33, 64 = widths 2, 16 and 64; at
most 3 pieces a clip; 7 clips; 328 640 scores; clip scores above -2^24) do not:
  test_viterbi_widths / test_hmm_widths     vt_launch / hm_launch at C <= 4, C <= 8 and C <= 32: vt_transfer_kernel,
                                            vt_forward_kernel, hm_transfer_kernel, hm_forward_kernel and hm_backward_kernel<*, true
                                            and false> of widths 4 (C = 3, 4), 8 (C = 5, 8) and 32 (C = 17, 32), each with all of
                                            its registers live (C == CP) and with CP / 2 - 1 of them masked (C == CP / 2 + 1);
                                            width 16 at C == CP = 16
  test_viterbi_long_clips                   vt_compose_kernel with L = 1 and all 16 segments full (17 pieces), L = 2 with a last
                                            segment of one map and seven empty segments (18 pieces: ``lo = max(hi - L + 1, 1)``
                                            clamps, ``pieces - 1 - g * L >= 1`` fails), L = 3 (34 pieces); vt_scan_kernel's
                                            matrix product 15, 16 and 32 times in a row; at C = 64 vt_backmap_kernel and
                                            vt_emit_kernel stage exactly 64 KB
  test_hmm_long_clips                       both branches of hm_scan_kernel over 15 to 33 products in a row, each renormalised;
                                            hm_reduce_kernel's inner sum over up to 34 partials
  test_viterbi_score_range                  the high words of vt_scan_kernel's two ``readlane`` halves and of t_off, vbase, acc
                                            and clip_score: clip scores of about -5.4e9 and +5.4e9, positive transitions included
  test_viterbi_grid_stride                  the second trip of vt_scores_kernel's and vt_check_kernel's loops, element 524 288
                                            onwards: scores, the NaN flag and the refusal of a score out of range
  test_viterbi_many_clips / test_hmm_many_clips
                                            vt_find / hm_find over 300 entries of ``offsets`` and ``loffsets`` with runs of ties
                                            (clips of no frame; in ``loffsets`` every clip of one piece), clips of several pieces
                                            around entries 64 and 256 of the offset scan, hm_reduce_kernel's loglik and Pi over
                                            300 clips
  test_hmm_posterior_flag                   CBASX_HMM_FLAG_POSTERIOR from hm_backward_kernel: the NaN rows, and hm_backward_step's
                                            promise that such a step counts nothing in Xi
"""
import numpy as np
import pytest
import torch

import hmm_ref as H
import seq_seam_cases as S
import viterbi_ref as V
from test_gpu_bouts import raw_decode
from test_gpu_hmm import SENTINEL, bars, raw

from cbas_amd import bouts

pytestmark = pytest.mark.gpu
P = S.P


def first_wrong(got, want, table):
    """The first frame whose label differs, its clip, and its piece k of the clip's pieces."""
    f = int(np.flatnonzero(got != want)[0])
    where = "in no clip"
    for c, (first, n) in enumerate(table):
        if first <= f < first + n:
            where = f"clip {c} = ({first}, {n}), piece {(f - first) // P} of {S.pieces_of(n)}, frame {f - first} of the clip"
    return f"{int((got != want).sum())} labels differ, the first at frame {f}: got {got[f]}, expected {want[f]}; {where}"


def decode_and_compare(case, alone=False):
    labels, clip_score = raw_decode(case.scores, case.table, case.A, case.prior)
    got, got_score = labels.cpu().numpy(), clip_score.cpu().numpy()
    assert got.dtype == np.int32 and got_score.dtype == np.int64
    if not np.array_equal(got, case.labels):
        pytest.fail(f"{case.name}: " + first_wrong(got, case.labels, case.table))
    wrong = np.flatnonzero(got_score != case.clip_score)
    assert wrong.size == 0, (case.name, "clip", int(wrong[0]), case.table[wrong[0]].tolist(), int(got_score[wrong[0]]), int(case.clip_score[wrong[0]]))
    owned = S.owned_rows(case.table, case.scores.shape[0])
    assert (got[~owned] == -1).all() and (got[owned] >= 0).all() and (got_score[case.table[:, 1] == 0] == 0).all()
    again, again_score = raw_decode(case.scores, case.table, case.A, case.prior)
    assert torch.equal(again, labels) and torch.equal(again_score, clip_score)
    if alone:
        for c, (first, n) in enumerate(case.table):
            if S.pieces_of(n) > 1:
                one, one_score = raw_decode(case.scores[first:first + n], [(0, n)], case.A, case.prior)      # alone, and at another place
                assert torch.equal(one, labels[first:first + n]), (case.name, c, n)
                assert int(one_score[0]) == int(clip_score[c])
    return got, got_score


@pytest.mark.parametrize("regime", S.REGIMES)
@pytest.mark.parametrize("C", S.WIDTH_CLASSES)
def test_viterbi_widths(C, regime):
    decode_and_compare(S.viterbi_width(C, regime))


@pytest.mark.parametrize("regime", S.REGIMES)
@pytest.mark.parametrize("C,shape", S.LONG_SHAPES)
def test_viterbi_long_clips(C, shape, regime):
    case = S.viterbi_long(C, shape, regime)
    assert [S.pieces_of(n) for n in case.table[:, 1]] == ([17, 18, 34] if shape == "three" else [18])
    decode_and_compare(case, alone=shape == "three")


@pytest.mark.parametrize("variant", S.RANGE_VARIANTS)
def test_viterbi_score_range(variant):
    case = S.viterbi_range(variant)
    _, score = decode_and_compare(case)
    assert abs(int(score[0])) > 1 << 32


@pytest.mark.parametrize("regime", S.REGIMES)
def test_viterbi_many_clips(regime):
    case = S.viterbi_many(regime)
    got, score = decode_and_compare(case, alone=True)
    empty = case.table[:, 1] == 0
    assert empty.sum() >= 60 and (score[empty] == 0).all() and (score[~empty] != 0).any()
    assert (got[~S.owned_rows(case.table, got.size)] == -1).all()


def device_scores(probs):
    scores, flags = bouts.device_scores(torch.from_numpy(probs).cuda())
    return scores.cpu().numpy(), int(flags.item())


def test_viterbi_grid_stride():
    stride = S.viterbi_stride()
    case = stride.decode
    N, C = stride.probs.shape
    grid, last = S.STRIDE_GRID, N * C - 1
    assert last > grid
    got, flag = device_scores(stride.probs)
    diff = np.abs(got.astype(np.int64) - case.scores)
    print(f"scores over {got.size} elements: max |device - float64| = {int(diff.max())}, differing {int((diff > 0).sum())}, "
          f"of them behind element {grid}: {int((diff.reshape(-1)[grid:] > 0).sum())}")
    assert flag == 0 and diff.max() <= 1, np.flatnonzero(diff.reshape(-1) > 1)[:8]
    assert np.array_equal(got.reshape(-1)[stride.planted], case.scores.reshape(-1)[stride.planted])
    for at in (last, grid):
        bad = stride.probs.copy()
        bad.reshape(-1)[at] = np.nan
        nan_got, nan_flag = device_scores(bad)
        assert nan_flag == bouts.FLAG_NAN, at
        assert nan_got.reshape(-1)[at] == V.SCORE_MIN and np.array_equal(np.delete(nan_got.reshape(-1), at), np.delete(got.reshape(-1), at))
    decode_and_compare(case)
    # a score out of range behind the first trip is refused, also in a frame of no clip, and nothing is written
    too_high, too_low = case.scores.copy(), case.scores.copy()
    too_high.reshape(-1)[grid] = 1
    too_low.reshape(-1)[last] = V.SCORE_MIN - 1
    assert not S.owned_rows(case.table, N)[last // C]
    for scores in (too_high, too_low):
        labels = torch.full((N,), 77, dtype=torch.int32, device="cuda:0")
        clip_score = torch.full((len(case.table),), 77, dtype=torch.int64, device="cuda:0")
        with pytest.raises(RuntimeError, match="cbasx_viterbi_decode"):
            raw_decode(scores, case.table, case.A, case.prior, labels=labels, clip_score=clip_score)
        torch.cuda.synchronize()
        assert bool((labels == 77).all()) and bool((clip_score == 77).all())


# ---- forward-backward ---------------------------------------------------------------------------------------------------------------
def posteriors_and_compare(key, alone=False):
    case = S.hmm_case(key)
    probs, table, A, prior, ref = case.probs, case.table, case.A, case.prior, case.ref
    r32 = S.restatement(key)
    assert r32[4] == 0
    gamma, xi, pi, loglik, flags = raw(probs, table, A, prior)
    g, x, p, ll = (v.cpu().numpy() for v in (gamma, xi, pi, loglik))
    assert int(flags.item()) == 0
    # frames outside every clip are rows of zeros; a clip of no frame has loglik 0
    owned = S.owned_rows(table, probs.shape[0])
    assert (g[~owned] == 0).all() and (ll[table[:, 1] == 0] == 0.0).all() and np.isfinite(g).all()
    # the bars, measured on the case by the float32 restatement
    bar = bars(ref, r32[:4])
    xi_top, mag = max(ref[1].max(), 1e-300), np.abs(ref[3])
    with np.errstate(divide="ignore", invalid="ignore"):
        ll_err = np.where(mag > 0, np.abs(ll - ref[3]) / mag, np.where(ll == ref[3], 0.0, np.inf)).max()
    err = {"gamma": np.abs(g.astype(np.float64) - ref[0]).max(), "xi": np.abs(x - ref[1]).max() / xi_top, "loglik": ll_err}
    print(f"hmm {case.name}: " + " ".join(f"{k} e32={bar[k][0]:.3g} device={err[k]:.3g} bar={bar[k][1]:.3g}" for k in err)
          + f" pi={np.abs(p - ref[2]).max():.3g}")
    for k in err:
        if not err[k] <= bar[k][1]:
            where = ""
            if k == "gamma":
                f = int(np.abs(g.astype(np.float64) - ref[0]).max(axis=1).argmax())
                c = int(np.flatnonzero((table[:, 0] <= f) & (f < table.sum(axis=1)))[0])
                where = f"; worst at frame {f}, clip {c} = {table[c].tolist()}, piece {(f - table[c, 0]) // P} of {S.pieces_of(table[c, 1])}"
            pytest.fail(f"{case.name}: {k} is off by {err[k]:.3g}, the bar is {bar[k][1]:.3g} (e32 = {bar[k][0]:.3g}){where}")
    assert np.abs(p - ref[2]).max() <= len(table) * bar["gamma"][1]               # Pi is a sum of gamma rows, one per clip
    # the identities of the definition, on the device output
    T = int(table[:, 1].sum())
    rows, total, occupancy, first = H.identities(g, x, p, table)
    assert rows <= 1e-5 and total <= 1e-5 * T and occupancy <= 1e-5 * T and first <= 1e-5 * len(table), (rows, total, occupancy, first)
    # two calls agree bit for bit, and gamma does not depend on which sums are asked for
    again = raw(probs, table, A, prior)
    assert all(torch.equal(u, v) for u, v in zip(again[:4], (gamma, xi, pi, loglik)))
    spare = (torch.empty_like(gamma), torch.full_like(xi, SENTINEL), torch.full_like(pi, SENTINEL), torch.full_like(loglik, SENTINEL))
    only = raw(probs, table, A, prior, outputs=spare, null=("xi", "pi", "loglik"))
    assert torch.equal(only[0], gamma) and all(bool((v == SENTINEL).all()) for v in spare[1:])
    if alone:
        for c, (first, n) in enumerate(table):
            if S.pieces_of(n) > 1:
                one, _, _, one_ll, _ = raw(probs[first:first + n], [(0, n)], A, prior)          # alone, and at another place
                assert torch.equal(one, gamma[first:first + n]), (case.name, c, n)
                assert torch.equal(one_ll[0], loglik[c])


@pytest.mark.parametrize("inputs,kind", S.WIDTH_HMM)
@pytest.mark.parametrize("C", S.WIDTH_CLASSES)
def test_hmm_widths(C, inputs, kind):
    posteriors_and_compare(("width", C, inputs, kind))


@pytest.mark.parametrize("inputs,kind", S.LONG_HMM)
@pytest.mark.parametrize("C,shape", S.LONG_SHAPES)
def test_hmm_long_clips(C, shape, inputs, kind):
    posteriors_and_compare(("long", C, shape, inputs, kind), alone=shape == "three")


@pytest.mark.parametrize("inputs,kind", S.MANY_HMM)
def test_hmm_many_clips(inputs, kind):
    posteriors_and_compare(("many", inputs, kind), alone=True)


def test_hmm_posterior_flag():
    probs, table, A, prior, clean, clean_table = S.posterior_flag_case()
    host = bouts.posteriors_host(probs, table, A, prior)
    r32 = bouts.posteriors_host(probs, table, A, prior, dtype=np.float32)
    assert host[4] == bouts.FLAG_POSTERIOR and np.isfinite(host[1]).all() and host[1].max() > 0
    gamma, xi, _, loglik, flags = raw(probs, table, A, prior)
    base = raw(clean, clean_table, A, prior)
    assert int(base[4].item()) == 0 and int(flags.item()) & bouts.FLAG_POSTERIOR and int(flags.item()) == bouts.FLAG_POSTERIOR
    g, x = gamma.cpu().numpy(), xi.cpu().numpy()
    nan_rows = np.flatnonzero(np.isnan(g).any(axis=1))
    assert nan_rows.tolist() == np.flatnonzero(np.isnan(host[0]).any(axis=1)).tolist() == [40, 41] and np.isnan(g[40:42]).all()
    # the clips beside it are what they are without it, bit for bit
    assert torch.equal(gamma[:40], base[0][:40]) and torch.equal(gamma[42:], base[0][40:])
    assert torch.equal(loglik[0], base[3][0]) and torch.equal(loglik[2], base[3][1])
    # the step without a posterior counts nothing in Xi
    top = host[1].max()
    e32 = np.abs(r32[1] - host[1]).max() / top
    err = np.abs(x - host[1]).max() / top
    print(f"hmm posterior flag: xi e32={e32:.3g} device={err:.3g} bar={4 * e32 + 2.0 ** -23:.3g}")
    assert np.isfinite(x).all() and err <= 4 * e32 + 2.0 ** -23
    assert torch.equal(xi, base[1])                                                # and so Xi is the two ordinary clips'
