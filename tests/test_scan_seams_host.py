"""The seam cases of tests/scan_seam_cases.py without a GPU: every closed-form expectation equals what the package's numpy
routines (``median_host``, ``label_runs_host``, ``disagreement_runs_host``, ``activity_bins_host``, ``top1_host``) compute on the
same input - records identical, confidences bit for bit - and, where scipy is there and the kernel size is at most 31, the median
equals ``scipy.signal.medfilt``; and the cases hold the phases they were built for.  A wrong builder or a wrong host routine
fails here, before anything runs on a GPU."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scan_seam_cases as S  # noqa: E402

from cbas_amd import postprocess as P, train as T  # noqa: E402

try:
    from scipy.signal import medfilt
except ImportError:
    medfilt = None


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def assert_label_case_equals_host(case):
    want = [(c, a, b, k, m) for c, (base, n) in enumerate(case.table.tolist())
            for a, b, k, m in P.label_runs_host(case.key[base:base + n], case.conf[base:base + n], case.threshold)]
    got = case.records
    assert [tuple(r)[:4] for r in got.tolist()] == [w[:4] for w in want], case.name
    assert np.array_equal(bits(got["confidence"]), bits([w[4] for w in want])), case.name
    assert np.array_equal(np.bincount(got["clip"], minlength=len(case.table)), case.counts), case.name
    assert case.conf.dtype == np.float32 and case.conf.min() >= np.float32(1.0 / 64) and case.conf.max() <= 1.0


def assert_runs_case_equals_host(case):
    want = []
    for i, (c, s, e, label) in enumerate(case.inst.tolist()):
        base, n = case.table[c].tolist()
        want += [(i,) + r for r in T.disagreement_runs_host(case.pred[base:base + n], case.conf[base:base + n], s, e, label, case.rank)]
    got = case.records
    assert [tuple(r)[:4] for r in got.tolist()] == [w[:4] for w in want], case.name
    assert np.array_equal(bits(got["model_confidence"]), bits([w[4] for w in want])), case.name
    assert np.array_equal(np.bincount(got["instance"], minlength=len(case.inst)), case.counts), case.name
    assert case.conf.min() >= np.float32(1.0 / 64) and case.conf.max() <= 1.0


def test_record_layouts_are_the_packages():
    assert S.LABEL_RUN_DTYPE == P.LABEL_RUN_DTYPE and S.RUN_DTYPE == T.RUN_DTYPE


def test_comb_holds_every_lane_and_wave_phase_and_equals_the_host_routine():
    cases = S.comb_cases()
    comb = cases[0]
    assert comb.key.size == 4 * 67 * 68 // 2 + 300 and len(comb.records) > 4 * 67
    starts, ends = comb.records["start_frame"], comb.records["end_frame"]
    lengths = (ends - starts + 1).tolist()
    assert lengths[:67 * 4] == list(range(1, 68)) * 4 and ends[-1] == comb.key.size - 1 and starts[0] == 0
    shifted = cases[3]
    assert shifted.table[:, 1].tolist() == [comb.key.size + p for p in S.COMB_SHIFTS]
    for field in ("start_frame", "end_frame"):
        frames = np.concatenate([comb.records[field], shifted.records[field]])
        assert set((frames % 256).tolist()) == set(range(256))                     # every frame of a tile, so every lane of a wave
        assert {63, 64, 255, 0} <= set((comb.records[field] % 256).tolist())       # the comb alone: both sides of both seams
    gaps = starts[1:] - ends[:-1] - 1                                              # alternately nothing and one frame
    assert gaps.tolist() == [0, 1] * (len(gaps) // 2) + [0] * (len(gaps) % 2)
    assert len(cases[2].records) == 0
    for case in cases:
        assert_label_case_equals_host(case)


def test_seam_variants_put_their_boundaries_where_they_say():
    seams = {k: S.segment_runs(v) for k, v in S.SEAM_SEGMENTS.items()}
    assert [r[:2] for r in seams["change_on_seams"]] == [(0, 63), (64, 255), (256, 555)]
    assert [r[:2] for r in seams["gap_on_63_and_255"]] == [(1, 62), (64, 254), (256, 355)]
    assert [r[:2] for r in seams["gap_on_64_and_256"]] == [(0, 63), (65, 255), (257, 306)]
    assert [r[:2] for r in seams["single_frames_on_seams"]] == [(0, 0), (63, 63), (64, 64), (255, 255), (256, 256), (266, 266)]
    assert sum(n for n, _ in S.SEAM_SEGMENTS["single_frames_on_seams"]) == 267
    runs = seams["no_boundary_in_a_wave_or_tile"]
    assert (60, 139, 3) in runs and (151, 850, 2) in runs                          # wave 1, and the tile 256 .. 511, hold no boundary
    edges = {f for a, b, _ in runs for f in (a, b)}
    assert not any(64 <= f <= 127 or 256 <= f <= 511 for f in edges)
    assert any(f < 64 for f in edges) and any(128 <= f < 192 for f in edges)


def test_dips_split_the_run_only_with_the_threshold():
    with_threshold, without = S.dip_cases()
    first = with_threshold.records[with_threshold.records["clip"] == 0]
    assert [tuple(r)[1:3] for r in first.tolist()] == [(0, 62), (65, 254), (257, 699)]
    assert [tuple(r)[1:3] for r in without.records.tolist()] == [(0, 699)] * len(S.DIP_FRAMES)
    assert_label_case_equals_host(with_threshold)
    assert (without.conf == np.float32(0.25)).sum() == sum(len(d) for d in S.DIP_FRAMES.values())
    base = [(c, a, b, k, m) for c, (b0, n) in enumerate(without.table.tolist())
            for a, b, k, m in P.label_runs_host(without.key[b0:b0 + n], without.conf[b0:b0 + n], None)]
    assert [tuple(r)[:4] for r in without.records.tolist()] == [w[:4] for w in base]
    assert np.array_equal(bits(without.records["confidence"]), bits([w[4] for w in base]))


@pytest.mark.parametrize("n", S.MANY_N)
def test_many_clips_and_instances_have_the_stated_counts_and_equal_the_host_routines(n):
    clips = S.many_clips_case(n)
    assert clips.counts.tolist() == [(i * 7) % 5 for i in range(n)] and len(clips.records) == clips.counts.sum()
    assert clips.table[0].tolist() == [0, 0] and (clips.table[:, 1] <= 40).all() and clips.table[:, 1].max() == 40
    assert_label_case_equals_host(clips)
    inst = S.many_instances_case(n)
    assert inst.counts.tolist() == [(i * 7) % 5 for i in range(n)] and len(inst.records) == inst.counts.sum()
    lengths = inst.table[inst.inst[:, 0], 1]
    assert (inst.inst[:, 1] >= lengths).any() and (inst.inst[:, 2] >= lengths).any() and (inst.inst[:, 3] == -1).any()
    assert len(inst.table) == 4
    assert_runs_case_equals_host(inst)


def test_many_records_pass_two_sweeps_of_the_reduce_grid():
    plain, dipped, five = S.many_records_cases()
    assert len(plain.records) == 40000 > 2 * 16384 and len(dipped.records) == 26666 > 16384 and len(five.records) == 40020
    f = np.arange(40000)
    assert np.array_equal(plain.records["start_frame"], f) and np.array_equal(plain.records["end_frame"], f)
    assert np.array_equal(plain.records["label"], f % 2) and np.array_equal(bits(plain.records["confidence"]), bits(plain.conf))
    assert five.counts.tolist() == [10, 7001, 20000, 12999, 10]
    for case in (plain, dipped, five):
        assert_label_case_equals_host(case)


def test_walks_of_the_disagreement_scan_on_the_comb_equal_the_host_routine():
    case = S.walk_instances_case()
    assert len(case.records) > 300 and (case.inst[:, 1] > 0).any()
    assert_runs_case_equals_host(case)


def test_winner_cases_equal_the_host_routine():
    case = S.winner_case()
    rank = case.rank
    assert rank[[5, 40, 63, 62, 1]].tolist() == [61, 11, 32, 0, 63]
    assert [int(r["model_prediction"]) for r in case.records] == [w for _n, _c, _k, w in S.WINNER_RUNS]
    assert case.records["end_frame"][2] - case.records["start_frame"][2] + 1 == 64
    assert_runs_case_equals_host(case)


@pytest.mark.parametrize("n_classes", [2, 64])
def test_median_expectations_equal_the_host_routine_and_scipy(n_classes):
    flat, table, parts = S.median_table_case(n_classes)
    assert table[:, 1].tolist() == list(S.MEDIAN_CLIPS) and flat.size == sum(S.MEDIAN_CLIPS) + S.MEDIAN_GAP
    assert table[S.MEDIAN_GAP_AFTER + 1, 0] - table[S.MEDIAN_GAP_AFTER].sum() == S.MEDIAN_GAP
    long_x, long_block = parts[-1]
    assert long_block[65535] != long_block[65536] and long_block[66559] != long_block[66560] and table[-2, 1] == 3
    for (base, n), (x, block) in zip(table.tolist(), parts):
        assert np.array_equal(flat[base:base + n], x) and x.min() >= -1 and x.max() <= n_classes - 1
        for k in S.MEDIAN_KSIZES + ((S.MEDIAN_WIDE[1],) if n == S.MEDIAN_WIDE[0] else ()):
            want = S.median_expected(x, k, n_classes)
            assert np.array_equal(want, P.median_host(x, k)), (n_classes, n, k)
            inside = S.median_interior(n, k)
            assert np.array_equal(want[inside], block[inside]), (n_classes, n, k)                 # the closed form of the pattern
            if k == 1:
                assert np.array_equal(want, x)
            if (k + 1) // 2 <= k - n:                                                            # more padding than half a window
                assert not want.any()
            if medfilt is not None and k <= 31:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", UserWarning)
                    assert np.array_equal(medfilt(x.astype(np.int64), kernel_size=k), want), (n_classes, n, k)
    assert S.median_interior(S.MEDIAN_LONG, 301).sum() > 20000 and (long_x != long_block).sum() > 1000
    # the padding pulls: within k // 2 frames of a clip's ends, and wherever a kernel wider than the clip meets it, the median
    # leaves the block's value
    x, block = parts[5]
    assert (S.median_expected(x, 2001, n_classes) != block).any()
    ends = np.r_[0:150, 1025 - 150:1025]
    assert (S.median_expected(x, 301, n_classes)[ends] != block[ends]).any()


def test_bins_and_top1_expectations_equal_the_host_routines():
    for n in S.BIN_N:
        p = S.bins_rows(n)
        for bin_frames in S.bin_frames_of(n):
            want = S.bins_expected(n, bin_frames)
            assert np.array_equal(want, P.activity_bins_host(p, S.BIN_BEHAVIOR, S.BIN_THRESHOLD, bin_frames)), (n, bin_frames)
        assert S.bins_expected(n, n).tolist() == [len([f for f in range(0, n, 3) if f not in (60, 255, 63, 192)])]
    for n in S.TOP1_N:
        p, pred, conf = S.top1_rows(n)
        clean = ~np.isnan(p).any(axis=1)
        assert (~clean).sum() == sum(t < n for t in S.TOP1_NAN_ROWS) and (pred[~clean] == -1).all() and np.isnan(conf[~clean]).all()
        host_pred, host_conf = P.top1_host(p)
        assert np.array_equal(host_pred[clean], pred[clean]) and np.array_equal(host_conf[clean], conf[clean].astype(np.float64))
        assert np.array_equal(p[clean].argmax(axis=1), pred[clean]) and (pred[1:][clean[1:]] != pred[:-1][clean[1:]]).all()
