"""The run-scan, median, winner, bin and top-1 kernels at their wave, tile and grid seams: every case of tests/scan_seam_cases.py
through the public calls (``labels_median``, ``label_runs``, ``disagreement_runs``, ``activity_bins_device``, ``probs_top1``)
against its closed-form expectation, exactly - records field by field as bytes, confidences as float64 bit patterns - and a second
call gives the same bytes.  tests/test_scan_seams_host.py pins the same expectations to the numpy routines without a GPU.

What each test reaches that the fixtures of test_gpu_postprocess.py and test_gpu_disagreement.py do not:
  test_many_clips / test_many_instances   runs_scan_kernel's ``before`` (counts of the waves below, entry 64 onwards) and ``carry``
                                          (the steps before, entry 256 onwards)
  test_many_records                       label_runs_reduce_kernel's stride over its 4096 x 4 waves (record 16 384 onwards)
  test_median_table / test_median_alone   labels_median_kernel's ``tile += gridDim.y`` (frame 65 536 onwards), the 8-frame
                                          segments and the 1024-frame tiles
  test_winner_over_64_classes             runs_reduce_kernel's key (count, 255 - name rank, lane) on lanes up to 63
  test_comb_* / test_walks_*              the ballot ranks of walk_clip / walk_instance on every lane and tile phase
"""
import ctypes as C

import numpy as np
import pytest
import torch

import scan_seam_cases as S
from cbas_amd import _lib, postprocess as P, train as T

pytestmark = pytest.mark.gpu

EINVAL = -1
SENTINEL = -77                                         # no median: the values are -1 .. 63
CANARY = 16


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def seam_of(i):
    return f"{i} (>= 64: {i >= 64}, >= 256: {i >= 256})"


def assert_records(got, want, owner, what):
    """Field by field as bytes.  The first wrong record is named with the clip or instance it belongs to and the one whose record
    was found in its place, each with whether it lies behind the first wave (>= 64) or the first step (>= 256) of the offset scan:
    an entry whose offset is wrong writes over the records of an earlier one."""
    assert got.dtype == want.dtype
    n = min(len(got), len(want))
    for field in want.dtype.names:
        g, w = np.ascontiguousarray(got[field][:n]), np.ascontiguousarray(want[field][:n])
        if g.tobytes() != w.tobytes():
            k = int(np.flatnonzero(bits(g) != bits(w))[0]) if g.dtype == np.float64 else int(np.flatnonzero(g != w)[0])
            pytest.fail(f"{what}: record {k} differs in {field}: got {got[k]}, expected {want[k]}; it belongs to {owner} "
                        f"{seam_of(int(want[owner][k]))}, found there: a record of {owner} {seam_of(int(got[owner][k]))}")
    if len(got) != len(want):
        i = int(want[owner][n]) if n < len(want) else int(got[owner][n])
        pytest.fail(f"{what}: {len(got)} records, expected {len(want)}; the first missing or surplus one belongs to {owner} {seam_of(i)}")


def run_label_case(case):
    key, conf = dev(case.key), dev(case.conf)
    got = P.label_runs(key, conf, case.table, case.n_classes, case.threshold)
    assert_records(got, case.records, "clip", case.name)
    again = P.label_runs(key, conf, case.table, case.n_classes, case.threshold)
    assert got.tobytes() == again.tobytes(), case.name
    return key, conf


def run_runs_case(case):
    pred, conf = dev(case.pred), dev(case.conf)
    i = case.inst
    got = T.disagreement_runs(pred, conf, case.table, i[:, 0], i[:, 1], i[:, 2], i[:, 3], case.rank)
    assert_records(got, case.records, "instance", case.name)
    again = T.disagreement_runs(pred, conf, case.table, i[:, 0], i[:, 1], i[:, 2], i[:, 3], case.rank)
    assert got.tobytes() == again.tobytes(), case.name


def count_query(case, key, conf):
    """cbas_label_runs with capacity 0: refused for want of room, ``needed`` = the number of records."""
    needed = C.c_int64(-5)
    table = dev(case.table)
    rc = _lib.load().cbas_label_runs(key.data_ptr(), conf.data_ptr(), int(key.shape[0]), table.data_ptr(), int(case.table.shape[0]),
                                     case.n_classes, 0 if case.threshold is None else 1,
                                     0.0 if case.threshold is None else float(case.threshold), None, 0, C.byref(needed), None)
    assert rc == (EINVAL if len(case.records) else 0), case.name
    return needed.value


# ---------------------------------------------------------------------------------------------------------------
# the walks
# ---------------------------------------------------------------------------------------------------------------
SEAM_CASES = ["comb", "comb_threshold_all_pass", "comb_threshold_none_pass", "comb_shifted", "seams", "seams_threshold_all_pass",
              "dips_threshold", "dips_no_threshold"]


@pytest.fixture(scope="module")
def seam_cases():
    cases = {c.name.split("[")[0]: c for c in S.comb_cases() + S.dip_cases()}
    assert sorted(cases) == sorted(SEAM_CASES)
    return cases


@pytest.mark.parametrize("name", SEAM_CASES)
def test_comb_and_seam_boundaries_of_label_runs(seam_cases, name):
    run_label_case(seam_cases[name])


def test_walks_of_the_disagreement_scan_on_the_comb_and_the_seams():
    run_runs_case(S.walk_instances_case())


# ---------------------------------------------------------------------------------------------------------------
# the offset scan
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.MANY_N)
def test_many_clips_land_on_their_prefix_sums(n):
    case = S.many_clips_case(n)
    key, conf = run_label_case(case)
    assert count_query(case, key, conf) == int(case.counts.sum()) == len(case.records)


@pytest.mark.parametrize("n", S.MANY_N)
def test_many_instances_land_on_their_prefix_sums(n):
    run_runs_case(S.many_instances_case(n))


# ---------------------------------------------------------------------------------------------------------------
# the reduce pass over more records than its grid has waves
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_records():
    return {c.name: c for c in S.many_records_cases()}


@pytest.mark.parametrize("name", ["many_records", "many_records_threshold", "many_records_five_clips"])
def test_many_records_keep_their_confidence_past_one_sweep_of_the_grid(many_records, name):
    case = many_records[name]
    assert len(case.records) > 16384
    key, conf = run_label_case(case)
    assert count_query(case, key, conf) == len(case.records)


# ---------------------------------------------------------------------------------------------------------------
# the winner
# ---------------------------------------------------------------------------------------------------------------
def test_winner_over_64_classes_is_the_smallest_rank_among_the_largest_counts():
    case = S.winner_case()
    assert case.n_classes == 64 and len(case.rank) == 64
    run_runs_case(case)


# ---------------------------------------------------------------------------------------------------------------
# the median
# ---------------------------------------------------------------------------------------------------------------
def median_with_canary(flat, table, n_classes, ksize):
    """cbas_labels_median into a buffer 16 values longer than the frames, filled with a value no median is."""
    lib = _lib.load()
    pred, tab = dev(flat), dev(table)
    out = torch.full((flat.size + CANARY,), SENTINEL, dtype=torch.int32, device="cuda")
    rc = lib.cbas_labels_median(pred.data_ptr(), int(flat.size), tab.data_ptr(), int(table.shape[0]), n_classes, ksize, out.data_ptr(), None)
    assert rc == 0, lib.cbas_last_error()
    got = out.cpu().numpy()
    assert (got[flat.size:] == SENTINEL).all(), "the median wrote past the frames"
    public = P.labels_median(pred, table, n_classes, ksize).cpu().numpy()
    for base, n in table.tolist():
        assert public[base:base + n].tobytes() == got[base:base + n].tobytes()
    return got[:flat.size]


@pytest.fixture(scope="module", params=[2, 64])
def median_case(request):
    n_classes = request.param
    flat, table, parts = S.median_table_case(n_classes)
    expected = {}

    def want(clip, ksize):                             # computed once per (clip, kernel size), shared by the tests of this C
        if (clip, ksize) not in expected:
            expected[clip, ksize] = S.median_expected(parts[clip][0], ksize, n_classes)
        return expected[clip, ksize]
    return n_classes, flat, table, parts, want


@pytest.mark.parametrize("ksize", S.MEDIAN_KSIZES)
def test_median_table_of_all_clip_lengths(median_case, ksize):
    n_classes, flat, table, parts, want = median_case
    got = median_with_canary(flat, table, n_classes, ksize)
    covered = np.zeros(flat.size, bool)
    for c, (base, n) in enumerate(table.tolist()):
        w = want(c, ksize)
        bad = np.flatnonzero(got[base:base + n] != w)
        assert bad.size == 0, (f"C={n_classes} k={ksize}: clip {c} of {n} frames differs at frame {bad[0]} (tile {bad[0] // 1024}, "
                               f"segment {bad[0] % 1024 // 8}): got {got[base + bad[0]]}, expected {w[bad[0]]}")
        covered[base:base + n] = True
    assert (~covered).sum() == S.MEDIAN_GAP and (got[~covered] == SENTINEL).all()       # frames of no clip are not written
    assert got.tobytes() == median_with_canary(flat, table, n_classes, ksize).tobytes()


def test_median_of_every_clip_alone(median_case):
    n_classes, flat, table, parts, want = median_case
    for c, (x, _block) in enumerate(parts):
        n = x.size
        for ksize in S.MEDIAN_KSIZES + ((S.MEDIAN_WIDE[1],) if n == S.MEDIAN_WIDE[0] else ()):
            got = median_with_canary(x, np.array([[0, n]], np.int64), n_classes, ksize)
            w = want(c, ksize) if ksize in S.MEDIAN_KSIZES else S.median_expected(x, ksize, n_classes)
            bad = np.flatnonzero(got != w)
            assert bad.size == 0, (f"C={n_classes} k={ksize}: the clip of {n} frames alone differs at frame {bad[0]} "
                                   f"(tile {bad[0] // 1024}): got {got[bad[0]]}, expected {w[bad[0]]}")


# ---------------------------------------------------------------------------------------------------------------
# the bins and the top-1
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.BIN_N)
def test_bins_with_edges_on_and_beside_the_wave_edge(n):
    probs = dev(S.bins_rows(n))
    for bin_frames in S.bin_frames_of(n):
        want = S.bins_expected(n, bin_frames)
        got = P.activity_bins_device(probs, S.BIN_BEHAVIOR, S.BIN_THRESHOLD, bin_frames)
        assert got.dtype == torch.int64 and tuple(got.shape) == (len(want),) == (-(-n // bin_frames),)
        assert got.cpu().numpy().tobytes() == want.tobytes(), (n, bin_frames, got.cpu().tolist(), want.tolist())
        again = P.activity_bins_device(probs, S.BIN_BEHAVIOR, S.BIN_THRESHOLD, bin_frames)
        assert again.cpu().numpy().tobytes() == want.tobytes(), (n, bin_frames)


@pytest.mark.parametrize("n", S.TOP1_N)
def test_top1_of_64_classes_around_one_workgroup(n):
    p, want_pred, want_conf = S.top1_rows(n)
    pred, conf, flags = T.probs_top1(dev(p))
    assert int(flags.item()) == T.TOP1_FLAG_NAN
    assert pred.cpu().numpy().tobytes() == want_pred.tobytes()
    got = conf.cpu().numpy()
    nan = np.isnan(want_conf)
    assert np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want_conf[~nan].tobytes()
    pred2, conf2, _ = T.probs_top1(dev(p))
    assert pred2.cpu().numpy().tobytes() == pred.cpu().numpy().tobytes() and conf2.cpu().numpy().tobytes() == got.tobytes()
