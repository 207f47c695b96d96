"""Events, pre-labels and actogram bins without a GPU: the numpy routines of cbas_amd.postprocess against what the reference's
own methods returned for the same CSV files (tests/golden/postprocess.npz, made by tests/golden/make_goldens_postprocess.py),
the numpy median against scipy, the library surface of the three entry points, file ordering and bin-size edge cases."""
import ctypes as C
import fnmatch
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import postprocess_cases as PC  # noqa: E402

from cbas_amd import _lib, pipeline as PL, postprocess as P  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "postprocess.npz"))
REL = 2.0 ** -24           # the CSV holds the shortest decimal of each float32: DESIGN.md "Events, pre-labels and actogram bins"


@pytest.fixture(autouse=True)
def host_only(monkeypatch):
    monkeypatch.setattr(P, "_gpu", lambda: False)


def golden(key):
    return json.loads(str(GOLDEN[key]))


@pytest.mark.parametrize("seed,n,n_classes,threshold", PC.EVENT_CASES)
def test_events_equal_the_references(seed, n, n_classes, threshold, tmp_path):
    p = PC.probabilities(seed, n, n_classes)
    assert PC.clear_of(p, threshold)
    video = f"ev{seed}.mp4"
    want = golden(f"events/{seed}")
    assert P.predictions_to_instances(p, PC.names(n_classes), video, threshold) == want
    path = str(tmp_path / f"ev{seed}_{PC.MODEL}_outputs.csv")
    PL.write_probs_csv(path, p, PC.names(n_classes))
    got = P.predictions_to_instances(path, PC.names(n_classes), str(tmp_path / video), threshold, project_path=str(tmp_path))
    assert got == want and [list(g) for g in got] == [["video", "start", "label", "end"]] * len(got)


@pytest.mark.parametrize("seed,n,n_classes,window", PC.BLOCK_CASES)
def test_blocks_equal_the_references(seed, n, n_classes, window, tmp_path):
    p = PC.probabilities(seed, n, n_classes)
    want = golden(f"blocks/{seed}")
    path = str(tmp_path / f"bl{seed}_{PC.MODEL}_outputs.csv")
    PL.write_probs_csv(path, p, PC.names(n_classes))
    for source in (p, path):
        got, df = P.predictions_to_instances_with_confidence(source, PC.names(n_classes), str(tmp_path / f"bl{seed}.mp4"),
                                                             smoothing_window=window, project_path=str(tmp_path))
        assert [{k: v for k, v in g.items() if k != "confidence"} for g in got] == \
               [{k: v for k, v in w.items() if k != "confidence"} for w in want]
        for g, w in zip(got, want):
            assert abs(g["confidence"] - w["confidence"]) <= REL * w["confidence"], (g, w)
        assert list(df.columns) == golden(f"blocks/{seed}/columns") and len(df) == n
        assert np.array_equal(df["block_start"].to_numpy(), GOLDEN[f"blocks/{seed}/block_start"])
        if window > 1:
            assert df["smoothed_index"].dtype == np.int64
            assert np.array_equal(df["smoothed_index"].to_numpy(), GOLDEN[f"blocks/{seed}/smoothed_index"])
            assert np.array_equal(df["predicted_index"].to_numpy(), p.argmax(axis=1))
        top = p.max(axis=1).astype(np.float64)                 # from the file: the decimals, within 2^-24 of the float32 values
        assert np.all(np.abs(df["max_prob"].to_numpy() - top) <= (REL * top if source is path else 0.0))


def test_a_missing_file_and_a_missing_column(tmp_path):
    assert P.predictions_to_instances(str(tmp_path / "none.csv"), ["a"], "v.mp4") == []
    assert P.predictions_to_instances_with_confidence(str(tmp_path / "none.csv"), ["a"], "v.mp4") == ([], None)
    path = str(tmp_path / "x_m_outputs.csv")
    PL.write_probs_csv(path, PC.probabilities(1, 10, 2), ["a", "b"])
    assert P.predictions_to_instances(path, ["a", "c"], "v.mp4") == []
    got, df = P.predictions_to_instances_with_confidence(path, ["a", "c"], "v.mp4")
    assert got == [] and list(df.columns) == ["a", "b"] and len(df) == 10
    assert P.predictions_to_instances(path, [], "v.mp4") == []


def test_median_is_scipys():
    medfilt = pytest.importorskip("scipy.signal").medfilt
    rng = np.random.default_rng(7)
    for n in (1, 2, 5, 64, 300):
        for k in (1, 3, 7, 31, 601):
            for n_classes in (1, 9, 64):
                x = rng.integers(-1, n_classes, n)
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", UserWarning)          # "kernel_size exceeds volume extent"
                    want = medfilt(x, kernel_size=k)
                got = P.median_host(x, k)
                assert got.dtype == np.int64 and want.dtype == np.int64 and np.array_equal(got, want), (n, k, n_classes)
    ones = np.full(20, 3)
    assert list(P.median_host(ones, 5)) == [3] * 20                       # two padding zeros never outvote three frames
    assert list(P.median_host(ones, 41)) == [0] * 20                      # 21 of the 41 values of every window are padding
    assert list(P.median_host(np.array([3, 1, 3, 3, 1, 3]), 3)) == [1, 3, 3, 3, 3, 1]     # (0, 3, 1) and (1, 3, 0): the ends move towards 0
    with pytest.raises(ValueError):
        P.median_host(ones, 4)


def test_run_mean_is_the_mean():
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 1000):
        x = rng.uniform(1 / 64, 1, n).astype(np.float32)
        assert P.run_mean(x) == float(np.cumsum(x.astype(np.float64))[-1] / n)       # exact partial sums: any order gives these bits


def test_label_runs_host_state_machine():
    key = np.array([0, 0, 1, 1, 1, -1, 2, 2, 0])
    conf = np.array([.9, .8, .9, .4, .9, .9, .9, .9, .9], np.float32)
    assert [r[:3] for r in P.label_runs_host(key, conf)] == [(0, 1, 0), (2, 4, 1), (6, 7, 2), (8, 8, 0)]
    # the label changes at frame 2 with the probability above the threshold: one event closes and the next opens there
    assert [r[:3] for r in P.label_runs_host(key, conf, 0.5)] == [(0, 1, 0), (2, 2, 1), (4, 4, 1), (6, 7, 2), (8, 8, 0)]
    assert P.label_runs_host(key, conf, 0.95) == [] and P.label_runs_host(key[:0], conf[:0]) == []
    nan = np.array([np.nan, .9], np.float32)
    assert [r[:3] for r in P.label_runs_host(np.array([1, 1]), nan, 0.0)] == [(1, 1, 1)]


@pytest.mark.parametrize("seed,n,n_classes,b,threshold,framerate,minutes", PC.ACTO_DF_CASES)
def test_activity_bins_equal_the_references(seed, n, n_classes, b, threshold, framerate, minutes):
    p = PC.probabilities(seed, n, n_classes)
    want = GOLDEN[f"acto_df/{seed}"]
    got = P.activity_bins(p, None, PC.names(n_classes), PC.names(n_classes)[b], framerate, minutes, threshold)
    assert all(type(x) is float for x in got) and np.array_equal(np.array(got), want) and len(got) == len(want)


@pytest.mark.parametrize("k", range(len(PC.ACTO_DIR_CASES)))
def test_activity_bins_of_a_directory_equal_the_references(k, tmp_path):
    n_classes, b, threshold, framerate, minutes = PC.ACTO_DIR_CASES[k]
    for name, seed, n in PC.ACTO_DIR_FILES:
        PL.write_probs_csv(str(tmp_path / name), PC.probabilities(seed, n, n_classes), PC.names(n_classes))
    (tmp_path / "rec_3_m_outputs.csv").write_text(",".join(PC.names(n_classes)) + "\n")        # no rows: skipped
    PL.write_probs_csv(str(tmp_path / "rec_4_m_outputs.csv"), PC.probabilities(1, 9, 2), ["x", "y"])     # no such column: skipped
    PL.write_probs_csv(str(tmp_path / "rec_5_other_outputs.csv"), PC.probabilities(1, 9, n_classes), PC.names(n_classes))
    got = P.activity_bins(str(tmp_path), PC.MODEL, None, PC.names(n_classes)[b], framerate, minutes, threshold)
    assert np.array_equal(np.array(got), GOLDEN[f"acto_dir/{k}"])
    files = [str(tmp_path / f"rec_{i}_m_outputs.csv") for i in (1, 2, 3, 4, 10)]
    assert P.activity_bins(files, None, None, PC.names(n_classes)[b], framerate, minutes, threshold) == got


def test_file_order_and_bin_sizes(tmp_path):
    for name in ("a_10_m_outputs.csv", "a_9_m_outputs.csv", "a_100_m_outputs.csv", "a_9_mm_outputs.csv", "notes.txt"):
        (tmp_path / name).write_text("")
    assert [os.path.basename(f) for f in P.outputs_files(str(tmp_path), "m")] == \
        ["a_9_m_outputs.csv", "a_10_m_outputs.csv", "a_100_m_outputs.csv"]
    (tmp_path / "b_m_outputs.csv").write_text("")                  # a name without a number: plain sort for all
    assert [os.path.basename(f) for f in P.outputs_files(str(tmp_path), "m")] == \
        ["a_100_m_outputs.csv", "a_10_m_outputs.csv", "a_9_m_outputs.csv", "b_m_outputs.csv"]
    assert P.outputs_files(str(tmp_path), "zz") == []
    assert P.binsize_frames(10.0, 1) == 600 and P.binsize_frames(0.1, 1) == 6 and P.binsize_frames(29.97, 2) == 3596
    assert P.binsize_frames(0.001, 1) == 0 and P.binsize_frames(0, 5) == 0 and P.binsize_frames(-1, 5) == 0
    assert P.binsize_frames(10, 0) == 0 and P.binsize_frames(10, 1.9) == 600          # int(binsize_minutes), :963
    p = PC.probabilities(1, 20, 3)
    assert P.activity_bins(p, None, PC.names(3), "beh0", 0.001, 1, 0.5) == []
    assert P.activity_bins(p, None, PC.names(3), "nobody", 0.1, 1, 0.5) == []
    assert P.activity_bins(str(tmp_path), "zz", None, "beh0", 0.1, 1, 0.5) == []
    one = P.activity_bins(p, None, PC.names(3), "beh0", 1.0, 1, 0.0)              # a bin larger than the clip: one tail bin
    assert one == [20.0]


def test_activity_semantics_on_the_host():
    nan = np.nan
    rows = np.array([[.5, .5, .0], [.6, .4, .0], [nan, .3, .2], [.3, nan, .2], [.3, nan, nan], [.2, .7, .1]], np.float32)
    assert list(P.activity_bins_host(rows, 0, 0.25, 1)) == [0, 1, 0, 1, 0, 0]     # a tie is no maximum; NaN others are skipped
    assert list(P.activity_bins_host(rows, 0, 0.0, 4)) == [3, 2]                    # threshold 0: every frame but the NaN one
    assert list(P.activity_bins_host(rows, 0, -1.0, 7)) == [5]
    assert list(P.activity_bins_host(rows[:, :1], 0, 0.25, 2)) == [0, 0, 0]         # one class: never the maximum of the others
    assert list(P.activity_bins_host(rows[:, :1], 0, 0.0, 6)) == [5]


def test_what_stands_for_a_file_as_float32(tmp_path):
    rng = np.random.default_rng(4)
    p = np.concatenate([PC.probabilities(3, 500, 9), rng.random((200, 9), dtype=np.float32) * np.float32(1e-6),
                        np.array([[0, 1, 1e-30, 3e38, 1e-45, 0.1, 0.5, np.nan, 1e10]], np.float32)])
    path = str(tmp_path / "a_m_outputs.csv")
    PL.write_probs_csv(path, p, PC.names(9))
    header, parsed, exact = PL.read_outputs_csv(path)
    assert header == PC.names(9) and parsed.dtype == np.float64 and not np.array_equal(parsed, p.astype(np.float64), equal_nan=True)
    assert exact is not None and exact.dtype == np.float32 and exact.tobytes() == p.tobytes()     # the text of float32 values
    # other text: values rounded to 4 decimals (0.7000 is not the float32 nearest 0.7), float64 digits, a quoted field
    for k, text in enumerate(["a,b\n0.7000,0.3000\n", "a,b\n0.7,0.30000000000000004\n", 'a,b\n"0.7",0.3\n', "a,b\r\n0.7,0.3\r\n"]):
        other = tmp_path / f"o{k}.csv"
        other.write_bytes(text.encode())
        header, parsed, exact = PL.read_outputs_csv(str(other))
        assert header == ["a", "b"] and parsed.shape == (1, 2) and parsed[0, 0] == 0.7 and exact is None, text
    (tmp_path / "ok.csv").write_bytes(b"a,b\n0.7,0.3\n")
    assert PL.read_outputs_csv(str(tmp_path / "ok.csv"))[2].tobytes() == np.array([[0.7, 0.3]], np.float32).tobytes()
    (tmp_path / "none.csv").write_bytes(b"")
    assert PL.read_outputs_csv(str(tmp_path / "none.csv"))[0] == []
    (tmp_path / "head.csv").write_bytes(b"a,b\n")
    header, parsed, exact = PL.read_outputs_csv(str(tmp_path / "head.csv"))
    assert header == ["a", "b"] and parsed.shape == (0, 2) and exact is None
    # arrays: float32, or float64 that holds float32 values
    assert P._as_float32(p) is not None and P._as_float32(p.astype(np.float64)).tobytes() == p.tobytes()
    assert P._as_float32(rng.random((50, 3))) is None and P._as_float32(np.array([[0.7, 0.3]])) is None
    assert P._as_float32(np.array([[0.5, 1e300]])) is None


def test_mixed_headers_do_not_depend_on_the_order_of_calls(tmp_path):
    """Files of one recording with different columns: every file that has the behaviour counts, whichever behaviour was
    asked for before (nothing of such a recording is kept between calls)."""
    P.clear_cache()
    nine, two = PC.probabilities(31, 70, 9), PC.probabilities(32, 45, 2)
    PL.write_probs_csv(str(tmp_path / "rec_1_m_outputs.csv"), nine, PC.names(9))
    PL.write_probs_csv(str(tmp_path / "rec_2_m_outputs.csv"), two, ["x", "beh4"])
    want4 = [float(v) for v in P._rebin(np.concatenate([P.activity_bins_host(nine, 4, 0.3, 1), P.activity_bins_host(two, 1, 0.3, 1)]), 6)]
    wantx = [float(v) for v in P.activity_bins_host(two, 0, 0.3, 6)]
    for order in (("beh4", "x"), ("x", "beh4"), ("beh4", "beh4")):
        got = {b: P.activity_bins(str(tmp_path), "m", None, b, 0.1, 1, 0.3) for b in order}
        assert got["beh4"] == want4 and got.get("x", wantx) == wantx and sum(want4) > 0 and sum(wantx) > 0
    assert len(P._cache) == 0


def test_library_surface():
    header = open(os.path.join(REPO, "include", "cbas_mi355x.h")).read()
    exported = re.search(r"global:\s*([^;]+);", open(os.path.join(REPO, "cbas_amd", "csrc", "exports.map")).read()).group(1).split()
    want = {"cbas_labels_median": (C.c_int, 8, r"\bint cbas_labels_median\(const int32_t\* pred_dev, int64_t n_frames_total,"),
            "cbas_label_runs": (C.c_int64, 12, r"\bint64_t cbas_label_runs\(const int32_t\* key_dev, const float\* conf_dev,"),
            "cbas_activity_bins": (C.c_int, 9, r"\bint cbas_activity_bins\(const float\* probs_dev, int64_t n_total,")}
    lib = _lib.load()
    for name, (res, n_args, decl) in want.items():
        assert re.search(decl, header), name
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported)
        assert _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == n_args
        assert hasattr(lib, name)
    assert int(re.search(r"#define CBAS_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.EXPECTED_ABI == 11
    assert lib.cbas_abi_version() == 11
    assert re.search(r"typedef struct cbas_label_run \{", header) and P.LABEL_RUN_DTYPE.itemsize == 24
    readme = open(os.path.join(REPO, "README.md")).read()
    assert f"{len(_lib.SIGNATURES)} entry points" in readme and "CBAS_ACTOGRAM_CACHE_MB" in readme
    assert "cbas_amd/postprocess.py" in readme
    # refusals that need no device: nothing is dereferenced before the checks
    assert lib.cbas_labels_median(None, 4, None, 1, 3, 3, None, None) == -1 and b"NULL" in lib.cbas_last_error()
    assert lib.cbas_label_runs(None, None, 4, None, 1, 3, 0, 0.0, None, 0, None, None) == -1 and b"NULL" in lib.cbas_last_error()
    assert lib.cbas_activity_bins(None, 4, 3, 0, 0.5, 2, None, 2, None) == -1 and b"NULL" in lib.cbas_last_error()
