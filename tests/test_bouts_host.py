"""cbas_amd/bouts.py without a GPU: the numpy reference of the Viterbi decode against brute-force enumeration, the transition
builders against matrices worked out by hand, the extension header against the ctypes table and both built libraries, the
command line, and the CPU path of ``viterbi_labels``."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viterbi_ref as V  # noqa: E402

from cbas_amd import _lib, bouts, build as B, postprocess  # noqa: E402


# ---- the reference itself -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,T", [(2, 1), (2, 2), (2, 7), (3, 1), (3, 4), (3, 7)])
def test_reference_equals_brute_force(C, T):
    rng = np.random.default_rng(100 * C + T)
    ties = 0
    for trial in range(12):
        e = rng.integers(-2, 1, size=(T, C))
        A = rng.integers(-2, 1, size=(C, C))
        prior = None if trial % 2 else rng.integers(-2, 1, size=C)
        labels, score = V.viterbi_clip(e, A, prior)
        want, want_score = V.brute_force(e, A, prior)
        assert score == want_score
        assert np.array_equal(labels, want), (e, A, prior)
        best = [p for p in np.ndindex(*([C] * T)) if V.path_score(p, e, A, prior) == score]
        ties += len(best) > 1
    assert T == 1 or ties > 0                                  # the draw does exercise the tie rules


def test_reference_tie_rules_by_hand():
    # everything ties: the lowest end state, then the lowest predecessor at every frame
    labels, score = V.viterbi_clip(np.zeros((5, 3), int), np.zeros((3, 3), int))
    assert labels.tolist() == [0] * 5 and score == 0
    # state 1 is better only at the last frame; both predecessors tie, the lower one is kept
    e = np.array([[0, 0], [0, 0], [-1, 0]])
    labels, score = V.viterbi_clip(e, np.zeros((2, 2), int))
    assert labels.tolist() == [0, 0, 1] and score == 0
    # a forbidden self-transition: the path alternates
    A = np.array([[-(1 << 20), 0], [0, -(1 << 20)]])
    labels, score = V.viterbi_clip(np.zeros((4, 2), int), A)
    assert labels.tolist() == [1, 0, 1, 0] and score == 0     # ends in the lowest state, 0
    labels, score = V.viterbi_clip(np.zeros((0, 2), int), A)
    assert labels.size == 0 and score == 0


def test_reference_scores():
    p = np.array([1.0, 0.5, 2.0 ** -31, 2.0 ** -32, 2.0 ** -33, 0.0, 1.5, -0.25, np.nan, 1e-45, 0.3])
    want = [0, -256, -7936, -8192, -8192, -8192, 0, -8192, -8192, -8192, int(np.rint(256 * np.log2(0.3)))]
    assert V.scores_ref(p).tolist() == want
    assert bouts.scores_host(p).tolist() == want


# ---- the transition builders ----------------------------------------------------------------------------------------------------------
def test_sticky_transitions_by_hand():
    A = bouts.sticky_transitions(3, stay=0.5)
    assert A.dtype == np.int32 and A.tolist() == [[-256, -512, -512], [-512, -256, -512], [-512, -512, -256]]      # 1/2, 1/4, 1/4
    A = bouts.sticky_transitions(2, mean_duration=4)           # stay 3/4, leave 1/4
    assert A.tolist() == [[int(np.rint(256 * np.log2(0.75))), -512], [-512, int(np.rint(256 * np.log2(0.75)))]]
    assert A[0, 0] == -106
    assert np.array_equal(bouts.sticky_transitions(5), bouts.sticky_transitions(5, stay=0.98))
    assert bouts.sticky_transitions(5)[0, 0] == int(np.rint(256 * np.log2(0.98))) == -7
    assert bouts.sticky_transitions(5)[0, 1] == int(np.rint(256 * np.log2(0.005)))
    assert bouts.sticky_transitions(1).tolist() == [[0]]
    for bad in (dict(stay=0.0), dict(stay=1.0), dict(stay=-0.1), dict(stay=1.5), dict(stay=float("nan")), dict(mean_duration=1.0),
                dict(mean_duration=0.5), dict(stay=0.9, mean_duration=10)):
        with pytest.raises(ValueError):
            bouts.sticky_transitions(3, **bad)
    for bad in (0, 65):
        with pytest.raises(ValueError):
            bouts.sticky_transitions(bad)


def test_transitions_from_instances_by_hand():
    names = ["a", "b", "c"]
    inst = [("x_cls.h5", 0, 3, "a"), ("x_cls.h5", 4, 5, "b"), ("x_cls.h5", 6, 9, "a"), ("x_cls.h5", 10, 11, "b"),
            ("y_cls.h5", 0, 3, "b"), ("y_cls.h5", 4, 7, "a"),
            ("y_cls.h5", 8, -1, "a"), ("y_cls.h5", 9, 12, "zzz")]          # skipped: no end; not a behaviour
    # bouts: a of 4, 4, 4 frames (mean 4: stay 3/4); b of 2, 2, 4 (mean 8/3: stay 5/8); c none: the mean of all six, 10/3: stay 7/10
    # successions: x: a>b, b>a, a>b; y: b>a.  With smoothing 1: a -> (b 3, c 1), b -> (a 3, c 1), c -> (a 1, b 1)
    P = np.array([[3 / 4, 1 / 4 * 3 / 4, 1 / 4 * 1 / 4],
                  [3 / 8 * 3 / 4, 5 / 8, 3 / 8 * 1 / 4],
                  [3 / 10 / 2, 3 / 10 / 2, 7 / 10]])
    want = np.rint(256 * np.log2(P)).astype(np.int32)
    assert np.array_equal(bouts.transitions_from_instances(inst, names), want)
    # smoothing 0: a never goes to c; c, never seen, leaves evenly
    A0 = bouts.transitions_from_instances(inst, names, smoothing=0.0)
    assert A0[0, 2] == -(1 << 20) and A0[0, 1] == int(np.rint(256 * np.log2(0.25))) and A0[2, 0] == A0[2, 1] == int(np.rint(256 * np.log2(0.15)))
    # a bout of one frame: stay 0, which is the strongest "never"
    A1 = bouts.transitions_from_instances([("f", 5, 5, "a"), ("f", 6, 9, "b")], ["a", "b"])
    assert A1[0, 0] == -(1 << 20) and A1[0, 1] == 0
    with pytest.raises(ValueError):
        bouts.transitions_from_instances([("f", 0, 3, "zzz")], names)
    with pytest.raises(ValueError):
        bouts.transitions_from_instances([("f", 5, 3, "a")], names)
    assert bouts.transitions_from_instances([("f", 0, 3, "a")], ["a"]).tolist() == [[0]]


def test_transitions_from_counts_by_hand():
    counts = np.array([[5, 1], [0, 2]])
    want = np.rint(256 * np.log2(np.array([[6 / 8, 2 / 8], [1 / 4, 3 / 4]]))).astype(np.int32)
    assert np.array_equal(bouts.transitions_from_counts(counts), want)
    assert np.array_equal(bouts.transitions_from_counts(torch.from_numpy(counts)), want)
    A0 = bouts.transitions_from_counts(counts, smoothing=0.0)
    assert A0[1, 0] == -(1 << 20) and A0[1, 1] == 0
    for bad in (np.zeros((2, 3)), -np.ones((2, 2))):
        with pytest.raises(ValueError):
            bouts.transitions_from_counts(bad)
    with pytest.raises(ValueError):
        bouts.transitions_from_counts(np.zeros((2, 2)), smoothing=0.0)


# ---- header <-> EXT_SIGNATURES <-> both libraries -------------------------------------------------------------------------------------
def _declared_ext():
    header = open(os.path.join(os.path.dirname(B.HERE), "include", "cbas_mi355x_ext.h")).read()
    return set(re.findall(r"\b(cbasx_[a-z0-9_]+)\s*\(", header))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_extension_surface_is_declared_bound_and_exported():
    declared = _declared_ext()
    assert declared and declared == set(_lib.EXT_SIGNATURES), declared ^ set(_lib.EXT_SIGNATURES)
    assert all(name.startswith("cbasx_") for name in _lib.EXT_SIGNATURES)
    for debug in (False, True):
        path = B.build_library(debug=debug)
        assert {e for e in _exported(path) if e.startswith("cbasx_")} == declared
        assert not B.probe_library(path, sorted(declared))["missing"]
    assert len(_lib.SIGNATURES) == 88 and not set(_lib.SIGNATURES) & set(_lib.EXT_SIGNATURES)
    header = open(os.path.join(os.path.dirname(B.HERE), "include", "cbas_mi355x_ext.h")).read()
    for name, value in (("UNIT", bouts.UNIT), ("SCORE_MIN", bouts.SCORE_MIN), ("MAX_CLASSES", bouts.MAX_CLASSES), ("CHUNK", bouts.CHUNK)):
        m = re.search(rf"#define CBASX_VITERBI_{name} \(?(-?\d+)\)?", header)
        assert m and int(m.group(1)) == value, name
    assert "seq_viterbi.hip" in B.SOURCES and B.EXTRA_FLAGS["seq_viterbi.hip"] == B.NO_PACKED


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_parser():
    _, a = bouts.parse_cli(["--dir", "d", "--model", "m", "--out", "o.csv"])
    assert (a.dir, a.model, a.out, a.stay, a.mean_duration, a.instances, a.write_outputs, a.min_frames) == ("d", "m", "o.csv", None, None, None, None, 1)
    _, a = bouts.parse_cli(["--dir", "d", "--model", "m", "--out", "o.csv", "--mean-duration", "40", "--write-outputs", "m_viterbi"])
    assert a.mean_duration == 40.0 and a.write_outputs == "m_viterbi"
    for bad in (["--stay", "0.9", "--mean-duration", "40"], ["--stay", "1.0"], ["--stay", "0"], ["--mean-duration", "1"], ["--min-frames", "0"],
                ["--write-outputs", "m"], ["--stay", "0.9", "--instances", "x.csv"]):
        with pytest.raises(SystemExit):
            bouts.parse_cli(["--dir", "d", "--model", "m", "--out", "o.csv"] + bad)
    with pytest.raises(SystemExit):
        bouts.parse_cli(["--dir", "d", "--out", "o.csv"])


def test_csv_writer(tmp_path):
    records = np.array([(0, 0, 9, 1, 0.75), (1, 3, 3, 0, 1.0)], dtype=postprocess.LABEL_RUN_DTYPE)
    out = tmp_path / "bouts.csv"
    bouts.write_csv(str(out), ["a_m_outputs.csv", "b_m_outputs.csv"], records, ["rest", "groom"])
    assert out.read_text() == ("file,start_frame,end_frame,label,confidence\n"
                               "a_m_outputs.csv,0,9,groom,0.750000\n"
                               "b_m_outputs.csv,3,3,rest,1.000000\n")


def test_cli_end_to_end_on_the_host(tmp_path):
    """--dir / --model / --mean-duration / --out / --write-outputs with --device cpu: a flicker is decoded away, the one-hot file
    is written beside the input and read back by the loader of postprocess."""
    from cbas_amd import pipeline
    probs = np.tile(np.array([[0.9, 0.1]], np.float32), (40, 1))
    probs[20:] = [0.1, 0.9]
    probs[7] = [0.4, 0.6]
    pipeline.write_probs_csv(str(tmp_path / "rec_1_net_outputs.csv"), probs, ["rest", "groom"])
    out = tmp_path / "bouts.csv"
    assert bouts.main(["--dir", str(tmp_path), "--model", "net", "--mean-duration", "20", "--out", str(out), "--write-outputs", "net_viterbi",
                       "--device", "cpu"]) == 0
    lines = out.read_text().splitlines()
    assert lines[0] == "file,start_frame,end_frame,label,confidence" and len(lines) == 3
    assert lines[1].split(",")[1:4] == ["0", "19", "rest"] and lines[2].split(",")[1:4] == ["20", "39", "groom"]
    header, values, _ = pipeline.read_outputs_csv(str(tmp_path / "rec_1_net_viterbi_outputs.csv"))
    assert header == ["rest", "groom"] and values[:, 0].tolist() == [1.0] * 20 + [0.0] * 20
    assert postprocess.outputs_files(str(tmp_path), "net_viterbi") == [str(tmp_path / "rec_1_net_viterbi_outputs.csv")]


# ---- the CPU path ---------------------------------------------------------------------------------------------------------------------
def test_cpu_path_equals_the_reference():
    rng = np.random.default_rng(5)
    for C in (1, 2, 9):
        N = 90
        probs = rng.dirichlet(np.ones(C), size=N).astype(np.float32)
        probs[3, 0] = np.nan
        table = np.array([[0, 30], [30, 0], [35, 50], [85, 1]])       # a clip of no frame; frames 30 .. 34 and 86 .. 89 unowned
        A = rng.integers(-600, 1, size=(C, C)).astype(np.int32)
        prior = rng.integers(-600, 1, size=C).astype(np.int32)
        want, want_score = V.viterbi_ref(V.scores_ref(probs), table, A, prior)
        labels, score = bouts.viterbi_labels(torch.from_numpy(probs), table, A, prior, return_scores=True)
        assert labels.dtype == torch.int32 and score.dtype == torch.int64 and not labels.is_cuda
        assert np.array_equal(labels.numpy(), want) and np.array_equal(score.numpy(), want_score)
        assert (want[30:35] == -1).all() and (want[86:] == -1).all() and want_score[1] == 0
        assert np.array_equal(bouts.viterbi_labels(probs, table, A, prior).numpy(), want)         # an array, too
        # hard labels are one-hot scores
        hard = rng.integers(-1, C, size=N)
        one_hot = np.where((hard[:, None] == np.arange(C)[None, :]) | (hard[:, None] < 0), 0, -8192)
        want_hard, _ = V.viterbi_ref(one_hot, table, A, None)
        assert np.array_equal(bouts.viterbi_labels(torch.from_numpy(hard), table, A).numpy(), want_hard)
    with pytest.raises(ValueError):
        bouts.viterbi_labels(torch.zeros(4, 3), [(0, 4)], np.zeros((2, 2), np.int32))
    with pytest.raises(ValueError):
        bouts.viterbi_labels(torch.zeros(4, 2), [(0, 4)], np.full((2, 2), 1 << 21, np.int32))
    with pytest.raises(ValueError):
        bouts.viterbi_labels(torch.zeros(4, 2), [(0, 5)], np.zeros((2, 2), np.int32))


def flicker_clip():
    """Three long bouts (classes 0, 2, 1 over 120, 150 and 90 frames) whose probabilities flicker to another class on isolated
    single frames: ``(probs (360, 3) float32, the three bouts)``."""
    truth = np.repeat([0, 2, 1], [120, 150, 90])
    probs = np.full((360, 3), 0.1, np.float32)
    probs[np.arange(360), truth] = 0.8
    for t in (5, 40, 71, 100, 130, 200, 250, 275, 330, 359):          # isolated frames, the clip's last frame among them
        other = (truth[t] + 1) % 3
        probs[t] = 0.15
        probs[t, other] = 0.7
    return probs, [(0, 119, 0), (120, 269, 2), (270, 359, 1)]


def test_sticky_decode_removes_flicker_on_the_host():
    probs, want = flicker_clip()
    assert len(postprocess.label_runs_host(probs.argmax(1), probs.max(1))) > 3               # argmax does flicker
    A = bouts.sticky_transitions(3, mean_duration=50)
    labels, _ = V.viterbi_ref(V.scores_ref(probs), [(0, 360)], A)                          # the reference alone
    assert [(a, b, k) for a, b, k, _ in postprocess.label_runs_host(labels, np.ones(360, np.float32))] == want
    records = bouts.decode_bouts(torch.from_numpy(probs), [(0, 360)], A)
    assert [(int(r["start_frame"]), int(r["end_frame"]), int(r["label"])) for r in records] == want
    assert records.dtype == postprocess.LABEL_RUN_DTYPE and (records["clip"] == 0).all()
    assert abs(float(records["confidence"][0]) - probs[np.arange(120), 0].astype(np.float64).mean()) < 1e-6
