"""The disagreement report without a GPU: the numpy routine (cbas_amd.train.disagreement_runs_host) against the pandas
restatement (tests/disagreement_ref.py) and, through ``disagreement_report`` on clips that have their CSV, against the records
the reference method itself wrote (tests/golden/disagreement_report.npz, made by tests/golden/make_goldens_disagreement.py)."""
import json
import os

import numpy as np
import pytest

pd = pytest.importorskip("pandas")

import disagreement_ref as R  # noqa: E402
from cbas_amd import train as T  # noqa: E402
from cbas_amd.pipeline import format_probs_csv  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "disagreement_report.npz")


def golden_project(root):
    """The recording's project: an (empty) _cls.h5 and the CSV of every clip, written by the package's own formatter."""
    fx = np.load(GOLDEN)
    behaviors, task = [str(b) for b in fx["behaviors"]], str(fx["task"])
    for k, video in enumerate(str(v) for v in fx["videos"]):
        stem = os.path.splitext(os.path.join(root, video))[0]
        os.makedirs(os.path.dirname(stem), exist_ok=True)
        open(stem + "_cls.h5", "wb").close()
        with open(f"{stem}_{task}_outputs.csv", "w") as f:
            f.write(format_probs_csv(fx[f"probs/{k}"], behaviors))
    return fx, behaviors, task, json.loads(str(fx["instances_json"])), json.loads(str(fx["records_json"]))


def parse_bound(confidence):
    """Both sides average float64 values parsed from the same decimals: pandas' default parser may miss the nearest double
    by an ulp (2^-52), and a mean of n <= 300 values adds n * 2^-53 of summation noise in either order."""
    return 1e-13 * abs(confidence)


def test_report_from_existing_csvs_equals_the_reference_records(tmp_path):
    fx, behaviors, task, instances, records = golden_project(str(tmp_path))
    logged = []
    ours = T.disagreement_report(None, instances, behaviors, 31, str(tmp_path), task, device="cpu", log=logged.append)
    worst = R.assert_same_report(ours, records, parse_bound)
    print(f"{len(ours)} records, largest relative confidence gap to the reference {worst:.2e}")
    assert [o["model_prediction"] for o in ours] == [r["model_prediction"] for r in records]          # no near-tie in this recording
    assert sum("malformed" in line for line in logged) == 2, logged
    assert all(type(o["model_prediction"]) is str and set(o) == set(records[0]) for o in ours)
    # the restatement gives the reference's records too: it is the yardstick of the GPU tests
    tables = {str(v): R.frame_table(os.path.splitext(os.path.join(str(tmp_path), str(v)))[0] + f"_{task}_outputs.csv", behaviors)
              for v in fx["videos"]}
    restated = R.report(tables, instances)
    assert R.assert_same_report(restated, records, lambda c: 0.0) == 0.0
    assert [r["start_frame"] for r in restated] == [r["start_frame"] for r in records]


def test_numpy_routine_equals_the_restatement_on_random_instances():
    rng = np.random.default_rng(5)
    behaviors = ["walk", "eat", "groom", "drink"]
    rank = T.name_ranks(behaviors)
    assert rank.tolist() == [3, 1, 2, 0]
    for n in (1, 2, 40, 97):
        pred = rng.integers(-1, 4, n)
        pred[rng.random(n) < 0.5] = 1                                     # long stretches of one class
        conf = rng.random(n).astype(np.float32).astype(np.float64)
        df = R.frame_table_from(pred, conf, behaviors)
        for _ in range(200):
            start, end = int(rng.integers(-n - 2, n + 3)), int(rng.integers(-n - 2, n + 3))
            index = int(rng.integers(-1, 4))
            label = behaviors[index] if index >= 0 else "flying"
            want = R.instance_records(df, "v", start, end, label)
            got = T.disagreement_runs_host(pred, conf, start, end, index, rank)
            assert [(w["start_frame"], w["end_frame"], w["model_prediction"]) for w in want] == \
                   [(a, b, behaviors[c] if c >= 0 else None) for a, b, c, _ in got], (n, start, end, label)
            for w, g in zip(want, got):
                assert abs(w["model_confidence"] - g[3]) <= 1e-15 * n + 1e-16, (w, g)


def test_mode_ties_go_to_the_name_that_sorts_first():
    behaviors = ["walk", "eat", "groom", "drink"]
    rank = T.name_ranks(behaviors)
    pred = np.array([0, 0, 2, 2, 1, 1, 3, 3, -1, -1])                   # a four-way tie; index order says walk, name order drink
    conf = np.full(10, 0.5)
    assert T.disagreement_runs_host(pred, conf, 0, 9, -1, rank) == [(0, 9, 3, 0.5)]
    assert T.disagreement_runs_host(pred, conf, 0, 5, -1, rank) == [(0, 5, 1, 0.5)]                 # eat < groom < walk
    assert T.disagreement_runs_host(pred, conf, 8, 9, 1, rank) == [(8, 9, -1, 0.5)]                 # no prediction in the run
    assert R.instance_records(R.frame_table_from(pred, conf, behaviors), "v", 0, 9, "x")[0]["model_prediction"] == "drink"


def test_equal_confidences_keep_their_order_and_bad_csvs_are_skipped(tmp_path):
    root = str(tmp_path)
    behaviors = ["b", "a"]
    p = np.tile(np.array([[0.25, 0.75]], np.float32), (12, 1))           # every frame: "a" with confidence 0.75
    for name in ("v0", "v1", "v2", "v3"):
        open(os.path.join(root, f"{name}_cls.h5"), "wb").close()
    for name in ("v0", "v1"):
        with open(os.path.join(root, f"{name}_t_outputs.csv"), "w") as f:
            f.write(format_probs_csv(p, behaviors))
    q = p.copy()
    q[3, 0] = np.nan
    with open(os.path.join(root, "v2_t_outputs.csv"), "w") as f:
        f.write(format_probs_csv(q, behaviors))                          # a NaN: the clip is skipped with a warning
    with open(os.path.join(root, "v3_t_outputs.csv"), "w") as f:
        f.write("a,c\n0.5,0.5\n")                                        # no column "b"
    inst = [{"video": "v1.mp4", "start": 4, "end": 6, "label": "b"}, {"video": "v0.mp4", "start": 0, "end": 2, "label": "b"},
            {"video": "v1.mp4", "start": 0, "end": 1, "label": "b"}, {"video": "v2.mp4", "start": 0, "end": 5, "label": "b"},
            {"video": "v3.mp4", "start": 0, "end": 0, "label": "b"}, {"video": "v0.mp4", "start": 3, "end": 9, "label": "a"}]
    logged = []
    out = T.disagreement_report(None, inst, behaviors, 31, root, "t", device="cpu", log=logged.append)
    assert [(o["video_path"], o["start_frame"], o["end_frame"]) for o in out] == [("v1.mp4", 4, 6), ("v1.mp4", 0, 1), ("v0.mp4", 0, 2)]
    assert all(o["model_confidence"] == 0.75 and o["model_prediction"] == "a" and o["human_label"] == "b" for o in out)
    assert len(logged) == 2 and all(line.startswith("Could not read or process CSV") for line in logged), logged
    before = {n: open(os.path.join(root, n), "rb").read() for n in os.listdir(root)}
    T.disagreement_report(None, inst, behaviors, 31, root, "t", device="cpu", log=logged.append)
    assert before == {n: open(os.path.join(root, n), "rb").read() for n in os.listdir(root)}       # nothing is rewritten


def test_write_disagreement_report_round_trips(tmp_path):
    yaml = pytest.importorskip("yaml")
    items = [{"video_path": "a/b.mp4", "start_frame": 3, "end_frame": 7, "human_label": "eat", "model_prediction": "grün",
              "model_confidence": 0.8125}]
    path = str(tmp_path / "disagreement_report.yaml")
    T.write_disagreement_report(path, items)
    text = open(path, encoding="utf-8").read()
    assert text == yaml.dump(items, allow_unicode=True) and "grün" in text
    assert yaml.safe_load(text) == items
