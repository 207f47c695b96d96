"""Test-local restatement, in pandas, of the per-clip part of the reference's disagreement report
(TrainingThread._generate_disagreement_report, backend/workthreads.py:760-805): what the device scan (cbas_probs_top1 +
cbas_disagreement_runs) and the numpy routine (cbas_amd.train.disagreement_runs_host) are held to.  It follows the
reference statement by statement - read_csv, idxmax / max, iloc[start:end+1], the `block` column from the index differences,
groupby, mean() and mode()[0] - and is itself checked against records the reference method produced
(tests/golden/disagreement_report.npz, tests/test_disagreement_host.py)."""
import numpy as np
import pandas as pd

NO_LABEL = "\0none"        # what a frame without a prediction (pred -1) carries here; it is dropped before mode(), as NaN is


def frame_table(csv_path, behaviors):
    """:761-763"""
    df = pd.read_csv(csv_path)
    df["model_label"] = df[behaviors].idxmax(axis=1)
    df["model_confidence"] = df[behaviors].max(axis=1)
    return df


def frame_table_from(pred, conf, behaviors):
    """The same table from per-frame class indices (-1: none) and confidences, for tests of the scan alone."""
    names = np.array(list(behaviors) + [NO_LABEL], dtype=object)
    return pd.DataFrame({"model_label": names[np.asarray(pred)], "model_confidence": np.asarray(conf, np.float64)})


def instance_records(df, video, start, end, true_label):
    """:777-803 for one instance."""
    out = []
    instance_preds = df.iloc[start:end + 1].copy()
    if instance_preds.empty:
        return out
    error_frames = instance_preds[instance_preds["model_label"] != true_label].copy()
    if error_frames.empty:
        return out
    error_frames["block"] = (error_frames.index.to_series().diff() != 1).cumsum()
    for _block, block_df in error_frames.groupby("block"):
        if block_df.empty:
            continue
        labels = block_df["model_label"]
        labels = labels[labels != NO_LABEL]
        out.append({"video_path": video, "start_frame": int(block_df.index.min()), "end_frame": int(block_df.index.max()),
                    "human_label": true_label, "model_prediction": labels.mode()[0] if len(labels) else None,
                    "model_confidence": float(block_df["model_confidence"].mean())})
    return out


def report(tables, instances):
    """:738-805 given ``tables`` {video: frame table} (a video without one is skipped, as one without an h5 or a readable CSV
    is) and the instance dicts; malformed instances are skipped as in :769-775."""
    by_video = {}
    for inst in instances:
        if inst.get("video"):
            by_video.setdefault(inst["video"], []).append(inst)
    out = []
    for video, insts in by_video.items():
        if video not in tables:
            continue
        for inst in insts:
            try:
                start, end, label = int(inst["start"]), int(inst["end"]), inst["label"]
            except (ValueError, KeyError, TypeError):
                continue
            out += instance_records(tables[video], video, start, end, label)
    out.sort(key=lambda x: x["model_confidence"], reverse=True)
    return out


def confidence_bound(confidence):
    """|ours - reference| for one record: the reference averages float64 values parsed from the shortest decimals of the
    float32 probabilities, each within half a float32 ulp (2^-24 relative) of the float32 value we average; float64
    summation noise rides on top (1.2e-7 > 2^-24 = 5.96e-8 leaves room for it)."""
    return 1.2e-7 * abs(confidence)


def match(ours, theirs):
    """Records matched by (video_path, start_frame, end_frame): the sorted lists may differ in the order of records whose
    confidences are closer than the bound.  Overlapping instances can report one run twice, so the match is on multisets,
    in order of appearance."""
    def keyed(items):
        d = {}
        for it in items:
            d.setdefault((it["video_path"], it["start_frame"], it["end_frame"], repr(it["human_label"])), []).append(it)
        return d
    a, b = keyed(ours), keyed(theirs)
    assert a.keys() == b.keys(), (sorted(set(a) ^ set(b))[:5], len(a), len(b))
    pairs = []
    for k in a:
        assert len(a[k]) == len(b[k]), k
        pairs += list(zip(a[k], b[k]))
    return pairs


def assert_same_report(ours, theirs, bound=confidence_bound):
    assert len(ours) == len(theirs), (len(ours), len(theirs))
    worst = 0.0
    for x, y in match(ours, theirs):
        assert x["model_prediction"] == y["model_prediction"] and x["human_label"] == y["human_label"], (x, y)
        gap = abs(x["model_confidence"] - y["model_confidence"])
        worst = max(worst, gap / abs(y["model_confidence"]))
        assert gap <= bound(y["model_confidence"]), (x, y, gap)
        assert type(x["start_frame"]) is int and type(x["end_frame"]) is int and type(x["model_confidence"]) is float, x
    conf = [x["model_confidence"] for x in ours]
    assert all(a >= b for a, b in zip(conf, conf[1:])), "not sorted by confidence, highest first"
    return worst
