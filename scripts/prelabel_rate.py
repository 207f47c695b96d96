#!/usr/bin/env python3
"""Time of what a person waits for when guided labelling starts, and of an actogram redraw.

Flow one, the pre-labels of one 18 000-frame clip (width 768, seq_len 31, 9 classes), smoothing windows 1 and 31:
  * ``prelabel_file``: the probabilities stay on the device for cbas_probs_top1 -> cbas_labels_median -> cbas_label_runs while
    a thread writes the CSV;
  * the route before it, for the same result: ``infer_file`` (classifies, writes the CSV), ``pandas.read_csv`` of that file
    and the numpy routine of cbas_amd.postprocess.
Flow two, ``activity_bins`` over a recording of 144 files of 6 000 frames (9 classes): cold (files parsed and uploaded), cached
(one launch), and the route before it: ``pandas.read_csv`` of all files and the numpy routine.

Every figure is the median of REPEATS runs after one warm-up run; every sample is kept.  The two routes' results are compared.

    python scripts/prelabel_rate.py [--out profiles/prelabel.json]
"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbas_amd import config as C, h5io, postprocess as P, synth, weights as W  # noqa: E402
from cbas_amd.head import ClassifierLSTMDeltas  # noqa: E402
from cbas_amd.pipeline import infer_file, write_probs_csv  # noqa: E402

FRAMES, DIM, SEQ, CLASSES, REPEATS = 18000, 768, 31, 9, 5
FILES, FILE_FRAMES = 144, 6000
NAMES = [f"b{i}" for i in range(CLASSES)]
TASK = "rate"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def median_of(fn, prepare=lambda: None):
    prepare()
    fn()                                                       # warm-up
    samples, out = [], None
    for _ in range(REPEATS):
        prepare()
        t, out = timed(fn)
        samples.append(t)
    return {"median_s": statistics.median(samples), "samples_s": samples}, out


def main():
    import pandas as pd
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    dev = torch.device("cuda")
    model = ClassifierLSTMDeltas(DIM, CLASSES, seq_len=SEQ)
    model.load_state_dict(W.synth_head_weights(C.HeadConfig(in_features=DIM, out_features=CLASSES, seq_len=SEQ), 7))
    model.to(dev)
    res = {"shape": {"frames": FRAMES, "dim": DIM, "seq_len": SEQ, "classes": CLASSES, "repeats": REPEATS, "files": FILES,
                     "file_frames": FILE_FRAMES}, "device": torch.cuda.get_device_name(0), "prelabel": {}, "actogram": {}}
    with tempfile.TemporaryDirectory() as root:
        h5 = os.path.join(root, "clip_cls.h5")
        with h5io.ClsWriter(h5, DIM) as w:
            w.append(synth.cls_walk(3, FRAMES, DIM))
        csv = h5.replace("_cls.h5", f"_{TASK}_outputs.csv")

        def drop_csv():
            if os.path.exists(csv):
                os.remove(csv)

        for window in (1, 31):
            def before():
                path = infer_file(file_path=h5, model=model, dataset_name=TASK, behaviors=NAMES, seq_len=SEQ, device=dev)
                values = pd.read_csv(path)[NAMES].to_numpy()
                return P._blocks("host", values, NAMES, "clip.mp4", window)

            ours, got = median_of(lambda: P.prelabel_file(h5, model, TASK, NAMES, SEQ, smoothing_window=window, project_path=root),
                                  drop_csv)
            theirs, want = median_of(before, drop_csv)
            same = [(g["start"], g["end"], g["label"]) for g in got[0]] == [(w_["start"], w_["end"], w_["label"]) for w_ in want[0]]
            res["prelabel"][f"window_{window}"] = {"prelabel_file": ours, "infer_file_read_csv_numpy": theirs, "instances": len(got[0]),
                                                   "same_instances": same, "speedup": theirs["median_s"] / ours["median_s"]}

        rec = os.path.join(root, "recording")
        os.makedirs(rec)
        rng = np.random.default_rng(11)
        for k in range(FILES):
            z = rng.standard_normal((FILE_FRAMES, CLASSES)).astype(np.float32) * 2
            p = np.exp(z - z.max(axis=1, keepdims=True))
            write_probs_csv(os.path.join(rec, f"cam_{k}_{TASK}_outputs.csv"), p / p.sum(axis=1, keepdims=True), NAMES)
        args = (TASK, None, NAMES[2], 10.0, 5, 0.5)

        def before_bins():
            parts = [pd.read_csv(f) for f in P.outputs_files(rec, TASK)]
            values = np.concatenate([d.to_numpy() for d in parts])
            return [float(x) for x in P.activity_bins_host(values, list(parts[0].columns).index(NAMES[2]), 0.5,
                                                           P.binsize_frames(10.0, 5))]

        cold, bins = median_of(lambda: P.activity_bins(rec, *args), P.clear_cache)
        cached, bins2 = median_of(lambda: P.activity_bins(rec, *args))
        theirs, want = median_of(before_bins)
        res["actogram"] = {"cold": cold, "cached": cached, "read_csv_numpy": theirs, "bins": len(bins), "same_bins": bins == want == bins2,
                           "speedup_cold": theirs["median_s"] / cold["median_s"], "speedup_cached": theirs["median_s"] / cached["median_s"]}
        P.clear_cache()
    model.close()
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
