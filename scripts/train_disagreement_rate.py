#!/usr/bin/env python3
"""Time of the last step of a training job, the disagreement report, over the clips of the 20 004-window manifest of
profiles/train_tail.json (4 files x 5 031 rows of width 768, seq_len 31, 9 classes; every frame labelled):

  * host path (CBAS_TRAIN_RESIDENT=0), how the reference does it: infer_file per clip (reads the _cls.h5 again, classifies,
    writes the CSV), the CSV parsed back, the instances scanned on the host;
  * resident, outside keep_rows(): each clip's rows uploaded once, probabilities kept on the device for cbas_probs_top1 and
    one cbas_disagreement_runs call, the CSVs written by a thread meanwhile;
  * resident inside keep_rows(), the rows already in the store the training run built: what an installed CBAS does.

The three are run alternately, REPEATS times after one warm-up round, in one process; the CSVs are deleted before every run
(a clip that has one is not classified again).  Medians are reported, with every sample.  Also timed alone, to say where the
time goes: the native CSV writer and the CSV parse over the same clips, and the device scan (top-1 + runs) over all frames.

    python scripts/train_disagreement_rate.py [--out profiles/train_disagreement.json]
"""
import glob
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbas_amd import config as C, datasets as D, synth, weights as W  # noqa: E402
from cbas_amd import train as T  # noqa: E402
from cbas_amd.head import ClassifierLSTMDeltas  # noqa: E402
from cbas_amd.pipeline import write_probs_csv  # noqa: E402

ROWS, FILES, DIM, SEQ, CLASSES, REPEATS = 5031, 4, 768, 31, 9, 5
NAMES = [f"b{i}" for i in range(CLASSES)]
TASK = "rate"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    dev = torch.device("cuda")
    hcfg = C.HeadConfig(in_features=DIM, out_features=CLASSES, seq_len=SEQ)
    model = ClassifierLSTMDeltas(DIM, CLASSES, seq_len=SEQ)
    model.load_state_dict(W.synth_head_weights(hcfg, 7))
    model.to(dev)
    res = {"shape": {"files": FILES, "rows_per_file": ROWS, "dim": DIM, "seq_len": SEQ, "classes": CLASSES, "repeats": REPEATS},
           "device": torch.cuda.get_device_name(0)}
    quiet = lambda line: None  # noqa: E731
    with tempfile.TemporaryDirectory() as root:
        paths, labels = synth.cls_project(root, [ROWS] * FILES, DIM, CLASSES, 5)
        insts = [{"video": f"clip{f}.mp4", "start": a, "end": b, "label": NAMES[c]}
                 for f, lab in enumerate(labels) for a, b, c in synth.label_runs(lab)]
        manifest = D.make_manifest([(p, a, b, NAMES[c]) for p, l in zip(paths, labels) for a, b, c in synth.label_runs(l)], SEQ, NAMES)
        res["instances"] = len(insts)

        def report(mode):
            for f in glob.glob(os.path.join(root, "*_outputs.csv")):
                os.remove(f)
            os.environ["CBAS_TRAIN_RESIDENT"] = mode
            return timed(lambda: T.disagreement_report(model, insts, NAMES, SEQ, root, TASK, device=dev, log=quiet))

        samples = {"host_path": [], "resident_upload": [], "resident_kept_store": []}
        lists = {}
        stdout, sys.stdout = sys.stdout, open(os.devnull, "w")          # the "training data: ..." lines
        try:
            with T.keep_rows():
                for rnd in range(REPEATS + 1):
                    T._row_cache.drop()                                  # no kept store: every clip is uploaded
                    t_host, lists["host_path"] = report("0")
                    t_up, lists["resident_upload"] = report("1")
                    T.open_store([D.LazyStandardDataset(manifest, SEQ)], ("training",), SEQ, DIM, dev, quiet)
                    t_kept, lists["resident_kept_store"] = report("1")
                    if rnd:                                              # round 0 warms up
                        samples["host_path"].append(t_host), samples["resident_upload"].append(t_up)
                        samples["resident_kept_store"].append(t_kept)
        finally:
            sys.stdout = stdout
        for k, v in samples.items():
            res[k] = {"median_s": statistics.median(v), "samples_s": v}
        res["records"] = len(lists["host_path"])
        key = lambda it: (it["video_path"], it["start_frame"], it["end_frame"], it["model_prediction"])  # noqa: E731
        res["records_equal"] = all(sorted(map(key, lists[k])) == sorted(map(key, lists["host_path"])) for k in lists)
        by = {k: {key(it): it["model_confidence"] for it in v} for k, v in lists.items()}
        res["largest_relative_confidence_gap"] = max(abs(by["resident_kept_store"][k] - c) / c for k, c in by["host_path"].items())

        # where the time goes: the pieces alone, on the files the last run left
        csvs = sorted(glob.glob(os.path.join(root, "*_outputs.csv")))
        probs = [T._read_outputs_csv(f, NAMES).astype(np.float32) for f in csvs]
        t_write = [timed(lambda: [write_probs_csv(f + ".again", p, NAMES) for f, p in zip(csvs, probs)])[0] for _ in range(REPEATS)]
        t_parse = [timed(lambda: [T._read_outputs_csv(f, NAMES) for f in csvs])[0] for _ in range(REPEATS)]
        allp = torch.from_numpy(np.concatenate(probs)).to(dev)
        rank = T.name_ranks(NAMES)
        table = [(k * ROWS, ROWS) for k in range(FILES)]
        ic = [int(i["video"][4]) for i in insts]
        ia, ib = [i["start"] for i in insts], [i["end"] for i in insts]
        il = [NAMES.index(i["label"]) for i in insts]

        def scan():
            pred, conf, _ = T.probs_top1(allp)
            return T.disagreement_runs(pred, conf, table, ic, ia, ib, il, rank)

        scan()
        t_scan = [timed(scan)[0] for _ in range(REPEATS)]
        res["alone"] = {"csv_write_s": statistics.median(t_write), "csv_parse_s": statistics.median(t_parse),
                        "device_top1_and_runs_s": statistics.median(t_scan), "frames": FILES * ROWS}
    res["ratio_kept_store"] = res["host_path"]["median_s"] / res["resident_kept_store"]["median_s"]
    res["ratio_upload"] = res["host_path"]["median_s"] / res["resident_upload"]["median_s"]
    model.close()
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
