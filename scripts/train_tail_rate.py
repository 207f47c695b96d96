#!/usr/bin/env python3
"""Time of the tail of a training job - scoring the held-out split and fitting the calibration temperature - over the
20 004-window manifest of profiles/train_resident_epoch.json (4 files x 5 031 rows of width 768, seq_len 31, 9 classes):

  * host loader (CBAS_TRAIN_RESIDENT=0): one HDF5 slice per window, batches of 512 windows copied to the device, argmax
    copied back per batch, the logits collected on the device - how the tail ran before it was built;
  * resident, each call building its own store (outside keep_rows());
  * resident inside keep_rows(), the store already built by the training run: what an installed CBAS does.

The second run of each is reported (the first one warms up).  Also: one cbas_logits_nll closure call.

    python scripts/train_tail_rate.py [--out profiles/train_tail.json]
"""
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbas_amd import config as C, datasets as D, synth, weights as W  # noqa: E402
from cbas_amd import train as T  # noqa: E402
from cbas_amd.head import ClassifierLSTMDeltas  # noqa: E402

ROWS, FILES, DIM, SEQ, BATCH, CLASSES = 5031, 4, 768, 31, 512, 9
NAMES = [f"b{i}" for i in range(CLASSES)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def tail(model, manifest):
    ds = D.LazyStandardDataset(manifest, SEQ)
    dev = torch.device("cuda")
    t_eval, res = timed(lambda: T.evaluate_on_split(model, ds, NAMES, device=dev))
    t_fit, temp = timed(lambda: T.fit_temperature(model, torch.utils.data.DataLoader(ds, batch_size=BATCH, num_workers=0), dev))
    return {"evaluate_on_split_s": t_eval, "fit_temperature_s": t_fit, "tail_s": t_eval + t_fit, "temperature": temp,
            "accuracy": res["report"]["accuracy"]}


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    hcfg = C.HeadConfig(in_features=DIM, out_features=CLASSES, seq_len=SEQ)
    model = ClassifierLSTMDeltas(DIM, CLASSES, seq_len=SEQ)
    model.load_state_dict(W.synth_head_weights(hcfg, 7))
    model.to("cuda")
    res = {"shape": {"files": FILES, "rows_per_file": ROWS, "dim": DIM, "seq_len": SEQ, "batch": BATCH, "classes": CLASSES},
           "device": torch.cuda.get_device_name(0)}
    quiet = open(os.devnull, "w")
    with tempfile.TemporaryDirectory() as root:
        paths, labels = synth.cls_project(root, [ROWS] * FILES, DIM, CLASSES, 5)
        manifest = D.make_manifest([(p, a, b, NAMES[c]) for p, l in zip(paths, labels) for a, b, c in synth.label_runs(l)], SEQ, NAMES)
        res["windows"] = len(manifest)
        stdout, sys.stdout = sys.stdout, quiet                      # the "training data: ..." lines
        try:
            for key, mode in (("host_loader", "0"), ("resident_own_store", "1")):
                os.environ["CBAS_TRAIN_RESIDENT"] = mode
                for _ in range(2):
                    res[key] = tail(model, manifest)
                D.close_readers()
            with T.keep_rows():
                t_store, _ = timed(lambda: T.open_store([D.LazyStandardDataset(manifest, SEQ)], ("training",), SEQ, DIM,
                                                        torch.device("cuda"), lambda line: None))
                for _ in range(2):
                    res["resident_kept_store"] = tail(model, manifest)
                res["resident_kept_store"]["store_built_by_training_s"] = t_store
        finally:
            sys.stdout = stdout
        # one closure call of the fit: a cbas_logits_nll launch and its 8-byte copy
        logits = torch.randn(len(manifest), CLASSES, device="cuda")
        f = T.device_nll(logits, torch.randint(0, CLASSES, (len(manifest),), device="cuda"))
        f(1.3)
        t, _ = timed(lambda: [f(1.3) for _ in range(100)])
        res["logits_nll_call_us"] = t / 100 * 1e6
    same = {res[k]["temperature"] for k in ("host_loader", "resident_own_store", "resident_kept_store")}
    res["temperatures_equal"] = len(same) == 1
    res["tail_ratio_kept_store"] = res["host_loader"]["tail_s"] / res["resident_kept_store"]["tail_s"]
    res["tail_ratio_own_store"] = res["host_loader"]["tail_s"] / res["resident_own_store"]["tail_s"]
    model.close()
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
