#!/usr/bin/env python3
"""Wall time of the trials of one run, 4 trials x 2 epochs on the 20 004-window manifest profiles/train_resident_epoch.json was
measured on (4 files x 5 031 rows of width 768, seq_len 31, batch 512, every frame labelled; 9 classes):

  (a) four train_lstm_model calls one after another inside keep_rows() (one store; the code path before train_lstm_trials),
  (b) train_lstm_trials(max_concurrent=4) on the same store.

Alternated a b a b ..., REPEATS pairs after one warm-up pair, in one process; medians, every sample and the spread
(max - min) are reported.  The weights of (b) are compared with those of (a), bit for bit.

The time of the small kernels, launched per trainer against once for all four, comes from two kernel traces of their own,
without counters: this script starts `rocprofv3 --kernel-trace` over `--steps solo`, a child that takes STEPS solo steps with
each of 4 trainers, and over `--steps together`, a child that takes STEPS steps of the 4 together, and sums the kernels'
durations by base name.  The phase, not the kernel's name, tells the launches apart.

    python scripts/train_trials_rate.py [--out profiles/train_trials.json] [--no-trace]
"""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbas_amd import config as C, datasets as D, synth, weights as W  # noqa: E402
from cbas_amd import train as T  # noqa: E402

ROWS, FILES, DIM, SEQ, CLASSES, BATCH = 5031, 4, 768, 31, 9, 512
TRIALS, EPOCHS, REPEATS, STEPS = 4, 2, 5, 20
NAMES = [f"b{i}" for i in range(CLASSES)]
SMALL = ("adam_step", "colsum_stage1", "colsum_stage2", "ce_terms", "ce_grad", "cov_offdiag", "add_vec", "copy_vec",
         "gelu_dropout_fwd", "gelu_dropout_bwd")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(samples):
    return {"median_s": statistics.median(samples), "spread_s": max(samples) - min(samples), "samples_s": samples}


def steps_only(phase):
    """The traced child: STEPS steps of 4 trainers one after another ("solo") or STEPS steps of the 4 together."""
    hcfg = C.HeadConfig(in_features=DIM, out_features=CLASSES, seq_len=SEQ)
    rows = torch.from_numpy(synth.cls_walk(3, FILES * ROWS, DIM)).cuda()
    rng = np.random.default_rng(1)
    batches = [(torch.from_numpy(rng.integers(0, FILES * ROWS - SEQ, BATCH)), torch.from_numpy(rng.integers(0, CLASSES, BATCH)))
               for _ in range(TRIALS)]
    trainers = [T.HeadTrainer(hcfg, W.synth_head_weights(hcfg, s), "cuda", max_batch=BATCH, seed=s) for s in range(TRIALS)]
    for _ in range(STEPS):
        if phase == "solo":
            for t, (f, y) in zip(trainers, batches):
                t.step_rows(rows, f, y, want_loss=False)
        else:
            T.step_rows_multi(rows, [(t, f, y) for t, (f, y) in zip(trainers, batches)], want_loss=False)
    torch.cuda.synchronize()
    for t in trainers:
        t.close()


def kernel_trace():
    """{"solo": {kernel: [launches, total us]}, "together": {...}} of the small kernels, from one rocprofv3 kernel trace per phase."""
    out = {}
    for phase in ("solo", "together"):
        out[phase] = {}
        with tempfile.TemporaryDirectory() as td:
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__),
                   "--steps", phase]
            r = subprocess.run(cmd, capture_output=True, text=True)
            files = glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True)
            if r.returncode != 0 or not files:
                return {"error": f"rocprofv3 ({phase}) ended with {r.returncode} and {len(files)} trace file(s)", "stderr_tail": r.stderr[-400:]}
            for path in files:
                with open(path, newline="") as f:
                    for row in csv.DictReader(f):
                        name = row.get("Kernel_Name", "")
                        base = next((s for s in SMALL if s + "_kernel" in name or s + "_multi_kernel" in name), None)
                        if base is None:
                            continue
                        n, us = out[phase].get(base, [0, 0.0])
                        out[phase][base] = [n + 1, us + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3]
        out[f"{phase}_total_us_per_step_of_4"] = sum(v[1] for v in out[phase].values()) / STEPS
    out["steps"] = STEPS
    return out


def main():
    if "--steps" in sys.argv:
        return steps_only(sys.argv[sys.argv.index("--steps") + 1])
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    dev = torch.device("cuda")
    res = {"shape": {"files": FILES, "rows_per_file": ROWS, "dim": DIM, "seq_len": SEQ, "classes": CLASSES, "batch": BATCH,
                     "trials": TRIALS, "epochs": EPOCHS, "repeats": REPEATS},
           "device": torch.cuda.get_device_name(0)}
    quiet = lambda line: None  # noqa: E731
    seeds = list(range(1, TRIALS + 1))
    kw = dict(batch_size=BATCH, epochs=EPOCHS, device=dev, patience=EPOCHS + 1, log=quiet)
    with tempfile.TemporaryDirectory() as root:
        paths, labels = synth.cls_project(root, [ROWS] * FILES, DIM, CLASSES, 5)
        manifest = D.make_manifest([(p, a, b, NAMES[c]) for p, l in zip(paths, labels) for a, b, c in synth.label_runs(l)], SEQ, NAMES)
        res["windows"] = len(manifest)
        val = manifest[::10]

        def sets():
            return D.LazyStandardDataset(manifest, SEQ), D.LazyStandardDataset(val, SEQ)

        def one_after_another():
            return [T.train_lstm_model(*sets(), SEQ, NAMES, threading.Event(), seed=s, **kw) for s in seeds]

        def together():
            return T.train_lstm_trials(*sets(), SEQ, NAMES, threading.Event(), trial_seeds=seeds, max_concurrent=TRIALS, **kw)

        def weights_of(results):
            out = []
            for model, _, _ in results:
                out.append({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
                model.close()
            return out

        samples = {"one_after_another": [], "together": []}
        same = True
        stdout, sys.stdout = sys.stdout, open(os.devnull, "w")          # the per-epoch lines
        try:
            with T.keep_rows():
                for rnd in range(REPEATS + 1):
                    ta, a = timed(one_after_another)
                    tb, b = timed(together)
                    wa, wb = weights_of(a), weights_of(b)
                    same = same and all(torch.equal(x[k], y[k]) for x, y in zip(wa, wb) for k in x)
                    if rnd:                                               # round 0 warms up
                        samples["one_after_another"].append(ta)
                        samples["together"].append(tb)
        finally:
            sys.stdout.close()
            sys.stdout = stdout
        D.close_readers()
    res["weights_bit_identical"] = bool(same)
    res["one_after_another"], res["together"] = summary(samples["one_after_another"]), summary(samples["together"])
    res["gain_s"] = res["one_after_another"]["median_s"] - res["together"]["median_s"]
    res["ratio"] = res["one_after_another"]["median_s"] / res["together"]["median_s"]
    res["faster_by_more_than_the_spread"] = bool(res["gain_s"] > res["one_after_another"]["spread_s"])
    if "--no-trace" not in sys.argv:
        res["small_kernels"] = kernel_trace()
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
