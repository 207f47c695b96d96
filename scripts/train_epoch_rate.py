"""What an epoch of head training costs with the CLS rows resident in device memory, next to the host loader.

A synthetic project of 4 `_cls.h5` files (5031 rows each, D = 768) gives a manifest of 20 004 windows (T = 31); batch 512.
Measured, each after a warm-up call of the same kind:

  * `train_lstm_model(epochs=1, no validation set)` - one training pass and one scoring pass, with everything the call
    does (reading the files, creating the trainer, the sklearn report) - with `CBAS_TRAIN_RESIDENT=0` (the host loader:
    the baseline) and with the rows resident;
  * the resident training pass alone (the index-only DataLoader, the index upload and `cbas_head_train_step_rows`,
    synchronised at the end), per step, next to `cbas_head_train_step` on one batch already on the device (the
    "device step"): the difference is the host share that is left;
  * one `cbas_rows_gather_windows` launch of 512 x 31 x 768 (hipEvent-timed over 200 launches; the kernel's own time
    comes from a `rocprofv3 --kernel-trace --stats` run of this script with `--gather-only`).

    python scripts/train_epoch_rate.py [--out profiles/train_resident_epoch.json] [--gather-only]
"""
import json
import os
import sys
import tempfile
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbas_amd import config as C, datasets as D, synth  # noqa: E402
from cbas_amd import train as T  # noqa: E402

ROWS, FILES, DIM, SEQ, BATCH, CLASSES = 5031, 4, 768, 31, 512, 9
NAMES = [f"b{i}" for i in range(CLASSES)]


def gather_time(launches=200):
    rows = torch.from_numpy(synth.cls_walk(1, ROWS * FILES, DIM)).cuda()
    first = torch.randint(0, ROWS * FILES - SEQ, (BATCH,), generator=torch.Generator().manual_seed(0)).cuda()
    out = torch.empty((BATCH, SEQ, DIM), device="cuda")
    for _ in range(10):
        T.gather_windows(rows, first, SEQ, out=out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        T.gather_windows(rows, first, SEQ, out=out)
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / launches
    moved = BATCH * SEQ * DIM * (2 + 4)
    return {"launch_us": us, "bytes_moved": moved, "GB_per_s": moved / us / 1e3}


def whole_call(manifest, mode):
    os.environ["CBAS_TRAIN_RESIDENT"] = mode
    best = None
    for _ in range(2):                                     # the first call warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model, reports, _ = T.train_lstm_model(D.LazyStandardDataset(manifest, SEQ), None, SEQ, NAMES, threading.Event(),
                                               batch_size=BATCH, epochs=1, device="cuda", seed=2, log=lambda s: None)
        torch.cuda.synchronize()
        best = time.perf_counter() - t0
        model.close()
    D.close_readers()
    return best


def resident_pass(manifest):
    """The resident training pass alone, and the device step on a batch that is already there."""
    hcfg = C.HeadConfig(in_features=DIM, out_features=CLASSES, seq_len=SEQ)
    ds = D.LazyStandardDataset(manifest, SEQ)
    plan = D.plan_store([manifest], DIM)
    t0 = time.perf_counter()
    store = T.ResidentRows(plan, "cuda")
    torch.cuda.synchronize()
    load_s = time.perf_counter() - t0
    view = T._IndexView(ds, SEQ, store.files)
    g = torch.Generator()
    g.manual_seed(0)
    loader = torch.utils.data.DataLoader(view, BATCH, shuffle=True, collate_fn=T._collate_index, num_workers=0, generator=g)
    tr = T.HeadTrainer(hcfg, T.initial_head_weights(hcfg, 0), "cuda", max_batch=BATCH, seed=1)
    out = {"load_rows_s": load_s, "store_MB": plan.nbytes / 1e6}
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for first, labels in loader:
            store.check(first.numpy(), SEQ)
            tr.step_rows(store.rows, first, labels, want_loss=False)
            n += 1
        host_done = time.perf_counter() - t0
        torch.cuda.synchronize()
        out.update(steps=n, pass_s=time.perf_counter() - t0, host_loop_s=host_done)
    out["ms_per_step"] = out["pass_s"] / out["steps"] * 1e3
    # the device step: cbas_head_train_step on one resident batch of explicit windows
    x = T.gather_windows(store.rows, torch.arange(BATCH, device="cuda"), SEQ).clone()
    y = torch.zeros(BATCH, dtype=torch.int64, device="cuda")
    for _ in range(3):
        tr.step(x, y, want_loss=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(30):
        tr.step(x, y, want_loss=False)
    torch.cuda.synchronize()
    out["device_step_ms"] = (time.perf_counter() - t0) / 30 * 1e3
    tr.close()
    return out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    res = {"shape": {"files": FILES, "rows_per_file": ROWS, "dim": DIM, "seq_len": SEQ, "batch": BATCH},
           "device": torch.cuda.get_device_name(0), "gather": gather_time()}
    if "--gather-only" not in sys.argv:
        with tempfile.TemporaryDirectory() as root:
            paths, labels = synth.cls_project(root, [ROWS] * FILES, DIM, CLASSES, 5)
            manifest = D.make_manifest([(p, a, b, NAMES[c]) for p, l in zip(paths, labels) for a, b, c in synth.label_runs(l)], SEQ, NAMES)
            res["windows"] = len(manifest)
            res["host_loader_call_s"] = whole_call(manifest, "0")
            res["resident_call_s"] = whole_call(manifest, "1")
            res["call_ratio"] = res["host_loader_call_s"] / res["resident_call_s"]
            res["resident_train_pass"] = resident_pass(manifest)
            D.close_readers()
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
