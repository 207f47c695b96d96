#!/usr/bin/env python3
"""sha256 of what training steps leave (weights, gradients, both Adam moments), one line per trainer, for the configurations of
the entry-point tests of tests/test_gpu_train_trials.py: three steps by `step_rows` and three by `step_rows_multi` of

  h64        lstm_hidden_size 64, one trainer, 37 windows
  h32_l2     lstm_hidden_size 32, two layers, no acceleration stream, class weights, label smoothing, weight decay;
             three trainers with 64 / 37 / 1 windows

Two builds of the library compute the same thing exactly when the lines are equal: run it from each checkout on one device
and diff the output.  `--repo DIR` takes `cbas_amd` (and its built library) from another checkout of this repository.

    python scripts/train_step_digests.py [--repo DIR]
"""
import hashlib
import os
import sys

import numpy as np
import torch

REPO = sys.argv[sys.argv.index("--repo") + 1] if "--repo" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(REPO))
from cbas_amd import config as C, synth, weights as W  # noqa: E402
from cbas_amd import build as B, train as T  # noqa: E402

SEQ, BATCH, STEPS = 31, 64, 3
CONFIGS = {
    "h64": (dict(lstm_hidden_size=64), dict(lr=1e-3), [37]),
    "h32_l2": (dict(lstm_hidden_size=32, lstm_layers=2, use_acceleration=False),
               dict(lr=1e-3, weight_decay=1e-2, label_smoothing=0.1, class_weights=[0.5, 1.0, 2.0, 1.5, 0.25]), [64, 37, 1]),
}


def digest(tr):
    h = hashlib.sha256()
    for state in (tr.weights(), tr.grads()) + tuple(tr.adam_moments()):
        for key in sorted(state):
            h.update(key.encode())
            h.update(np.ascontiguousarray(state[key]).tobytes())
    return h.hexdigest()


def main():
    print(f"library: {B.lib_path()}", file=sys.stderr)
    rows = torch.from_numpy(synth.cls_walk(3, 610, 768).astype(np.float16)).cuda()
    for name, (head, opts, counts) in CONFIGS.items():
        hcfg = C.HeadConfig(in_features=768, out_features=5, **head)
        rng = np.random.default_rng(5)
        batches = [(torch.from_numpy(rng.integers(0, 610 - SEQ + 1, n).astype(np.int64)), torch.from_numpy(rng.integers(0, 5, n).astype(np.int64)))
                   for n in counts]

        def trainers():
            return [T.HeadTrainer(hcfg, W.synth_head_weights(hcfg, 4000 + s), "cuda", max_batch=BATCH, seed=s, dropout=True, **opts)
                    for s in range(1, len(counts) + 1)]
        alone, together = trainers(), trainers()
        for _ in range(STEPS):
            for t, (f, y) in zip(alone, batches):
                t.step_rows(rows, f, y)
            T.step_rows_multi(rows, [(t, f, y) for t, (f, y) in zip(together, batches)])
        for way, trs in (("step_rows", alone), ("step_rows_multi", together)):
            for t, n in zip(trs, counts):
                print(f"{name} {way} batch={n} steps={STEPS} sha256={digest(t)}")
        for t in alone + together:
            t.close()


if __name__ == "__main__":
    main()
