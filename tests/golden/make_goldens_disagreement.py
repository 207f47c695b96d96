#!/usr/bin/env python3
"""Generate tests/golden/disagreement_report.npz by running the REFERENCE's disagreement report.

Runs only where the reference tree is present (the build machine), on the CPU.  Nothing is copied from the reference:
``TrainingThread._generate_disagreement_report`` (backend/workthreads.py) is executed from the reference's own file - the text
of that one method is cut out at run time and compiled here, because importing the module needs the GUI's packages while
the method needs only os, pandas and yaml.  ``eel``, ``gui_state``, ``log_message`` and ``cbas`` are stand-ins; every clip
has its ``_outputs.csv`` already, written from fixed float32 probabilities the way ``infer_file`` writes it
(backend/cbas.py:565), so ``cbas.infer_file`` must not be called.

The fixture holds the behaviours, the probabilities, the instance dicts (as JSON) and the records the method wrote to
``disagreement_report.yaml`` (as JSON), nothing else.

Usage:  python tests/golden/make_goldens_disagreement.py [--out tests/golden]
"""
from __future__ import annotations

import argparse
import ast
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("CBAS_REFERENCE", "/root/reference")

BEHAVIORS = ["walk", "eat", "groom", "drink", "rear"]          # sorted by name: drink, eat, groom, rear, walk
SIZES = {"day1/cam_a.mp4": 40, "day1/cam_b.mp4": 97, "cam_c.mp4": 300}
TASK = "mice"


def probabilities(seed: int, n: int) -> np.ndarray:
    """Softmax-like float32 rows whose winner changes in blocks, with exact ties between the top two in some rows."""
    rng = np.random.default_rng(seed)
    C = len(BEHAVIORS)
    z = rng.standard_normal((n, C)) * 0.7
    winner = np.repeat(rng.integers(0, C, n // 5 + 1), 5)[:n]
    flip = rng.random(n) < 0.3
    winner = np.where(flip, rng.integers(0, C, n), winner)
    z[np.arange(n), winner] += 2.0
    p = np.exp(z)
    p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
    for r in range(3, n, 11):                                   # the first maximum must win
        order = np.argsort(p[r])
        p[r, order[-2]] = p[r, order[-1]]
    return p


def instances():
    inst = []
    for video, n in SIZES.items():
        rng = np.random.default_rng(n)
        a = 0
        while a < n:                                            # back-to-back instances of 3 - 25 frames with random labels
            b = min(n - 1, a + int(rng.integers(3, 26)))
            inst.append({"video": video, "start": a, "end": b, "label": BEHAVIORS[int(rng.integers(0, len(BEHAVIORS)))]})
            a = b + 1
    inst += [
        {"video": "day1/cam_a.mp4", "start": 10, "end": 10, "label": "eat"},         # one frame
        {"video": "day1/cam_a.mp4", "start": 30, "end": 60, "label": "groom"},       # runs past the clip
        {"video": "day1/cam_a.mp4", "start": 40, "end": 50, "label": "groom"},       # begins past the clip
        {"video": "day1/cam_b.mp4", "start": 20, "end": 70, "label": "flying"},      # no behaviour: every frame differs
        {"video": "day1/cam_b.mp4", "start": 50, "end": 90, "label": "walk"},        # overlaps the one before
        {"video": "day1/cam_b.mp4", "start": -10, "end": -2, "label": "eat"},        # pandas: from the end
        {"video": "day1/cam_b.mp4", "start": 30, "end": 20, "label": "eat"},         # empty
        {"video": "day1/cam_b.mp4", "start": "12", "end": "18", "label": "drink"},   # numbers as text
        {"video": "cam_c.mp4", "start": 5, "label": "eat"},                          # malformed: no end
        {"video": "cam_c.mp4", "start": "five", "end": 9, "label": "eat"},           # malformed: no number
        {"video": "cam_c.mp4", "start": 0, "end": 299, "label": "rear"},             # the whole clip
        {"video": "gone.mp4", "start": 0, "end": 9, "label": "eat"},                 # no _cls.h5
        {"start": 0, "end": 9, "label": "eat"},                                      # no video
    ]
    return inst


def reference_method():
    import pandas as pd
    import yaml
    path = os.path.join(REF, "backend", "workthreads.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "TrainingThread")
    node = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_generate_disagreement_report")
    logged = []

    def no_infer(**kw):
        raise AssertionError("every clip of the recording has its CSV")

    status = types.SimpleNamespace(updateTrainingStatusOnUI=lambda *a: (lambda: None))
    ns = {"os": os, "pd": pd, "yaml": yaml, "eel": status, "cbas": types.SimpleNamespace(infer_file=no_infer),
          "gui_state": types.SimpleNamespace(proj=types.SimpleNamespace(path=None)),
          "log_message": lambda msg, level="INFO": logged.append((level, msg))}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["_generate_disagreement_report"], ns, logged


def main():
    import pandas as pd
    import yaml
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    method, ns, logged = reference_method()
    inst = instances()
    fx = {"behaviors": np.array(BEHAVIORS), "task": np.array(TASK), "videos": np.array(list(SIZES)),
          "instances_json": np.array(json.dumps(inst))}
    with tempfile.TemporaryDirectory() as root:
        ns["gui_state"].proj.path = root
        for k, (video, n) in enumerate(SIZES.items()):
            stem = os.path.splitext(os.path.join(root, video))[0]
            os.makedirs(os.path.dirname(stem), exist_ok=True)
            open(stem + "_cls.h5", "wb").close()                  # the method only asks whether it exists
            p = probabilities(100 + k, n)
            pd.DataFrame(p, columns=BEHAVIORS).to_csv(f"{stem}_{TASK}_outputs.csv", index=False)       # backend/cbas.py:565
            fx[f"probs/{k}"] = p
        task = types.SimpleNamespace(name=TASK, behaviors=BEHAVIORS, sequence_length=31, dataset=types.SimpleNamespace(path=root))
        method(types.SimpleNamespace(device="cpu"), task, None, inst)
        with open(os.path.join(root, "disagreement_report.yaml")) as f:
            records = yaml.safe_load(f)
    warned = [m for level, m in logged if level == "WARN"]
    assert len(warned) == 2 and all("malformed" in m for m in warned), logged
    fx["records_json"] = np.array(json.dumps(records))
    fx["pandas_version"] = np.array(pd.__version__)
    out = os.path.join(args.out, "disagreement_report.npz")
    np.savez_compressed(out, **fx)
    print(f"{out}: {os.path.getsize(out)} bytes, {len(inst)} instances, {len(records)} records, pandas {pd.__version__}")


if __name__ == "__main__":
    main()
