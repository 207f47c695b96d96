#!/usr/bin/env python3
"""Generate tests/golden/postprocess.npz by running the REFERENCE's post-processing of `_outputs.csv` files.

Runs only where the reference tree is present (the build machine), on the CPU.  The reference's own
``Dataset.predictions_to_instances``, ``Dataset.predictions_to_instances_with_confidence`` and ``Actogram`` (backend/cbas.py)
are imported as tests/golden/make_goldens.py imports them and called on CSV files written with pandas, the way ``infer_file``
writes them (:565), from the seeded probabilities of tests/postprocess_cases.py.  The two methods get a stand-in ``self`` that
carries ``config["behaviors"]``; ``gui_state.proj.path`` is the temporary directory.

The fixture holds the reference's outputs (as JSON) next to the pandas / scipy versions; the inputs are regenerated from the
seeds and parameters of tests/postprocess_cases.py, which asserts that no probability lies within 2^-24 relative of a threshold.

Usage:  python tests/golden/make_goldens_postprocess.py [--out tests/golden]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_goldens as MG  # noqa: E402  (sets up sys.path and the h5 / decord stand-ins)
import postprocess_cases as PC  # noqa: E402


def main():
    import pandas as pd
    import scipy
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    cbas, _ = MG.import_reference()
    import gui_state
    fx = {}
    with tempfile.TemporaryDirectory() as root:
        gui_state.proj = types.SimpleNamespace(path=root)

        def write(name, p, n_classes):
            path = os.path.join(root, name)
            pd.DataFrame(p, columns=PC.names(n_classes)).to_csv(path, index=False)          # backend/cbas.py:565
            return path

        for seed, n, n_classes, threshold in PC.EVENT_CASES:
            p = PC.probabilities(seed, n, n_classes)
            assert PC.clear_of(p, threshold), (seed, threshold)
            path = write(f"ev{seed}_{PC.MODEL}_outputs.csv", p, n_classes)
            me = types.SimpleNamespace(config={"behaviors": PC.names(n_classes)})
            got = cbas.Dataset.predictions_to_instances(me, path, PC.MODEL, threshold)
            for g in got:
                g["video"] = os.path.relpath(g["video"], root)
                g["start"], g["end"] = int(g["start"]), int(g["end"])
            fx[f"events/{seed}"] = np.array(json.dumps(got))
        for seed, n, n_classes, window in PC.BLOCK_CASES:
            p = PC.probabilities(seed, n, n_classes)
            path = write(f"bl{seed}_{PC.MODEL}_outputs.csv", p, n_classes)
            me = types.SimpleNamespace(config={"behaviors": PC.names(n_classes)})
            got, df = cbas.Dataset.predictions_to_instances_with_confidence(me, path, PC.MODEL, smoothing_window=window)
            for g in got:
                g["start"], g["end"], g["confidence"] = int(g["start"]), int(g["end"]), float(g["confidence"])
            fx[f"blocks/{seed}"] = np.array(json.dumps(got))
            fx[f"blocks/{seed}/columns"] = np.array(json.dumps([str(c) for c in df.columns]))
            if "smoothed_index" in df.columns:
                fx[f"blocks/{seed}/smoothed_index"] = df["smoothed_index"].to_numpy().astype(np.int64)
            fx[f"blocks/{seed}/block_start"] = df["block_start"].to_numpy().astype(bool)
        for seed, n, n_classes, b, threshold, framerate, minutes in PC.ACTO_DF_CASES:
            p = PC.probabilities(seed, n, n_classes)
            assert PC.clear_of(p, threshold), (seed, threshold)
            df = pd.read_csv(write(f"ac{seed}_{PC.MODEL}_outputs.csv", p, n_classes))
            acto = cbas.Actogram(PC.names(n_classes)[b], framerate, 0, minutes, threshold, "LD", preloaded_df=df)
            fx[f"acto_df/{seed}"] = np.asarray(acto.binned_activity, np.float64)
        rec = os.path.join(root, "recording")
        os.makedirs(rec)
        for k, (n_classes, b, threshold, framerate, minutes) in enumerate(PC.ACTO_DIR_CASES):
            for name, seed, n in PC.ACTO_DIR_FILES:
                p = PC.probabilities(seed, n, n_classes)
                assert PC.clear_of(p, threshold), (seed, threshold)
                pd.DataFrame(p, columns=PC.names(n_classes)).to_csv(os.path.join(rec, name), index=False)
            acto = cbas.Actogram(PC.names(n_classes)[b], framerate, 0, minutes, threshold, "LD", directory=rec, model=PC.MODEL)
            fx[f"acto_dir/{k}"] = np.asarray(acto.binned_activity, np.float64)
    fx["pandas_version"] = np.array(pd.__version__)
    fx["scipy_version"] = np.array(scipy.__version__)
    out = os.path.join(args.out, "postprocess.npz")
    np.savez_compressed(out, **fx)
    print(f"{out}: {os.path.getsize(out)} bytes, {len(fx)} entries, pandas {pd.__version__}, scipy {scipy.__version__}")


if __name__ == "__main__":
    main()
