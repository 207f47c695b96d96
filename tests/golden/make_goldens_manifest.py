#!/usr/bin/env python3
"""Generate tests/golden/train_manifest_order.npz by running the REFERENCE's manifest datasets.

Runs only where the reference tree is present (the build machine).  What is imported from the reference (nothing is
copied): ``LazyStandardDataset``, ``LazyBalancedDataset`` and ``Project.convert_instances`` of ``backend/cbas.py``,
with stub modules for the absent ``cv2`` / ``decord`` and an ``h5py`` stub whose ``File`` wraps
``cbas_amd.h5io.ClsReader`` (and records every slice it is asked for: that is the sample order).

The project is synthetic (``cbas_amd.synth.cls_project``: the same bytes on any machine) and the fixture holds recorded
results and the settings they were recorded with, nothing else:

  * the instance list handed to ``convert_instances`` (windows clipped at both file ends, a label outside ``behaviors``,
    a missing file, a file shorter than ``seq_len``, an instance without an end) and the manifest it returned;
  * for each dataset class, over three consecutive passes of one seeded ``DataLoader(shuffle=True, generator=...)``:
    ``__len__``, the (file index, centre, label) sequence and a strided sample of the window values.

Usage:  python tests/golden/make_goldens_manifest.py [--out tests/golden]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = os.environ.get("CBAS_REFERENCE", "/root/reference")

import torch  # noqa: E402

from cbas_amd import h5io, synth  # noqa: E402

# the settings of the recording (stored in the fixture; tests/test_train_manifest_host.py reads them from there)
SIZES = [300, 420, 260, 20]            # rows per file; the last one is shorter than seq_len
DIM, SEQ_LEN, SEED, BATCH, PASSES, STRIDE = 768, 31, 7, 64, 3, 4099
BEHAVIORS = ["eating", "drinking", "rearing", "climbing", "resting"]     # "climbing" (3) gets no samples
SKIP = (3,)
LOADER_SEED = 11

READS = []                            # (path, start, stop) of every slice the reference asked for, in order


class _Cls:
    def __init__(self, reader):
        self._r = reader
        self.shape = reader.shape

    def __getitem__(self, key):
        a, b, step = key.indices(self.shape[0])
        assert step == 1
        READS.append((self._r.path, a, b))
        return self._r.read(a, b)


class _File:
    """h5py.File(path, 'r') as far as the reference's datasets and convert_instances use it."""

    def __init__(self, path, mode="r"):
        assert mode == "r"
        self._r = h5io.ClsReader(path)

    def __getitem__(self, name):
        assert name == "cls"
        return _Cls(self._r)

    def close(self):
        self._r.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def import_reference():
    for name in ("cv2", "decord", "h5py"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["cv2"].VideoCapture = object
    sys.modules["decord"].VideoReader = object
    sys.modules["decord"].cpu = lambda i=0: None
    sys.modules["h5py"].File = _File
    for p in (REF, os.path.join(REF, "backend")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import cbas  # noqa
    return cbas


def instances(labels):
    """(file index, start, end, label name) - file index 4 does not exist; ends are inclusive."""
    inst = []
    for f, lab in enumerate(labels[:3]):
        inst += [(f, a, b, BEHAVIORS[c]) for a, b, c in synth.label_runs(lab)]      # run 0 / the last run are clipped by the window
    inst += [(0, 40, 44, "flying"),             # not in the behaviour list
             (1, 100, 104, " resting "),        # stripped by the reference
             (2, 50, -1, "eating"),             # no end
             (3, 2, 15, "eating"),              # file shorter than seq_len
             (4, 10, 60, "eating"),             # missing file
             (2, 250, 290, "drinking")]         # runs past the end of a 260-row file
    return inst


def record_passes(ds, paths, half):
    g = torch.Generator()
    g.manual_seed(LOADER_SEED)
    loader = torch.utils.data.DataLoader(ds, BATCH, shuffle=True, num_workers=0, generator=g)
    out = {"len": np.int64(len(ds))}
    index = {p: i for i, p in enumerate(paths)}
    for p in range(PASSES):
        del READS[:]
        labels, values = [], []
        for x, y in loader:
            labels.append(y.numpy())
            values.append(x.numpy().reshape(-1))
        out[f"pass{p}/file"] = np.array([index[r[0]] for r in READS], np.int32)
        out[f"pass{p}/centre"] = np.array([r[1] + half for r in READS], np.int32)
        out[f"pass{p}/label"] = np.concatenate(labels).astype(np.int32)
        out[f"pass{p}/values"] = np.concatenate(values)[::STRIDE].astype(np.float32)
        assert len(READS) == len(out[f"pass{p}/label"]) == len(ds)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    cbas = import_reference()
    with tempfile.TemporaryDirectory() as root:
        paths, labels = synth.cls_project(root, SIZES, DIM, len(BEHAVIORS), SEED, skip_classes=SKIP)
        paths.append(os.path.join(root, "clip4_cls.h5"))                # never written
        inst = instances(labels)
        # convert_instances takes CBAS's instance dicts: "video" is relative to the project root, <video>_cls.h5 beside it
        dicts = [{"video": f"clip{f}.mp4", "start": a, "end": b, "label": lab} for f, a, b, lab in inst]
        manifest = cbas.Project.convert_instances(None, root, dicts, SEQ_LEN, BEHAVIORS)
        index = {p: i for i, p in enumerate(paths)}
        fx = {"sizes": np.array(SIZES, np.int32), "dim": np.int32(DIM), "seq_len": np.int32(SEQ_LEN), "seed": np.int32(SEED),
              "batch": np.int32(BATCH), "passes": np.int32(PASSES), "stride": np.int32(STRIDE), "loader_seed": np.int32(LOADER_SEED),
              "behaviors": np.array(BEHAVIORS), "skip_classes": np.array(SKIP, np.int32),
              "inst/file": np.array([i[0] for i in inst], np.int32), "inst/start": np.array([i[1] for i in inst], np.int32),
              "inst/end": np.array([i[2] for i in inst], np.int32), "inst/label": np.array([i[3] for i in inst]),
              "manifest/file": np.array([index[m[0]] for m in manifest], np.int32),
              "manifest/centre": np.array([m[1] for m in manifest], np.int32),
              "manifest/label": np.array([m[2] for m in manifest], np.int32)}
        half = SEQ_LEN // 2
        for tag, ds in (("standard", cbas.LazyStandardDataset(manifest, SEQ_LEN)),
                        ("balanced", cbas.LazyBalancedDataset(manifest, SEQ_LEN, BEHAVIORS))):
            for k, v in record_passes(ds, paths, half).items():
                fx[f"{tag}/{k}"] = v
            if tag == "balanced":
                fx["balanced/counter"] = np.int64(ds.counter)
                fx["balanced/available"] = np.array(ds.available_behaviors)
        for h in cbas._worker_h5_handles.values():
            h.close()
    out = os.path.join(args.out, "train_manifest_order.npz")
    np.savez_compressed(out, **fx)
    print(f"{out}: {os.path.getsize(out)} bytes, manifest {len(manifest)} entries, "
          f"balanced len {int(fx['balanced/len'])}, torch {torch.__version__}")


if __name__ == "__main__":
    main()
