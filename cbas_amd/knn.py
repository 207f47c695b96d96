"""Label every resident frame from its nearest labelled frames: "I have labelled a few hundred bouts; what does that say about
every frame of every recording, and how good is this encoder for my behaviours?"

    python -m cbas_amd.knn --dir RECORDINGS | --files A_cls.h5 B_cls.h5 ...
                           --instances labels.csv | --labels-yaml labels.yaml --project-root DIR
                           [--k 20] [--temperature 0.07] [--stride 1] [--group instance|file]
                           [--report report.json] [--write-outputs MODEL_NAME]

The weighted k-nearest-neighbour classifier of the self-supervised encoders (DINO, DINOv2, DINOv3): every frame of a
``search.FrameIndex`` takes its k most similar labelled frames by cosine, and each votes for its label with weight
``exp(cos / T)`` (``cbas_rows_knn``, csrc/rows_knn.hip: one fused pass, the similarity matrix is never in memory).  The ``(N, C)``
probabilities are pre-labels without a trained head - they go into ``postprocess.predictions_to_instances*``, ``activity_bins`` and
``_outputs.csv`` files as a head's would - and, with the labelled frames' own instance or file left out, a per-behaviour accuracy
report of the encoder (``knn_report``).  DESIGN.md section 20.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

MAX_BANK, MAX_K, MAX_CLASSES = 65536, 64, 64          # the limits of one cbas_rows_knn call (include/cbas_mi355x.h)
TILE, BLOCK = 128, 64                                 # csrc/rows_knn.hip: store rows per workgroup, bank entries per block
GROUPS = ("instance", "file")


class LabelBank:
    """The labelled rows of an index: ``rows`` (M, D) fp16 on the index's device, ``label`` (M) and ``group`` (M) int32 (``group``
    None when the bank was built without groups), ``row_group`` (N) int32 for the index's rows (-1: in no group), ``store_row``
    (M) int64 on the host = each bank row's row in the index, ``behaviors`` and ``dim``."""

    def __init__(self, rows, label, group, row_group, store_row, behaviors, dim, group_kind):
        self.rows, self.label, self.group, self.row_group = rows, label, group, row_group
        self.store_row, self.behaviors, self.dim, self.group_kind = store_row, list(behaviors), int(dim), group_kind

    def __len__(self) -> int:
        return int(self.store_row.shape[0])

    @classmethod
    def from_instances(cls, index, instances, behaviors: Sequence[str], stride: int = 1, group: Optional[str] = "instance") -> "LabelBank":
        """Every ``stride``-th frame of ``[start, end]`` (inside its file) of the ``(cls_path, start, end, label)`` tuples
        ``datasets.make_manifest`` takes.  Skipped, with ``make_manifest``'s warnings: labels that are not in ``behaviors``,
        instances with a start or end of -1, files the index does not hold.  ``group``: "instance" (an entry's group is its
        instance's position in ``instances``; every frame of the instance carries it in ``row_group``, a frame of two instances
        the later one's), "file" (the file's number in the index) or None."""
        stride = int(stride)
        if stride < 1:
            raise ValueError(f"stride = {stride}: at least 1")
        if group is not None and group not in GROUPS:
            raise ValueError(f"group = {group!r}: 'instance', 'file' or None")
        behaviors = list(behaviors)
        if not 1 <= len(behaviors) <= MAX_CLASSES:
            raise ValueError(f"{len(behaviors)} behaviours: cbas_rows_knn takes 1 .. {MAX_CLASSES}")
        N = index.n_rows
        row_group = np.full(N, -1, np.int32)
        if group == "file":
            for f, (first, n) in enumerate(index._table):
                row_group[first:first + n] = f
        store_row, label, grp = [], [], []
        warned = set()
        for number, (path, start, end, name) in enumerate(instances):
            f = index._by_path.get(os.path.abspath(os.fspath(path))) if path else None
            if f is None:
                if path not in warned:
                    print(f"Warning: H5 file not found, skipping instances for {path}")
                    warned.add(path)
                continue
            start, end = int(start), int(end)
            if start == -1 or end == -1:
                continue
            try:
                c = behaviors.index(str(name).strip())
            except ValueError:
                print(f"WARNING: The label '{name}' in '{path}' is not in the master behavior list. This instance will be SKIPPED.")
                continue
            first, n = int(index._table[f, 0]), int(index._table[f, 1])
            a, b = max(start, 0), min(end, n - 1)
            if b < a:
                continue
            frames = np.arange(a, b + 1, stride, dtype=np.int64)
            store_row.append(first + frames)
            label.append(np.full(frames.size, c, np.int32))
            grp.append(np.full(frames.size, number if group == "instance" else f, np.int32))
            if group == "instance":
                row_group[first + a:first + b + 1] = number
        M = int(sum(x.size for x in store_row))
        if M == 0:
            raise ValueError("the bank is empty: no instance of a known behaviour lies in a file of the index")
        if M > MAX_BANK:
            raise ValueError(f"{M} labelled frames, a bank holds {MAX_BANK}: raise stride (now {stride})")
        store_row = np.concatenate(store_row)
        dev = index.device
        rows = torch.index_select(index.rows, 0, torch.from_numpy(store_row).to(dev)).contiguous()
        return cls(rows, torch.from_numpy(np.concatenate(label)).to(dev), None if group is None else torch.from_numpy(np.concatenate(grp)).to(dev),
                   None if group is None else torch.from_numpy(row_group).to(dev), store_row, behaviors, index.dim, group)


def knn_labels(index, bank: LabelBank, k: int = 20, temperature: float = 0.07, exclude: bool = False, class_weights=None,
               return_neighbours: bool = False):
    """``probs`` (N, C) float32 on the index's device: the weighted k-NN vote of every row (``cbas_rows_knn``); with
    ``return_neighbours`` also ``nn_index`` (N, k) int32 (rows of the bank, -1 past the last) and ``nn_score`` (N, k) float32.
    ``exclude=True`` leaves out, for every row, the bank entries of its own group: leave-one-instance-out or leave-one-file-out,
    as the bank was built."""
    k = int(k)
    if index.device.type != "cuda":
        raise RuntimeError(f"the k-NN pass runs on a GPU (cbas_rows_knn); this index was built on {index.device}")
    if bank.dim != index.dim or bank.rows.device != index.device:
        raise ValueError(f"the bank holds rows of width {bank.dim} on {bank.rows.device}; the index rows of width {index.dim} on {index.device}")
    if k < 1 or k > MAX_K:
        raise ValueError(f"k = {k}: 1 .. {MAX_K}")
    if not (np.isfinite(temperature) and temperature > 0):
        raise ValueError(f"temperature = {temperature}: finite and greater than 0")
    if exclude and (bank.group is None or bank.row_group is None or int(bank.row_group.shape[0]) != index.n_rows):
        raise ValueError("exclude=True needs a bank built from this index with group='instance' or 'file'")
    C, N, M = len(bank.behaviors), index.n_rows, len(bank)
    lib = _lib.load()
    with torch.cuda.device(index.device):
        stream = torch.cuda.current_stream(index.device).cuda_stream
        cw = None
        if class_weights is not None:
            cw = torch.as_tensor(np.asarray(class_weights, np.float32)).to(index.device).contiguous()
            if tuple(cw.shape) != (C,):
                raise ValueError(f"class_weights of shape {tuple(cw.shape)}: ({C},)")
        probs = torch.empty((N, C), dtype=torch.float32, device=index.device)
        nn_index = torch.empty((N, k), dtype=torch.int32, device=index.device) if return_neighbours else None
        nn_score = torch.empty((N, k), dtype=torch.float32, device=index.device) if return_neighbours else None
        ws, need = _lib.workspace("cbas_rows_knn_workspace_bytes", index.device, N, M, k)
        _lib.check(lib.cbas_rows_knn(index.rows.data_ptr(), N, index.dim, index.dim, bank.rows.data_ptr(), M, bank.dim, bank.label.data_ptr(),
                                     bank.group.data_ptr() if exclude else None, bank.row_group.data_ptr() if exclude else None, C,
                                     None if cw is None else cw.data_ptr(), k, float(temperature), probs.data_ptr(),
                                     None if nn_index is None else nn_index.data_ptr(), None if nn_score is None else nn_score.data_ptr(),
                                     None, ws.data_ptr(), need, stream), "cbas_rows_knn")
    return (probs, nn_index, nn_score) if return_neighbours else probs


def report_from_predictions(y_true, y_pred, behaviors: Sequence[str]) -> dict:
    """``classification_report(y_true, y_pred, labels=range(C), target_names=behaviors, output_dict=True, zero_division=0)`` in
    numpy, plus ``"confusion_matrix"`` (C, C) as lists, rows the truth.  A prediction of -1 (a frame without a neighbour) is in no
    column: it counts against its behaviour's recall and the accuracy."""
    y_true, y_pred = np.asarray(y_true, np.int64), np.asarray(y_pred, np.int64)
    C = len(behaviors)
    ok = y_pred >= 0
    conf = np.zeros((C, C), np.int64)
    np.add.at(conf, (y_true[ok], y_pred[ok]), 1)
    tp = np.diag(conf).astype(np.float64)
    support = np.bincount(y_true, minlength=C).astype(np.float64)
    predicted = conf.sum(axis=0).astype(np.float64)
    precision = np.divide(tp, predicted, out=np.zeros(C), where=predicted > 0)
    recall = np.divide(tp, support, out=np.zeros(C), where=support > 0)
    f1 = np.divide(2 * precision * recall, precision + recall, out=np.zeros(C), where=precision + recall > 0)
    out = {name: {"precision": float(precision[c]), "recall": float(recall[c]), "f1-score": float(f1[c]), "support": int(support[c])}
           for c, name in enumerate(behaviors)}
    total = float(support.sum())
    out["accuracy"] = float(tp.sum() / total) if total else 0.0
    out["macro avg"] = {"precision": float(precision.mean()), "recall": float(recall.mean()), "f1-score": float(f1.mean()), "support": int(total)}
    w = support / total if total else np.zeros(C)
    out["weighted avg"] = {"precision": float((precision * w).sum()), "recall": float((recall * w).sum()), "f1-score": float((f1 * w).sum()),
                           "support": int(total)}
    out["confusion_matrix"] = conf.tolist()
    return out


def predictions_of(probs: torch.Tensor, bank: LabelBank) -> np.ndarray:
    """The first maximum (``cbas_probs_top1``) of the bank's own store rows; -1 for a row of zeros (no neighbour)."""
    from . import train as _train
    own = torch.index_select(probs, 0, torch.from_numpy(bank.store_row).to(probs.device)).contiguous()
    pred, conf, _ = _train.probs_top1(own)
    pred, conf = pred.cpu().numpy().astype(np.int64), conf.cpu().numpy()
    pred[~(conf > 0)] = -1
    return pred


def knn_report(index, bank: LabelBank, k: int = 20, temperature: float = 0.07, class_weights=None) -> dict:
    """The leave-group-out report of the bank's own frames (``report_from_predictions``): each labelled frame is classified by
    the labelled frames of the OTHER instances or files."""
    probs = knn_labels(index, bank, k=k, temperature=temperature, exclude=True, class_weights=class_weights)
    return report_from_predictions(bank.label.cpu().numpy(), predictions_of(probs, bank), bank.behaviors)


def outputs_path(cls_path: str, model_name: str) -> str:
    return cls_path.replace("_cls.h5", f"_{model_name}_outputs.csv")          # pipeline.infer_file's naming


def write_outputs(index, probs, behaviors: Sequence[str], model_name: str) -> List[str]:
    """One ``<stem>_<model_name>_outputs.csv`` per file of the index (``pipeline.write_probs_csv``); the paths."""
    from . import pipeline as _pipeline
    host = probs.detach().to("cpu", torch.float32).numpy() if torch.is_tensor(probs) else np.asarray(probs, np.float32)
    if host.shape != (index.n_rows, len(behaviors)):
        raise ValueError(f"probabilities of shape {host.shape}: ({index.n_rows}, {len(behaviors)})")
    paths = []
    for path, (first, n) in zip(index.files, index._table):
        paths.append(outputs_path(path, model_name))
        _pipeline.write_probs_csv(paths[-1], host[int(first):int(first) + int(n)], list(behaviors))
    return paths


# ---- command line ---------------------------------------------------------------------------------------------------------------
def read_instances_csv(path: str) -> Tuple[List[Tuple[str, int, int, str]], List[str]]:
    """``file,start,end,label`` lines -> the instances and the labels in order of first appearance."""
    instances, names = [], []
    with open(path, newline="") as f:
        r = csv.DictReader(f)
        if r.fieldnames is None or not {"file", "start", "end", "label"} <= set(r.fieldnames):
            raise ValueError(f"{path}: the columns file,start,end,label are needed")
        for row in r:
            instances.append((row["file"], int(row["start"]), int(row["end"]), row["label"].strip()))
            if instances[-1][3] not in names:
                names.append(instances[-1][3])
    return instances, names


def read_labels_yaml(path: str, project_root: str) -> Tuple[List[Tuple[str, int, int, str]], List[str]]:
    """CBAS's labels.yaml ``{"behaviors": [...], "labels": {behaviour: [{video, start, end, label}, ...]}}``; ``video`` becomes
    ``<stem>_cls.h5`` under ``project_root`` (absolute paths stay)."""
    import yaml
    with open(path) as f:
        doc = yaml.safe_load(f) or {}
    instances = []
    for name, items in (doc.get("labels") or {}).items():
        for it in items or []:
            video = str(it["video"])
            cls_path = os.path.splitext(video)[0] + "_cls.h5"
            if not os.path.isabs(cls_path):
                cls_path = os.path.join(project_root, cls_path)
            instances.append((cls_path, int(it["start"]), int(it["end"]), str(it.get("label", name))))
    return instances, [str(b) for b in doc.get("behaviors") or []]


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m cbas_amd.knn", description=__doc__.split("\n\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--dir", help="a directory searched for *_cls.h5 files")
    src.add_argument("--files", nargs="+", help="_cls.h5 files")
    lab = ap.add_mutually_exclusive_group(required=True)
    lab.add_argument("--instances", help="a CSV with the columns file,start,end,label")
    lab.add_argument("--labels-yaml", help="CBAS's labels.yaml (needs --project-root)")
    ap.add_argument("--project-root", default=None, help="where the videos of --labels-yaml live")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--temperature", type=float, default=0.07)
    ap.add_argument("--stride", type=int, default=1, help="every stride-th frame of an instance enters the bank")
    ap.add_argument("--group", choices=GROUPS, default="instance", help="what the report leaves out: a frame's own instance or its file")
    ap.add_argument("--report", default=None, help="write the leave-group-out report to this JSON file")
    ap.add_argument("--write-outputs", default=None, metavar="MODEL_NAME", help="write <stem>_<MODEL_NAME>_outputs.csv beside every file")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--max-gb", type=float, default=None)
    return ap


def parse_cli(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.k < 1 or a.k > MAX_K:
        ap.error(f"--k {a.k}: 1 .. {MAX_K}")
    if not (np.isfinite(a.temperature) and a.temperature > 0):
        ap.error(f"--temperature {a.temperature}: finite and greater than 0")
    if a.stride < 1:
        ap.error(f"--stride {a.stride}: at least 1")
    if a.labels_yaml and not a.project_root:
        ap.error("--labels-yaml needs --project-root")
    if not a.report and not a.write_outputs:
        ap.error("nothing to do: give --report and / or --write-outputs")
    return ap, a


def main(argv=None) -> int:
    from . import search as _search
    ap, a = parse_cli(argv)
    try:
        instances, behaviors = read_instances_csv(a.instances) if a.instances else read_labels_yaml(a.labels_yaml, a.project_root)
        index = _search.FrameIndex(a.dir if a.dir else a.files, a.device, a.max_gb)
        bank = LabelBank.from_instances(index, instances, behaviors, stride=a.stride, group=a.group)
    except (ValueError, MemoryError, OSError) as e:
        ap.error(str(e))
    print(f"{len(bank)} labelled frames of {len(behaviors)} behaviours against {index.n_rows} frames of {len(index.files)} files")
    if a.report:
        report = knn_report(index, bank, k=a.k, temperature=a.temperature)
        with open(a.report, "w") as f:
            json.dump(report, f, indent=1)
        print(f"leave-one-{a.group}-out: accuracy {report['accuracy']:.4f}, macro F1 {report['macro avg']['f1-score']:.4f} -> {a.report}")
    if a.write_outputs:
        paths = write_outputs(index, knn_labels(index, bank, k=a.k, temperature=a.temperature), behaviors, a.write_outputs)
        print(f"{len(paths)} files like {paths[0]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
