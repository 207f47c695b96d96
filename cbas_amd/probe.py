"""Fit a linear probe on the labelled frames of resident CLS rows: "how good is this encoder for my behaviours - by the number that
still ranks encoders when k-NN saturates - and can one small matrix pre-label every later recording?"

    python -m cbas_amd.probe --dir RECORDINGS | --files A_cls.h5 B_cls.h5 ...
                             --instances labels.csv | --labels-yaml labels.yaml --project-root DIR
                             [--l2 1e-4] [--iters 1000] [--stride 1] [--group instance|file] [--folds 5]
                             [--report report.json] [--save probe.npz] [--load probe.npz] [--write-outputs MODEL_NAME]

The linear evaluation of the self-supervised encoders (DINO, DINOv2, DINOv3 report it beside k-NN): softmax regression on the frozen,
normalised rows of a ``knn.LabelBank`` (``cbas_rows_probe_fit``, csrc/rows_probe.hip: Nesterov's constant-step scheme, a fixed number
of steps, everything on the device).  ``probe_labels`` gives the ``(N, C)`` probabilities of every frame of a ``search.FrameIndex``
from the ``(C, D)`` weights (``cbas_rows_probe_predict``: one streaming pass) - they go where a head's and ``knn_labels``' go - and
``probe_report`` the cross-validated report over the bank's groups, with the keys of ``knn.knn_report``.  A ``LinearProbe`` is a few
hundred kilobytes: ``save`` / ``load`` carry it to later recordings.  DESIGN.md section 22.
"""
from __future__ import annotations

import argparse
import json
import sys
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, knn as _knn

MAX_CLASSES, MAX_DIM, MAX_TRAIN = 64, 1536, 4194304   # the limits of cbas_rows_probe_* (include/cbas_mi355x.h)
SEGMENT, TILE = 1024, 128                             # CBAS_ROWS_PROBE_SEGMENT; csrc/rows_probe.hip: rows per workgroup of the pass


class LinearProbe:
    """A fitted probe: ``weights`` (C, D) and ``bias`` (C) float32, ``behaviors``, ``dim``, ``l2`` and ``iters`` of the fit, ``loss``
    (iters + 1) float32 - the objective at every step's point and, last, at the weights returned - and ``class_weights`` (C) float32
    or None."""

    def __init__(self, weights, bias, behaviors: Sequence[str], dim: int, l2: float, iters: int, loss, class_weights=None):
        self.weights = np.ascontiguousarray(weights, np.float32)
        self.bias = np.ascontiguousarray(bias, np.float32)
        self.behaviors = [str(b) for b in behaviors]
        self.dim, self.l2, self.iters = int(dim), float(l2), int(iters)
        self.loss = np.asarray(loss, np.float32)
        self.class_weights = None if class_weights is None else np.asarray(class_weights, np.float32)
        C = len(self.behaviors)
        if self.weights.shape != (C, self.dim) or self.bias.shape != (C,):
            raise ValueError(f"weights of shape {self.weights.shape} and bias of shape {self.bias.shape} for {C} behaviours of width {self.dim}")
        if self.class_weights is not None and self.class_weights.shape != (C,):
            raise ValueError(f"class_weights of shape {self.class_weights.shape}: ({C},)")

    @property
    def n_classes(self) -> int:
        return len(self.behaviors)

    def save(self, path: str) -> None:
        cw = self.class_weights
        np.savez(path, weights=self.weights, bias=self.bias, behaviors=np.array(self.behaviors, dtype=np.str_), dim=np.int64(self.dim),
                 l2=np.float64(self.l2), iters=np.int64(self.iters), loss=self.loss, has_class_weights=np.int64(cw is not None),
                 class_weights=np.zeros(0, np.float32) if cw is None else cw)

    @classmethod
    def load(cls, path: str) -> "LinearProbe":
        with np.load(path, allow_pickle=False) as z:
            return cls(z["weights"], z["bias"], z["behaviors"].tolist(), int(z["dim"]), float(z["l2"]), int(z["iters"]), z["loss"],
                       z["class_weights"] if int(z["has_class_weights"]) else None)


def balanced_weights(labels, n_classes: int, keep=None) -> np.ndarray:
    """``M / (C * count_c)`` over the entries of ``keep`` (all when None), M their number; 0 for a class with no entry."""
    labels = np.asarray(labels, np.int64)
    if keep is not None:
        labels = labels[np.asarray(keep, bool)]
    count = np.bincount(labels, minlength=n_classes).astype(np.float64)
    return np.divide(labels.size, n_classes * count, out=np.zeros(n_classes), where=count > 0).astype(np.float32)


def deal_folds(groups, folds: int) -> np.ndarray:
    """The fold of every entry: the sorted unique group ids are dealt round-robin, the i-th id to fold ``i % folds``."""
    groups = np.asarray(groups, np.int64)
    ids = np.unique(groups)
    folds = int(folds)
    if not 2 <= folds <= ids.size:
        raise ValueError(f"folds = {folds}: 2 .. the {ids.size} groups of the bank")
    return (np.searchsorted(ids, groups) % folds).astype(np.int64)


def sample_weights(labels, n_classes: int, class_weights="balanced", holdout=None):
    """``(omega, class_weights)``: omega (M) float32 or None (all ones) and the (C) float32 class weights or None."""
    labels = np.asarray(labels, np.int64)
    M = labels.size
    keep = None
    if holdout is not None:
        hold = np.asarray(holdout)
        if hold.dtype != np.bool_ or hold.shape != (M,):
            raise ValueError(f"holdout of dtype {hold.dtype} and shape {hold.shape}: a boolean ({M},)")
        keep = ~hold
    if class_weights is None:
        cw = None
    elif isinstance(class_weights, str):
        if class_weights != "balanced":
            raise ValueError(f"class_weights = {class_weights!r}: 'balanced', None or {n_classes} numbers")
        cw = balanced_weights(labels, n_classes, keep)
    else:
        cw = np.asarray(class_weights, np.float32)
        if cw.shape != (n_classes,) or not np.isfinite(cw).all() or (cw < 0).any():
            raise ValueError(f"class_weights of shape {cw.shape}: ({n_classes},) finite numbers, none negative")
    if cw is None and keep is None:
        return None, None
    omega = np.ones(M, np.float32) if cw is None else cw[labels]
    if keep is not None:
        omega = np.where(keep, omega, np.float32(0)).astype(np.float32)
    return np.ascontiguousarray(omega, np.float32), cw


def _check(index, bank) -> None:
    if index.device.type != "cuda":
        raise RuntimeError(f"the probe runs on a GPU (cbas_rows_probe_*); this index was built on {index.device}")
    if bank is not None and (bank.dim != index.dim or bank.rows.device != index.device):
        raise ValueError(f"the bank holds rows of width {bank.dim} on {bank.rows.device}; the index rows of width {index.dim} on {index.device}")


def _start(init, C: int, D: int):
    if init is None:
        return None, None
    w, b = (init.weights, init.bias) if isinstance(init, LinearProbe) else init
    w, b = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)
    if w.shape != (C, D) or b.shape != (C,):
        raise ValueError(f"init of shapes {w.shape} and {b.shape}: ({C}, {D}) and ({C},)")
    if not (np.isfinite(w).all() and np.isfinite(b).all()):
        raise ValueError("an initial weight is not finite")
    return w, b


def fit_probe(index, bank, l2: float = 1e-4, iters: int = 1000, class_weights="balanced", holdout=None, init=None) -> LinearProbe:
    """Softmax regression on the bank's rows (``cbas_rows_probe_fit``): exactly ``iters`` steps, from zeros or from ``init`` (a
    ``LinearProbe`` or ``(weights, bias)``; the momentum starts anew).  ``class_weights``: "balanced" (``M / (C * count_c)`` over the
    entries that train, 0 for a class without one), None, or C numbers; an entry's sample weight is its class's.  ``holdout``: a
    boolean (M,) array of bank entries that get weight 0 - they do not train."""
    _check(index, bank)
    iters = int(iters)
    C, D, M, dev = len(bank.behaviors), index.dim, len(bank), index.device
    if not 2 <= C <= MAX_CLASSES:
        raise ValueError(f"{C} behaviours: cbas_rows_probe_fit takes 2 .. {MAX_CLASSES}")
    if iters < 0:
        raise ValueError(f"iters = {iters}: at least 0")
    if not (np.isfinite(l2) and l2 > 0):
        raise ValueError(f"l2 = {l2}: finite and greater than 0")
    omega, cw = sample_weights(bank.label.cpu().numpy(), C, class_weights, holdout)
    w0, b0 = _start(init, C, D)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        om = None if omega is None else torch.from_numpy(omega).to(dev)
        w0d = None if w0 is None else torch.from_numpy(w0).to(dev)
        b0d = None if b0 is None else torch.from_numpy(b0).to(dev)
        weights = torch.empty((C, D), dtype=torch.float32, device=dev)
        bias = torch.empty(C, dtype=torch.float32, device=dev)
        loss = torch.empty(iters + 1, dtype=torch.float32, device=dev)
        ws, need = _lib.workspace("cbas_rows_probe_workspace_bytes", dev, M, D, C)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _lib.check(lib.cbas_rows_probe_fit(bank.rows.data_ptr(), M, D, bank.dim, bank.label.data_ptr(), ptr(om), C, float(l2), iters, ptr(w0d),
                                           ptr(b0d), weights.data_ptr(), bias.data_ptr(), loss.data_ptr(), ws.data_ptr(), need, stream),
                   "cbas_rows_probe_fit")
        return LinearProbe(weights.cpu().numpy(), bias.cpu().numpy(), bank.behaviors, D, l2, iters, loss.cpu().numpy(), cw)


def predict_rows(rows: torch.Tensor, probe: LinearProbe, return_logits: bool = False):
    """``cbas_rows_probe_predict`` on a contiguous (n, D) fp16 device tensor: ``probs`` (n, C) float32, with ``return_logits`` also
    the logits."""
    if rows.device.type != "cuda" or rows.dtype != torch.float16 or rows.dim() != 2 or not rows.is_contiguous():
        raise ValueError("rows: a contiguous (n, D) float16 tensor on a GPU")
    n, D, C, dev = int(rows.shape[0]), int(rows.shape[1]), probe.n_classes, rows.device
    if probe.dim != D:
        raise ValueError(f"the probe was fitted on rows of width {probe.dim}; these rows have width {D}")
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        w, b = torch.from_numpy(probe.weights).to(dev), torch.from_numpy(probe.bias).to(dev)
        probs = torch.empty((n, C), dtype=torch.float32, device=dev)
        logits = torch.empty((n, C), dtype=torch.float32, device=dev) if return_logits else None
        _lib.check(lib.cbas_rows_probe_predict(rows.data_ptr(), n, D, D, w.data_ptr(), b.data_ptr(), C, probs.data_ptr(),
                                               None if logits is None else logits.data_ptr(), stream), "cbas_rows_probe_predict")
    return (probs, logits) if return_logits else probs


def probe_labels(index, probe: LinearProbe, return_logits: bool = False):
    """``probs`` (N, C) float32 on the index's device: the probe's softmax of every row; with ``return_logits`` also the logits."""
    _check(index, None)
    if probe.dim != index.dim:
        raise ValueError(f"the probe was fitted on rows of width {probe.dim}; this index holds rows of width {index.dim}")
    return predict_rows(index.rows, probe, return_logits)


def probe_report(index, bank, folds: int = 5, l2: float = 1e-4, iters: int = 1000, class_weights="balanced") -> dict:
    """The cross-validated report of the bank's own frames (``knn.report_from_predictions``, the keys of ``knn.knn_report``): the
    bank's sorted unique group ids are dealt to ``folds`` folds round-robin; per fold a probe is fitted with that fold held out
    (weight 0) and predicts the held-out entries, so every labelled frame is classified by a probe that never trained on its
    instance or file."""
    if bank.group is None:
        raise ValueError("probe_report needs a bank built with group='instance' or 'file'")
    fold_of = deal_folds(bank.group.cpu().numpy(), folds)
    y_true = bank.label.cpu().numpy().astype(np.int64)
    y_pred = np.full(y_true.size, -1, np.int64)
    for f in range(int(folds)):
        hold = fold_of == f
        fitted = fit_probe(index, bank, l2=l2, iters=iters, class_weights=class_weights, holdout=hold)
        probs = predict_rows(bank.rows, fitted)
        host = probs.detach().cpu().numpy() if torch.is_tensor(probs) else np.asarray(probs)
        y_pred[hold] = host[hold].argmax(axis=1)                 # numpy: the first of equal maxima
    return _knn.report_from_predictions(y_true, y_pred, bank.behaviors)


# ---- command line ---------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m cbas_amd.probe", description=__doc__.split("\n\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--dir", help="a directory searched for *_cls.h5 files")
    src.add_argument("--files", nargs="+", help="_cls.h5 files")
    lab = ap.add_mutually_exclusive_group()
    lab.add_argument("--instances", help="a CSV with the columns file,start,end,label")
    lab.add_argument("--labels-yaml", help="CBAS's labels.yaml (needs --project-root)")
    ap.add_argument("--project-root", default=None, help="where the videos of --labels-yaml live")
    ap.add_argument("--l2", type=float, default=1e-4)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--stride", type=int, default=1, help="every stride-th frame of an instance enters the bank")
    ap.add_argument("--group", choices=_knn.GROUPS, default="instance", help="what a fold of the report holds out: whole instances or files")
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--report", default=None, help="write the cross-validated report to this JSON file")
    ap.add_argument("--save", default=None, help="write the fitted probe to this .npz")
    ap.add_argument("--load", default=None, help="label with the probe of this .npz instead of fitting (needs no labels)")
    ap.add_argument("--write-outputs", default=None, metavar="MODEL_NAME", help="write <stem>_<MODEL_NAME>_outputs.csv beside every file")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--max-gb", type=float, default=None)
    return ap


def parse_cli(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    labelled = bool(a.instances or a.labels_yaml)
    if not (np.isfinite(a.l2) and a.l2 > 0):
        ap.error(f"--l2 {a.l2}: finite and greater than 0")
    if a.iters < 0:
        ap.error(f"--iters {a.iters}: at least 0")
    if a.stride < 1:
        ap.error(f"--stride {a.stride}: at least 1")
    if a.folds < 2:
        ap.error(f"--folds {a.folds}: at least 2")
    if a.labels_yaml and not a.project_root:
        ap.error("--labels-yaml needs --project-root")
    if not a.report and not a.save and not a.write_outputs:
        ap.error("nothing to do: give --report, --save and / or --write-outputs")
    if not labelled and not a.load:
        ap.error("give --instances or --labels-yaml to fit, or --load probe.npz")
    if not labelled and (a.report or a.save):
        ap.error("--report and --save need labels: --instances or --labels-yaml")
    if a.load and a.save:
        ap.error("--save writes a fitted probe; with --load nothing is fitted")
    return ap, a


def main(argv=None) -> int:
    from . import search as _search
    ap, a = parse_cli(argv)
    bank = None
    try:
        index = _search.FrameIndex(a.dir if a.dir else a.files, a.device, a.max_gb)
        if a.instances or a.labels_yaml:
            instances, behaviors = _knn.read_instances_csv(a.instances) if a.instances else _knn.read_labels_yaml(a.labels_yaml, a.project_root)
            bank = _knn.LabelBank.from_instances(index, instances, behaviors, stride=a.stride, group=a.group)
            print(f"{len(bank)} labelled frames of {len(behaviors)} behaviours against {index.n_rows} frames of {len(index.files)} files")
        fitted = LinearProbe.load(a.load) if a.load else None
        if a.report:
            report = probe_report(index, bank, folds=a.folds, l2=a.l2, iters=a.iters)
            with open(a.report, "w") as f:
                json.dump(report, f, indent=1)
            print(f"{a.folds} folds over {a.group}s: accuracy {report['accuracy']:.4f}, macro F1 {report['macro avg']['f1-score']:.4f} -> {a.report}")
        if fitted is None and (a.save or a.write_outputs):
            fitted = fit_probe(index, bank, l2=a.l2, iters=a.iters)
            print(f"objective {fitted.loss[0]:.6f} -> {fitted.loss[-1]:.6f} in {fitted.iters} steps")
        if a.save:
            fitted.save(a.save)
        if a.write_outputs:
            paths = _knn.write_outputs(index, probe_labels(index, fitted), fitted.behaviors, a.write_outputs)
            print(f"{len(paths)} files like {paths[0]}")
    except (ValueError, MemoryError, OSError) as e:
        ap.error(str(e))
    return 0


if __name__ == "__main__":
    sys.exit(main())
