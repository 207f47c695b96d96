"""Head training on the MI355X: drop-in for the reference's ``train_lstm_model``
(backend/cbas.py:1274-1422) with the optimisation step (forward in train() mode, loss, backward,
Adam) running in the fp32 HIP kernels of libcbas_mi355x.so (``cbas_head_train_*``).

What stays on the host, exactly as in the reference: the DataLoader iteration (shuffle, collate that
drops failed samples, cbas.py:1253-1260), the per-epoch evaluation reports from scikit-learn
(cbas.py:1364-1392), early stopping on the chosen F1 (cbas.py:1394-1411) and the returned triple
``(final_model, epoch_reports, best_epoch)``.  The per-epoch evaluation runs through the HIP inference
head (``cbas_amd.head.ClassifierLSTMDeltas``).

Manifest datasets (cbas_amd.datasets, or CBAS's own LazyStandardDataset / LazyBalancedDataset, recognised by their
attribute names) are trained from rows RESIDENT in device memory: every distinct ``_cls.h5`` is read once into one
half-precision device tensor, the same DataLoaders then iterate an index-only view of the datasets (same generator,
shuffle and batch size, so the same draws and the same batches as the host loader), and each batch is a vector of
first-row indices that ``cbas_head_train_step_rows`` / ``cbas_rows_gather_windows`` expand on the device.
``CBAS_TRAIN_RESIDENT=0`` or rows that do not fit (free device memory minus 2 GiB, ``CBAS_TRAIN_RESIDENT_MAX_GB``) keep
the host loader; the ``log`` line "training data: ..." says which path runs and why.

The tail of a training job runs from the same rows: ``evaluate_on_split`` (backend/cbas.py:1222-1251) scores a split with one
``cbas_head_score_rows`` call and copies back the confusion matrix, ``fit_temperature`` (backend/workthreads.py:103-137) keeps
the logits on the device and evaluates the L-BFGS closure with ``cbas_logits_nll``; inside ``keep_rows()`` they and
``train_lstm_model`` share one store.

The last step of a job, the disagreement report (backend/workthreads.py:728-811), runs from them too: ``disagreement_report``
classifies every training clip that has no ``_outputs.csv`` yet from its resident rows, keeps the probabilities on the device
for ``cbas_probs_top1`` and ``cbas_disagreement_runs`` and writes the CSV the reference writes on a thread beside them.

Dropout keep-masks come from a counter-based hash (seed, step, layer, element) instead of torch's
global RNG, so a run is reproducible from its seed; the masks have the reference's rates (0.1 after
the three bottleneck GELUs, 0.15 after lin0's GELU).
"""
from __future__ import annotations

import contextlib
import copy
import ctypes as C
import os
import queue
import threading
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch

from . import _lib, datasets as _ds, h5io
from .config import HeadConfig
from .head import ClassifierLSTMDeltas, pack_head_weights
from .weights import head_param_shapes


def head_weight_names(cfg: HeadConfig) -> List[str]:
    names = ["gate", "attention_temp"]
    streams = ("cls", "delta", "acc") if cfg.use_acceleration else ("cls", "delta")      # classifier_head.py:74-84
    for s in streams:
        names += [f"{s}_bottleneck.0.weight", f"{s}_bottleneck.0.bias"]
    for s in streams:
        names += [f"{s}_ln.weight", f"{s}_ln.bias"]
    names += ["lin0.0.weight", "lin0.0.bias", "lin1.weight", "lin1.bias"]
    for layer in range(cfg.lstm_layers):
        for sfx in ("", "_reverse"):
            names += [f"lstm.weight_ih_l{layer}{sfx}", f"lstm.weight_hh_l{layer}{sfx}",
                      f"lstm.bias_ih_l{layer}{sfx}", f"lstm.bias_hh_l{layer}{sfx}"]
    names += ["attention_head.weight", "attention_head.bias", "lin2.weight", "lin2.bias"]
    return names


def unpack_head_weights(cfg: HeadConfig, blob: np.ndarray) -> Dict[str, np.ndarray]:
    """Inverse of ``pack_head_weights``: blob (include/cbas_mi355x.h order) -> state dict of arrays."""
    shapes = head_param_shapes(cfg)
    out, o = {}, 0
    for n in head_weight_names(cfg):
        k = int(np.prod(shapes[n])) if len(shapes[n]) else 1
        out[n] = blob[o:o + k].reshape(shapes[n]).copy()
        o += k
    if o != blob.shape[0]:
        raise ValueError(f"blob has {blob.shape[0]} floats, the config describes {o}")
    return out


class HeadTrainer:
    """One ``cbas_head_trainer`` handle: parameters, gradients and Adam state live on the device."""

    def __init__(self, cfg: HeadConfig, weights: Mapping[str, np.ndarray], device, lr: float = 1e-4,
                 weight_decay: float = 0.0, label_smoothing: float = 0.0, class_weights: Optional[Sequence[float]] = None,
                 max_batch: int = 512, seed: int = 0, dropout: bool = True):
        cfg.validate()
        if cfg.lstm_hidden_size % 16 or not 16 <= cfg.lstm_hidden_size <= 128:
            raise NotImplementedError("on-device training is built for lstm_hidden_size = 16, 32, ... 128 (train_lstm_model's "
                                      f"default is 64, sweep_runner.py uses 128); got {cfg.lstm_hidden_size}")
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"head training runs only on a GPU device (got {self.device}); there is no CPU path")
        self._lib = _lib.load()
        dev = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._cc = _lib.HeadConfigC(cfg.in_features, cfg.out_features, cfg.seq_len, cfg.bottleneck_dim, cfg.lin0_dim,
                                    cfg.lstm_hidden_size, cfg.center_window_size, cfg.ema_alpha, cfg.lstm_layers, int(cfg.use_acceleration))
        tc = _lib.TrainConfigC(float(lr), float(weight_decay), float(label_smoothing), int(max_batch), int(seed) & (2 ** 64 - 1),
                               1 if dropout else 0)
        blob = pack_head_weights(cfg, weights)
        self.n_blob = int(blob.shape[0])
        cw = None
        if class_weights is not None:
            cw = np.ascontiguousarray(np.asarray(class_weights, np.float32))
            if cw.shape != (cfg.out_features,):
                raise ValueError(f"class_weights has shape {cw.shape}, expected ({cfg.out_features},)")
        h = C.c_void_p()
        _lib.check(self._lib.cbas_head_train_create(C.byref(self._cc), C.byref(tc), blob.ctypes.data, self.n_blob,
                                                    cw.ctypes.data if cw is not None else None, dev, C.byref(h)),
                   "cbas_head_train_create")
        self._h = h
        self.max_batch = int(max_batch)

    def step(self, x: torch.Tensor, labels: torch.Tensor, update: bool = True, want_loss: bool = True):
        """One optimisation step on windows x (B, T, I) float32 and labels (B,).  Returns
        (loss, cross_entropy, covariance_penalty) when ``want_loss`` (synchronises), else None."""
        if x.dim() != 3 or x.shape[1] != self.cfg.seq_len or x.shape[2] != self.cfg.in_features:
            raise ValueError(f"expected (B, {self.cfg.seq_len}, {self.cfg.in_features}), got {tuple(x.shape)}")
        B = int(x.shape[0])
        if labels.shape != (B,):
            raise ValueError(f"labels has shape {tuple(labels.shape)}, expected ({B},)")
        x = x.to(self.device, torch.float32).contiguous()
        y = labels.to(self.device, torch.int32).contiguous()
        out = (C.c_float * 3)() if want_loss else None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.cbas_head_train_step(self._h, x.data_ptr(), y.data_ptr(), B, 1 if update else 0, out, stream),
                   "cbas_head_train_step")
        self._keep = (x, y)            # keep the inputs alive until the next call (the step is asynchronous)
        return (float(out[0]), float(out[1]), float(out[2])) if want_loss else None

    def step_rows(self, rows: torch.Tensor, first_row: torch.Tensor, labels: torch.Tensor, update: bool = True,
                  want_loss: bool = True):
        """``step`` on windows named by their first row in ``rows`` (N, I), a float16 tensor on this device: window w is
        ``rows[first_row[w] : first_row[w] + seq_len]`` converted to float32 (exact), gathered on the device into a buffer
        the trainer owns.  A row outside ``rows`` reads as zeros; callers validate their indices."""
        if rows.dim() != 2 or rows.dtype != torch.float16 or rows.device != self._index_device() or not rows.is_contiguous():
            raise ValueError(f"rows must be a contiguous float16 (N, {self.cfg.in_features}) tensor on {self.device}, got "
                             f"{rows.dtype} {tuple(rows.shape)} on {rows.device}")
        B = int(first_row.shape[0])
        if first_row.dim() != 1 or labels.shape != (B,):
            raise ValueError(f"first_row {tuple(first_row.shape)} and labels {tuple(labels.shape)} must both be ({B},)")
        f = first_row.to(self.device, torch.int64).contiguous()
        y = labels.to(self.device, torch.int32).contiguous()
        out = (C.c_float * 3)() if want_loss else None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.cbas_head_train_step_rows(self._h, rows.data_ptr(), int(rows.shape[0]), int(rows.shape[1]),
                                                       f.data_ptr(), y.data_ptr(), B, self.cfg.seq_len, 1 if update else 0, out,
                                                       stream), "cbas_head_train_step_rows")
        self._keep = (rows, f, y)
        return (float(out[0]), float(out[1]), float(out[2])) if want_loss else None

    def _index_device(self) -> torch.device:
        return torch.device("cuda", self.device.index if self.device.index is not None else torch.cuda.current_device())

    def _read(self, what: int) -> Dict[str, np.ndarray]:
        blob = np.empty(self.n_blob, np.float32)
        _lib.check(self._lib.cbas_head_train_read(self._h, what, blob.ctypes.data, self.n_blob), "cbas_head_train_read")
        self._keep_multi = []          # the read synchronised the device: no queued step reads its inputs any more
        return unpack_head_weights(self.cfg, blob)

    def weights(self) -> Dict[str, np.ndarray]:
        return self._read(0)

    def grads(self) -> Dict[str, np.ndarray]:
        return self._read(1)

    def adam_moments(self):
        """(first moment, second moment) of Adam, named like the parameters."""
        return self._read(2), self._read(3)

    def last_outputs(self, n: int):
        logits = np.empty((n, self.cfg.out_features), np.float32)
        latent = np.empty((n, 2 * self.cfg.lstm_hidden_size), np.float32)
        _lib.check(self._lib.cbas_head_train_last_outputs(self._h, logits.ctypes.data, latent.ctypes.data, n),
                   "cbas_head_train_last_outputs")
        return logits, latent

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._lib.cbas_head_train_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def step_rows_multi(rows: torch.Tensor, jobs, want_loss: bool = True):
    """One optimisation step for each of up to ``_lib.TRAIN_MULTI_MAX`` trainers from one store of rows
    (``cbas_head_train_step_rows_multi``): ``jobs`` is a sequence of ``(HeadTrainer, first_row, labels)`` as
    ``HeadTrainer.step_rows`` takes them, all trainers of one head configuration on the device of ``rows``.  Every trainer
    steps on its own stream and ends, bit for bit, where ``step_rows`` on the same windows leaves it.  Returns one
    ``(loss, cross_entropy, covariance_penalty)`` per job when ``want_loss`` (one wait for all), else None."""
    jobs = list(jobs)
    k = len(jobs)
    if not 1 <= k <= _lib.TRAIN_MULTI_MAX:
        raise ValueError(f"{k} trainers in one call: 1 to {_lib.TRAIN_MULTI_MAX} are possible")
    lead = jobs[0][0]
    if rows.dim() != 2 or rows.dtype != torch.float16 or rows.device != lead._index_device() or not rows.is_contiguous():
        raise ValueError(f"rows must be a contiguous float16 (N, {lead.cfg.in_features}) tensor on {lead.device}, got "
                         f"{rows.dtype} {tuple(rows.shape)} on {rows.device}")
    held = []
    for trainer, first_row, labels in jobs:
        B = int(first_row.shape[0])
        if first_row.dim() != 1 or labels.shape != (B,):
            raise ValueError(f"first_row {tuple(first_row.shape)} and labels {tuple(labels.shape)} must both be ({B},)")
        # a copy from pageable host memory has completed when .to() returns, so the trainer's own stream may read it
        held.append((first_row.to(trainer.device, torch.int64).contiguous(), labels.to(trainer.device, torch.int32).contiguous()))
    if any(f.device != rows.device for f, _ in held):
        raise ValueError(f"every trainer must be on the device of rows, {rows.device}")
    torch.cuda.current_stream(rows.device).synchronize()       # what the caller queued for rows / first_row / labels is done
    handles = (C.c_void_p * k)(*[t._h.value for t, _, _ in jobs])
    firsts = (C.c_void_p * k)(*[f.data_ptr() for f, _ in held])
    labs = (C.c_void_p * k)(*[y.data_ptr() for _, y in held])
    counts = (C.c_int32 * k)(*[int(f.shape[0]) for f, _ in held])
    out = (C.c_float * (3 * k))() if want_loss else None
    for (trainer, _, _), pair in zip(jobs, held):       # alive until the step that reads them has run
        trainer._keep_multi = (getattr(trainer, "_keep_multi", None) or []) + [(rows,) + pair]
    _lib.check(lead._lib.cbas_head_train_step_rows_multi(handles, k, rows.data_ptr(), int(rows.shape[0]), int(rows.shape[1]), firsts,
                                                         labs, counts, out), "cbas_head_train_step_rows_multi")
    if not want_loss:
        return None
    for (trainer, _, _), pair in zip(jobs, held):       # the call waited for every trainer: earlier inputs are free
        trainer._keep_multi = [(rows,) + pair]
    return [(float(out[3 * j]), float(out[3 * j + 1]), float(out[3 * j + 2])) for j in range(k)]


class PerformanceReport:
    """Same attribute bundle as the reference's (backend/cbas.py:1267-1272)."""

    def __init__(self, train_report: dict, train_cm: np.ndarray, val_report: dict, val_cm: np.ndarray):
        self.train_report = train_report
        self.train_cm = train_cm
        self.val_report = val_report
        self.val_cm = val_cm


def collate_fn(batch):
    """backend/cbas.py:1253-1260: drop samples whose label is -1 (failed to load)."""
    batch = [b for b in batch if int(b[1]) != -1]
    if not batch:
        return torch.tensor([]), torch.tensor([])
    dcls, lbls = zip(*batch)
    return torch.stack([torch.as_tensor(d) for d in dcls]), torch.stack([torch.as_tensor(l) for l in lbls])


def initial_head_weights(cfg: HeadConfig, seed: Optional[int] = None) -> Dict[str, np.ndarray]:
    """Fresh parameters with the reference constructor's initialisation (torch's nn.Linear / nn.LSTM /
    nn.LayerNorm defaults, gate = 0.2, attention_temp = 1.0; classifier_head.py:62-100), built from torch
    modules of the same shapes - not from the reference class."""
    g = torch.Generator()
    if seed is not None:
        g.manual_seed(int(seed))
    state = torch.random.get_rng_state()
    try:
        if seed is not None:
            torch.manual_seed(int(seed))
        I, Cn, Bn, L0, h = cfg.in_features, cfg.out_features, cfg.bottleneck_dim, cfg.lin0_dim, cfg.lstm_hidden_size
        w: Dict[str, np.ndarray] = {"gate": np.float32(0.2).reshape(()), "attention_temp": np.float32(1.0).reshape(())}
        for s in ("cls", "delta", "acc"):
            lin = torch.nn.Linear(I, Bn)
            w[f"{s}_bottleneck.0.weight"], w[f"{s}_bottleneck.0.bias"] = lin.weight.detach().numpy(), lin.bias.detach().numpy()
        for s in ("cls", "delta", "acc"):
            w[f"{s}_ln.weight"], w[f"{s}_ln.bias"] = np.ones(Bn, np.float32), np.zeros(Bn, np.float32)
        lin0 = torch.nn.Linear(3 * Bn, L0)
        w["lin0.0.weight"], w["lin0.0.bias"] = lin0.weight.detach().numpy(), lin0.bias.detach().numpy()
        att = torch.nn.Linear(2 * h, 1)
        lin1, lin2 = torch.nn.Linear(I, Cn), torch.nn.Linear(2 * h, Cn)
        lstm = torch.nn.LSTM(L0, h, num_layers=cfg.lstm_layers, batch_first=True, bidirectional=True)
        w["lin1.weight"], w["lin1.bias"] = lin1.weight.detach().numpy(), lin1.bias.detach().numpy()
        for k, v in lstm.state_dict().items():
            w[f"lstm.{k}"] = v.detach().numpy()
        w["attention_head.weight"], w["attention_head.bias"] = att.weight.detach().numpy(), att.bias.detach().numpy()
        w["lin2.weight"], w["lin2.bias"] = lin2.weight.detach().numpy(), lin2.bias.detach().numpy()
    finally:
        torch.random.set_rng_state(state)
    # (np.ascontiguousarray would promote the 0-d gate / attention_temp to shape (1,))
    return {k: np.array(v, dtype=np.float32, copy=True, order="C") for k, v in w.items()}


def _predict(model: ClassifierLSTMDeltas, loader, device, cancel_event=None):
    actual, pred = [], []
    for d, l in loader:
        if cancel_event is not None and cancel_event.is_set():
            break
        if d.numel() == 0:
            continue
        logits, _ = model(d.to(device).float())
        actual.extend(np.asarray(l.cpu().numpy()).tolist())
        pred.extend(logits.argmax(1).cpu().numpy().tolist())
    return actual, pred


def gather_windows(rows: torch.Tensor, first_row: torch.Tensor, seq_len: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[w] = rows[first_row[w] : first_row[w] + seq_len].float()`` on the device (``cbas_rows_gather_windows``):
    ``rows`` (N, D) float16, ``first_row`` (B,) int64, both on one GPU; rows outside ``rows`` read as zeros.  ``out``: a
    contiguous float32 buffer of at least B windows to reuse; the first B windows of it are returned."""
    if rows.dim() != 2 or rows.dtype != torch.float16 or not rows.is_cuda or not rows.is_contiguous():
        raise ValueError(f"rows must be a contiguous float16 (N, D) tensor on a GPU, got {rows.dtype} {tuple(rows.shape)} on {rows.device}")
    B, D = int(first_row.shape[0]), int(rows.shape[1])
    f = first_row.to(rows.device, torch.int64).contiguous()
    if out is None:
        out = torch.empty((B, seq_len, D), dtype=torch.float32, device=rows.device)
    if (out.dtype != torch.float32 or out.device != rows.device or not out.is_contiguous() or out.dim() != 3
            or out.shape[0] < B or tuple(out.shape[1:]) != (seq_len, D)):
        raise ValueError(f"out must be a contiguous float32 (>= {B}, {seq_len}, {D}) tensor on {rows.device}")
    if B:
        with torch.cuda.device(rows.device):
            stream = torch.cuda.current_stream(rows.device).cuda_stream
            _lib.check(_lib.load().cbas_rows_gather_windows(rows.data_ptr(), int(rows.shape[0]), D, f.data_ptr(), B, int(seq_len),
                                                            out.data_ptr(), stream), "cbas_rows_gather_windows")
    return out[:B]


class _IndexView(torch.utils.data.Dataset):
    """What the DataLoader iterates on the resident path: sample ``idx`` of a manifest dataset as
    ``(first row of its window in the store, label)``, or ``(-1, -1)`` for a sample the host loader would drop.  The
    manifest index comes from ``datasets.resolve_index``, so a balanced dataset's ``counter`` advances as it does under
    ``__getitem__``; nothing is read."""

    def __init__(self, dataset, seq_len: int, files):
        self.dataset = dataset
        self.first, self.label = _ds.manifest_windows(dataset.manifest, seq_len, files)

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, idx):
        m = _ds.resolve_index(self.dataset, idx)
        return int(self.first[m]), int(self.label[m])


def _collate_index(batch):
    """collate_fn for ``_IndexView``: drops the -1 samples, as ``collate_fn`` does."""
    a = np.asarray(batch, np.int64).reshape(-1, 2)
    a = a[a[:, 1] != -1]
    return torch.from_numpy(np.ascontiguousarray(a[:, 0])), torch.from_numpy(np.ascontiguousarray(a[:, 1]))


class ResidentRows:
    """The half-precision rows of every readable file of a ``datasets.StorePlan`` in one contiguous device tensor."""

    READ_ROWS = 65536

    def __init__(self, plan: "_ds.StorePlan", device):
        self.device = torch.device(device)
        self.files = dict(plan.files)
        self.dim = int(plan.dim)
        self.rows = torch.zeros((plan.total_rows, plan.dim), dtype=torch.float16, device=self.device)
        for path, (base, n) in plan.files.items():
            try:
                with h5io.ClsReader(path) as r:
                    for a in range(0, n, self.READ_ROWS):
                        b = min(n, a + self.READ_ROWS)
                        block = r.read(a, b)
                        if block.dtype != np.float16 or block.shape != (b - a, plan.dim):
                            raise OSError(f"read {block.dtype} {block.shape} for rows [{a}, {b})")
                        self.rows[base + a:base + b].copy_(torch.from_numpy(block))
            except Exception as e:  # noqa: BLE001 - a file that cannot be read gets no rows: its windows are dropped
                print(f"WORKER-ERROR: Could not read {path}. {e}")
                del self.files[path]
        self._bases = np.array([b for b, _ in self.files.values()], np.int64)
        self._ends = np.array([b + n for b, n in self.files.values()], np.int64)
        order = np.argsort(self._bases, kind="stable")
        self._bases, self._ends = self._bases[order], self._ends[order]

    def check(self, first_row: np.ndarray, seq_len: int) -> None:
        """Every window ``[first, first + seq_len)`` lies inside the rows of ONE file of the store, or ValueError."""
        first_row = np.asarray(first_row, np.int64)
        if first_row.size == 0:
            return
        f = np.searchsorted(self._bases, first_row, side="right") - 1
        ok = f >= 0
        fc = np.clip(f, 0, max(len(self._bases) - 1, 0))
        if len(self._bases):
            ok &= (first_row >= self._bases[fc]) & (first_row + seq_len <= self._ends[fc])
        else:
            ok[:] = False
        if not ok.all():
            bad = first_row[~ok]
            raise ValueError(f"{bad.size} window(s) reach outside their file's rows in the resident store (first: row {int(bad[0])})")


def _resident_budget(device) -> float:
    """Bytes the resident rows may take: free device memory minus 2 GiB of headroom, and CBAS_TRAIN_RESIDENT_MAX_GB."""
    free, _total = torch.cuda.mem_get_info(device)
    allowed = float(free) - 2.0 * 2 ** 30
    cap = os.environ.get("CBAS_TRAIN_RESIDENT_MAX_GB", "").strip()
    if cap:
        allowed = min(allowed, float(cap) * 2 ** 30)
    return allowed


def _thousands(n: int) -> str:
    return f"{n:,}".replace(",", " ")


def _plan_sets(sets, names, seq_len: int, in_features: int):
    """``(StorePlan, None)`` for manifest datasets whose half-precision rows can lie in one store, else ``(None, the
    "training data: host loader (...)" line that says why not)``."""
    if os.environ.get("CBAS_TRAIN_RESIDENT", "1").strip() == "0":
        return None, "training data: host loader (CBAS_TRAIN_RESIDENT=0)"
    for name, ds in zip(names, sets):
        if _ds.manifest_kind(ds) is None:
            return None, f"training data: host loader (the {name} set is not a manifest dataset)"
        if int(ds.seq_len) != int(seq_len):
            return None, f"training data: host loader (the {name} set has seq_len {ds.seq_len}, the model {seq_len})"
    plan = _ds.plan_store([ds.manifest for ds in sets], in_features)
    if plan.not_half:
        return None, f"training data: host loader ({plan.not_half[0]} does not hold half-precision rows)"
    if plan.total_rows == 0:
        return None, "training data: host loader (no readable _cls.h5 file in the manifests)"
    return plan, None


def _fit_line(plan, device):
    """The memory rule: ``(True, "training data: resident in HBM (...)")`` or ``(False, "... host loader (...)")``."""
    allowed = _resident_budget(device)
    if plan.nbytes > allowed:
        return False, (f"training data: host loader ({_thousands(plan.total_rows)} rows need {plan.nbytes / 1e6:.0f} MB, "
                       f"{max(allowed, 0.0) / 1e6:.0f} MB may be used)")
    return True, (f"training data: resident in HBM ({len(plan.files)} files, {_thousands(plan.total_rows)} rows, "
                  f"{plan.nbytes / 1e6:.0f} MB)")


def plan_training_data(train_set, test_set, seq_len: int, in_features: int, device):
    """Decide between rows resident in device memory and the host loader.  Returns ``(plan or None, one line that says
    which and why)``; raises ValueError for files whose row width is not ``in_features``."""
    sets = [train_set] + ([test_set] if test_set is not None and len(test_set) > 0 else [])
    plan, why_not = _plan_sets(sets, ("training", "test"), seq_len, in_features)
    if plan is None:
        return None, why_not
    fits, line = _fit_line(plan, device)
    return (plan if fits else None), line


# ---------------------------------------------------------------------------------------------------------------
# keep_rows(): one store for a whole training job
# ---------------------------------------------------------------------------------------------------------------
class _RowCache:
    """The last ``ResidentRows`` built inside a ``keep_rows()`` scope, with the size and mtime each of its files had."""

    def __init__(self):
        self.store = None
        self.stamps: Dict[str, tuple] = {}

    def drop(self):
        self.store = None
        self.stamps = {}


_row_cache: Optional[_RowCache] = None
_row_cache_lock = threading.RLock()


def _file_stamp(path: str):
    try:
        st = os.stat(path)
        return (int(st.st_size), int(st.st_mtime_ns))
    except OSError:
        return None


@contextlib.contextmanager
def keep_rows():
    """Scope in which the resident rows outlive the call that read them: ``train_lstm_model``, ``evaluate_on_split`` and
    ``fit_temperature`` keep the last store they built and reuse it when the next plan needs only files it holds, each
    with the size and mtime it had when it was read.  Any other plan builds a new store, which replaces the kept one.  The
    store is released when the OUTERMOST scope ends, also by an exception; outside a scope nothing is kept."""
    global _row_cache
    with _row_cache_lock:
        outermost = _row_cache is None
        if outermost:
            _row_cache = _RowCache()
        cache = _row_cache
    try:
        yield cache
    finally:
        if outermost:
            with _row_cache_lock:
                cache.drop()
                _row_cache = None


def _kept_store(plan, device):
    """The kept store when it can serve ``plan`` on ``device``, else None."""
    cache = _row_cache
    if cache is None or cache.store is None:
        return None
    store = cache.store
    if torch.device(store.device) != torch.device(device) or store.dim != plan.dim:
        return None
    for path, (_base, n) in plan.files.items():
        held = store.files.get(path)
        if held is None or held[1] != n or cache.stamps.get(path) is None or cache.stamps[path] != _file_stamp(path):
            return None
    return store


def open_store(sets, names, seq_len: int, in_features: int, device, log=print):
    """The resident store for the manifest datasets ``sets`` or None for the host loader; ``log`` gets the one line that
    says which.  Inside ``keep_rows()`` a kept store that holds the files is reused ("training data: kept rows ...": no
    file is read, no memory is taken) and a new one is kept."""
    plan, why_not = _plan_sets(sets, names, seq_len, in_features)
    if plan is None:
        log(why_not)
        return None
    with _row_cache_lock:
        store = _kept_store(plan, device)
        if store is not None:
            log(f"training data: kept rows reused ({len(plan.files)} of the {len(store.files)} files in device memory, "
                f"{_thousands(plan.total_rows)} rows)")
            return store
        if _row_cache is not None:
            _row_cache.drop()                           # its memory counts as free for the store that replaces it
        fits, line = _fit_line(plan, device)
        log(line)
        if not fits:
            return None
        stamps = {path: _file_stamp(path) for path in plan.files}       # before the read: a later write changes them
        store = ResidentRows(plan, device)
        if _row_cache is not None:
            _row_cache.store, _row_cache.stamps = store, stamps
        return store


def _predict_resident(model: ClassifierLSTMDeltas, loader, store: ResidentRows, seq_len: int, xbuf: torch.Tensor, cancel_event=None):
    """``_predict`` from resident rows: windows gathered into ``xbuf``, argmax kept on the device, one copy back."""
    actual, pred = [], []
    for first, labels in loader:
        if cancel_event is not None and cancel_event.is_set():
            break
        if first.numel() == 0:
            continue
        store.check(first.numpy(), seq_len)
        x = gather_windows(store.rows, first.to(store.device), seq_len, out=xbuf)
        logits, _ = model(x)
        actual.extend(labels.numpy().tolist())
        pred.append(logits.argmax(1))
    return actual, (torch.cat(pred).cpu().numpy().tolist() if pred else [])


def train_lstm_model(train_set, test_set, seq_len: int, behaviors: list, cancel_event, batch_size=512, lr=1e-4,
                     epochs=10, device=None, class_weights=None, patience=3, progress_callback=None,
                     optimization_target="weighted avg", weight_decay=0.0, label_smoothing=0.0, lstm_hidden_size=64,
                     lstm_layers=1, seed: int = 0, in_features: int = 768, log=print):
    """Same signature, control flow and return value as backend/cbas.py:1274-1422 (plus ``seed`` for the
    dropout stream / shuffling / initialisation, ``in_features`` for non-768 encoders, and ``log``)."""
    if len(train_set) == 0:
        return None, None, -1
    device = torch.device(device) if device is not None else torch.device("cuda")
    if device.type != "cuda":
        raise RuntimeError("cbas_amd.train.train_lstm_model runs on a GPU device only")
    has_test = test_set is not None and len(test_set) > 0
    store = open_store([train_set] + ([test_set] if has_test else []), ("training", "test"), seq_len, in_features, device, log)
    if store is not None:
        # the same loaders over an index-only view: the sampler's randperm, the loader's per-iterator seed draw and the
        # balanced counter are consumed exactly as on the host path, so the batches are the same, draw for draw
        train_set = _IndexView(train_set, seq_len, store.files)
        test_set = _IndexView(test_set, seq_len, store.files) if test_set is not None and len(test_set) > 0 else None
    trial = _trial(train_set, test_set, store, seq_len, behaviors, cancel_event, batch_size, lr, epochs, device, class_weights,
                   patience, progress_callback, optimization_target, weight_decay, label_smoothing, lstm_hidden_size, lstm_layers,
                   seed, in_features, log, defer_steps=False)
    try:
        next(trial)
    except StopIteration as done:
        return done.value
    raise AssertionError("a trial that takes its own steps has nothing to hand out")


def _trial(train_set, test_set, store, seq_len, behaviors, cancel_event, batch_size, lr, epochs, device, class_weights, patience,
           progress_callback, optimization_target, weight_decay, label_smoothing, lstm_hidden_size, lstm_layers, seed,
           in_features, log, defer_steps):
    """One trial of ``train_lstm_model`` as a generator whose return value is the trial's.  ``store``: the resident rows
    (``train_set`` / ``test_set`` are then ``_IndexView``s) or None for the host loader.  With ``defer_steps`` a step from
    resident rows is not taken here: the generator yields ``(trainer, first_row, labels, want_loss)`` and is sent the
    loss triple (or None), so that ``train_lstm_trials`` can take the steps of several trials in one call.  Everything else -
    the seed's three streams of randomness, scoring, selection, patience, cancel - is this one code path for both."""
    from sklearn.metrics import classification_report, confusion_matrix

    gen = torch.Generator()
    gen.manual_seed(int(seed))
    xbuf = None
    collate = collate_fn
    if store is not None:
        xbuf = torch.empty((batch_size, seq_len, in_features), dtype=torch.float32, device=device)
        collate = _collate_index
    train_loader = torch.utils.data.DataLoader(train_set, batch_size, shuffle=True, collate_fn=collate, num_workers=0,
                                               drop_last=False, generator=gen)
    test_loader = (torch.utils.data.DataLoader(test_set, batch_size, shuffle=False, collate_fn=collate, num_workers=0)
                   if test_set is not None and len(test_set) > 0 else None)
    cfg = HeadConfig(in_features=in_features, out_features=len(behaviors), seq_len=seq_len,
                     lstm_hidden_size=lstm_hidden_size, lstm_layers=lstm_layers)
    trainer = HeadTrainer(cfg, initial_head_weights(cfg, seed), device, lr=lr, weight_decay=weight_decay,
                          label_smoothing=label_smoothing, class_weights=class_weights, max_batch=batch_size, seed=seed)
    log(f"--- Training Trial Hyperparameters ---\n  Learning Rate: {lr}\n  Weight Decay: {weight_decay}\n"
        f"  Label Smoothing: {label_smoothing}\n  LSTM Hidden Size: {lstm_hidden_size}\n  LSTM Layers: {lstm_layers}")

    def eval_model() -> ClassifierLSTMDeltas:
        m = ClassifierLSTMDeltas(in_features, len(behaviors), seq_len=seq_len, lstm_hidden_size=lstm_hidden_size,
                                 lstm_layers=lstm_layers)
        m.load_state_dict(trainer.weights())
        return m.to(device).eval()

    labels_range = list(range(len(behaviors)))

    def score(loader, cancel=None):
        """(sklearn report dict, confusion matrix) of the current parameters on one loader; ({}, empty) for no data."""
        model = eval_model()
        try:
            if store is not None:
                actual, predicted = _predict_resident(model, loader, store, seq_len, xbuf, cancel)
            else:
                actual, predicted = _predict(model, loader, device, cancel)
        finally:
            model.close()
        if not actual:
            return {}, np.array([])
        report = classification_report(actual, predicted, target_names=behaviors, output_dict=True, zero_division=0,
                                       labels=labels_range)
        return report, confusion_matrix(actual, predicted, labels=labels_range)

    def f1_of(report) -> float:
        return report.get(optimization_target, {}).get("f1-score", -1.0)

    # selection state: the parameters of the best validation epoch so far, and how long it has been since
    best = {"f1": -1.0, "weights": None, "epoch": -1}
    stale_epochs = 0
    epoch_reports = []
    try:
        for epoch in range(epochs):
            if cancel_event is not None and cancel_event.is_set():
                return None, epoch_reports, best["epoch"]
            if progress_callback:
                progress_callback(f"Training Epoch {epoch + 1}/{epochs}...")
            # one pass over the shuffled windows: forward, loss, backward and Adam all inside cbas_head_train_step
            n_batches = len(train_loader)
            for i, (windows, labels) in enumerate(train_loader):
                if cancel_event is not None and cancel_event.is_set():
                    break
                if windows.numel() == 0:
                    continue
                if store is not None:                   # `windows` are first rows in the resident store
                    store.check(windows.numpy(), seq_len)
                    if defer_steps:
                        loss = yield trainer, windows, labels, i % 50 == 0
                    else:
                        loss = trainer.step_rows(store.rows, windows, labels, want_loss=(i % 50 == 0))
                else:
                    loss = trainer.step(windows.float(), labels, want_loss=(i % 50 == 0))
                if loss is not None:
                    print(f"[Epoch {epoch + 1}/{epochs} Batch {i}/{n_batches}] Loss: {loss[0]:.4f}")
            train_report, train_cm = score(train_loader)
            if not train_report:                        # nothing could be scored (every sample failed to load)
                stale_epochs += 1
                if stale_epochs >= patience:
                    break
                continue
            val_report, val_cm = score(test_loader, cancel_event) if test_loader else ({}, np.array([]))
            epoch_reports.append(PerformanceReport(train_report, train_cm, val_report, val_cm))
            val_f1 = f1_of(val_report)
            val_str = f"{val_f1:.4f}" if test_loader else "N/A"
            if progress_callback:
                progress_callback(f"Epoch {epoch + 1} Val F1: {val_str}")
            print(f"--- Epoch {epoch + 1} | Train F1: {f1_of(train_report):.4f} | Val F1: {val_str} ({optimization_target}) ---")
            if val_f1 > best["f1"]:
                best.update(f1=val_f1, weights=trainer.weights(), epoch=epoch)
                stale_epochs = 0
            else:
                stale_epochs += 1
            if test_loader and stale_epochs >= patience:
                log(f"Early stopping triggered at epoch {epoch + 1}.")
                break
        if best["weights"] is None and epochs > 0 and not test_loader:      # no validation set: keep the last epoch
            best.update(weights=trainer.weights(), epoch=epochs - 1)
    finally:
        trainer.close()
    best_state, best_epoch = best["weights"], best["epoch"]
    if best_state:
        final_model = ClassifierLSTMDeltas(in_features, len(behaviors), seq_len=seq_len, lstm_hidden_size=lstm_hidden_size,
                                           lstm_layers=lstm_layers)
        final_model.load_state_dict(best_state)
        return final_model.to(device).eval(), epoch_reports, best_epoch
    return None, None, -1


# ---------------------------------------------------------------------------------------------------------------
# the trials of a run, beside each other (backend/workthreads.py:596-690 trains num_runs x num_trials heads in sequence)
# ---------------------------------------------------------------------------------------------------------------
def _own_counter(dataset):
    """``dataset`` for one trial: a balanced dataset draws its classes round-robin from a ``counter`` on the instance, so
    every trial counts on a shallow copy of its own (manifest and buckets shared) from where the caller's stands."""
    return copy.copy(dataset) if _ds.manifest_kind(dataset) == "balanced" else dataset


def _run_trial_slots(seeds, max_concurrent: int, start, step_many) -> list:
    """The slot scheduler of ``train_lstm_trials``.  ``start(seed)`` gives a ``_trial``-style generator: it yields step
    requests, is sent each step's loss and returns the trial's result.  At most ``max_concurrent`` generators are alive; in
    every round ``step_many([request, ...])`` takes one step for each of them (in seed order) and returns their losses; a
    trial that returns frees its slot for the next seed.  Returns the results in seed order."""
    results = [None] * len(seeds)
    waiting = list(enumerate(seeds))
    alive: Dict[int, list] = {}                     # position in seeds -> [generator, its pending request]

    def advance(i, trial, loss):
        try:
            alive[i] = [trial, trial.send(loss)]
        except StopIteration as done:
            alive.pop(i, None)
            results[i] = done.value

    try:
        while waiting or alive:
            while waiting and len(alive) < max_concurrent:
                i, seed = waiting.pop(0)
                advance(i, start(seed), None)
            if alive:
                order = sorted(alive)
                losses = step_many([alive[i][1] for i in order])
                for i, loss in zip(order, losses):
                    advance(i, alive[i][0], loss)
    finally:
        for trial, _ in alive.values():             # an exception: every trial still releases its trainer
            trial.close()
    return results


def train_lstm_trials(train_set, test_set, seq_len: int, behaviors: list, cancel_event, *, trial_seeds: Sequence[int],
                      max_concurrent: int = 4, batch_size=512, lr=1e-4, epochs=10, device=None, class_weights=None, patience=3,
                      progress_callback=None, optimization_target="weighted avg", weight_decay=0.0, label_smoothing=0.0,
                      lstm_hidden_size=64, lstm_layers=1, in_features: int = 768, log=print) -> list:
    """The trials of one run - same sets and hyper-parameters, one seed each - trained beside each other from ONE resident row
    store: ``[(model | None, epoch_reports | None, best_epoch), ...]`` in the order of ``trial_seeds``, entry i being what
    ``train_lstm_model(..., seed=trial_seeds[i])`` returns when it is called alone (weights bit for bit, reports, best
    epoch; "alone" for a balanced dataset: with its ``counter`` where it stands at this call).

    Up to ``max_concurrent`` (1..8) trainers are alive at a time, each on a stream of its own in this process; their steps go
    out together (``cbas_head_train_step_rows_multi``); a trial that ends - its epochs, its patience, ``cancel_event`` - frees
    its slot for the next seed.  When the rows cannot be resident (``CBAS_TRAIN_RESIDENT=0``, rows that do not fit, datasets
    that are no manifest datasets) the trials run one after another through ``train_lstm_model`` and ``log`` gets one line
    that says why."""
    seeds = [int(s) for s in trial_seeds]
    if isinstance(max_concurrent, bool) or int(max_concurrent) != max_concurrent or not 1 <= max_concurrent <= _lib.TRAIN_MULTI_MAX:
        raise ValueError(f"max_concurrent={max_concurrent!r}: 1 to {_lib.TRAIN_MULTI_MAX} trials can train beside each other")
    if not seeds:
        return []
    if len(train_set) == 0:
        return [(None, None, -1) for _ in seeds]
    device = torch.device(device) if device is not None else torch.device("cuda")
    if device.type != "cuda":
        raise RuntimeError("cbas_amd.train.train_lstm_trials runs on a GPU device only")
    has_test = test_set is not None and len(test_set) > 0
    said = []
    store = open_store([train_set] + ([test_set] if has_test else []), ("training", "test"), seq_len, in_features, device, said.append)
    if store is None:
        why = said[-1][said[-1].index("(") + 1:said[-1].rindex(")")]
        log(f"training trials: {len(seeds)} one after another ({why})")
        return [train_lstm_model(_own_counter(train_set), _own_counter(test_set), seq_len, behaviors, cancel_event,
                                 batch_size=batch_size, lr=lr, epochs=epochs, device=device, class_weights=class_weights,
                                 patience=patience, progress_callback=progress_callback, optimization_target=optimization_target,
                                 weight_decay=weight_decay, label_smoothing=label_smoothing, lstm_hidden_size=lstm_hidden_size,
                                 lstm_layers=lstm_layers, seed=seed, in_features=in_features, log=log) for seed in seeds]
    for line in said:
        log(line)
    log(f"training trials: {len(seeds)} on one row store, up to {int(max_concurrent)} beside each other")
    # one window table per set, shared by all trials
    train_view = _IndexView(train_set, seq_len, store.files)
    test_view = _IndexView(test_set, seq_len, store.files) if has_test else None

    def view_of(view):
        if view is None:
            return None
        mine = copy.copy(view)
        mine.dataset = _own_counter(view.dataset)
        return mine

    def start(seed):
        return _trial(view_of(train_view), view_of(test_view), store, seq_len, behaviors, cancel_event, batch_size, lr, epochs,
                      device, class_weights, patience, progress_callback, optimization_target, weight_decay, label_smoothing,
                      lstm_hidden_size, lstm_layers, seed, in_features, log, defer_steps=True)

    def step_many(requests):
        wanted = [want for _, _, _, want in requests]
        losses = step_rows_multi(store.rows, [(t, first, labels) for t, first, labels, _ in requests], want_loss=any(wanted))
        return [loss if want else None for loss, want in zip(losses or [None] * len(requests), wanted)]

    return _run_trial_slots(seeds, int(max_concurrent), start, step_many)


# ---------------------------------------------------------------------------------------------------------------
# the tail of a training job: the held-out split and the calibration temperature (backend/workthreads.py:671-677, 838-852)
# ---------------------------------------------------------------------------------------------------------------
def _resident_for(model, dataset, name: str, device):
    """The store to score ``dataset`` from with ``model``, or None for the host loader."""
    if not isinstance(model, ClassifierLSTMDeltas) or device.type != "cuda" or _ds.manifest_kind(dataset) is None:
        return None
    if len(dataset) == 0:
        return None
    return open_store([dataset], (name,), model.seq_len, model.in_features, device, print)


def evaluate_on_split(model, dataset, behaviors, device=None):
    """backend/cbas.py:1222-1251: ``{"report": sklearn's classification_report dict, "cm": confusion matrix}`` of ``model`` on
    ``dataset``, ``{"report": {}, "cm": np.array([])}`` when nothing could be scored.  A manifest dataset is scored from rows
    resident in device memory (``cbas_head_score_rows``: one call for the split, the confusion matrix is all that comes back);
    anything else, or ``CBAS_TRAIN_RESIDENT=0``, takes the reference's loop over a host ``DataLoader``.  The report is a
    function of the confusion matrix alone, so both paths return equal reports."""
    from sklearn.metrics import classification_report, confusion_matrix

    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    labels_range = range(len(behaviors))
    store = _resident_for(model, dataset, "test", device)
    model.to(device).eval()
    if store is not None:
        loader = torch.utils.data.DataLoader(_IndexView(dataset, model.seq_len, store.files), batch_size=512, shuffle=False,
                                             num_workers=0, collate_fn=_collate_index)
        batches = [(f, l) for f, l in loader if f.numel()]
        if not batches:
            return {"report": {}, "cm": np.array([])}
        first, labels = torch.cat([f for f, _ in batches]), torch.cat([l for _, l in batches])
        store.check(first.numpy(), model.seq_len)
        _, _, confusion = model.score_rows(store.rows, first, labels)
        cm = confusion.cpu().numpy().astype(np.int64)
        true_idx, pred_idx = np.nonzero(cm)
        y_true, y_pred = np.repeat(true_idx, cm[true_idx, pred_idx]), np.repeat(pred_idx, cm[true_idx, pred_idx])
    else:
        loader = torch.utils.data.DataLoader(dataset, batch_size=512, shuffle=False, num_workers=0, collate_fn=collate_fn)
        y_true, y_pred = [], []
        with torch.no_grad():
            for x, y in loader:
                valid = (y != -1)
                if not valid.any():
                    continue
                logits, _ = model(x[valid].to(device))
                y_true.extend(y[valid].cpu().numpy())
                y_pred.extend(logits.argmax(1).cpu().numpy())
        if not y_true:
            return {"report": {}, "cm": np.array([])}
        cm = confusion_matrix(y_true, y_pred, labels=labels_range)
    rep = classification_report(y_true, y_pred, target_names=behaviors, output_dict=True, zero_division=0, labels=labels_range)
    return {"report": rep, "cm": cm}


def lbfgs_scalar(closure, x0, lr: float = 1.0, max_iter: int = 20, max_eval: Optional[int] = None, tolerance_grad: float = 1e-7,
                 tolerance_change: float = 1e-9, history_size: int = 100):
    """One ``torch.optim.LBFGS([x], lr, max_iter, ...).step(closure)`` without line search, for ONE float32 parameter,
    statement for statement: the same evaluations in the same order, the same stopping tests, every quantity that is a
    float32 tensor there a float32 here (a one-element dot product is a product).  ``closure(x)`` returns
    ``(loss, d loss / d x)`` at the float32 ``x``.  Returns ``(x, iterations, closure calls)``."""
    f32 = np.float32
    if max_eval is None:
        max_eval = max_iter * 5 // 4                      # torch's default
    tol_grad, tol_change = f32(tolerance_grad), f32(tolerance_change)

    def evaluate(x):
        loss, grad = closure(x)
        return float(f32(loss)), f32(grad)

    x = f32(x0)
    loss, g = evaluate(x)
    evals, n_iter = 1, 0
    if abs(g) <= tol_grad:
        return x, n_iter, evals
    old_dirs, old_stps, ro = [], [], []
    d = t = prev_g = None
    h_diag = f32(1.0)
    with np.errstate(all="ignore"):
        while n_iter < max_iter:
            n_iter += 1
            # the direction: -H g by the two-loop recursion over the (y, s) pairs kept so far
            if n_iter == 1:
                d = -g
            else:
                y = f32(g - prev_g)
                s = f32(d * t)
                ys = f32(y * s)
                if ys > f32(1e-10):
                    if len(old_dirs) == history_size:
                        old_dirs.pop(0), old_stps.pop(0), ro.pop(0)
                    old_dirs.append(y), old_stps.append(s), ro.append(f32(f32(1.0) / ys))
                    h_diag = f32(ys / f32(y * y))
                k = len(old_dirs)
                al = [None] * k
                q = f32(-g)
                for i in range(k - 1, -1, -1):
                    al[i] = f32(f32(old_stps[i] * q) * ro[i])
                    q = f32(q + f32(old_dirs[i] * f32(-al[i])))
                d = f32(q * h_diag)
                for i in range(k):
                    be_i = f32(f32(old_dirs[i] * d) * ro[i])
                    d = f32(d + f32(old_stps[i] * f32(al[i] - be_i)))
            prev_g, prev_loss = g, loss
            # the step length: lr, scaled down by the gradient's size in the first iteration
            if n_iter == 1:
                inv = f32(f32(1.0) / abs(g))
                t = f32(inv * f32(lr)) if inv < 1.0 else f32(lr)
            else:
                t = f32(lr)
            if f32(g * d) > -tol_change:                  # the directional derivative is below the tolerance
                break
            x = f32(x + f32(d * t))
            evaluated = 0
            if n_iter != max_iter:
                loss, g = evaluate(x)
                evaluated = 1
            evals += evaluated
            if n_iter == max_iter or evals >= max_eval:
                break
            if abs(g) <= tol_grad:
                break
            if abs(f32(d * t)) <= tol_change:
                break
            if abs(loss - prev_loss) < tolerance_change:
                break
    return x, n_iter, evals


def calibration_temperature(T) -> np.float32:
    """``clamp(softplus(T) + 1e-3, max=10)`` of workthreads.py:130 and :136, in float32 with torch's own softplus."""
    t = torch.as_tensor(np.float32(T))
    return np.float32(torch.clamp(torch.nn.functional.softplus(t) + 1e-3, max=10.0).item())


def calibration_chain(T) -> np.float32:
    """d calibration_temperature / d T as autograd forms it: softplus' derivative ``z / (z + 1)``, ``z = exp(T)`` (1 beyond
    torch's threshold of 20), and the clamp, which passes the gradient on where its input is <= 10."""
    t = torch.as_tensor(np.float32(T))
    if float(torch.nn.functional.softplus(t) + 1e-3) > 10.0:
        return np.float32(0.0)
    if float(t) > 20.0:
        return np.float32(1.0)
    z = torch.exp(t)
    return np.float32((z / (z + 1.0)).item())


FIT_TEMPERATURE_LBFGS = dict(lr=0.01, max_iter=50)        # workthreads.py:111; everything else torch's default
FIT_TEMPERATURE_START = 1.0                               # workthreads.py:110


def fit_temperature_from(mean_nll_and_slope):
    """The fit of workthreads.py:110-137 given ``mean_nll_and_slope(temp) -> (mean cross-entropy of logits / temp, its
    derivative with respect to temp)``.  Returns ``(temperature as a Python float, iterations, closure calls)``."""
    def closure(T):
        loss, slope = mean_nll_and_slope(calibration_temperature(T))
        return loss, np.float32(np.float32(slope) * calibration_chain(T))

    T, n_iter, evals = lbfgs_scalar(closure, FIT_TEMPERATURE_START, **FIT_TEMPERATURE_LBFGS)
    return float(calibration_temperature(T)), n_iter, evals


def device_nll(logits: torch.Tensor, labels: torch.Tensor):
    """``temp -> (loss, d loss / d temp)`` over logits (n, C) float32 and labels (n,) that stay on the device: one
    ``cbas_logits_nll`` launch and one 8-byte copy per call."""
    if logits.dim() != 2 or not logits.is_cuda or logits.shape[0] < 1:
        raise ValueError(f"logits must be a (n >= 1, C) tensor on a GPU, got {tuple(logits.shape)} on {logits.device}")
    logits = logits.detach().to(torch.float32).contiguous()
    y = labels.to(logits.device, torch.int32).contiguous()
    n, n_classes = int(logits.shape[0]), int(logits.shape[1])
    if tuple(y.shape) != (n,):
        raise ValueError(f"labels has shape {tuple(y.shape)}, expected ({n},)")
    lo, hi = int(y.min()), int(y.max())
    if lo < 0 or hi >= n_classes:
        raise ValueError(f"labels span [{lo}, {hi}], the logits have {n_classes} classes")
    lib = _lib.load()
    out2 = torch.empty(2, dtype=torch.float32, device=logits.device)

    def mean_nll_and_slope(temp):
        with torch.cuda.device(logits.device):
            stream = torch.cuda.current_stream(logits.device).cuda_stream
            _lib.check(lib.cbas_logits_nll(logits.data_ptr(), y.data_ptr(), n, n_classes, float(temp), out2.data_ptr(), stream),
                       "cbas_logits_nll")
        v = out2.cpu().numpy()
        return np.float32(v[0]), np.float32(v[1])

    return mean_nll_and_slope


def _loader_index_batches(loader):
    """The index batches a DataLoader would draw, in its order (its batch sampler, or its sampler one by one)."""
    if getattr(loader, "batch_sampler", None) is not None:
        return iter(loader.batch_sampler)
    return ([i] for i in loader.sampler)


def fit_temperature(model, val_loader, device):
    """backend/workthreads.py:103-137: the calibration temperature ``infer_file`` divides the logits by, as a Python float
    (1.0 for an empty loader).  The logits stay on the device: a manifest dataset behind ``val_loader`` is scored from
    resident rows in the loader's order, anything else by iterating the loader as the reference does.  The loss and its
    derivative come from ``cbas_logits_nll`` (summed in a fixed order), the optimiser is ``lbfgs_scalar``.  A window the
    store cannot serve is a ValueError that names its file (the reference fails on its label -1 inside the loss)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"cbas_amd.train.fit_temperature runs on a GPU device only (got {device}); there is no CPU path")
    model.to(device)
    model.eval()
    dataset = getattr(val_loader, "dataset", None)
    store = _resident_for(model, dataset, "validation", device)
    if store is not None:
        seq_len = model.seq_len
        first_of, label_of = _ds.manifest_windows(dataset.manifest, seq_len, store.files)
        first, labels = [], []
        for batch in _loader_index_batches(val_loader):
            for idx in batch:
                m = _ds.resolve_index(dataset, idx)
                if first_of[m] < 0:
                    path, centre = dataset.manifest[m][0], dataset.manifest[m][1]
                    raise ValueError(f"fit_temperature: the window of frame {centre} of {path} cannot be read (its file is "
                                     f"unreadable or the window reaches outside it); calibrating on the rest would not be "
                                     f"what the reference computes")
                first.append(int(first_of[m]))
                labels.append(int(label_of[m]))
        if not first:
            return 1.0
        first = np.asarray(first, np.int64)
        store.check(first, seq_len)
        logits, _, _ = model.score_rows(store.rows, torch.from_numpy(first), want_logits=True)
        labels = torch.from_numpy(np.asarray(labels, np.int64))
    else:
        all_logits, all_labels = [], []
        with torch.no_grad():
            for d, l in val_loader:
                logits, _ = model(d.to(device))
                all_logits.append(logits)
                all_labels.append(l)
        if not all_logits:
            return 1.0
        logits, labels = torch.cat(all_logits).detach(), torch.cat(all_labels)
    temperature, _, _ = fit_temperature_from(device_nll(logits, labels))
    return temperature


# ---------------------------------------------------------------------------------------------------------------
# the disagreement report (backend/workthreads.py:728-811): where the trained head and the human labels differ
# ---------------------------------------------------------------------------------------------------------------
RUN_DTYPE = np.dtype([("instance", "<i4"), ("start_frame", "<i4"), ("end_frame", "<i4"), ("model_prediction", "<i4"),
                      ("model_confidence", "<f8")])          # cbas_disagreement_run of include/cbas_mi355x.h
TOP1_FLAG_NAN = 1                                           # CBAS_TOP1_FLAG_NAN


def name_ranks(behaviors: Sequence[str]) -> np.ndarray:
    """``rank[c]`` = position of ``behaviors[c]`` among the sorted names: pandas' ``mode()`` returns its values sorted and the
    reference takes the first (workthreads.py:794), so equally frequent predictions are decided by name."""
    rank = np.empty(len(behaviors), np.int32)
    rank[sorted(range(len(behaviors)), key=lambda c: behaviors[c])] = np.arange(len(behaviors), dtype=np.int32)
    return rank


def disagreement_runs_host(pred: np.ndarray, conf: np.ndarray, start: int, end: int, label: int, name_rank: np.ndarray) -> list:
    """workthreads.py:777-803 for ONE instance of a clip whose per-frame prediction (class index, -1 for none) and confidence
    are ``pred`` / ``conf``: ``[(start_frame, end_frame, model_prediction, model_confidence)]``, one entry per maximal run of
    consecutive frames of ``iloc[start:end+1]`` (negative bounds count from the end, as there) whose prediction is not
    ``label`` (-1: a label that is no behaviour, every frame differs).  The prediction of a run is its most frequent one, ties
    to the smallest ``name_rank``; its confidence the float64 mean, summed in ascending frame order."""
    frames = np.arange(len(pred))[start:end + 1]
    if frames.size == 0:
        return []
    wrong = frames[np.ones(frames.size, bool) if label < 0 else pred[frames] != label]
    if wrong.size == 0:
        return []
    out = []
    for run in np.split(wrong, np.flatnonzero(np.diff(wrong) != 1) + 1):
        p = pred[run]
        counts = np.bincount(p[p >= 0], minlength=len(name_rank))
        best = np.flatnonzero(counts == counts.max()) if counts.max() > 0 else np.empty(0, np.int64)
        winner = int(best[np.argmin(name_rank[best])]) if best.size else -1
        mean = float(np.cumsum(np.asarray(conf[run], np.float64))[-1] / run.size)
        out.append((int(run[0]), int(run[-1]), winner, mean))
    return out


def probs_top1(probs: torch.Tensor, pred: Optional[torch.Tensor] = None, conf: Optional[torch.Tensor] = None,
               flags: Optional[torch.Tensor] = None):
    """``cbas_probs_top1``: ``(pred int32 (n,), conf float32 (n,), flags int32 (1,))`` of device probabilities (n, C): the first
    index of each row's maximum and the maximum; a row with a NaN gets -1 / NaN and sets ``TOP1_FLAG_NAN`` in ``flags``
    (OR-ed into a word the caller passes).  Asynchronous on the current stream."""
    if probs.dim() != 2 or probs.dtype != torch.float32 or not probs.is_cuda or not probs.is_contiguous() or probs.shape[0] < 1:
        raise ValueError(f"probs must be a contiguous float32 (n >= 1, C) tensor on a GPU, got {probs.dtype} {tuple(probs.shape)} on {probs.device}")
    n = int(probs.shape[0])
    pred = torch.empty(n, dtype=torch.int32, device=probs.device) if pred is None else pred
    conf = torch.empty(n, dtype=torch.float32, device=probs.device) if conf is None else conf
    flags = torch.zeros(1, dtype=torch.int32, device=probs.device) if flags is None else flags
    for t, dt in ((pred, torch.int32), (conf, torch.float32)):
        if t.dtype != dt or t.device != probs.device or tuple(t.shape) != (n,) or not t.is_contiguous():
            raise ValueError(f"pred / conf must be contiguous ({n},) int32 / float32 tensors on {probs.device}")
    if flags.dtype != torch.int32 or flags.device != probs.device or flags.numel() != 1:
        raise ValueError(f"flags must be one int32 word on {probs.device}")
    with torch.cuda.device(probs.device):
        stream = torch.cuda.current_stream(probs.device).cuda_stream
        _lib.check(_lib.load().cbas_probs_top1(probs.data_ptr(), n, int(probs.shape[1]), pred.data_ptr(), conf.data_ptr(),
                                               flags.data_ptr(), stream), "cbas_probs_top1")
    return pred, conf, flags


def disagreement_runs(pred: torch.Tensor, conf: torch.Tensor, clip_table, clip, start, end, label, name_rank) -> np.ndarray:
    """``cbas_disagreement_runs``: the records (``RUN_DTYPE``, ordered by instance and run start) of the instances
    ``(clip[i], start[i], end[i], label[i])`` over the per-frame ``pred`` (int32) / ``conf`` (float32) of all clips back to back
    on one GPU; ``clip_table`` (n_clips, 2) = (first frame, frames) per clip.  The semantics are those of
    ``disagreement_runs_host`` for ``0 <= start <= end``; anything else is refused."""
    dev = pred.device
    if pred.dtype != torch.int32 or conf.dtype != torch.float32 or not pred.is_cuda or conf.device != dev or pred.shape != conf.shape \
            or pred.dim() != 1 or not pred.is_contiguous() or not conf.is_contiguous():
        raise ValueError("pred (int32) and conf (float32) must be contiguous 1-d tensors of one length on one GPU")
    table = np.ascontiguousarray(np.asarray(clip_table, np.int64).reshape(-1, 2))
    arrays = [np.ascontiguousarray(np.asarray(a, np.int32)) for a in (clip, start, end, label)]
    rank = np.ascontiguousarray(np.asarray(name_rank, np.int32))
    n_inst = int(arrays[0].shape[0])
    if any(a.shape != (n_inst,) for a in arrays) or n_inst < 1 or table.shape[0] < 1:
        raise ValueError("clip, start, end and label must be four 1-d arrays of one length >= 1, the table (n_clips >= 1, 2)")
    # a run needs an error frame and, before the next run, a frame that is none: at most (frames + 1) // 2 per instance
    frames_of = table[np.clip(arrays[0], 0, table.shape[0] - 1), 1]
    length = np.clip(np.minimum(arrays[2].astype(np.int64), frames_of - 1) - arrays[1] + 1, 0, None)
    capacity = max(1, int(((length + 1) // 2).sum()))
    dev_arrays = [torch.from_numpy(a).to(dev) for a in [table] + arrays + [rank]]
    records = torch.empty(capacity * RUN_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    needed = C.c_int64(0)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        n = _lib.load().cbas_disagreement_runs(pred.data_ptr(), conf.data_ptr(), int(pred.shape[0]), dev_arrays[0].data_ptr(),
                                               int(table.shape[0]), dev_arrays[1].data_ptr(), dev_arrays[2].data_ptr(),
                                               dev_arrays[3].data_ptr(), dev_arrays[4].data_ptr(), n_inst, dev_arrays[5].data_ptr(),
                                               int(rank.shape[0]), records.data_ptr(), capacity, C.byref(needed), stream)
    if n < 0:
        _lib.check(int(n), "cbas_disagreement_runs")
    return records[:n * RUN_DTYPE.itemsize].cpu().numpy().view(RUN_DTYPE).copy()


def _read_outputs_csv(path: str, behaviors: Sequence[str]) -> np.ndarray:
    """The behaviour columns of an ``_outputs.csv`` as float64 (n, C), selected by name as ``pred_df[task.behaviors]`` does
    (workthreads.py:761-763); an empty field is NaN.  Raises when a column is missing or a field is no number."""
    from .pipeline import read_outputs_csv
    header, values, _ = read_outputs_csv(path)
    if not header:
        raise ValueError("empty file")
    cols = [header.index(b) for b in behaviors]                       # ValueError: a behaviour without a column
    return np.ascontiguousarray(values[:, cols])


class _CsvWriter:
    """The thread that writes the ``_outputs.csv`` files while the device classifies the next clip: it waits for the event
    behind a clip's device-to-host copy, then runs the native writer.  ``failed``: the clips whose file could not be written."""

    def __init__(self, behaviors):
        self.behaviors = list(behaviors)
        self.failed: Dict[int, Exception] = {}
        self._q: "queue.Queue" = queue.Queue()
        self._t = threading.Thread(target=self._run, name="cbas-report-csv", daemon=True)
        self._t.start()

    def _run(self):
        from .pipeline import write_probs_csv
        while True:
            item = self._q.get()
            if item is None:
                return
            k, path, host, event = item
            try:
                event.synchronize()
                write_probs_csv(path, host.numpy(), self.behaviors)
            except Exception as e:  # noqa: BLE001 - reported by the caller, which drops the clip as infer_file's failure does
                self.failed[k] = e

    def put(self, k: int, path: str, host: torch.Tensor, event) -> None:
        self._q.put((k, path, host, event))

    def close(self) -> None:
        self._q.put(None)
        self._t.join()


def _kept_rows_of(path: str, dim: int, device):
    """``(store, (base, n))`` for ``path`` in the store kept by the enclosing ``keep_rows()`` when that store holds the file as
    it is on disk now, else None."""
    with _row_cache_lock:
        cache = _row_cache
        if cache is None or cache.store is None:
            return None
        store = cache.store
        held = store.files.get(path)
        if held is None or torch.device(store.device) != torch.device(device) or store.dim != dim:
            return None
        if cache.stamps.get(path) is None or cache.stamps[path] != _file_stamp(path):
            return None
        return store, held


def _clip_rows(path: str, dim: int, device, log, what: str = "disagreement report"):
    """The half-precision rows of one ``_cls.h5`` on ``device``: a view of the kept store, or the file uploaded once.  None
    (with the reason logged) when the file is not what the device path takes: the caller hands the clip to ``infer_file``."""
    kept = _kept_rows_of(path, dim, device)
    if kept is not None:
        store, (base, n) = kept
        return store.rows[base:base + n]
    try:
        with h5io.ClsReader(path) as r:
            shape, half = tuple(r.shape), bool(r.is_half)
            if len(shape) != 2 or shape[1] != dim or not half or shape[0] == 0:
                return None
            if shape[0] * dim * 2 > _resident_budget(device):
                log(f"{what}: {path} does not fit in device memory, classified through infer_file")
                return None
            rows = torch.empty((shape[0], dim), dtype=torch.float16, device=device)
            for a in range(0, shape[0], ResidentRows.READ_ROWS):
                b = min(shape[0], a + ResidentRows.READ_ROWS)
                rows[a:b].copy_(torch.from_numpy(r.read(a, b)))
            return rows
    except Exception:  # noqa: BLE001 - infer_file reports what is wrong with the file
        return None


def disagreement_report(model, train_insts, behaviors, seq_len: int, project_path: str, task_name: str, device=None,
                        log=print) -> List[dict]:
    """``TrainingThread._generate_disagreement_report`` (backend/workthreads.py:728-805) up to the sort: for every training
    instance ``{"video", "start", "end", "label"}`` the runs of frames where ``model`` disagrees with the label, as
    ``{"video_path", "start_frame", "end_frame", "human_label", "model_prediction", "model_confidence"}``, sorted by
    confidence, highest first (stable: videos by first appearance, instances in list order, runs ascending).

    A clip that has a ``<video>_<task_name>_outputs.csv`` is read from it, as the reference does.  Any other clip is classified
    at temperature 1.0 (:753-756 passes none) and its CSV is written, byte for byte what ``infer_file`` writes: on a GPU with
    this package's head the rows come from the store kept by ``keep_rows()`` (or are uploaded once), the probabilities stay on
    the device for ``cbas_probs_top1`` and ONE ``cbas_disagreement_runs`` call over all clips, and a thread writes the files
    meanwhile.  ``CBAS_TRAIN_RESIDENT=0``, another device or head, or a file the store cannot take, go through ``infer_file``
    and the numpy routine on the parsed file; the records are the same, the confidences within 2^-24 relative (the file holds
    the shortest decimals of the float32 values)."""
    from . import pipeline as _pl

    device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    behaviors = list(behaviors)
    n_classes = len(behaviors)
    rank = name_ranks(behaviors)
    on_device = (device.type == "cuda" and isinstance(model, ClassifierLSTMDeltas) and model.seq_len == seq_len
                 and model.out_features == n_classes and 1 <= n_classes <= 64
                 and os.environ.get("CBAS_TRAIN_RESIDENT", "1").strip() != "0")

    by_video: Dict[str, list] = {}
    for inst in train_insts:
        video = inst.get("video")
        if video:
            by_video.setdefault(video, []).append(inst)

    # per clip that yields records: the parsed instances and where its predictions are
    clips = []                    # dicts: video, insts [(start, end, label, label index)], and "host": (pred, conf) or "dev": (base, n)
    pred_parts, conf_parts, total = [], [], 0
    writer = _CsvWriter(behaviors) if on_device else None
    flags = None
    try:
        for video, instances in by_video.items():
            h5_path = os.path.splitext(os.path.join(project_path, video))[0] + "_cls.h5"
            if not os.path.exists(h5_path):
                continue
            csv_path = h5_path.replace("_cls.h5", f"_{task_name}_outputs.csv")
            clip = {"video": video, "insts": []}
            rows = None
            if not os.path.exists(csv_path):
                rows = _clip_rows(h5_path, model.in_features, device, log) if on_device else None
                if rows is None:
                    csv_path = _pl.infer_file(file_path=h5_path, model=model, dataset_name=task_name, behaviors=behaviors,
                                              seq_len=seq_len, device=device)
                    if not csv_path:
                        continue
            if rows is not None:
                n = int(rows.shape[0])
                model.to(device)
                probs = torch.empty((n, n_classes), dtype=torch.float32, device=device)
                for a, b, r0, r1 in _pl.infer_spans(n, model.seq_len // 2):      # the calls infer_file makes, on resident rows
                    model.infer_range_into(rows[r0:r1], r1 - r0, a - r0, b - a, probs[r0:], 1.0)
                if flags is None:
                    flags = torch.zeros(len(by_video), dtype=torch.int32, device=device)
                k = len(clips)
                pred = torch.empty(n, dtype=torch.int32, device=device)
                conf = torch.empty(n, dtype=torch.float32, device=device)
                probs_top1(probs, pred, conf, flags[k:k + 1])
                host = torch.empty((n, n_classes), dtype=torch.float32, pin_memory=True)
                host.copy_(probs, non_blocking=True)
                event = torch.cuda.Event()
                event.record(torch.cuda.current_stream(device))
                writer.put(k, csv_path, host, event)
                pred_parts.append(pred)
                conf_parts.append(conf)
                clip.update(dev=(total, n), csv=csv_path, probs=host, event=event)
                total += n
            else:
                try:
                    values = _read_outputs_csv(csv_path, behaviors)
                    if np.isnan(values).any():
                        raise ValueError("a probability is NaN")
                    if values.shape[0] == 0:
                        raise ValueError("no rows")
                except Exception as e:  # noqa: BLE001 - workthreads.py:764-766
                    log(f"Could not read or process CSV {csv_path}: {e}")
                    continue
                clip["host"] = (values.argmax(axis=1).astype(np.int64), values.max(axis=1))
            for inst in instances:
                try:
                    start, end, label = int(inst["start"]), int(inst["end"]), inst["label"]
                except (ValueError, KeyError, TypeError) as e:
                    log(f"Skipping malformed instance in disagreement report: {inst}. Error: {e}")
                    continue
                clip["insts"].append((start, end, label, behaviors.index(label) if label in behaviors else -1))
            if "probs" in clip and all(0 <= a <= b for a, b, _l, _i in clip["insts"]):
                del clip["probs"]                           # only the host routine (negative bounds) reads them again
            clips.append(clip)

        # the device clips: one scan over all their instances; what pandas' negative bounds mean is left to the host routine
        runs_of: Dict[tuple, list] = {}                     # (clip, instance) -> [(start, end, prediction index, confidence)]
        dev_clips = [(k, c) for k, c in enumerate(clips) if "dev" in c]
        if dev_clips:
            nan = flags.cpu().numpy()                       # synchronises: every clip has been classified
            table, ic, ia, ib, il, where = [], [], [], [], [], []
            for k, c in dev_clips:
                if nan[k] & TOP1_FLAG_NAN:
                    log(f"Could not read or process CSV {c['csv']}: a probability is NaN")
                    c["insts"] = []
                    continue
                n = c["dev"][1]
                for j, (start, end, _label, index) in enumerate(c["insts"]):
                    if 0 <= start <= end:
                        if start < n:
                            ic.append(len(table)), ia.append(start), ib.append(min(end, n - 1)), il.append(index), where.append((k, j))
                    else:
                        c["event"].synchronize()
                        p = c["probs"].numpy()
                        runs_of[(k, j)] = disagreement_runs_host(p.argmax(axis=1), p.max(axis=1), start, end, index, rank)
                table.append(c["dev"])
            if ic:
                records = disagreement_runs(torch.cat(pred_parts), torch.cat(conf_parts), table, ic, ia, ib, il, rank)
                for r in records:
                    runs_of.setdefault(where[int(r["instance"])], []).append(
                        (int(r["start_frame"]), int(r["end_frame"]), int(r["model_prediction"]), float(r["model_confidence"])))
    finally:
        if writer is not None:
            writer.close()
    if writer is not None:
        for k, e in writer.failed.items():
            log(f"Error during buffered inference on {clips[k]['csv']}: {e}")
            clips[k]["insts"] = []

    disagreements = []
    for k, c in enumerate(clips):
        for j, (start, end, label, index) in enumerate(c["insts"]):
            runs = runs_of.get((k, j), []) if "dev" in c else disagreement_runs_host(c["host"][0], c["host"][1], start, end, index, rank)
            for a, b, winner, confidence in runs:
                disagreements.append({"video_path": c["video"], "start_frame": int(a), "end_frame": int(b), "human_label": label,
                                      "model_prediction": behaviors[winner] if winner >= 0 else None,
                                      "model_confidence": float(confidence)})
    disagreements.sort(key=lambda x: x["model_confidence"], reverse=True)
    return disagreements


def write_disagreement_report(path: str, items: List[dict]) -> None:
    """workthreads.py:807-809: ``disagreement_report.yaml`` as the labelling UI reads it."""
    import yaml
    with open(path, "w") as f:
        yaml.dump(items, f, allow_unicode=True)
