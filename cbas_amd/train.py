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

Dropout keep-masks come from a counter-based hash (seed, step, layer, element) instead of torch's
global RNG, so a run is reproducible from its seed; the masks have the reference's rates (0.1 after
the three bottleneck GELUs, 0.15 after lin0's GELU).
"""
from __future__ import annotations

import ctypes as C
import os
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
        return unpack_head_weights(self.cfg, blob)

    def weights(self) -> Dict[str, np.ndarray]:
        return self._read(0)

    def grads(self) -> Dict[str, np.ndarray]:
        return self._read(1)

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


def plan_training_data(train_set, test_set, seq_len: int, in_features: int, device):
    """Decide between rows resident in device memory and the host loader.  Returns ``(plan or None, one line that says
    which and why)``; raises ValueError for files whose row width is not ``in_features``."""
    if os.environ.get("CBAS_TRAIN_RESIDENT", "1").strip() == "0":
        return None, "training data: host loader (CBAS_TRAIN_RESIDENT=0)"
    sets = [train_set] + ([test_set] if test_set is not None and len(test_set) > 0 else [])
    for name, ds in zip(("training", "test"), sets):
        if _ds.manifest_kind(ds) is None:
            return None, f"training data: host loader (the {name} set is not a manifest dataset)"
        if int(ds.seq_len) != int(seq_len):
            return None, f"training data: host loader (the {name} set has seq_len {ds.seq_len}, the model {seq_len})"
    plan = _ds.plan_store([ds.manifest for ds in sets], in_features)
    if plan.not_half:
        return None, f"training data: host loader ({plan.not_half[0]} does not hold half-precision rows)"
    if plan.total_rows == 0:
        return None, "training data: host loader (no readable _cls.h5 file in the manifests)"
    allowed = _resident_budget(device)
    if plan.nbytes > allowed:
        return None, (f"training data: host loader ({_thousands(plan.total_rows)} rows need {plan.nbytes / 1e6:.0f} MB, "
                      f"{max(allowed, 0.0) / 1e6:.0f} MB may be used)")
    return plan, (f"training data: resident in HBM ({len(plan.files)} files, {_thousands(plan.total_rows)} rows, "
                  f"{plan.nbytes / 1e6:.0f} MB)")


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
    from sklearn.metrics import classification_report, confusion_matrix

    if len(train_set) == 0:
        return None, None, -1
    device = torch.device(device) if device is not None else torch.device("cuda")
    if device.type != "cuda":
        raise RuntimeError("cbas_amd.train.train_lstm_model runs on a GPU device only")
    gen = torch.Generator()
    gen.manual_seed(int(seed))
    plan, line = plan_training_data(train_set, test_set, seq_len, in_features, device)
    log(line)
    store = xbuf = None
    collate = collate_fn
    if plan is not None:
        # the same loaders over an index-only view: the sampler's randperm, the loader's per-iterator seed draw and the
        # balanced counter are consumed exactly as on the host path, so the batches are the same, draw for draw
        store = ResidentRows(plan, device)
        train_set = _IndexView(train_set, seq_len, store.files)
        test_set = _IndexView(test_set, seq_len, store.files) if test_set is not None and len(test_set) > 0 else None
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
