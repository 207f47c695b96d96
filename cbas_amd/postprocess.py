"""What CBAS does with a clip's probabilities after inference, on the device: thresholded events
(``Dataset.predictions_to_instances``, backend/cbas.py:903-926), the guided-labelling pre-labels
(``Dataset.predictions_to_instances_with_confidence``, :928-956, called straight after ``infer_file`` in
``start_labeling_with_preload``, backend/label_train_page.py:1071-1083) and the actogram's binned activity
(``Actogram.__init__``, :958-1000).  The reference reads ``_outputs.csv`` back with pandas and walks it in Python; here the
probabilities stay on the device: ``cbas_probs_top1`` -> ``cbas_labels_median`` -> ``cbas_label_runs``, and
``cbas_activity_bins`` over all files of a recording in one launch.

Without a GPU, for more than 64 classes, for values that are no float32 (a foreign CSV) or when ``cbas_probs_top1`` flags a NaN
the numpy routines of this module (``top1_host``, ``median_host``, ``label_runs_host``, ``activity_bins_host``) compute the same
records - the only host arithmetic here.  DESIGN.md "Events, pre-labels and actogram bins" states the semantics.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import re
import threading
import warnings
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .pipeline import read_outputs_csv

LABEL_RUN_DTYPE = np.dtype([("clip", "<i4"), ("start_frame", "<i4"), ("end_frame", "<i4"), ("label", "<i4"),
                            ("confidence", "<f8")])          # cbas_label_run of include/cbas_mi355x.h
MAX_CLASSES = 64
TOP1_FLAG_NAN = 1


# ---------------------------------------------------------------------------------------------------------------
# the numpy statement of the semantics
# ---------------------------------------------------------------------------------------------------------------
def top1_host(values: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``idxmax(axis=1)`` / ``max(axis=1)`` of :908-909 as (index int64, maximum float64): the first maximum, NaN skipped as
    pandas skips it; a row of NaN only gets -1 / NaN."""
    v = np.asarray(values)
    nan = np.isnan(v)
    filled = np.where(nan, -np.inf, v)
    pred = filled.argmax(axis=1).astype(np.int64)
    conf = filled.max(axis=1).astype(np.float64)
    empty = nan.all(axis=1)
    pred[empty] = -1
    conf[empty] = np.nan
    return pred, conf


def median_host(pred: np.ndarray, kernel_size: int) -> np.ndarray:
    """``scipy.signal.medfilt(pred, kernel_size)`` (:939) of ONE clip as int64: the clip is padded with ``kernel_size // 2``
    zeros at both ends, so its first and last frames are pulled towards class 0."""
    k = int(kernel_size)
    if k < 1 or k % 2 == 0:
        raise ValueError(f"kernel_size={kernel_size} must be odd and >= 1")
    x = np.asarray(pred, np.int64)
    if k == 1 or x.size == 0:
        return x.copy()
    padded = np.concatenate([np.zeros(k // 2, np.int64), x, np.zeros(k // 2, np.int64)])
    windows = np.lib.stride_tricks.sliding_window_view(padded, k)
    out = np.empty(x.size, np.int64)
    step = max(1, (1 << 22) // k)                              # rows per piece: the sorted copy stays near 32 MB
    for a in range(0, x.size, step):
        out[a:a + step] = np.partition(windows[a:a + step], k // 2, axis=1)[:, k // 2]
    return out


def run_mean(conf: np.ndarray) -> float:
    """The float64 mean of one run's confidences in the order the device adds them (csrc/run_sum.h): 64 interleaved partial
    sums, each in ascending frame order, combined by a fixed butterfly."""
    x = np.asarray(conf, np.float64)
    rows = -(-x.size // 64)
    padded = np.zeros(rows * 64, np.float64)
    padded[:x.size] = x
    s = np.cumsum(padded.reshape(rows, 64), axis=0)[-1]        # cumsum adds one after the other (np.sum adds pairwise)
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        s = s + s[lanes ^ d]
    return float(s[0] / x.size)


def label_runs_host(key: np.ndarray, conf: np.ndarray, threshold: Optional[float] = None) -> list:
    """``[(start, end, label, confidence)]`` of ONE clip: one entry per maximal run of consecutive frames with equal
    ``key`` != -1, where with a threshold a frame's key counts as -1 unless ``conf >= threshold``.  With the threshold these
    are the events of :910-925, without it the blocks of :944-955."""
    k = np.asarray(key, np.int64).copy()
    c = np.asarray(conf)
    if threshold is not None:
        with np.errstate(invalid="ignore"):
            k[~(c.astype(np.float64) >= float(threshold))] = -1
    if k.size == 0:
        return []
    change = np.flatnonzero(k[1:] != k[:-1]) + 1
    starts = np.concatenate([[0], change])
    ends = np.concatenate([change - 1, [k.size - 1]])
    return [(int(a), int(b), int(k[a]), run_mean(c[a:b + 1])) for a, b in zip(starts, ends) if k[a] >= 0]


def activity_bins_host(values: np.ndarray, behavior: int, threshold: float, bin_frames: int) -> np.ndarray:
    """:977-979 and :999 on rows (n, C): int64 counts per bin of ``bin_frames`` frames of
    ``values[:, behavior] * is_max >= threshold``, ``is_max`` = (max of the other columns, NaN skipped) < the behaviour's."""
    v = np.asarray(values)
    p = v[:, behavior].astype(np.float64)
    others = np.delete(v, behavior, axis=1)
    if others.shape[1] == 0:
        m = np.full(p.shape, np.nan)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)    # a row of NaN only: its maximum is NaN, as pandas' is
            m = np.nanmax(others, axis=1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        active = (p * (m < p) >= float(threshold)).astype(np.int64)
    n_bins = -(-active.size // bin_frames)
    padded = np.zeros(n_bins * bin_frames, np.int64)
    padded[:active.size] = active
    return padded.reshape(n_bins, bin_frames).sum(axis=1)


# ---------------------------------------------------------------------------------------------------------------
# the device calls
# ---------------------------------------------------------------------------------------------------------------
def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _table(clip_table, dev) -> Tuple[np.ndarray, torch.Tensor]:
    table = np.ascontiguousarray(np.asarray(clip_table, np.int64).reshape(-1, 2))
    if table.shape[0] < 1:
        raise ValueError("the clip table must hold at least one (first frame, frames) row")
    return table, torch.from_numpy(table).to(dev)


def labels_median(pred: torch.Tensor, clip_table, n_classes: int, kernel_size: int) -> torch.Tensor:
    """``cbas_labels_median``: the zero-padded median filter of every clip of ``pred`` (int32, all clips back to back on one GPU)."""
    if pred.dtype != torch.int32 or not pred.is_cuda or pred.dim() != 1 or not pred.is_contiguous():
        raise ValueError("pred must be a contiguous 1-d int32 tensor on a GPU")
    table, table_dev = _table(clip_table, pred.device)
    out = torch.empty_like(pred)
    with torch.cuda.device(pred.device):
        _lib.check(_lib.load().cbas_labels_median(pred.data_ptr(), int(pred.shape[0]), table_dev.data_ptr(), int(table.shape[0]),
                                                  int(n_classes), int(kernel_size), out.data_ptr(), _stream(pred.device)),
                   "cbas_labels_median")
    return out


def label_runs(key: torch.Tensor, conf: torch.Tensor, clip_table, n_classes: int, threshold: Optional[float] = None) -> np.ndarray:
    """``cbas_label_runs``: the records (``LABEL_RUN_DTYPE``, ordered by clip and start) of ``key`` (int32) / ``conf`` (float32)."""
    dev = key.device
    if key.dtype != torch.int32 or conf.dtype != torch.float32 or not key.is_cuda or conf.device != dev or key.shape != conf.shape \
            or key.dim() != 1 or not key.is_contiguous() or not conf.is_contiguous():
        raise ValueError("key (int32) and conf (float32) must be contiguous 1-d tensors of one length on one GPU")
    table, table_dev = _table(clip_table, dev)
    capacity = max(1, int(key.shape[0]))                      # at most one run per frame
    records = torch.empty(capacity * LABEL_RUN_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    needed = C.c_int64(0)
    with torch.cuda.device(dev):
        n = _lib.load().cbas_label_runs(key.data_ptr(), conf.data_ptr(), int(key.shape[0]), table_dev.data_ptr(), int(table.shape[0]),
                                        int(n_classes), 0 if threshold is None else 1, 0.0 if threshold is None else float(threshold),
                                        records.data_ptr(), capacity, C.byref(needed), _stream(dev))
    if n < 0:
        _lib.check(int(n), "cbas_label_runs")
    return records[:n * LABEL_RUN_DTYPE.itemsize].cpu().numpy().view(LABEL_RUN_DTYPE).copy()


def activity_bins_device(probs: torch.Tensor, behavior: int, threshold: float, bin_frames: int) -> torch.Tensor:
    """``cbas_activity_bins``: int64 counts per bin of device rows (n, C) float32; asynchronous on the current stream."""
    if probs.dim() != 2 or probs.dtype != torch.float32 or not probs.is_cuda or not probs.is_contiguous() or probs.shape[0] < 1:
        raise ValueError(f"probs must be a contiguous float32 (n >= 1, C) tensor on a GPU, got {probs.dtype} {tuple(probs.shape)}")
    n = int(probs.shape[0])
    n_bins = -(-n // int(bin_frames)) if bin_frames >= 1 else 0
    bins = torch.empty(max(n_bins, 1), dtype=torch.int64, device=probs.device)
    with torch.cuda.device(probs.device):
        _lib.check(_lib.load().cbas_activity_bins(probs.data_ptr(), n, int(probs.shape[1]), int(behavior), float(threshold),
                                                  int(bin_frames), bins.data_ptr(), n_bins, _stream(probs.device)),
                   "cbas_activity_bins")
    return bins[:n_bins]


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def _gpu() -> bool:
    return torch.cuda.is_available()


def _as_float32(values: np.ndarray) -> Optional[np.ndarray]:
    """An array as float32 when that loses nothing - it is float32, or every value is a float32 value (NaN included) - else
    None: other values stay in float64 on the host, where every comparison is the reference's.  (A CSV is decided by
    ``read_outputs_csv``: its float32 rows stand for it only when they reproduce its text byte for byte.)"""
    v = np.asarray(values)
    if v.dtype == np.float32:
        return np.ascontiguousarray(v)
    v = v.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = v.astype(np.float32)
    return np.ascontiguousarray(f) if np.array_equal(f.astype(np.float64), v, equal_nan=True) else None


def _on_device(n_rows: int, n_classes: int) -> bool:
    return _gpu() and 1 <= n_classes <= MAX_CLASSES and n_rows >= 1


def _load_rows(probs_or_csv, behaviors: Sequence[str]):
    """``("dev", tensor)``, ``("host", array)`` or None (a file that is missing or lacks a behaviour's column: the reference
    returns no instances, :905-907)."""
    if isinstance(probs_or_csv, (str, os.PathLike)):
        try:
            header, values, exact = read_outputs_csv(os.fspath(probs_or_csv))
        except FileNotFoundError:
            return None
        if any(b not in header for b in behaviors):
            return None
        cols = [header.index(b) for b in behaviors]
        if exact is not None and _on_device(values.shape[0], len(behaviors)):
            return "dev", torch.from_numpy(np.ascontiguousarray(exact[:, cols])).cuda()
        return "host", values[:, cols]
    if isinstance(probs_or_csv, torch.Tensor):
        if probs_or_csv.dim() != 2 or probs_or_csv.shape[1] != len(behaviors):
            raise ValueError(f"{len(behaviors)} behaviours for probabilities of shape {tuple(probs_or_csv.shape)}")
        if probs_or_csv.is_cuda and probs_or_csv.dtype == torch.float32 and 1 <= len(behaviors) <= MAX_CLASSES and probs_or_csv.shape[0] >= 1:
            return "dev", probs_or_csv.contiguous()
        values = probs_or_csv.detach().cpu().numpy()
    else:
        values = np.asarray(probs_or_csv)
        if values.ndim != 2 or values.shape[1] != len(behaviors):
            raise ValueError(f"{len(behaviors)} behaviours for probabilities of shape {values.shape}")
    if _on_device(values.shape[0], len(behaviors)):
        f = _as_float32(values)
        if f is not None:
            return "dev", torch.from_numpy(f).cuda()
    return "host", values


def _video_name(video_path: str, project_path: Optional[str]) -> str:
    if project_path:
        return os.path.relpath(video_path, start=project_path).replace("\\", "/")       # :953
    return video_path


def _top1(kind: str, rows):
    """``(kind, pred, conf)``: device tensors, or numpy arrays when the rows are on the host or hold a NaN."""
    if kind == "dev":
        from .train import probs_top1
        pred, conf, flags = probs_top1(rows)
        if not int(flags.item()) & TOP1_FLAG_NAN:
            return "dev", pred, conf
        rows = rows.cpu().numpy()                              # pandas skips a NaN where the kernel refuses the row
    pred, conf = top1_host(rows)
    return "host", pred, conf


def predictions_to_instances(probs_or_csv, behaviors: Sequence[str], video_path: str, threshold: float = 0.7,
                             project_path: Optional[str] = None) -> list:
    """``Dataset.predictions_to_instances`` (:903-926): ``[{"video", "start", "label", "end"}]``, one event per maximal run of
    frames whose top-1 probability is ``>= threshold`` and whose top-1 label stays the same.  ``probs_or_csv``: an
    ``_outputs.csv`` path, a numpy array or a tensor (n, len(behaviors)); a device tensor goes straight into the kernels,
    anything else is uploaded once.  ``video`` is ``video_path``, relative to ``project_path`` when one is given."""
    behaviors = list(behaviors)
    if not behaviors:
        return []
    loaded = _load_rows(probs_or_csv, behaviors)
    if loaded is None or loaded[1].shape[0] == 0:
        return []
    kind, pred, conf = _top1(*loaded)
    if kind == "dev":
        runs = [(int(r["start_frame"]), int(r["end_frame"]), int(r["label"]))
                for r in label_runs(pred, conf, [(0, int(pred.shape[0]))], len(behaviors), threshold)]
    else:
        runs = [r[:3] for r in label_runs_host(pred, conf, threshold)]
    video = _video_name(video_path, project_path)
    return [{"video": video, "start": a, "label": behaviors[k], "end": b} for a, b, k in runs]


def predictions_to_instances_with_confidence(probs_or_csv, behaviors: Sequence[str], video_path: str, threshold: float = 0.5,
                                             smoothing_window: int = 1, project_path: Optional[str] = None):
    """``Dataset.predictions_to_instances_with_confidence`` (:928-956): ``(instances, DataFrame)``.  The instances are
    ``{"video", "start", "end", "label", "confidence"}``, one per block of equal label - the top-1 label, or for
    ``smoothing_window > 1`` its zero-padded median filter (an even window is raised by one, :936) - with the block's mean
    top-1 probability.  ``threshold`` is accepted and unused, as in the reference.  The DataFrame has the reference's columns:
    the behaviours, ``predicted_label``, ``max_prob``, with smoothing ``predicted_index`` and ``smoothed_index``, then
    ``label_for_grouping`` and ``block_start``; it is built from the arrays the kernels wrote, not by reading a file again.  A
    missing file gives ``([], None)``, a file without a behaviour's column ``([], the file as it is)``."""
    import pandas as pd
    behaviors = list(behaviors)
    loaded = _load_rows(probs_or_csv, behaviors) if behaviors else None
    if loaded is None:
        if isinstance(probs_or_csv, (str, os.PathLike)) and os.path.exists(probs_or_csv):
            return [], pd.read_csv(probs_or_csv)               # :932
        return [], None
    return _blocks(loaded[0], loaded[1], behaviors, _video_name(video_path, project_path), smoothing_window)


def _blocks(kind: str, rows, behaviors: List[str], video: str, smoothing_window: int, host_rows: Optional[np.ndarray] = None):
    import pandas as pd
    n = int(rows.shape[0])
    window = int(smoothing_window)
    if window > 1 and window % 2 == 0:
        window += 1
    smooth = window > 1
    kind, pred, conf = _top1(kind, rows) if n else ("host", np.empty(0, np.int64), np.empty(0, np.float64))
    if kind == "dev":
        table = [(0, n)]
        key = labels_median(pred, table, len(behaviors), window) if smooth else pred
        records = label_runs(key, conf, table, len(behaviors), None)
        runs = [(int(r["start_frame"]), int(r["end_frame"]), int(r["label"]), float(r["confidence"])) for r in records]
        values = rows.cpu().numpy() if host_rows is None else host_rows
        pred, conf, key = pred.cpu().numpy(), conf.cpu().numpy(), key.cpu().numpy()
    else:
        values = rows.cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
        key = median_host(pred, window) if smooth else pred
        runs = label_runs_host(key, conf, None)
    names = np.array(behaviors + [None], dtype=object)        # index -1: no label (NaN in the reference's column)
    df = pd.DataFrame(np.asarray(values, np.float64), columns=behaviors)
    df["predicted_label"] = names[pred]
    df["max_prob"] = np.asarray(conf, np.float64)
    if smooth:
        df["predicted_index"] = np.asarray(pred, np.int64)
        df["smoothed_index"] = np.asarray(key, np.int64)
    df["label_for_grouping"] = pd.Series(names[key], dtype=object).where(np.asarray(key) >= 0, np.nan)
    k = np.asarray(key, np.int64)
    df["block_start"] = np.concatenate([[True], k[1:] != k[:-1]])[:n] | (k < 0)       # NaN != NaN: such a frame starts a block (:944)
    instances = [{"video": video, "start": a, "end": b, "label": behaviors[label], "confidence": confidence}
                 for a, b, label, confidence in runs]
    return instances, df


def prelabel_file(h5_path: str, model, dataset_name: str, behaviors: Sequence[str], seq_len: int, smoothing_window: int = 1,
                  temperature: float = 1.0, project_path: Optional[str] = None, device=None, log=print):
    """Lines :1071-1083 of ``start_labeling_with_preload``: classify ``h5_path`` (a ``_cls.h5``), write the ``_outputs.csv``
    ``infer_file`` writes, byte for byte, and return ``predictions_to_instances_with_confidence`` of it - ``(instances, df)``.
    On a GPU the probabilities stay on the device for ``cbas_probs_top1`` -> ``cbas_labels_median`` -> ``cbas_label_runs``
    while a thread writes the file; a file the device path does not take (no half-precision rows, more than 64 classes) goes
    through ``infer_file`` and the CSV.  Raises RuntimeError when no CSV could be written (:1075-1076)."""
    from . import pipeline as _pl
    from . import train as _tr

    behaviors = list(behaviors)
    device = torch.device(device) if device is not None else torch.device("cuda" if _gpu() else "cpu")
    csv_path = h5_path.replace("_cls.h5", f"_{dataset_name}_outputs.csv")
    video = _video_name(h5_path.replace("_cls.h5", ".mp4"), project_path)
    rows = None
    if device.type == "cuda" and 1 <= len(behaviors) <= MAX_CLASSES:
        head = _pl._as_mi355x_head(model, device)
        if head.seq_len != seq_len:
            raise ValueError(f"seq_len={seq_len} does not match the model's seq_len={head.seq_len}")
        if head.out_features != len(behaviors):
            raise ValueError(f"{len(behaviors)} behaviour names for {head.out_features} model outputs")
        rows = _tr._clip_rows(h5_path, head.in_features, device, log, what="pre-labels")
    if rows is None:
        out = _pl.infer_file(file_path=h5_path, model=model, dataset_name=dataset_name, behaviors=behaviors, seq_len=seq_len,
                             device=device, temperature=temperature)
        if not out or not os.path.exists(out):
            raise RuntimeError("Inference failed to produce a CSV output file.")
        return predictions_to_instances_with_confidence(out, behaviors, h5_path.replace("_cls.h5", ".mp4"),
                                                        smoothing_window=smoothing_window, project_path=project_path)
    n = int(rows.shape[0])
    with torch.cuda.device(device):
        probs = torch.empty((n, len(behaviors)), dtype=torch.float32, device=device)
        for a, b, r0, r1 in _pl.infer_spans(n, head.seq_len // 2):          # the calls infer_file makes, on resident rows
            head.infer_range_into(rows[r0:r1], r1 - r0, a - r0, b - a, probs[r0:], temperature)
        host = torch.empty((n, len(behaviors)), dtype=torch.float32, pin_memory=True)
        host.copy_(probs, non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(device))
        writer = _tr._CsvWriter(behaviors)
        try:
            writer.put(0, csv_path, host, event)
            event.synchronize()                                 # the DataFrame's columns are this copy
            result = _blocks("dev", probs, behaviors, video, smoothing_window, host_rows=host.numpy())
        finally:
            writer.close()
    if writer.failed:
        raise RuntimeError(f"Inference failed to produce a CSV output file: {writer.failed[0]}")
    return result


# ---------------------------------------------------------------------------------------------------------------
# the actogram
# ---------------------------------------------------------------------------------------------------------------
_cache_lock = threading.Lock()
_cache: "collections.OrderedDict" = collections.OrderedDict()      # (path, size, mtime_ns) per file -> (columns, device rows)


def _cache_budget() -> int:
    """``CBAS_ACTOGRAM_CACHE_MB``: device memory the parsed files of recordings may keep between calls (default 512, 0 = none)."""
    try:
        return max(0, int(float(os.environ.get("CBAS_ACTOGRAM_CACHE_MB", "512")) * (1 << 20)))
    except ValueError:
        return 512 << 20


def clear_cache() -> None:
    with _cache_lock:
        _cache.clear()


def outputs_files(directory: str, model_name: str) -> List[str]:
    """The ``_<model>_outputs.csv`` files of a directory in the reference's order (:981-986): by the number before
    ``_<model>``, or by plain sort when a name has none."""
    files = [os.path.join(directory, f) for f in os.listdir(directory) if f.endswith(f"_{model_name}_outputs.csv")]
    try:
        files.sort(key=lambda p: int(re.search(r"_(\d+)_" + model_name, os.path.basename(p)).group(1)))
    except (AttributeError, ValueError):
        files.sort()
    return files


def binsize_frames(framerate: float, binsize_minutes) -> int:
    """:969-971: 0 when the actogram is empty for these settings."""
    framerate, minutes = float(framerate), int(binsize_minutes)
    if framerate <= 0 or minutes <= 0:
        return 0
    return max(0, int(minutes * framerate * 60))


def _file_rows(files: Sequence[str]) -> list:
    """``[(columns, float64 rows, float32 rows or None)]`` of every file that has rows (:990 skips the others), whatever
    behaviour is asked for: what may be cached must not depend on the call."""
    parts = []
    for path in files:
        header, values, exact = read_outputs_csv(path)
        if values.shape[0]:
            parts.append((header, values, exact))
    return parts


def activity_bins(source, model_name: Optional[str], behaviors: Optional[Sequence[str]], behavior: str, framerate: float,
                  binsize_minutes, threshold: float) -> List[float]:
    """``Actogram.binned_activity`` (:969-999) as a list of floats.  ``source``: a recording directory (its
    ``_<model_name>_outputs.csv`` files in the reference's order), a list of such files in the caller's order, a DataFrame
    (``preloaded_df``) or rows (n, len(behaviors)) as an array or tensor.  A frame is active when the behaviour's probability
    is strictly the largest of ALL the file's columns and ``>= threshold``; bins of ``int(binsize_minutes * framerate * 60)``
    frames run across file boundaries.  A recording whose files all have the same columns and hold float32 text (what
    ``infer_file`` writes) stays on the device between calls (keyed by every file's path, size and mtime, bounded by
    ``CBAS_ACTOGRAM_CACHE_MB``), so another threshold, behaviour or bin size costs one launch; files with differing columns or
    other text are walked one by one on the host and nothing is kept."""
    bin_frames = binsize_frames(framerate, binsize_minutes)
    if bin_frames <= 0:
        return []
    threshold = float(threshold)
    if isinstance(source, (str, os.PathLike)) or (isinstance(source, (list, tuple)) and all(isinstance(s, (str, os.PathLike)) for s in source)):
        if isinstance(source, (str, os.PathLike)):
            if not model_name:
                return []
            files = outputs_files(os.fspath(source), model_name)
        else:
            files = [os.fspath(s) for s in source]
        if not files:
            return []
        key = tuple((p, os.path.getsize(p), os.stat(p).st_mtime_ns) for p in files)
        with _cache_lock:
            hit = _cache.get(key)
            if hit is not None:
                _cache.move_to_end(key)
        if hit is not None:
            columns, rows = hit
            if behavior not in columns:
                return []
            return [float(x) for x in activity_bins_device(rows, columns.index(behavior), threshold, bin_frames).cpu().numpy()]
        parts = _file_rows(files)
        if not parts:
            return []
        columns = parts[0][0]
        # one launch, and the cache, only for a recording whose files ALL have the same columns and ARE their float32 rows;
        # which files count then does not depend on the behaviour, so neither does what is cached under `key`
        if all(h == columns and e is not None for h, _v, e in parts) and _on_device(1, len(columns)):
            rows = torch.from_numpy(np.concatenate([e for _h, _v, e in parts])).cuda()
            budget = _cache_budget()
            with _cache_lock:
                if rows.numel() * 4 <= budget:
                    _cache[key] = (columns, rows)
                    while sum(r.numel() * 4 for _c, r in _cache.values()) > budget:
                        _cache.popitem(last=False)
            if behavior not in columns:
                return []
            return [float(x) for x in activity_bins_device(rows, columns.index(behavior), threshold, bin_frames).cpu().numpy()]
        # anything else per file on the host, as the reference walks them: a file without the column is skipped (:990)
        active = [activity_bins_host(v, h.index(behavior), threshold, 1) for h, v, _e in parts if behavior in h]
        return _rebin(np.concatenate(active), bin_frames) if active else []
    elif hasattr(source, "columns") and hasattr(source, "to_numpy"):
        columns = [str(c) for c in source.columns]
        if behavior not in columns:
            return []
        values = source.to_numpy(dtype=np.float64)
    else:
        columns = list(behaviors or [])
        if behavior not in columns:
            return []
        if isinstance(source, torch.Tensor) and source.is_cuda and source.dtype == torch.float32 and source.dim() == 2 \
                and source.shape[1] == len(columns) and 1 <= len(columns) <= MAX_CLASSES and source.shape[0] >= 1:
            return [float(x) for x in activity_bins_device(source.contiguous(), columns.index(behavior), threshold, bin_frames).cpu().numpy()]
        values = source.detach().cpu().numpy() if isinstance(source, torch.Tensor) else np.asarray(source)
        if values.ndim != 2 or values.shape[1] != len(columns):
            raise ValueError(f"{len(columns)} behaviours for probabilities of shape {values.shape}")
    if values.shape[0] == 0:
        return []
    b = columns.index(behavior)
    f = _as_float32(values) if _gpu() and 1 <= len(columns) <= MAX_CLASSES else None
    if f is None:
        return [float(x) for x in activity_bins_host(values, b, threshold, bin_frames)]
    rows = torch.from_numpy(f).cuda()
    return [float(x) for x in activity_bins_device(rows, b, threshold, bin_frames).cpu().numpy()]


def _rebin(active: np.ndarray, bin_frames: int) -> List[float]:
    n_bins = -(-active.size // bin_frames)
    padded = np.zeros(n_bins * bin_frames, np.int64)
    padded[:active.size] = active
    return [float(x) for x in padded.reshape(n_bins, bin_frames).sum(axis=1)]
