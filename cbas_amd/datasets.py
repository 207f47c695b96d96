"""Manifest datasets for head training, without h5py.

A *manifest* is the reference's memory-light description of a training split: a list of
``(h5_path, centre_frame, label_index)``, one entry per labelled frame whose window of ``seq_len`` rows lies inside its
``_cls.h5`` (``Project.convert_instances``, backend/cbas.py:1171-1219).  ``LazyStandardDataset`` and
``LazyBalancedDataset`` restate the reference's two dataset classes over such a manifest (backend/cbas.py:181-301) with
the same constructor arguments, attribute names, lengths and sample order; the rows are read through
``cbas_amd.h5io.ClsReader``, which works with h5py or with libhdf5 alone.

Window semantics: the window of centre ``c`` is the rows ``[c - seq_len // 2, c + seq_len // 2 + 1)``.  That is
``seq_len`` rows only for an odd ``seq_len`` (an even one makes the reference drop every sample), so an even ``seq_len``
is refused here.  A window that reaches outside its file is a dropped sample (label -1), never a wrapped or clamped read.

Two additions the reference lacks: ``resolve(idx)`` - the index arithmetic of ``__getitem__`` (with its effect on the
balanced ``counter``) without the read, which is what training from rows resident in device memory needs
(``cbas_amd.train``) - and ``make_manifest``, the arithmetic of ``convert_instances`` on plain tuples.  The helpers at the
end apply the same arithmetic to any object that carries the reference's attribute names (duck typing), so that CBAS's own
instances qualify without their h5py-bound ``__getitem__`` ever being called.
"""
from __future__ import annotations

import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import h5io

DEFAULT_DIM = 768           # row width of a dropped sample whose file never opened (the reference hard-codes 768)

# process-local cache of open readers, like the reference's _worker_h5_handles (backend/cbas.py:199-202)
_readers: Dict[str, h5io.ClsReader] = {}
_warned = set()


def _warn_once(path: str, what: str, err: Exception) -> None:
    if (path, what) not in _warned:
        _warned.add((path, what))
        print(f"WORKER-ERROR: Could not {what} {path}. {err}")


def close_readers() -> None:
    """Close every ``_cls.h5`` the datasets of this process have opened."""
    for r in _readers.values():
        try:
            r.close()
        except Exception:  # noqa: BLE001
            pass
    _readers.clear()


def check_seq_len(seq_len: int) -> int:
    seq_len = int(seq_len)
    if seq_len < 1 or seq_len % 2 == 0:
        raise ValueError(f"seq_len={seq_len}: a window is the rows [centre - seq_len // 2, centre + seq_len // 2 + 1), which is "
                         f"seq_len rows only for an odd seq_len (with an even one every sample is dropped)")
    return seq_len


def window_start(centre: int, seq_len: int, n_rows: int) -> int:
    """First row of the window of ``centre`` in a file of ``n_rows`` rows, or -1 when the window is not ``seq_len`` rows
    inside the file."""
    half = seq_len // 2
    start = int(centre) - half
    if 2 * half + 1 != seq_len or start < 0 or start + seq_len > n_rows:
        return -1
    return start


def _dropped(seq_len: int, dim: int):
    return torch.zeros(seq_len, dim), torch.tensor(-1).long()


def read_window(entry, seq_len: int, dim_hint: int = DEFAULT_DIM):
    """``(float32 (seq_len, D) tensor, int64 label)`` of one manifest entry; ``(zeros, -1)`` when the file cannot be
    opened, the slice cannot be read or the window is not ``seq_len`` rows inside the file."""
    h5_path, centre, label = entry
    reader = _readers.get(h5_path)
    if reader is None:
        try:
            reader = _readers[h5_path] = h5io.ClsReader(h5_path)
        except Exception as e:  # noqa: BLE001
            _warn_once(h5_path, "open H5 file", e)
            return _dropped(seq_len, dim_hint)
    dim = int(reader.shape[1]) if len(reader.shape) == 2 else dim_hint
    start = window_start(centre, seq_len, int(reader.shape[0])) if len(reader.shape) == 2 else -1
    if start < 0:
        return _dropped(seq_len, dim)
    try:
        window = reader.read(start, start + seq_len)
    except Exception as e:  # noqa: BLE001
        _warn_once(h5_path, "read slice from", e)
        return _dropped(seq_len, dim)
    if window.shape[0] != seq_len:
        return _dropped(seq_len, dim)
    return torch.from_numpy(window).float(), torch.tensor(int(label)).long()


class LazyStandardDataset(torch.utils.data.Dataset):
    """One sample per manifest entry, in manifest order (backend/cbas.py:181-228)."""

    def __init__(self, manifest: list, seq_len: int):
        self.manifest = manifest
        self.seq_len = check_seq_len(seq_len)
        self.half_seqlen = self.seq_len // 2

    def __len__(self):
        return len(self.manifest)

    def resolve(self, idx: int) -> int:
        """Manifest index of sample ``idx``."""
        idx = int(idx)
        if not -len(self.manifest) <= idx < len(self.manifest):
            raise IndexError(idx)
        return idx % len(self.manifest)

    def __getitem__(self, idx):
        return read_window(self.manifest[self.resolve(idx)], self.seq_len)


class LazyBalancedDataset(torch.utils.data.Dataset):
    """Oversampling by class (backend/cbas.py:231-301): the manifest indices are bucketed by behaviour, the class of a
    sample is chosen round-robin by ``counter`` (which lives on the instance and keeps counting across epochs and scoring
    passes) and the sample is ``bucket[idx % len(bucket)]``."""

    def __init__(self, manifest: list, seq_len: int, behaviors: list):
        self.manifest = manifest
        self.seq_len = check_seq_len(seq_len)
        self.behaviors = behaviors
        self.num_behaviors = len(behaviors)
        self.half_seqlen = self.seq_len // 2
        self.buckets = {b: [] for b in behaviors}
        for i, (_, _, label_index) in enumerate(manifest):
            if 0 <= label_index < self.num_behaviors:
                self.buckets[behaviors[label_index]].append(i)
        self.available_behaviors = [b for b in behaviors if self.buckets[b]]
        self.num_available_behaviors = len(self.available_behaviors)
        self.total_sequences = len(manifest)
        self.counter = 0

    def __len__(self):
        return balanced_len(self)

    def resolve(self, idx: int) -> int:
        """Manifest index of sample ``idx``; advances ``counter`` exactly as ``__getitem__`` does."""
        return balanced_resolve(self, idx)

    def __getitem__(self, idx: int):
        return read_window(self.manifest[self.resolve(idx)], self.seq_len)


# ---------------------------------------------------------------------------------------------------------------
# the same arithmetic on any object with the reference's attribute names
# ---------------------------------------------------------------------------------------------------------------
def manifest_kind(ds) -> Optional[str]:
    """"balanced" / "standard" for an object that carries a manifest dataset's attributes, else None.  By attribute
    names, not by class: CBAS's own instances (created inside an installed CBAS) qualify."""
    if ds is None or not hasattr(ds, "manifest") or not hasattr(ds, "seq_len") or not hasattr(ds, "__len__"):
        return None
    if all(hasattr(ds, a) for a in ("buckets", "available_behaviors", "counter")):
        return "balanced"
    return "standard"


def balanced_len(ds) -> int:
    """Length padded up to a multiple of the number of classes that have samples (backend/cbas.py:257-261)."""
    k = len(ds.available_behaviors)
    if k == 0:
        return 0
    total = getattr(ds, "total_sequences", len(ds.manifest))
    return total + (k - total % k) % k


def balanced_resolve(ds, idx: int) -> int:
    k = len(ds.available_behaviors)
    if k == 0:
        raise IndexError("No behaviors with samples available in this dataset split.")
    bucket = ds.buckets[ds.available_behaviors[ds.counter % k]]
    ds.counter += 1
    return bucket[int(idx) % len(bucket)]


def resolve_index(ds, idx: int) -> int:
    """Manifest index that ``ds[idx]`` would load, with the same effect on a balanced dataset's ``counter`` - through the
    object's own ``resolve`` when it has one, else by the reference's arithmetic on its fields."""
    own = getattr(ds, "resolve", None)
    if callable(own):
        return own(idx)
    if manifest_kind(ds) == "balanced":
        return balanced_resolve(ds, idx)
    return int(idx)


# ---------------------------------------------------------------------------------------------------------------
# manifests
# ---------------------------------------------------------------------------------------------------------------
def make_manifest(cls_paths_and_instances: Iterable[Tuple[str, int, int, str]], seq_len: int, behaviors: Sequence[str]) -> list:
    """The arithmetic of ``Project.convert_instances`` (backend/cbas.py:1171-1219) on plain
    ``(cls_path, start, end, label)`` tuples: one ``(cls_path, frame, label_index)`` per frame of ``[start, end]`` whose
    whole window is inside the file.  Files are visited in order of first appearance; a file that is missing, unreadable
    or shorter than ``seq_len`` is skipped, and so are instances with ``start`` or ``end`` of -1 and labels that are not in
    ``behaviors``."""
    seq_len = check_seq_len(seq_len)
    half = seq_len // 2
    behaviors = list(behaviors)
    by_file: Dict[str, list] = {}
    for path, start, end, label in cls_paths_and_instances:
        by_file.setdefault(path, []).append((start, end, label))
    manifest = []
    for path, insts in by_file.items():
        if not path:
            continue
        if not os.path.exists(path):
            print(f"Warning: H5 file not found, skipping instances for {path}")
            continue
        try:
            with h5io.ClsReader(path) as r:
                num_frames = int(r.shape[0])
        except Exception as e:  # noqa: BLE001
            print(f"Warning: Could not read H5 file {path}: {e}")
            continue
        if num_frames < seq_len:
            continue
        for start, end, label in insts:
            start, end = int(start), int(end)
            if start == -1 or end == -1:
                continue
            try:
                label_index = behaviors.index(str(label).strip())
            except ValueError:
                print(f"WARNING: The label '{label}' in '{path}' is not in the master behavior list. This instance will be SKIPPED.")
                continue
            for frame in range(start, end + 1):
                if frame - half >= 0 and frame + half < num_frames:
                    manifest.append((path, frame, label_index))
    return manifest


# ---------------------------------------------------------------------------------------------------------------
# the layout of a store that holds the rows of every file of some manifests back to back
# ---------------------------------------------------------------------------------------------------------------
class StorePlan:
    """``files``: {path: (base_row, n_rows)} of the readable files in order of first appearance, ``total_rows``, ``dim``;
    ``unreadable``: the paths that get no rows; ``not_half``: readable files whose ``cls`` dataset is not IEEE half."""

    def __init__(self):
        self.files: Dict[str, Tuple[int, int]] = {}
        self.unreadable: List[str] = []
        self.not_half: List[str] = []
        self.total_rows = 0
        self.dim = 0

    @property
    def nbytes(self) -> int:
        return self.total_rows * self.dim * 2


def plan_store(manifests: Sequence[list], in_features: int) -> StorePlan:
    """Open every distinct file of ``manifests`` once and lay their rows out back to back.  A file that cannot be opened
    gets no rows; a file whose row width is not ``in_features`` is a ``ValueError`` that names it."""
    plan = StorePlan()
    plan.dim = int(in_features)
    seen = set()
    for manifest in manifests:
        for path in dict.fromkeys(e[0] for e in manifest):
            if path in seen:
                continue
            seen.add(path)
            try:
                with h5io.ClsReader(path) as r:
                    shape, half = tuple(r.shape), bool(r.is_half)
            except Exception as e:  # noqa: BLE001
                _warn_once(path, "open H5 file", e)
                plan.unreadable.append(path)
                continue
            if len(shape) != 2 or shape[1] != plan.dim:
                raise ValueError(f"{path}: 'cls' has shape {shape}, but the head is trained on rows of width {plan.dim} "
                                 f"(all files of a training run must have the same row width, in_features)")
            if not half:
                plan.not_half.append(path)
            plan.files[path] = (plan.total_rows, int(shape[0]))
            plan.total_rows += int(shape[0])
    return plan


def plan_files(paths: Sequence[str], in_features: Optional[int] = None) -> StorePlan:
    """``plan_store`` for a plain list of files (no manifest): their rows back to back in the order given, a path named twice
    counted once.  ``in_features=None`` takes the width of the first readable file; a file of another width is a
    ``ValueError`` that names it."""
    plan = StorePlan()
    plan.dim = 0 if in_features is None else int(in_features)
    for path in dict.fromkeys(paths):
        try:
            with h5io.ClsReader(path) as r:
                shape, half = tuple(r.shape), bool(r.is_half)
        except Exception as e:  # noqa: BLE001
            _warn_once(path, "open H5 file", e)
            plan.unreadable.append(path)
            continue
        if len(shape) == 2 and plan.dim == 0:
            plan.dim = int(shape[1])
        if len(shape) != 2 or shape[1] != plan.dim:
            raise ValueError(f"{path}: 'cls' has shape {shape}, but the other files hold rows of width {plan.dim} "
                             f"(all files of one store must have the same row width)")
        if not half:
            plan.not_half.append(path)
        plan.files[path] = (plan.total_rows, int(shape[0]))
        plan.total_rows += int(shape[0])
    return plan


def manifest_windows(manifest: list, seq_len: int, files: Dict[str, Tuple[int, int]]):
    """Per manifest entry: the first row of its window in the store laid out by ``files`` (int64; -1 when its file has no
    rows or the window is not inside the file) and its label (int64; -1 with it)."""
    n = len(manifest)
    first, label = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for i, (path, centre, lab) in enumerate(manifest):
        entry = files.get(path)
        if entry is None:
            continue
        start = window_start(centre, seq_len, entry[1])
        if start >= 0 and int(lab) != -1:
            first[i], label[i] = entry[0] + start, int(lab)
    return first, label
