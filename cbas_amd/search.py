"""Search resident CLS rows for frames like a query: "I have labelled three bouts of this behaviour; where else does it happen?"

    python -m cbas_amd.search --dir RECORDINGS | --files A_cls.h5 B_cls.h5 ...
                              --like FILE:FRAME[-END] [--like ...] [--k 20] [--min-gap 15] [--threshold T]
                              [--exclude FILE:A-B ...] --out hits.csv

``FrameIndex`` holds the fp16 rows of many ``_cls.h5`` files in one device tensor (``train.ResidentRows``) with one clip per
file; ``search`` scores every row against the queries by cosine (``cbas_rows_search``, csrc/rows_search.hip: one streaming
pass over the rows) and returns, per query, the k best PEAKS: rows that beat every row of their file within ``min_gap`` frames,
so a bout of near-identical neighbouring frames gives one hit.  The reference has no search over features (its guided
labelling needs a trained head); this is the nearest-neighbour protocol of the self-supervised encoders themselves.
DESIGN.md section 19.
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, datasets as _ds, h5io

MAX_QUERIES, MAX_K, MAX_GAP = 64, 64, 65535       # the limits of one cbas_rows_search call (include/cbas_mi355x.h)
CSV_COLUMNS = ["query", "rank", "file", "frame", "score"]


def find_cls_files(directory: str) -> List[str]:
    """Every ``*_cls.h5`` under ``directory``, sorted."""
    return sorted(glob.glob(os.path.join(directory, "**", "*_cls.h5"), recursive=True))


class FrameIndex:
    """The half-precision rows of ``paths_or_dir`` (a directory searched for ``*_cls.h5``, or a list of files) resident on
    ``device``; one clip per file, so no window of the peak rule crosses a file.  ``max_gb`` caps the bytes the rows may take
    below what ``train``'s memory rule allows (free device memory minus its headroom, CBAS_TRAIN_RESIDENT_MAX_GB)."""

    def __init__(self, paths_or_dir, device, max_gb: Optional[float] = None):
        from . import train as _train
        if isinstance(paths_or_dir, (str, os.PathLike)):
            if not os.path.isdir(paths_or_dir):
                raise ValueError(f"{paths_or_dir} is not a directory (pass a list for single files)")
            paths = find_cls_files(os.fspath(paths_or_dir))
            if not paths:
                raise ValueError(f"no *_cls.h5 file under {paths_or_dir}")
        else:
            paths = [os.fspath(p) for p in paths_or_dir]
            if not paths:
                raise ValueError("no files given")
        plan = _ds.plan_files(paths)                               # ValueError for files of mixed widths
        if plan.unreadable:
            raise ValueError(f"{plan.unreadable[0]} cannot be read as a _cls.h5 file")
        if plan.not_half:
            raise ValueError(f"{plan.not_half[0]} does not hold half-precision rows (the resident store is fp16)")
        if plan.total_rows == 0:
            raise ValueError("the files hold no rows")
        if plan.dim % 32 or plan.dim > 1536:
            raise ValueError(f"rows of width {plan.dim}: cbas_rows_search takes multiples of 32 up to 1536")
        if max_gb is not None and plan.nbytes > float(max_gb) * 2 ** 30:
            raise MemoryError(f"training data: host loader ({_train._thousands(plan.total_rows)} rows need {plan.nbytes / 1e6:.0f} MB, "
                              f"{max(float(max_gb) * 2 ** 30, 0.0) / 1e6:.0f} MB may be used)")
        self.device = torch.device(device)
        if self.device.type == "cuda":                             # a "cpu" index answers locate / query_from only: search refuses
            fits, line = _train._fit_line(plan, self.device)
            if not fits:
                raise MemoryError(line)
        store = _train.ResidentRows(plan, self.device)
        if len(store.files) != len(plan.files):
            missing = [p for p in plan.files if p not in store.files]
            raise ValueError(f"{missing[0]} could not be read")
        self.rows = store.rows
        self.files = list(plan.files)
        self.dim = int(plan.dim)
        self.n_rows = int(plan.total_rows)
        self._init_layout([plan.files[p] for p in self.files])
        self.clip_table = torch.from_numpy(self._table).to(self.device)

    def _init_layout(self, spans: Sequence[Tuple[int, int]]) -> None:
        self._table = np.asarray(spans, np.int64).reshape(-1, 2)
        self._bases = self._table[:, 0].copy()
        self._by_path = {os.path.abspath(p): i for i, p in enumerate(self.files)}

    # ---- host side: no device needed --------------------------------------------------------------------------------------------
    def _file(self, path) -> int:
        i = self._by_path.get(os.path.abspath(os.fspath(path)))
        if i is None:
            raise ValueError(f"{path} is not one of the {len(self.files)} files of this index")
        return i

    def _range(self, path, start, end) -> Tuple[int, int, int]:
        """(file number, first global row, rows) of frames [start, end] of a held file; ValueError outside it."""
        i = self._file(path)
        start = int(start)
        end = start if end is None else int(end)
        n = int(self._table[i, 1])
        if start < 0 or end < start or end >= n:
            raise ValueError(f"frames [{start}, {end}] lie outside the {n} frames of {self.files[i]}")
        return i, int(self._table[i, 0]) + start, end - start + 1

    def locate(self, index: int) -> Tuple[str, int]:
        """``(path, frame)`` of global row ``index``."""
        index = int(index)
        if index < 0 or index >= self.n_rows:
            raise ValueError(f"row {index} outside the {self.n_rows} rows of this index")
        # files without rows share their base with the next file: the last file that starts at or before the row holds it
        i = int(np.searchsorted(self._bases, index, side="right")) - 1
        return self.files[i], index - int(self._bases[i])

    def query_from(self, path, start: int, end: Optional[int] = None) -> np.ndarray:
        """The mean of the L2-normalised rows ``[start, end]`` of a held file: float64 on the host from the fp16 rows of the
        file, then float32.  A zero row stays zero."""
        i, _, n = self._range(path, start, end)
        with h5io.ClsReader(self.files[i]) as r:
            x = r.read(int(start), int(start) + n).astype(np.float64)
        norm = np.sqrt((x * x).sum(axis=1, keepdims=True))
        x = np.divide(x, norm, out=np.zeros_like(x), where=norm > 0)
        return x.mean(axis=0).astype(np.float32)

    def _queries(self, queries) -> np.ndarray:
        if torch.is_tensor(queries):
            queries = queries.detach().to("cpu", torch.float32).numpy()
        elif isinstance(queries, (list, tuple)) and queries and isinstance(queries[0], (list, tuple)) and isinstance(queries[0][0], (str, os.PathLike)):
            queries = np.stack([self.query_from(*q) for q in queries])
        q = np.asarray(queries, np.float32)
        if q.ndim == 1:
            q = q[None]
        if q.ndim != 2 or q.shape[1] != self.dim or q.shape[0] < 1:
            raise ValueError(f"queries of shape {tuple(q.shape)}: (D,) or (Q, D) with D = {self.dim}")
        if not np.isfinite(q).all():
            raise ValueError("a query is not finite")
        return np.ascontiguousarray(q)

    def _mask(self, exclude) -> Optional[np.ndarray]:
        if not exclude:
            return None
        mask = np.ones(self.n_rows, np.uint8)
        for path, a, b in exclude:
            _, first, n = self._range(path, a, b)
            mask[first:first + n] = 0
        return mask

    # ---- the search -------------------------------------------------------------------------------------------------------------
    def search(self, queries, k: int = 20, min_gap: int = 15, threshold: Optional[float] = None, exclude=None, return_trace: bool = False):
        """Per query a list of ``{"file", "frame", "score"}`` by descending score (at most ``k``, any two hits of one file more
        than ``min_gap`` frames apart).  ``queries``: a ``(D,)`` or ``(Q, D)`` array or tensor, or a list of ``(path, start[, end])``
        (``query_from``).  ``exclude``: ``(path, start, end)`` ranges never returned; they still suppress their neighbours.  With
        ``return_trace`` also the ``(Q, N)`` float32 device tensor of every row's score."""
        k, min_gap = int(k), int(min_gap)
        if self.device.type != "cuda":
            raise RuntimeError(f"the search runs on a GPU (cbas_rows_search); this index was built on {self.device}")
        if k < 1 or k > MAX_K:
            raise ValueError(f"k = {k}: 1 .. {MAX_K}")
        if min_gap < 0 or min_gap > MAX_GAP:
            raise ValueError(f"min_gap = {min_gap}: 0 .. {MAX_GAP}")
        q_host = self._queries(queries)
        mask_host = self._mask(exclude)
        lib = _lib.load()
        Q, N = q_host.shape[0], self.n_rows
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            q_dev = torch.from_numpy(q_host).to(self.device)
            mask = None if mask_host is None else torch.from_numpy(mask_host).to(self.device)
            trace = torch.empty((Q, N), dtype=torch.float32, device=self.device)
            index = torch.empty((Q, k), dtype=torch.int64, device=self.device)
            score = torch.empty((Q, k), dtype=torch.float32, device=self.device)
            ws, need = _lib.workspace("cbas_rows_search_workspace_bytes", self.device, N, min(Q, MAX_QUERIES), k)
            for a in range(0, Q, MAX_QUERIES):
                b = min(Q, a + MAX_QUERIES)
                _lib.check(lib.cbas_rows_search(self.rows.data_ptr(), N, self.dim, self.dim, q_dev[a:b].data_ptr(), b - a,
                                                self.clip_table.data_ptr(), int(self.clip_table.shape[0]),
                                                None if mask is None else mask.data_ptr(), min_gap, int(threshold is not None),
                                                float(0.0 if threshold is None else threshold), k, trace[a:b].data_ptr(),
                                                index[a:b].data_ptr(), score[a:b].data_ptr(), ws.data_ptr(), need, stream),
                           "cbas_rows_search")
            index_host, score_host = index.cpu().numpy(), score.cpu().numpy()
        results = []
        for qi in range(Q):
            hits = []
            for r in range(k):
                if index_host[qi, r] < 0:
                    break
                path, frame = self.locate(index_host[qi, r])
                hits.append({"file": path, "frame": frame, "score": float(score_host[qi, r])})
            results.append(hits)
        return (results, trace) if return_trace else results

    # ---- k-NN labels (cbas_amd/knn.py) -----------------------------------------------------------------------------------------
    def knn_labels(self, bank, k: int = 20, temperature: float = 0.07, exclude: bool = False, class_weights=None, return_neighbours: bool = False):
        """``knn.knn_labels(self, bank, ...)``: the (N, C) weighted k-NN probabilities of every row from a ``knn.LabelBank``."""
        from . import knn as _knn
        return _knn.knn_labels(self, bank, k=k, temperature=temperature, exclude=exclude, class_weights=class_weights,
                               return_neighbours=return_neighbours)

    # ---- linear probe (cbas_amd/probe.py) ------------------------------------------------------------------------------------
    def linear_probe(self, bank, **kw):
        """``probe.fit_probe(self, bank, ...)``: softmax regression on the rows of a ``knn.LabelBank``, a ``probe.LinearProbe``."""
        from . import probe as _probe
        return _probe.fit_probe(self, bank, **kw)

    def probe_labels(self, probe, **kw):
        """``probe.probe_labels(self, probe, ...)``: the (N, C) probabilities of every row from a ``probe.LinearProbe``."""
        from . import probe as _probe
        return _probe.probe_labels(self, probe, **kw)

    # ---- bouts (cbas_amd/bouts.py) ---------------------------------------------------------------------------------------------
    def bouts(self, probs, transitions, prior=None, min_frames: int = 1):
        """``bouts.index_bouts(self, probs, transitions, ...)``: the Viterbi bouts of every file from (N, C) probabilities."""
        from . import bouts as _bouts
        return _bouts.index_bouts(self, probs, transitions, prior=prior, min_frames=min_frames)

    def smooth(self, probs, transitions, prior=None, return_counts: bool = False, emission_prior=None):
        """``bouts.index_posteriors(self, probs, transitions, ...)``: the forward-backward posteriors of every file, (N, C)
        probabilities smoothed by the transition model and still graded."""
        from . import bouts as _bouts
        return _bouts.index_posteriors(self, probs, transitions, prior=prior, return_counts=return_counts, emission_prior=emission_prior)

    # ---- motifs (cbas_amd/motifs.py) -------------------------------------------------------------------------------------------
    def cluster(self, n_clusters: int = 16, iters: int = 20, normalize: bool = True, init=None, clusters=None):
        """``motifs.cluster_frames(self, ...)``: ``(labels, dist2, clusters)``, every row's k-means motif."""
        from . import motifs as _motifs
        return _motifs.cluster_frames(self, n_clusters=n_clusters, iters=iters, normalize=normalize, init=init, clusters=clusters)

    def motif_hmm(self, **kw):
        """``motif_hmm.fit(self, ...)``: ``(gamma, model)``, a motif HMM whose emissions are learned with its transitions."""
        from . import motif_hmm as _motif_hmm
        return _motif_hmm.fit(self, **kw)

    # ---- the map (cbas_amd/framemap.py) ----------------------------------------------------------------------------------------
    def pca(self, n_components: int = 3, normalize: bool = True, iters=None, basis=None):
        """``framemap.pca_frames(self, ...)``: ``(scores, basis)``, every row's principal-component scores and the ``FramePCA``."""
        from . import framemap as _framemap
        return _framemap.pca_frames(self, n_components=n_components, normalize=normalize, iters=iters, basis=basis)


# ---- command line ---------------------------------------------------------------------------------------------------------------
def parse_span(text: str, need_end: bool = False) -> Tuple[str, int, Optional[int]]:
    """``FILE:FRAME`` or ``FILE:A-B`` -> ``(file, start, end or None)``; the LAST colon separates, so a path may hold colons."""
    path, sep, span = text.rpartition(":")
    a, dash, b = span.partition("-")
    try:
        if not sep or not path:
            raise ValueError
        start = int(a)
        end = int(b) if dash else None
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r}: expected FILE:FRAME or FILE:FIRST-LAST") from None
    if start < 0 or (end is not None and end < start) or (need_end and end is None):
        raise argparse.ArgumentTypeError(f"{text!r}: expected FILE:FIRST-LAST with 0 <= FIRST <= LAST" if need_end
                                         else f"{text!r}: frames are FRAME or FIRST-LAST with 0 <= FIRST <= LAST")
    return path, start, end


def _like(text):
    return parse_span(text)


def _exclude(text):
    return parse_span(text, need_end=True)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m cbas_amd.search", description=__doc__.split("\n\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--dir", help="a directory searched for *_cls.h5 files")
    src.add_argument("--files", nargs="+", help="_cls.h5 files")
    ap.add_argument("--like", action="append", type=_like, required=True, metavar="FILE:FRAME[-END]",
                    help="a query: the mean of the normalised rows of these frames (repeat for more queries)")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--min-gap", type=int, default=15, help="two hits of one file are more than this many frames apart (0: plain top-k)")
    ap.add_argument("--threshold", type=float, default=None, help="only hits with at least this cosine")
    ap.add_argument("--exclude", action="append", type=_exclude, default=[], metavar="FILE:A-B", help="frames never returned")
    ap.add_argument("--out", required=True, help="the CSV to write: " + ",".join(CSV_COLUMNS))
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--max-gb", type=float, default=None)
    return ap


def parse_cli(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.k < 1 or a.k > MAX_K:
        ap.error(f"--k {a.k}: 1 .. {MAX_K}")
    if a.min_gap < 0 or a.min_gap > MAX_GAP:
        ap.error(f"--min-gap {a.min_gap}: 0 .. {MAX_GAP}")
    return ap, a


def write_csv(path: str, results) -> None:
    """One line per hit: the query's number (the order of --like), the rank from 0, the file, the frame, the cosine."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(CSV_COLUMNS)
        for qi, hits in enumerate(results):
            for rank, h in enumerate(hits):
                w.writerow([qi, rank, h["file"], h["frame"], f"{h['score']:.6f}"])


def main(argv=None) -> int:
    ap, a = parse_cli(argv)
    try:
        index = FrameIndex(a.dir if a.dir else a.files, a.device, a.max_gb)
        results = index.search([(p, s) if e is None else (p, s, e) for p, s, e in a.like], k=a.k, min_gap=a.min_gap, threshold=a.threshold,
                               exclude=[(p, s, e) for p, s, e in a.exclude])
    except (ValueError, MemoryError) as e:
        ap.error(str(e))
    write_csv(a.out, results)
    print(f"{sum(len(h) for h in results)} hits of {len(results)} queries over {index.n_rows} frames of {len(index.files)} files -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
