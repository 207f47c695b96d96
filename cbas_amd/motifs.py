"""Cluster every resident frame into motifs: "what behaviours are in these recordings at all, and which few frames should I look
at first?" - the question before any frame is labelled.

    python -m cbas_amd.motifs --dir RECORDINGS | --files A_cls.h5 B_cls.h5 ... --clusters K [--iters N] [--no-normalize]
                              [--smooth W] [--load clusters.npz] [--save clusters.npz] --out frames.csv [--runs runs.csv]
                              [--exemplars exemplars.csv] [--write-outputs MODEL_NAME]
                              [--hmm ITERS [--temperature T] [--mean-duration F] [--save-hmm hmm.npz] | --load-hmm hmm.npz]

k-means over the fp16 rows of a ``search.FrameIndex`` (``cbas_rows_kmeans_fit`` / ``cbas_rows_kmeans_assign``,
csrc/rows_kmeans.hip): deterministic farthest-point seeding, a fixed number of Lloyd rounds, clusters numbered by descending size.
The per-frame motif then goes where a behaviour goes: ``motif_runs`` (bouts per file through ``postprocess.labels_median`` /
``label_runs``), ``transition_counts``, ``exemplars`` (the index's own cosine search around every centroid) and ``write_outputs``
(one-hot ``_outputs.csv`` files that ``activity_bins`` and the actogram read).  The reference has no unsupervised grouping.
DESIGN.md section 21.  With ``--hmm`` the clustering only starts a motif HMM (``motif_hmm.fit``) and the
outputs come from its Viterbi labels and posteriors; without it every output is what it was.
"""
from __future__ import annotations

import argparse
import csv
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

MAX_CLUSTERS, MAX_DIM = 64, 1536                      # the limits of cbas_rows_kmeans_* (include/cbas_mi355x.h)
SEGMENT, TILE = 4096, 128                             # CBAS_ROWS_KMEANS_SEGMENT; csrc/rows_kmeans.hip: rows per workgroup of the pass
FRAME_COLUMNS = ["file", "frame", "motif", "dist2"]
RUN_COLUMNS = ["file", "motif", "start", "end"]
EXEMPLAR_COLUMNS = ["motif", "rank", "file", "frame", "score"]


def motif_names(k: int) -> List[str]:
    return [f"motif_{j:02d}" for j in range(int(k))]


class FrameClusters:
    """A fitted clustering: ``centroids`` (k, D) float32 by descending ``counts`` (k) int64, ``inertia`` (iters + 1) float32,
    ``seed_rows`` the ``(file, frame)`` the seeding chose, in seeding order (None for a fit started from ``init``), ``dim``,
    ``normalize``."""

    def __init__(self, centroids, counts, inertia, seed_rows, dim: int, normalize: bool):
        self.centroids = np.ascontiguousarray(centroids, np.float32)
        self.counts = np.asarray(counts, np.int64)
        self.inertia = np.asarray(inertia, np.float32)
        self.seed_rows = None if seed_rows is None else [(str(p), int(f)) for p, f in seed_rows]
        self.dim, self.normalize = int(dim), bool(normalize)
        if self.centroids.ndim != 2 or self.centroids.shape[1] != self.dim or self.counts.shape != (self.centroids.shape[0],):
            raise ValueError(f"centroids of shape {self.centroids.shape} and counts of shape {self.counts.shape} for rows of width {self.dim}")

    @property
    def n_clusters(self) -> int:
        return int(self.centroids.shape[0])

    def save(self, path: str) -> None:
        seeds = self.seed_rows or []
        np.savez(path, centroids=self.centroids, counts=self.counts, inertia=self.inertia, dim=np.int64(self.dim),
                 normalize=np.int64(self.normalize), has_seeds=np.int64(self.seed_rows is not None),
                 seed_files=np.array([p for p, _ in seeds], dtype=np.str_), seed_frames=np.array([f for _, f in seeds], np.int64))

    @classmethod
    def load(cls, path: str) -> "FrameClusters":
        with np.load(path, allow_pickle=False) as z:
            seeds = list(zip(z["seed_files"].tolist(), z["seed_frames"].tolist())) if int(z["has_seeds"]) else None
            return cls(z["centroids"], z["counts"], z["inertia"], seeds, int(z["dim"]), bool(int(z["normalize"])))


def _check_index(index, what: str) -> None:
    if index.device.type != "cuda":
        raise RuntimeError(f"{what} runs on a GPU (cbas_rows_kmeans_*); this index was built on {index.device}")


def _init_centroids(index, init, k: int) -> np.ndarray:
    if isinstance(init, (list, tuple)) and init and isinstance(init[0], (list, tuple)) and isinstance(init[0][0], (str, os.PathLike)):
        init = np.stack([index.query_from(*q) for q in init])
    c = np.asarray(init.detach().cpu().numpy() if torch.is_tensor(init) else init, np.float32)
    if c.ndim != 2 or c.shape != (k, index.dim):
        raise ValueError(f"init of shape {tuple(c.shape)}: ({k}, {index.dim})")
    if not np.isfinite(c).all():
        raise ValueError("an initial centroid is not finite")
    return np.ascontiguousarray(c)


def cluster_frames(index, n_clusters: int = 16, iters: int = 20, normalize: bool = True, init=None, clusters: Optional[FrameClusters] = None):
    """``(labels, dist2, clusters)``: ``labels`` (N,) int32 and ``dist2`` (N,) float32 on the index's device, the motif of every
    row and its squared distance to that centroid.  Fits ``n_clusters`` motifs in ``iters`` rounds - from farthest-point seeds, or
    from ``init``: a ``(k, D)`` array, or a list of ``(path, start[, end])`` (``index.query_from``) - unless ``clusters`` is
    given: then the rows are only assigned to those centroids, so later recordings carry the same motif numbers."""
    _check_index(index, "the clustering")
    lib = _lib.load()
    N, D, dev = index.n_rows, index.dim, index.device
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        labels = torch.empty(N, dtype=torch.int32, device=dev)
        dist2 = torch.empty(N, dtype=torch.float32, device=dev)
        if clusters is not None:
            if clusters.dim != D:
                raise ValueError(f"the clusters were fitted on rows of width {clusters.dim}; this index holds rows of width {D}")
            cent = torch.from_numpy(clusters.centroids).to(dev)
            _lib.check(lib.cbas_rows_kmeans_assign(index.rows.data_ptr(), N, D, D, clusters.n_clusters, int(clusters.normalize), cent.data_ptr(),
                                                   labels.data_ptr(), dist2.data_ptr(), stream), "cbas_rows_kmeans_assign")
            return labels, dist2, clusters
        k, iters = int(n_clusters), int(iters)
        if k < 2 or k > MAX_CLUSTERS or k > N:
            raise ValueError(f"n_clusters = {k}: 2 .. {MAX_CLUSTERS}, at most the {N} rows of the index")
        if iters < 0:
            raise ValueError(f"iters = {iters}: at least 0")
        start = None if init is None else torch.from_numpy(_init_centroids(index, init, k)).to(dev)
        cent = torch.empty((k, D), dtype=torch.float32, device=dev)
        counts = torch.empty(k, dtype=torch.int64, device=dev)
        inertia = torch.empty(iters + 1, dtype=torch.float32, device=dev)
        seeds = torch.empty(k, dtype=torch.int64, device=dev)
        ws, need = _lib.workspace("cbas_rows_kmeans_workspace_bytes", dev, N, D, k)
        _lib.check(lib.cbas_rows_kmeans_fit(index.rows.data_ptr(), N, D, D, k, iters, int(bool(normalize)), None if start is None else start.data_ptr(),
                                            cent.data_ptr(), counts.data_ptr(), inertia.data_ptr(), seeds.data_ptr(), labels.data_ptr(),
                                            dist2.data_ptr(), ws.data_ptr(), need, stream), "cbas_rows_kmeans_fit")
        seed_rows = None if init is not None else [index.locate(r) for r in seeds.cpu().numpy()]
        fitted = FrameClusters(cent.cpu().numpy(), counts.cpu().numpy(), inertia.cpu().numpy(), seed_rows, D, bool(normalize))
    return labels, dist2, fitted


def _labels_tensor(index, labels) -> torch.Tensor:
    t = labels if torch.is_tensor(labels) else torch.from_numpy(np.asarray(labels))
    t = t.to(index.device, torch.int32).contiguous()
    if t.dim() != 1 or int(t.shape[0]) != index.n_rows:
        raise ValueError(f"labels of shape {tuple(t.shape)}: ({index.n_rows},)")
    return t


def _smoothing(smooth_window: int, k: int) -> int:
    from . import postprocess as _post
    w = int(smooth_window)
    if w < 1 or w % 2 == 0:
        raise ValueError(f"smooth_window = {w}: odd and at least 1")
    if k < 1 or k > _post.MAX_CLASSES:
        raise ValueError(f"{k} motifs: labels_median and label_runs take 1 .. {_post.MAX_CLASSES} classes")
    return w


def runs_host(labels: np.ndarray, table: np.ndarray, smooth_window: int = 1, min_frames: int = 1) -> List[List[Tuple[int, int, int]]]:
    """``motif_runs`` on the host (``postprocess.median_host`` / ``label_runs_host``): per clip of ``table`` the bouts."""
    from . import postprocess as _post
    out = []
    for first, n in np.asarray(table, np.int64).reshape(-1, 2):
        x = _post.median_host(np.asarray(labels[first:first + n], np.int64), smooth_window)
        runs = _post.label_runs_host(x, np.ones(x.size, np.float32))
        out.append([(lab, a, b) for a, b, lab, _ in runs if b - a + 1 >= min_frames])
    return out


def motif_runs(index, labels, clusters: FrameClusters, smooth_window: int = 1, min_frames: int = 1) -> List[List[Tuple[int, int, int]]]:
    """Per file of the index the bouts ``(motif, start, end)`` (frames within the file, ``end`` inclusive) of at least
    ``min_frames`` frames, after a median filter of ``smooth_window`` frames (``postprocess.labels_median``: zero-padded per
    file, so no window and no bout crosses a file)."""
    from . import postprocess as _post
    _check_index(index, "motif_runs")
    k = clusters.n_clusters
    w = _smoothing(smooth_window, k)
    t = _labels_tensor(index, labels)
    if w > 1:
        t = _post.labels_median(t, index._table, k, w)
    records = _post.label_runs(t, torch.ones(index.n_rows, dtype=torch.float32, device=index.device), index._table, k)
    out: List[List[Tuple[int, int, int]]] = [[] for _ in index.files]
    for r in records:
        if int(r["end_frame"]) - int(r["start_frame"]) + 1 >= int(min_frames):
            out[int(r["clip"])].append((int(r["label"]), int(r["start_frame"]), int(r["end_frame"])))
    return out


def transition_counts(index, labels, k: int) -> torch.Tensor:
    """``(k, k)`` int64 on the index's device: how often motif a at frame t is followed by motif b at frame t + 1 of the same file."""
    t = _labels_tensor(index, labels).to(torch.int64)
    k = int(k)
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= k):
        raise ValueError(f"a label outside [0, {k})")
    pair = t[:-1] * k + t[1:]
    keep = torch.ones(max(index.n_rows - 1, 0), dtype=torch.bool, device=t.device)
    firsts = torch.from_numpy(index._table[:, 0][index._table[:, 1] > 0]).to(t.device)
    firsts = firsts[firsts > 0]
    keep[firsts - 1] = False                                       # the last frame of a file is followed by another file's first
    return torch.bincount(pair[keep], minlength=k * k).reshape(k, k)


def exemplars(index, clusters: FrameClusters, per_motif: int = 5, min_gap: int = 15):
    """Per motif the ``per_motif`` frames most like its centroid (``index.search``: cosine peaks, ``min_gap`` frames apart)."""
    return index.search(clusters.centroids, k=per_motif, min_gap=min_gap)


def write_outputs(index, labels, clusters: FrameClusters, model_name: str) -> List[str]:
    """One-hot ``(N, k)`` probabilities under the names ``motif_00 ...`` as ``<stem>_<model_name>_outputs.csv`` beside every file
    (``knn.write_outputs``): ``activity_bins`` and the actogram then take a motif as they take a behaviour."""
    from . import knn as _knn
    t = _labels_tensor(index, labels).to(torch.int64)
    probs = torch.nn.functional.one_hot(t, clusters.n_clusters).to(torch.float32)
    return _knn.write_outputs(index, probs, motif_names(clusters.n_clusters), model_name)


# ---- command line ---------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m cbas_amd.motifs", description=__doc__.split("\n\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--dir", help="a directory searched for *_cls.h5 files")
    src.add_argument("--files", nargs="+", help="_cls.h5 files")
    ap.add_argument("--clusters", type=int, default=None, metavar="K", help="how many motifs to fit (not with --load)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-normalize", action="store_true", help="cluster the rows as they are instead of their directions")
    ap.add_argument("--smooth", type=int, default=1, metavar="W", help="median filter (odd) before --runs")
    ap.add_argument("--min-frames", type=int, default=1, help="shortest bout of --runs")
    ap.add_argument("--load", default=None, help="assign to the centroids of this .npz instead of fitting")
    ap.add_argument("--save", default=None, help="write the fitted clusters to this .npz")
    ap.add_argument("--out", required=True, help="the CSV to write: " + ",".join(FRAME_COLUMNS))
    ap.add_argument("--runs", default=None, help="a CSV of bouts: " + ",".join(RUN_COLUMNS))
    ap.add_argument("--exemplars", default=None, help="a CSV of the frames most like each centroid: " + ",".join(EXEMPLAR_COLUMNS))
    ap.add_argument("--per-motif", type=int, default=5)
    ap.add_argument("--min-gap", type=int, default=15)
    ap.add_argument("--write-outputs", default=None, metavar="MODEL_NAME", help="write <stem>_<MODEL_NAME>_outputs.csv beside every file")
    ap.add_argument("--hmm", type=int, default=None, metavar="ITERS",
                    help="fit a motif HMM (motif_hmm.fit) in ITERS rounds from the clustering; the outputs come from its Viterbi labels")
    ap.add_argument("--temperature", type=float, default=None, metavar="T", help="1 / kappa of the HMM's emissions (default: calibrated)")
    ap.add_argument("--mean-duration", type=float, default=40.0, metavar="F", help="mean bout length in frames of the HMM's starting transitions")
    ap.add_argument("--save-hmm", default=None, metavar="hmm.npz", help="write the fitted HMM to this .npz")
    ap.add_argument("--load-hmm", default=None, metavar="hmm.npz", help="segment with the HMM of this .npz instead of fitting")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--max-gb", type=float, default=None)
    return ap


def parse_cli(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.load_hmm is not None:
        if a.clusters is not None or a.load is not None or a.hmm is not None or a.save_hmm is not None:
            ap.error("--load-hmm segments with a fitted model: not with --clusters, --load, --hmm or --save-hmm")
    elif (a.clusters is None) == (a.load is None):
        ap.error("give --clusters K to fit, or --load clusters.npz to assign")
    if a.hmm is not None and a.hmm < 0:
        ap.error(f"--hmm {a.hmm}: at least 0 rounds")
    if a.hmm is None and a.load_hmm is None and (a.temperature is not None or a.save_hmm is not None):
        ap.error("--temperature and --save-hmm belong to --hmm")
    if a.temperature is not None and not a.temperature > 0.0:
        ap.error(f"--temperature {a.temperature}: positive")
    if not a.mean_duration > 1.0:
        ap.error(f"--mean-duration {a.mean_duration}: more than 1 frame")
    if (a.hmm is not None or a.load_hmm is not None) and a.smooth != 1:
        ap.error("--smooth is the median filter; with an HMM the transitions do the smoothing")
    if a.clusters is not None and not 2 <= a.clusters <= MAX_CLUSTERS:
        ap.error(f"--clusters {a.clusters}: 2 .. {MAX_CLUSTERS}")
    if a.iters < 0:
        ap.error(f"--iters {a.iters}: at least 0")
    if a.smooth < 1 or a.smooth % 2 == 0:
        ap.error(f"--smooth {a.smooth}: odd and at least 1")
    if a.min_frames < 1:
        ap.error(f"--min-frames {a.min_frames}: at least 1")
    if not 1 <= a.per_motif <= 64:
        ap.error(f"--per-motif {a.per_motif}: 1 .. 64")
    return ap, a


def write_frames_csv(path: str, index, labels: np.ndarray, dist2: np.ndarray) -> None:
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(FRAME_COLUMNS)
        for file, (first, n) in zip(index.files, index._table):
            for t in range(int(n)):
                w.writerow([file, t, int(labels[first + t]), f"{float(dist2[first + t]):.6g}"])


HMM_FRAME_COLUMNS = ["file", "frame", "motif", "posterior"]


def main_hmm(ap, a) -> int:
    """``--hmm`` / ``--load-hmm``: the frames CSV (its last column the posterior of the frame's motif in place of dist2), ``--runs``
    and ``--write-outputs`` from the HMM's Viterbi labels; ``--write-outputs`` writes the graded posteriors.  On ``--device cpu`` the
    fit is the float64 numpy statement of the rounds (small files only) and ``--exemplars``, a search on the device, is refused."""
    from . import bouts as _bouts, knn as _knn, motif_hmm as _hmm, search as _search
    try:
        index = _search.FrameIndex(a.dir if a.dir else a.files, a.device, a.max_gb)
        on_gpu = index.device.type == "cuda"
        if a.exemplars and not on_gpu:
            raise ValueError("--exemplars searches on a GPU")
        if a.load_hmm:
            model = _hmm.MotifHMM.load(a.load_hmm)
            gamma = model.posteriors(index)
        else:
            init = FrameClusters.load(a.load) if a.load else None
            C = init.n_clusters if init is not None else a.clusters
            gamma, model = _hmm.fit(index, n_states=C, iters=a.hmm, temperature=a.temperature, init=init, normalize=not a.no_normalize,
                                    transitions=_bouts.sticky_transitions(C, mean_duration=a.mean_duration, as_probs=True))
        labels = model.labels(index)
    except (ValueError, MemoryError, OSError) as e:
        ap.error(str(e))
    if a.save_hmm:
        model.save(a.save_hmm)
    k = model.n_states
    host = labels.cpu().numpy()
    conf = gamma.cpu().numpy()[np.arange(index.n_rows), np.maximum(host, 0)]
    with open(a.out, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(HMM_FRAME_COLUMNS)
        for file, (first, n) in zip(index.files, index._table):
            for t in range(int(n)):
                w.writerow([file, t, int(host[first + t]), f"{float(conf[first + t]):.6g}"])
    rounds = model.loglik
    print(f"{k} motifs over {index.n_rows} frames of {len(index.files)} files, temperature {model.temperature:.6g}"
          + (f", log-likelihood {rounds[0]:.1f} -> {rounds[-1]:.1f} bits" if rounds.size and not a.load_hmm else "") + f" -> {a.out}")
    if a.runs:
        runs = motif_runs(index, labels, model, 1, a.min_frames) if on_gpu else runs_host(host, index._table, 1, a.min_frames)
        with open(a.runs, "w", newline="") as f:
            w = csv.writer(f, lineterminator="\n")
            w.writerow(RUN_COLUMNS)
            for file, file_runs in zip(index.files, runs):
                for motif, start, end in file_runs:
                    w.writerow([file, motif, start, end])
    if a.exemplars:
        with open(a.exemplars, "w", newline="") as f:
            w = csv.writer(f, lineterminator="\n")
            w.writerow(EXEMPLAR_COLUMNS)
            for motif, hits in enumerate(exemplars(index, model, a.per_motif, a.min_gap)):
                for rank, h in enumerate(hits):
                    w.writerow([motif, rank, h["file"], h["frame"], f"{h['score']:.6f}"])
    if a.write_outputs:
        paths = _knn.write_outputs(index, gamma, motif_names(k), a.write_outputs)
        print(f"{len(paths)} files like {paths[0]}")
    return 0


def main(argv=None) -> int:
    from . import search as _search
    ap, a = parse_cli(argv)
    if a.hmm is not None or a.load_hmm is not None:
        return main_hmm(ap, a)
    try:
        index = _search.FrameIndex(a.dir if a.dir else a.files, a.device, a.max_gb)
        loaded = FrameClusters.load(a.load) if a.load else None
        labels, dist2, clusters = cluster_frames(index, n_clusters=a.clusters or 2, iters=a.iters, normalize=not a.no_normalize, clusters=loaded)
    except (ValueError, MemoryError, OSError) as e:
        ap.error(str(e))
    if a.save:
        clusters.save(a.save)
    write_frames_csv(a.out, index, labels.cpu().numpy(), dist2.cpu().numpy())
    print(f"{clusters.n_clusters} motifs over {index.n_rows} frames of {len(index.files)} files -> {a.out}")
    if a.runs:
        with open(a.runs, "w", newline="") as f:
            w = csv.writer(f, lineterminator="\n")
            w.writerow(RUN_COLUMNS)
            for file, runs in zip(index.files, motif_runs(index, labels, clusters, a.smooth, a.min_frames)):
                for motif, start, end in runs:
                    w.writerow([file, motif, start, end])
    if a.exemplars:
        with open(a.exemplars, "w", newline="") as f:
            w = csv.writer(f, lineterminator="\n")
            w.writerow(EXEMPLAR_COLUMNS)
            for motif, hits in enumerate(exemplars(index, clusters, a.per_motif, a.min_gap)):
                for rank, h in enumerate(hits):
                    w.writerow([motif, rank, h["file"], h["frame"], f"{h['score']:.6f}"])
    if a.write_outputs:
        paths = write_outputs(index, labels, clusters, a.write_outputs)
        print(f"{len(paths)} files like {paths[0]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
