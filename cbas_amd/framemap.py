"""Map every resident frame: PCA over the CLS rows on the device - "what does the whole store look like?"

    python -m cbas_amd.framemap --dir RECORDINGS | --files A_cls.h5 B_cls.h5 ... [--components 3] [--no-normalize] [--whiten]
                                [--load map.npz] [--save map.npz] --out frames.csv [--png map.png]
                                [--color-by-motifs clusters.npz | --color-by-outputs MODEL_NAME] [--outliers outliers.csv]

``fit_pca`` fits the mean and the ``k <= 8`` leading principal directions of the rows of a ``search.FrameIndex``
(``cbas_rows_pca_fit``, csrc/rows_pca.hip: the covariance on the fp32 matrix pipe, then the eigenvector solver of ``patch_pca``);
``project`` gives every frame's ``k`` scores and, when asked, its squared distance from that subspace (``cbas_rows_pca_project``: one
streaming pass).  ``density_map`` / ``render_map`` turn two of the components into the picture every behaviour-embedding tool shows
first, coloured by motif (``motifs``) or by predicted behaviour (``knn_labels`` / ``probe_labels``); ``outliers`` lists the frames
that are like nothing else.  A ``FramePCA`` is a few kilobytes: ``save`` / ``load`` carry a map to later recordings.  DESIGN.md
section 23.
"""
from __future__ import annotations

import argparse
import colorsys
import csv
import sys
from typing import Optional

import numpy as np
import torch

from . import _lib

MAX_COMPONENTS, MAX_DIM, MAX_ROWS = 8, 1536, 16777216     # the limits of cbas_rows_pca_* (include/cbas_mi355x.h)
CHUNK, MAX_PARTS, TILE = 1024, 64, 128                    # CBAS_ROWS_PCA_CHUNK, CBAS_ROWS_PCA_MAX_PARTS; rows per workgroup of the projection
DEFAULT_ITERS = 64                                        # encoder.PCA_DEFAULT_ITERS: what patch_pca uses
OUTLIER_COLUMNS = ["rank", "file", "frame", "residual"]


def partition(n_rows: int):
    """``(chunks, chunks_per_part, parts)`` of the covariance pass: a function of ``n_rows`` alone."""
    chunks = -(-int(n_rows) // CHUNK)
    per = -(-chunks // MAX_PARTS)
    return chunks, per, -(-chunks // per)


class FramePCA:
    """A fitted map: ``mean`` (D), ``components`` (k, D), ``eigenvalues`` (k) float32 in descending order, ``total_variance`` (the
    trace of the covariance), ``dim``, ``normalize``, and the ``n_rows`` and ``iters`` of the fit."""

    def __init__(self, mean, components, eigenvalues, total_variance: float, dim: int, normalize: bool, n_rows: int, iters: int):
        self.mean = np.ascontiguousarray(mean, np.float32)
        self.components = np.ascontiguousarray(components, np.float32)
        self.eigenvalues = np.ascontiguousarray(eigenvalues, np.float32)
        self.total_variance = float(total_variance)
        self.dim, self.normalize, self.n_rows, self.iters = int(dim), bool(normalize), int(n_rows), int(iters)
        k = self.components.shape[0] if self.components.ndim == 2 else -1
        if self.mean.shape != (self.dim,) or self.components.shape != (k, self.dim) or self.eigenvalues.shape != (k,) or not 1 <= k <= MAX_COMPONENTS:
            raise ValueError(f"mean of shape {self.mean.shape}, components of shape {self.components.shape} and eigenvalues of shape "
                             f"{self.eigenvalues.shape} for rows of width {self.dim}")

    @property
    def n_components(self) -> int:
        return int(self.components.shape[0])

    @property
    def explained_variance_ratio(self) -> np.ndarray:
        tv = np.float32(self.total_variance)
        return self.eigenvalues / tv if tv > 0 else np.zeros_like(self.eigenvalues)

    def save(self, path: str) -> None:
        np.savez(path, mean=self.mean, components=self.components, eigenvalues=self.eigenvalues, total_variance=np.float64(self.total_variance),
                 dim=np.int64(self.dim), normalize=np.int64(self.normalize), n_rows=np.int64(self.n_rows), iters=np.int64(self.iters))

    @classmethod
    def load(cls, path: str) -> "FramePCA":
        with np.load(path, allow_pickle=False) as z:
            return cls(z["mean"], z["components"], z["eigenvalues"], float(z["total_variance"]), int(z["dim"]), bool(int(z["normalize"])),
                       int(z["n_rows"]), int(z["iters"]))


def _check_index(index, what: str) -> None:
    if index.device.type != "cuda":
        raise RuntimeError(f"{what} runs on a GPU (cbas_rows_pca_*); this index was built on {index.device}")


def fit_pca(index, n_components: int = 3, normalize: bool = True, iters: Optional[int] = None) -> FramePCA:
    """The mean and the ``n_components`` leading principal directions of the index's rows (``cbas_rows_pca_fit``).  ``normalize``: of
    the rows scaled to unit length (what cosine search, k-NN and the probe see).  ``iters``: rounds of subspace iteration,
    ``patch_pca``'s by default."""
    _check_index(index, "the fit")
    k, iters = int(n_components), DEFAULT_ITERS if iters is None else int(iters)
    N, D, dev = index.n_rows, index.dim, index.device
    if not 1 <= k <= min(MAX_COMPONENTS, D):
        raise ValueError(f"n_components = {k}: 1 .. {min(MAX_COMPONENTS, D)}")
    if not 2 <= N <= MAX_ROWS:
        raise ValueError(f"{N} rows: cbas_rows_pca_fit takes 2 .. {MAX_ROWS}")
    if iters < 1:
        raise ValueError(f"iters = {iters}: at least 1")
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        mean = torch.empty(D, dtype=torch.float32, device=dev)
        comp = torch.empty((k, D), dtype=torch.float32, device=dev)
        eig = torch.empty(k, dtype=torch.float32, device=dev)
        tv = torch.empty(1, dtype=torch.float32, device=dev)
        ws, need = _lib.workspace("cbas_rows_pca_workspace_bytes", dev, N, D, k)
        _lib.check(lib.cbas_rows_pca_fit(index.rows.data_ptr(), N, D, D, k, iters, int(bool(normalize)), mean.data_ptr(), comp.data_ptr(),
                                         eig.data_ptr(), tv.data_ptr(), ws.data_ptr(), need, stream), "cbas_rows_pca_fit")
        return FramePCA(mean.cpu().numpy(), comp.cpu().numpy(), eig.cpu().numpy(), float(tv.cpu().numpy()[0]), D, normalize, N, iters)


def project_rows(rows: torch.Tensor, basis: FramePCA, whiten: bool = False, return_residual: bool = False):
    """``cbas_rows_pca_project`` on a contiguous (n, D) fp16 device tensor: ``scores`` (n, k) float32 - divided by the square roots of
    the eigenvalues with ``whiten`` - and, with ``return_residual``, the (n,) squared distances from the basis' subspace."""
    if rows.device.type != "cuda" or rows.dtype != torch.float16 or rows.dim() != 2 or not rows.is_contiguous():
        raise ValueError("rows: a contiguous (n, D) float16 tensor on a GPU")
    n, D, k, dev = int(rows.shape[0]), int(rows.shape[1]), basis.n_components, rows.device
    if basis.dim != D:
        raise ValueError(f"the map was fitted on rows of width {basis.dim}; these rows have width {D}")
    scale_host = None
    if whiten:
        if not (basis.eigenvalues > 0).all():
            raise ValueError("whiten: an eigenvalue of the map is not positive")
        scale_host = (1.0 / np.sqrt(basis.eigenvalues.astype(np.float64))).astype(np.float32)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        mean, comp = torch.from_numpy(basis.mean).to(dev), torch.from_numpy(basis.components).to(dev)
        scale = None if scale_host is None else torch.from_numpy(scale_host).to(dev)
        scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        resid = torch.empty(n, dtype=torch.float32, device=dev) if return_residual else None
        _lib.check(lib.cbas_rows_pca_project(rows.data_ptr(), n, D, D, k, int(basis.normalize), mean.data_ptr(), comp.data_ptr(),
                                             None if scale is None else scale.data_ptr(), scores.data_ptr(),
                                             None if resid is None else resid.data_ptr(), stream), "cbas_rows_pca_project")
    return (scores, resid) if return_residual else scores


def project(index, basis: FramePCA, whiten: bool = False, return_residual: bool = False, normalize: Optional[bool] = None):
    """``scores`` (N, k) float32 on the index's device, with ``return_residual`` also the (N,) residuals.  ``normalize``, when given,
    is what the caller expects of the basis: another one is refused."""
    _check_index(index, "the projection")
    if basis.dim != index.dim:
        raise ValueError(f"the map was fitted on rows of width {basis.dim}; this index holds rows of width {index.dim}")
    if normalize is not None and bool(normalize) != basis.normalize:
        raise ValueError(f"the map was fitted with normalize = {basis.normalize}; this call asks for normalize = {bool(normalize)}")
    return project_rows(index.rows, basis, whiten, return_residual)


def pca_frames(index, n_components: int = 3, normalize: bool = True, iters: Optional[int] = None, basis: Optional[FramePCA] = None):
    """``(scores, basis)``: fits unless ``basis`` is given - then later recordings land on the earlier map."""
    if basis is None:
        basis = fit_pca(index, n_components, normalize, iters)
        return project(index, basis), basis
    return project(index, basis, normalize=normalize), basis


# ---- the picture: host side -------------------------------------------------------------------------------------------------------
def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def density_map(scores, bins: int = 256, extent=None, labels=None, n_labels: Optional[int] = None, components=(0, 1)):
    """``(counts, extent)``: int64 counts (bins, bins) of the frames per bin of two components - ``counts[iy, ix]``, x the first of
    ``components``, y the second - or (bins, bins, n_labels) per bin and label.  ``extent`` = (x0, x1, y0, y1), by default the data's
    own range; a frame outside it is not counted, one on the upper edge falls into the last bin."""
    s = _host(scores)
    bins = int(bins)
    cx, cy = (int(c) for c in components)
    if s.ndim != 2 or not (0 <= cx < s.shape[1] and 0 <= cy < s.shape[1]):
        raise ValueError(f"scores of shape {s.shape}: (N, k) with the components {cx} and {cy} inside k")
    if bins < 1:
        raise ValueError(f"bins = {bins}: at least 1")
    x, y = s[:, cx].astype(np.float64), s[:, cy].astype(np.float64)
    if extent is None:
        extent = (x.min(), x.max(), y.min(), y.max()) if x.size else (0.0, 1.0, 0.0, 1.0)
    x0, x1, y0, y1 = (float(v) for v in extent)
    if not (x1 >= x0 and y1 >= y0):
        raise ValueError(f"extent = {extent}: (x0, x1, y0, y1) with x0 <= x1 and y0 <= y1")
    wx, wy = (x1 - x0) or 1.0, (y1 - y0) or 1.0
    inside = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
    ix = np.minimum(((x[inside] - x0) / wx * bins).astype(np.int64), bins - 1)
    iy = np.minimum(((y[inside] - y0) / wy * bins).astype(np.int64), bins - 1)
    if labels is None:
        counts = np.bincount(iy * bins + ix, minlength=bins * bins).reshape(bins, bins)
    else:
        lab = _host(labels).astype(np.int64)
        if lab.shape != (s.shape[0],):
            raise ValueError(f"labels of shape {lab.shape}: ({s.shape[0]},)")
        n_labels = int(lab.max()) + 1 if n_labels is None and lab.size else int(n_labels or 1)
        if lab.size and (lab.min() < 0 or lab.max() >= n_labels):
            raise ValueError(f"a label lies outside [0, {n_labels})")
        counts = np.bincount((iy * bins + ix) * n_labels + lab[inside], minlength=bins * bins * n_labels).reshape(bins, bins, n_labels)
    return counts.astype(np.int64), (x0, x1, y0, y1)


def label_palette(n: int) -> np.ndarray:
    """(n, 3) float64 RGB in [0, 1]: hues a golden-ratio step apart, so neighbouring label numbers differ clearly."""
    return np.array([colorsys.hsv_to_rgb((j * 0.61803398875) % 1.0, 0.85, 1.0) for j in range(int(n))], np.float64).reshape(-1, 3)


def render_map(counts, path: Optional[str] = None, size: Optional[int] = None) -> np.ndarray:
    """The density map as a picture, uint8 (bins, bins, 3), y upwards: brightness = log(1 + count) / log(1 + the largest count); the
    hue, for (bins, bins, n_labels) counts, that of the bin's majority label (the lowest of equal ones), white for plain counts.  With
    ``path`` also written as a PNG through Pillow, resized to ``size`` x ``size`` (nearest) when given."""
    c = np.asarray(counts)
    if c.ndim not in (2, 3) or c.shape[0] != c.shape[1]:
        raise ValueError(f"counts of shape {c.shape}: (bins, bins) or (bins, bins, n_labels)")
    total = c if c.ndim == 2 else c.sum(axis=2)
    top = total.max() if total.size else 0
    bright = np.log1p(total.astype(np.float64)) / (np.log1p(float(top)) if top > 0 else 1.0)
    colour = np.ones((*total.shape, 3)) if c.ndim == 2 else label_palette(c.shape[2])[c.argmax(axis=2)]
    img = (bright[..., None] * colour * 255.0).astype(np.uint8)[::-1]
    if path is not None:
        from PIL import Image
        pic = Image.fromarray(np.ascontiguousarray(img))
        if size:
            pic = pic.resize((int(size), int(size)), Image.NEAREST)
        pic.save(path, format="PNG")
    return img


def write_frames_csv(path: str, index, scores, residual=None) -> None:
    """One line per frame: ``file,frame,pc1..pck[,residual]``."""
    s = _host(scores)
    r = None if residual is None else _host(residual)
    if s.ndim != 2 or s.shape[0] != index.n_rows or (r is not None and r.shape != (index.n_rows,)):
        raise ValueError(f"scores of shape {s.shape} for the {index.n_rows} rows of this index")
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["file", "frame", *[f"pc{j + 1}" for j in range(s.shape[1])], *(["residual"] if r is not None else [])])
        for file, (first, n) in zip(index.files, index._table):
            for i in range(int(n)):
                m = int(first) + i
                w.writerow([file, i, *[f"{v:.6g}" for v in s[m]], *([f"{r[m]:.6g}"] if r is not None else [])])


def outliers(index, residual, top: int = 50, min_gap: int = 15):
    """The ``top`` frames of largest residual as ``{"file", "frame", "residual"}``, by descending residual (ties to the earlier
    row): only PEAKS are listed - frames that no frame of their file within ``min_gap`` frames exceeds, nor an earlier one within
    the gap equals - the gap rule of ``search``, so one odd bout gives one line."""
    r = _host(residual).astype(np.float32)
    top, gap = int(top), int(min_gap)
    if r.shape != (index.n_rows,):
        raise ValueError(f"residual of shape {r.shape}: ({index.n_rows},)")
    if top < 1 or gap < 0:
        raise ValueError(f"top = {top}, min_gap = {gap}: at least 1 and at least 0")
    peak = np.ones(r.size, bool)
    for first, n in index._table:
        seg, pk = r[first:first + n], peak[first:first + n]
        for o in range(1, min(gap, int(n) - 1) + 1):
            pk[o:] &= seg[o:] > seg[:-o]                          # nothing o frames earlier is as large
            pk[:-o] &= seg[:-o] >= seg[o:]                        # nothing o frames later is larger
    rows = np.flatnonzero(peak)
    rows = rows[np.argsort(-r[rows], kind="stable")][:top]
    out = []
    for m in rows:
        file, frame = index.locate(int(m))
        out.append({"file": file, "frame": frame, "residual": float(r[m])})
    return out


def write_outliers_csv(path: str, hits) -> None:
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(OUTLIER_COLUMNS)
        for rank, h in enumerate(hits):
            w.writerow([rank, h["file"], h["frame"], f"{h['residual']:.6g}"])


def labels_from_outputs(index, model_name: str):
    """``(labels (N,) int64, n_labels)``: per frame the argmax of ``<stem>_<model_name>_outputs.csv`` beside every file of the index
    (what ``knn``, ``probe``, ``motifs`` and a head write)."""
    from . import pipeline as _pipeline
    labels, width = np.zeros(index.n_rows, np.int64), None
    for file, (first, n) in zip(index.files, index._table):
        path = file[:-len("_cls.h5")] + f"_{model_name}_outputs.csv" if file.endswith("_cls.h5") else file + f"_{model_name}_outputs.csv"
        names, f64, _ = _pipeline.read_outputs_csv(path)
        if f64.shape[0] != int(n) or (width is not None and f64.shape[1] != width):
            raise ValueError(f"{path} holds {f64.shape[0]} rows of {f64.shape[1]} columns; {file} has {int(n)} frames")
        width = f64.shape[1]
        labels[first:first + n] = np.nan_to_num(f64, nan=-np.inf).argmax(axis=1) if n else 0
    return labels, int(width or 1)


# ---- command line ---------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m cbas_amd.framemap", description=__doc__.split("\n\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--dir", help="a directory searched for *_cls.h5 files")
    src.add_argument("--files", nargs="+", help="_cls.h5 files")
    ap.add_argument("--components", type=int, default=3)
    ap.add_argument("--no-normalize", action="store_true", help="fit the rows as they are, not scaled to unit length")
    ap.add_argument("--whiten", action="store_true", help="divide every score by the square root of its eigenvalue")
    ap.add_argument("--iters", type=int, default=None, help="rounds of subspace iteration")
    ap.add_argument("--load", default=None, help="project onto the map of this .npz instead of fitting")
    ap.add_argument("--save", default=None, help="write the fitted map to this .npz")
    ap.add_argument("--out", required=True, help="the CSV to write: file,frame,pc1..pck,residual")
    ap.add_argument("--png", default=None, help="paint the density of the first two components")
    ap.add_argument("--bins", type=int, default=256)
    col = ap.add_mutually_exclusive_group()
    col.add_argument("--color-by-motifs", default=None, metavar="clusters.npz", help="colour by the motif of motifs.FrameClusters")
    col.add_argument("--color-by-outputs", default=None, metavar="MODEL_NAME", help="colour by the argmax of <stem>_<MODEL_NAME>_outputs.csv")
    ap.add_argument("--outliers", default=None, help="write the frames of largest residual to this CSV")
    ap.add_argument("--top", type=int, default=50)
    ap.add_argument("--min-gap", type=int, default=15)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--max-gb", type=float, default=None)
    return ap


def parse_cli(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if not 1 <= a.components <= MAX_COMPONENTS:
        ap.error(f"--components {a.components}: 1 .. {MAX_COMPONENTS}")
    if a.iters is not None and a.iters < 1:
        ap.error(f"--iters {a.iters}: at least 1")
    if a.bins < 1:
        ap.error(f"--bins {a.bins}: at least 1")
    if a.top < 1:
        ap.error(f"--top {a.top}: at least 1")
    if a.min_gap < 0:
        ap.error(f"--min-gap {a.min_gap}: at least 0")
    if a.load and a.save:
        ap.error("--save writes a fitted map; with --load nothing is fitted")
    if a.load and (a.no_normalize or a.iters is not None):
        ap.error("--no-normalize and --iters belong to a fit; with --load the map's own hold")
    if (a.color_by_motifs or a.color_by_outputs) and not a.png:
        ap.error("--color-by-motifs and --color-by-outputs colour the picture: give --png")
    if a.png and a.components < 2 and not a.load:
        ap.error("--png paints two components: --components at least 2")
    return ap, a


def main(argv=None) -> int:
    from . import motifs as _motifs, search as _search
    ap, a = parse_cli(argv)
    try:
        index = _search.FrameIndex(a.dir if a.dir else a.files, a.device, a.max_gb)
        basis = FramePCA.load(a.load) if a.load else fit_pca(index, a.components, not a.no_normalize, a.iters)
        scores, resid = project(index, basis, whiten=a.whiten, return_residual=True)
        ratio = basis.explained_variance_ratio
        print(f"{index.n_rows} frames of {len(index.files)} files on {basis.n_components} components: "
              f"{100.0 * float(ratio.sum()):.1f} % of the variance ({', '.join(f'{100.0 * v:.1f}' for v in ratio)})")
        if a.save:
            basis.save(a.save)
        write_frames_csv(a.out, index, scores, resid)
        if a.png:
            if basis.n_components < 2:
                raise ValueError("--png paints two components; this map has one")
            labels = n_labels = None
            if a.color_by_motifs:
                clusters = _motifs.FrameClusters.load(a.color_by_motifs)
                labels, n_labels = _motifs.cluster_frames(index, clusters=clusters)[0], clusters.n_clusters
            elif a.color_by_outputs:
                labels, n_labels = labels_from_outputs(index, a.color_by_outputs)
            counts, _ = density_map(scores, bins=a.bins, labels=labels, n_labels=n_labels)
            render_map(counts, a.png)
        if a.outliers:
            write_outliers_csv(a.outliers, outliers(index, resid, a.top, a.min_gap))
    except (ValueError, MemoryError, OSError) as e:
        ap.error(str(e))
    return 0


if __name__ == "__main__":
    sys.exit(main())
