"""What an encoder looks at: the last layer's attention from the CLS token to the patch tokens, averaged over the heads, for
frames of a video - the picture the reference's encoder comparison tool draws (compare_encoders.py:36-49, :72-79), computed on
the device by ``DinoEncoder.cls_attention`` beside the CLS rows.

    python -m cbas_amd.attention_maps --video V --frame N --encoder ID [--encoder ID ...] --out PNG [--precision P]
                                      [--kind attention|similarity|pca|rollout|clusters] [--query Y,X] [--pca-scope frame|batch]
                                      [--layer N|all] [--clusters K] [--cluster-scope frame|batch]

``--kind similarity`` draws the other picture of the same question, from ``DinoEncoder.similarity_map``: the cosine of the CLS
token's final hidden state (``--query Y,X``: of the patch under that pixel) to every patch token's.  It needs no attention, so it
is the kind DINOv3 ConvNeXt encoders have (their query row is the pooled one, their grid the last stage's 32 x 32 pixel cells).

``--kind pca`` draws the third picture, from ``DinoEncoder.patch_pca``: the patch rows' coordinates along their first three
principal components, each stretched to [0, 1] over the picture, as red, green and blue - what the encoder separates, with no
query and no attention, so every family has it and the pictures of two families can be compared.  ``--pca-scope batch`` fits one
basis for all frames asked for (the same colours mean the same directions in each), ``frame`` (the default) one per frame.

``--kind clusters`` draws the discrete picture, from ``DinoEncoder.patch_clusters``: k-means labels of the patch rows (``--clusters
K``, default 4), one fixed colour per cluster with cluster 0 the largest, enlarged without blending.  ``--cluster-scope batch`` fits
one set of centroids for all frames asked for, ``frame`` (the default) one per frame.  Every family has it.

``--kind attention --layer N`` draws layer N's CLS attention instead of the last one's (1 .. L, negative from the end), ``--layer
all`` one map per layer side by side.  ``--kind rollout`` draws attention rollout (Abnar and Zuidema) from
``DinoEncoder.attention_rollout``: what the whole network looks at, the CLS row (``--query Y,X``: the row of the patch under that
pixel) of the product of every layer's head-averaged attention mixed half and half with the identity.

One deliberate difference from that tool: the map here is the map of what the encoder sees INSIDE CBAS - the green plane / 255
replicated to three channels at the video's own size, exactly what ``encode_file`` feeds the model (backend/cbas.py:431) - not
of an RGB picture resized and ImageNet-normalised by the checkpoint's image processor, which no CBAS embedding was made from.
The patch grid is therefore (H // patch, W // patch) and need not be square.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Mapping, Sequence, Tuple, Union

import numpy as np


KINDS = ("attention", "similarity", "pca", "rollout", "clusters")
PCA_SCOPES = ("frame", "batch")
CLUSTER_SCOPES = ("frame", "batch")
DEFAULT_CLUSTERS = 4
# render_labels: one colour per cluster, 0 (the largest cluster) to 15 - fixed, so cluster j has one colour in every picture
LABEL_PALETTE = np.array([(31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194),
                          (127, 127, 127), (188, 189, 34), (23, 190, 207), (174, 199, 232), (255, 187, 120), (152, 223, 138), (255, 152, 150),
                          (197, 176, 213), (196, 156, 148)], dtype=np.uint8)


def refuse_kind(cfg, kind: str):
    """Why an encoder of config ``cfg`` has no map of ``kind``, or None."""
    from .config import is_convnext
    if kind not in KINDS:
        return f"unknown map kind {kind!r}: one of {', '.join(KINDS)}"
    if kind == "attention" and is_convnext(cfg):
        return "a ConvNeXt encoder has no attention: --kind similarity and --kind pca are the maps it has"
    if kind == "rollout" and is_convnext(cfg):
        return "a ConvNeXt encoder has no attention to roll out: --kind similarity and --kind pca are the maps it has"
    return None


def parse_layer(text):
    """``--layer``: None, "all", or an integer (negative: from the end)."""
    if text is None or text == "all":
        return text
    try:
        return int(text)
    except ValueError:
        raise ValueError(f"--layer {text!r}: an integer or 'all'") from None


def frame_maps(encoder, path: str, frame_indices: Sequence[int], kind: str = "attention", query=None, pca_scope: str = "frame", layer=None,
               n_clusters: int = DEFAULT_CLUSTERS, cluster_scope: str = "frame"):
    """Maps of the given frames of a video: ``kind`` "attention" (``cls_attention``), "similarity" (``similarity_map`` of
    ``query``: None, or a pixel (y, x)) or "pca" (``patch_pca``, three components).  Frames are read through
    ``pipeline.open_video`` (any source it knows) and encoded in batches of ``encoder.max_batch``.  Returns ``(maps, frames_green)``:
    float32 (n, nh, nw) and uint8 (n, H, W) numpy arrays, in the order of ``frame_indices``.  For "pca" ``maps`` is the finished
    picture instead, float32 (n, H, W, 3) in [0, 1] (``render_pca`` of each frame's scores); with ``pca_scope="batch"`` the basis
    fitted on the first batch of frames colours all of them.  "rollout": ``attention_rollout`` of ``query``.  ``layer`` ("attention"
    only): a layer number, or "all" - ``maps`` then is (n, L, nh, nw).  "clusters": ``patch_clusters`` with ``n_clusters`` - ``maps``
    is the int32 (n, nh, nw) label grid; with ``cluster_scope="batch"`` the set fitted on the first batch of frames labels all of them."""
    import torch
    from . import pipeline
    idx = [int(i) for i in frame_indices]
    why = refuse_kind(encoder.config, kind)
    if why:
        raise ValueError(why)
    if not idx:
        raise ValueError("no frame index given")
    if kind == "pca" and pca_scope not in PCA_SCOPES:
        raise ValueError(f"unknown PCA scope {pca_scope!r}: one of {', '.join(PCA_SCOPES)}")
    if kind == "clusters" and cluster_scope not in CLUSTER_SCOPES:
        raise ValueError(f"unknown cluster scope {cluster_scope!r}: one of {', '.join(CLUSTER_SCOPES)}")
    basis = clusters = None
    src = pipeline.open_video(path)
    try:
        n_total = len(src)
        bad = [i for i in idx if i < 0 or i >= n_total]
        if bad:
            raise IndexError(f"frame {bad[0]} is out of range: {os.path.basename(path)} has {n_total} frames")
        maps, greens = [], []
        for i in range(0, len(idx), encoder.max_batch):
            part = idx[i:i + encoder.max_batch]
            frames = np.asarray(src.get_batch(part) if part == list(range(part[0], part[0] + len(part)))
                                else np.concatenate([np.asarray(src.get_batch([j])) for j in part]))
            green = np.ascontiguousarray(frames[:, :, :, 1] if frames.ndim == 4 else frames)      # backend/cbas.py:431
            dev = torch.from_numpy(green).to(encoder.device)
            if kind == "pca":
                scores, fitted = encoder.patch_pca(dev, 3, pca_scope, basis)
                basis = fitted if pca_scope == "batch" else None
                size = (green.shape[2], green.shape[1])
                maps.append(np.stack([render_pca(sc, size) for sc in scores.cpu().numpy()]))
            elif kind == "clusters":
                labels, fitted = encoder.patch_clusters(dev, n_clusters, cluster_scope, clusters)
                clusters = fitted if cluster_scope == "batch" else None
                maps.append(labels.cpu().numpy())
            elif kind == "rollout":
                maps.append(encoder.attention_rollout(dev, query).cpu().numpy())
            else:
                maps.append((encoder.cls_attention(dev, layer=layer)[2] if kind == "attention" else encoder.similarity_map(dev, query)).cpu().numpy())
            greens.append(green)
        return np.concatenate(maps), np.concatenate(greens)
    finally:
        if hasattr(src, "close"):
            src.close()


def render_map(map2d, size: Tuple[int, int]) -> np.ndarray:
    """One (nh, nw) map as the picture the reference tool shows: stretched to [0, 1] by its own minimum and maximum when they
    differ (a constant map is left as it is), times 255 truncated to uint8, resized to ``size`` = (width, height) with Pillow's
    bicubic filter.  Returns a uint8 (height, width) array."""
    from PIL import Image
    a = np.asarray(map2d, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError(f"render_map takes one 2-D map, got shape {a.shape}")
    return np.asarray(Image.fromarray(_to_u8(a)).resize((int(size[0]), int(size[1])), Image.BICUBIC))


def render_pca(scores, size: Tuple[int, int]) -> np.ndarray:
    """One frame's (nh, nw, k >= 3) PCA scores as a picture: components 0, 1, 2 each stretched to [0, 1] by their own minimum and
    maximum over the frame (a constant one is 0), resized to ``size`` = (width, height) with Pillow's bicubic filter - the filter
    ``render_map`` uses - and clipped to [0, 1] (bicubic overshoots).  Returns a float32 (height, width, 3) array: R, G, B."""
    from PIL import Image
    a = np.asarray(scores, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] < 3:
        raise ValueError(f"render_pca takes one frame's (nh, nw, k >= 3) scores, got shape {a.shape}")
    out = np.empty((int(size[1]), int(size[0]), 3), np.float32)
    for c in range(3):
        ch = a[:, :, c]
        lo, hi = float(ch.min()), float(ch.max())
        ch = (ch - lo) / (hi - lo) if hi > lo else np.zeros_like(ch)
        out[:, :, c] = np.clip(np.asarray(Image.fromarray(ch, mode="F").resize((int(size[0]), int(size[1])), Image.BICUBIC)), 0.0, 1.0)
    return out


def render_labels(labels, size: Tuple[int, int]) -> np.ndarray:
    """One frame's (nh, nw) cluster labels as a picture: label j painted ``LABEL_PALETTE[j]``, resized to ``size`` = (width, height)
    with nearest-neighbour sampling (a label is a name, not a quantity: nothing is blended).  Returns uint8 (height, width, 3)."""
    from PIL import Image
    a = np.asarray(labels)
    if a.ndim != 2 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"render_labels takes one frame's (nh, nw) integer labels, got shape {a.shape} of {a.dtype}")
    if a.size and (a.min() < 0 or a.max() >= len(LABEL_PALETTE)):
        raise ValueError(f"labels outside 0 .. {len(LABEL_PALETTE) - 1}")
    return np.asarray(Image.fromarray(LABEL_PALETTE[a]).resize((int(size[0]), int(size[1])), Image.NEAREST))


def _to_u8(a: np.ndarray) -> np.ndarray:
    lo, hi = float(a.min()), float(a.max())
    if hi > lo:
        a = (a - lo) / (hi - lo)
    return (a * 255).astype(np.uint8)


def compare_encoders(video: str, frame_idx: int, encoders: Mapping[str, Union[str, object]], out_png: str, precision=None,
                     kind: str = "attention", query=None, pca_scope: str = "frame", layer=None, n_clusters: int = DEFAULT_CLUSTERS,
                     cluster_scope: str = "frame") -> str:
    """One figure row per encoder: the frame as the encoder receives it (green plane) beside its rendered map (``kind``, ``query``:
    see ``frame_maps``).
    ``encoders`` maps a display name to a checkpoint directory, an HF-cache id or a ready ``DinoEncoder``; encoders built here
    are closed again.  Returns ``out_png``."""
    if not encoders:
        raise ValueError("no encoder given")
    from matplotlib.backends.backend_agg import FigureCanvasAgg      # the Agg backend, without pyplot's global state
    from matplotlib.figure import Figure
    from .encoder import DinoEncoder, token_grid
    panels = []
    for name, enc in encoders.items():
        own = isinstance(enc, str)
        if own:
            enc = DinoEncoder(enc, **({} if precision is None else {"precision": int(precision)}))
        try:
            maps, green = frame_maps(enc, video, [frame_idx], kind, query, pca_scope, layer, n_clusters, cluster_scope)
            grid = token_grid(enc.config, green.shape[1], green.shape[2])[:2]
        finally:
            if own:
                enc.close()
        size = (green.shape[2], green.shape[1])
        pic = ((maps[0] * 255).astype(np.uint8) if kind == "pca" else render_labels(maps[0], size) if kind == "clusters" else
               np.concatenate([render_map(m, size) for m in maps[0]], axis=1) if maps[0].ndim == 3 else render_map(maps[0], size))
        panels.append((name, green[0], grid, pic))
    who = "CLS token" if query is None else f"patch at pixel {tuple(query)}"
    what = ("where its CLS token looks (" + ("last layer" if layer is None else "layers 1 .. L, left to right" if layer == "all" else f"layer {layer}") +
            ", mean of heads)" if kind == "attention" else
            f"attention rollout of the {who} over every layer" if kind == "rollout" else
            "patch features along their first three principal components (R, G, B)" if kind == "pca" else
            f"k-means clusters of the patch features (k = {n_clusters}, one colour each, largest first)" if kind == "clusters" else
            "cosine of the final hidden states: " + ("CLS / pooled row" if query is None else f"patch at pixel {tuple(query)}") + " to each patch")
    _draw(Figure, FigureCanvasAgg, panels, f"{os.path.basename(video)}, frame {frame_idx}", out_png, what)
    return out_png


PANEL_HEIGHT_IN = 3.2        # every panel is this tall; its width follows the video's aspect ratio
LABEL_WIDTH_IN = 0.6         # room at the left for the encoders' names


def _draw(Figure, Canvas, panels, caption: str, out_png: str, what: str) -> None:
    """panels: (name, green plane (H, W) uint8, patch grid (nh, nw), picture) per encoder, top to bottom.  The picture is a rendered
    map, (H, W) uint8, drawn through the inferno colour map - or, for the pca kind, (H, W, 3) uint8 drawn as the RGB it is."""
    H, W = panels[0][1].shape
    panel_w = PANEL_HEIGHT_IN * W / H
    fig = Figure(figsize=(LABEL_WIDTH_IN + 2 * panel_w, PANEL_HEIGHT_IN * len(panels) + 0.5), layout="constrained")
    Canvas(fig)
    grid = fig.subplots(len(panels), 2, squeeze=False)
    for r, (name, green, (nh, nw), pic) in enumerate(panels):
        left, right = grid[r]
        left.imshow(green, cmap="gray", vmin=0, vmax=255, interpolation="nearest")
        rgb = pic.ndim == 3
        right.imshow(pic, interpolation="nearest", **({} if rgb else {"cmap": "inferno", "vmin": 0, "vmax": 255}))
        left.set_ylabel(name, fontsize=10)
        right.set_xlabel(f"{nh} x {nw} patches, " + (("one colour per cluster" if pic.dtype == np.uint8 and what.startswith("k-means") else "each component stretched to its own range over the frame") if rgb else
                                                    "stretched to the map's own range"), fontsize=8)
        for a in (left, right):
            a.set_xticks([])
            a.set_yticks([])
        if r == 0:
            left.set_title("what the encoder is fed: green / 255", fontsize=10)
            right.set_title(what, fontsize=10)
    fig.supxlabel(f"{caption}, {H} x {W} pixels", fontsize=9)
    fig.savefig(out_png, dpi=110)


def parse_cli(argv=None):
    """``(parser, namespace)``: the command line with ``query`` a pixel or None and ``layer`` None, "all" or an int; argparse's exit
    on a combination that means nothing."""
    ap = argparse.ArgumentParser(prog="python -m cbas_amd.attention_maps", description=__doc__.split("\n\n")[0])
    ap.add_argument("--video", required=True)
    ap.add_argument("--frame", type=int, required=True)
    ap.add_argument("--encoder", action="append", default=[], metavar="ID", help="checkpoint directory or HF-cache id; repeatable")
    ap.add_argument("--out", required=True, metavar="PNG")
    ap.add_argument("--precision", type=int, default=None)
    ap.add_argument("--kind", choices=KINDS, default="attention", help="similarity, pca and clusters: the kinds a ConvNeXt encoder has")
    ap.add_argument("--pca-scope", choices=PCA_SCOPES, default=None, help="pca: one basis per frame (default) or one for all frames")
    ap.add_argument("--clusters", type=int, default=None, metavar="K", help=f"clusters: how many (2 .. {len(LABEL_PALETTE)}, default {DEFAULT_CLUSTERS})")
    ap.add_argument("--cluster-scope", choices=CLUSTER_SCOPES, default=None, help="clusters: one set per frame (default) or one for all frames")
    ap.add_argument("--query", default=None, metavar="Y,X", help="similarity, rollout: the pixel whose patch is the query (default: the CLS / pooled row)")
    ap.add_argument("--layer", default=None, metavar="N|all", help="attention: the layer whose CLS attention is drawn (default: the last), or every layer in a row")
    a = ap.parse_args(argv)
    query = None
    if a.layer is not None:
        if a.kind != "attention":
            ap.error("--layer goes with --kind attention")
        try:
            a.layer = parse_layer(a.layer)
        except ValueError as e:
            ap.error(str(e))
    if a.query is not None:
        if a.kind not in ("similarity", "rollout"):
            ap.error("--query goes with --kind similarity or --kind rollout")
        try:
            y, x = (int(v) for v in a.query.split(","))
        except ValueError:
            ap.error(f"--query {a.query!r}: two integers Y,X")
        query = (y, x)
    a.query = query
    if a.pca_scope is not None and a.kind != "pca":
        ap.error("--pca-scope goes with --kind pca")
    if a.cluster_scope is not None and a.kind != "clusters":
        ap.error("--cluster-scope goes with --kind clusters")
    if a.clusters is not None and a.kind != "clusters":
        ap.error("--clusters goes with --kind clusters")
    if a.clusters is not None and not 2 <= a.clusters <= len(LABEL_PALETTE):
        ap.error(f"--clusters {a.clusters}: 2 .. {len(LABEL_PALETTE)}")
    if not a.encoder:
        ap.error("at least one --encoder is needed")
    return ap, a


def main(argv=None) -> int:
    ap, a = parse_cli(argv)
    query = a.query
    if not os.path.exists(a.video):
        ap.error(f"no such video: {a.video}")
    from . import pipeline
    src = pipeline.open_video(a.video)          # the frame index is checked before any encoder is loaded
    try:
        n = len(src)
    finally:
        if hasattr(src, "close"):
            src.close()
    if a.frame < 0 or a.frame >= n:
        ap.error(f"--frame {a.frame} is out of range: {os.path.basename(a.video)} has {n} frames")
    from .config import encoder_config_from_json, find_checkpoint_dir
    names = {}
    for e in a.encoder:
        # the kind is checked against every checkpoint's config before any is loaded
        why = refuse_kind(encoder_config_from_json(os.path.join(find_checkpoint_dir(e), "config.json")), a.kind)
        if why:
            ap.error(f"--encoder {e}: {why}")
        names[e if e not in names else f"{e} ({len(names)})"] = e
    print(compare_encoders(a.video, a.frame, names, a.out, precision=a.precision, kind=a.kind, query=query,
                           pca_scope=a.pca_scope or "frame", layer=a.layer, n_clusters=a.clusters or DEFAULT_CLUSTERS,
                           cluster_scope=a.cluster_scope or "frame"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
