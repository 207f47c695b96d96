"""Generate the per-layer golden vectors (tests/golden/encoder_layers.npz) from transformers' own models: output_hidden_states
and output_attentions in fp32 on the CPU with eager attention, seeded synthetic weights (cbas_amd.weights) and frames
(cbas_amd.synth.cage_frames), fed the way DinoEncoder.forward feeds them (green / 255, three identical channels).

    python tests/golden/make_goldens_layers.py [--out DIR]

One file, keys prefixed by the fixture's name (L layers, T tokens, NP prefix rows, P = T - NP patches):
    <name>_hs_layers   the hidden-state indices kept (transformers' numbering: 0 = embeddings output, l = after block l)
    <name>_rows        the token rows kept (all T of the tiny fixtures; make_goldens_hidden_state.kept_rows of the 224^2 one)
    <name>_hidden      (len(hs_layers), n, len(rows), D) float32   o.hidden_states[l][:, rows] - raw, no final LayerNorm
    <name>_cls_heads   (L, n, NH, T) float32   o.attentions[l][:, :, 0, :]                      (tiny fixtures only)
    <name>_cls_map     (L, n, P) float32       its head mean over the patch columns, summed in float64
    <name>_attn_mean   (L, n, T, T) float32    o.attentions[l].mean(heads), summed in float64   (tiny fixtures only)
    <name>_rollout_cls / _rollout_patch   (n, P) float64: the CLS row / row <name>_patch_query of
                       A^_L ... A^_1, A^_l = 0.5 A_l + 0.5 I, multiplied in float64 from the STORED float32 head means (the tiny
                       fixtures) or from the model's float32 attentions averaged in float64 (the 224^2 one: CLS row only)
    <name>_patch_query / _patch_pixel     the patch query's token index and the pixel (y, x) that resolves to it
    <name>_n / _height / _width / _seed / _frames_sha
Needs transformers; the tests that read the file do not.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_goldens as MG  # noqa: E402  (sets up sys.path and torch)
from make_goldens import ENC_SEED, sha  # noqa: E402
from make_goldens_dinov2_plain import hf_dinov2_plain  # noqa: E402
from make_goldens_gated import hf_gated  # noqa: E402
from make_goldens_hidden_state import kept_rows  # noqa: E402

import torch  # noqa: E402

from cbas_amd import config as C  # noqa: E402
from cbas_amd import weights as W  # noqa: E402
from cbas_amd import synth  # noqa: E402

# name -> (config, model builder, n, H, W, frame seed, stride of the patch rows kept, hidden-state layers kept or None = all,
#          full = every layer's per-head CLS rows and T x T head means)
# the frames are hidden_state.npz's own (same seeds and sizes): LayerNorm of the last raw state must give that file's rows
FIXTURES = {
    "vit_tiny": (C.VIT_TINY, MG.hf_model, 3, 72, 88, 171, 1, None, True),
    "gated_tiny": (C.VIT_TINY_GATED, hf_gated, 3, 72, 88, 172, 1, None, True),
    "dinov2reg_tiny": (C.DINOV2_REG_TINY, MG.hf_dinov2, 3, 72, 88, 173, 1, None, True),
    "dinov2_tiny": (C.DINOV2_TINY, hf_dinov2_plain, 3, 72, 88, 174, 1, None, True),
    "vitb16": (C.VIT_B16, MG.hf_model, 1, 224, 224, 176, 7, (0, 6, 12), False),
}


def rollout64(attn_mean, start=1):
    """(L, n, T, T) head means -> (n, T, T) float64 product A^_L ... A^_start."""
    A = np.asarray(attn_mean, np.float64)
    L, n, T, _ = A.shape
    eye = np.eye(T)
    R = 0.5 * A[start - 1] + 0.5 * eye
    for l in range(start, L):
        R = np.matmul(0.5 * A[l] + 0.5 * eye, R)
    return R


def mint(name):
    cfg, build, n, H, W_, seed, stride, keep, full = FIXTURES[name]
    m = build(cfg, W.synth_encoder_weights(cfg, ENC_SEED))
    frames = synth.cage_frames(seed, n, H, W_)
    x = torch.from_numpy(frames[:, :, :, 1] / 255.0).float().unsqueeze(1).repeat(1, 3, 1, 1)
    with torch.no_grad():
        o = m(pixel_values=x, output_hidden_states=True, output_attentions=True)
    L, NH, NP = cfg.num_hidden_layers, cfg.num_attention_heads, cfg.num_prefix_tokens
    rows, T = kept_rows(cfg, H, W_, stride)
    assert len(o.hidden_states) == L + 1 and len(o.attentions) == L and o.attentions[0].shape == (n, NH, T, T)
    hs_layers = np.array(range(L + 1) if keep is None else keep, np.int32)
    ridx = torch.from_numpy(rows).long()
    hidden = np.stack([o.hidden_states[int(l)][:, ridx].numpy().astype(np.float32) for l in hs_layers])
    att = np.stack([a.numpy() for a in o.attentions])                                  # (L, n, NH, T, T) float32
    heads = att[:, :, :, 0, :].astype(np.float32)
    cls_map = heads[:, :, :, NP:].mean(axis=2, dtype=np.float64).astype(np.float32)
    mean64 = att.mean(axis=2, dtype=np.float64)
    mean32 = mean64.astype(np.float32)
    nw = W_ // cfg.patch_size
    py, px = 1, 2                                                                      # a patch off the grid's edge and diagonal
    qtok = NP + py * nw + px
    pixel = np.array([py * cfg.patch_size + 3, px * cfg.patch_size + 5], np.int32)
    R = rollout64(mean32 if full else mean64)
    res = {f"{name}_hs_layers": hs_layers, f"{name}_rows": rows, f"{name}_hidden": hidden, f"{name}_cls_map": cls_map,
           f"{name}_rollout_cls": R[:, 0, NP:], f"{name}_n": n, f"{name}_height": H, f"{name}_width": W_, f"{name}_seed": seed,
           f"{name}_frames_sha": sha(frames)}
    if full:
        res.update({f"{name}_cls_heads": heads, f"{name}_attn_mean": mean32, f"{name}_rollout_patch": R[:, qtok, NP:],
                    f"{name}_patch_query": qtok, f"{name}_patch_pixel": pixel})
    print(name, "hidden", hidden.shape, "T =", T, "rollout range", float(R[:, 0, NP:].min()), float(R[:, 0, NP:].max()))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    res = {"enc_seed": ENC_SEED, "names": np.array(list(FIXTURES))}
    for k in FIXTURES:
        res.update(mint(k))
    path = os.path.join(a.out, "encoder_layers.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")
