"""Generate the all-token golden vectors (tests/golden/hidden_state.npz) from transformers' own models: last_hidden_state in
fp32 on the CPU, with seeded synthetic weights (cbas_amd.weights) and frames (cbas_amd.synth.cage_frames), fed the way
DinoEncoder.forward feeds them (green / 255, three identical channels).

    python tests/golden/make_goldens_hidden_state.py [--out DIR]

One file, keys prefixed by the fixture's name:
    <name>_rows    the token rows kept (all T of the tiny fixtures; rows 0 .. NP and every 7th patch row of the 224^2 ones)
    <name>_hidden  (n, len(rows), D) float32  model(pixel_values=x).last_hidden_state[:, rows]
    <name>_n / _height / _width / _seed / _frames_sha
ViT rows are CLS, registers, then the patches in row-major grid order; DINOv3ConvNextModel's are LayerNorm(pooled mean), then
LayerNorm of each pixel of the last stage's grid.  Needs transformers; the tests that read the file do not.
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
from make_goldens_convnext import hf_convnext  # noqa: E402
from make_goldens_dinov2_plain import hf_dinov2_plain  # noqa: E402
from make_goldens_gated import hf_gated  # noqa: E402

import torch  # noqa: E402

from cbas_amd import config as C  # noqa: E402
from cbas_amd import weights as W  # noqa: E402
from cbas_amd import synth  # noqa: E402
from cbas_amd.encoder import token_grid  # noqa: E402

# name -> (config, model builder, n, H, W, frame seed, stride of the patch rows kept)
# 72 x 88: grids 4 x 5 (patch 16), 5 x 6 (patch 14), 2 x 2 (ConvNeXt) - none square, every one with an uncovered pixel margin
FIXTURES = {
    "vit_tiny": (C.VIT_TINY, MG.hf_model, 3, 72, 88, 171, 1),
    "gated_tiny": (C.VIT_TINY_GATED, hf_gated, 3, 72, 88, 172, 1),
    "dinov2reg_tiny": (C.DINOV2_REG_TINY, MG.hf_dinov2, 3, 72, 88, 173, 1),
    "dinov2_tiny": (C.DINOV2_TINY, hf_dinov2_plain, 3, 72, 88, 174, 1),
    "convnext_tiny": (C.CONVNEXT_TINY, hf_convnext, 3, 72, 88, 175, 1),
    "vitb16": (C.VIT_B16, MG.hf_model, 1, 224, 224, 176, 7),
    "convnext_t": (C.CONVNEXT_T, hf_convnext, 1, 224, 224, 177, 7),
}


def kept_rows(cfg, H, W_, stride):
    nh, nw, P0 = token_grid(cfg, H, W_)
    T = P0 + nh * nw
    return np.array(sorted(set(range(min(P0 + 1, T))) | set(range(P0, T, stride))), np.int32), T


def mint(name):
    cfg, build, n, H, W_, seed, stride = FIXTURES[name]
    weights = W.synth_convnext_weights(cfg, ENC_SEED) if C.is_convnext(cfg) else W.synth_encoder_weights(cfg, ENC_SEED)
    m = build(cfg, weights)
    frames = synth.cage_frames(seed, n, H, W_)
    x = torch.from_numpy(frames[:, :, :, 1] / 255.0).float().unsqueeze(1).repeat(1, 3, 1, 1)
    with torch.no_grad():
        hs = m(pixel_values=x).last_hidden_state
    rows, T = kept_rows(cfg, H, W_, stride)
    assert hs.shape == (n, T, cfg.hidden_size), (name, hs.shape, T)
    hidden = hs[:, torch.from_numpy(rows).long()].numpy().astype(np.float32)
    print(name, hidden.shape, "of T =", T)
    return {f"{name}_rows": rows, f"{name}_hidden": hidden, f"{name}_n": n, f"{name}_height": H, f"{name}_width": W_,
            f"{name}_seed": seed, f"{name}_frames_sha": sha(frames)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    res = {"enc_seed": ENC_SEED, "names": np.array(list(FIXTURES))}
    for k in FIXTURES:
        res.update(mint(k))
    path = os.path.join(a.out, "hidden_state.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")
