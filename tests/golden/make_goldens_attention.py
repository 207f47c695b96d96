"""Generate the CLS attention map golden vectors (tests/golden/cls_attention_*.npz) from transformers' own models: fp32, eager
attention, on the CPU, with seeded synthetic weights (cbas_amd.weights) and frames (cbas_amd.synth.cage_frames), fed the way
DinoEncoder.forward feeds them (green / 255, three identical channels).

    python tests/golden/make_goldens_attention.py [--only vit_tiny,gated_tiny,dinov2reg_tiny,dinov2_tiny,vitb16] [--out DIR]

Per input size each fixture holds
    heads  (n, NH, T)  model(pixel_values=x, output_attentions=True).attentions[-1][:, :, 0, :]  - the CLS query's softmax row
    map    (n, P)      its mean over the heads on the patch columns NP .. T-1
    cls    (n, D)      last_hidden_state[:, 0]
plus the seeds and sizes.  Needs transformers; the tests that read the fixtures do not.
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

import torch  # noqa: E402

from cbas_amd import config as C  # noqa: E402
from cbas_amd import weights as W  # noqa: E402
from cbas_amd import synth  # noqa: E402

# name -> (config, model builder, ((tag, n, H, W, frame seed), ...))
FIXTURES = {
    "vit_tiny": (C.VIT_TINY, MG.hf_model, (("a", 3, 64, 64, 71), ("b", 3, 72, 88, 72))),            # T = 21; grid 4 x 5, T = 25
    "gated_tiny": (C.VIT_TINY_GATED, hf_gated, (("a", 3, 64, 64, 73),)),
    "dinov2reg_tiny": (C.DINOV2_REG_TINY, MG.hf_dinov2, (("a", 3, 70, 70, 74),)),                 # T = 30
    "dinov2_tiny": (C.DINOV2_TINY, hf_dinov2_plain, (("a", 3, 70, 70, 75),)),                     # NP = 1, T = 26
    "vitb16": (C.VIT_B16, MG.hf_model, (("a", 4, 224, 224, 76),)),                                # T = 201, NH = 12
}


def mint(out, name):
    cfg, build, sizes = FIXTURES[name]
    m = build(cfg, W.synth_encoder_weights(cfg, ENC_SEED))
    NP = 1 + cfg.num_register_tokens
    res = {"enc_seed": ENC_SEED, "tags": np.array([s[0] for s in sizes])}
    for tag, n, H, W_, seed in sizes:
        frames = synth.cage_frames(seed, n, H, W_)
        x = torch.from_numpy(frames[:, :, :, 1] / 255.0).float().unsqueeze(1).repeat(1, 3, 1, 1)
        with torch.no_grad():
            o = m(pixel_values=x, output_attentions=True)
        att = o.attentions[-1]
        T = cfg.num_tokens(H, W_)
        assert att.shape == (n, cfg.num_attention_heads, T, T), att.shape
        heads = att[:, :, 0, :].numpy().astype(np.float32)
        assert np.abs(heads.astype(np.float64).sum(-1) - 1.0).max() < 1e-5
        res.update({f"{tag}_n": n, f"{tag}_height": H, f"{tag}_width": W_, f"{tag}_seed": seed, f"{tag}_frames_sha": sha(frames),
                    f"{tag}_heads": heads, f"{tag}_map": heads[:, :, NP:].mean(axis=1, dtype=np.float64).astype(np.float32),
                    f"{tag}_cls": o.last_hidden_state[:, 0].numpy().astype(np.float32)})
        print(name, tag, heads.shape, "map range", float(res[f"{tag}_map"].min()), float(res[f"{tag}_map"].max()))
    np.savez_compressed(os.path.join(out, f"cls_attention_{name}.npz"), **res)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for k in FIXTURES:
        if a.only and k not in a.only.split(","):
            continue
        mint(a.out, k)
