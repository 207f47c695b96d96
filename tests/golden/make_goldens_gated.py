"""Generate the gated-MLP (DINOv3 ViT-S+ / H+ family) golden vectors under tests/golden/ by running the REFERENCE's arithmetic:
transformers' DINOv3ViTModel (use_gated_mlp, hidden_act "silu") in fp32 with eager attention on the CPU, fed the way the
reference's DinoEncoder feeds it (backend/cbas.py:431, :672-677: green / 255, three equal channels, row 0 of last_hidden_state).

    python tests/golden/make_goldens_gated.py [--only tiny,splus,w1280] [--out DIR]

Weights and frames come from the counter-based generators (cbas_amd.weights / cbas_amd.synth).  Every fixture holds the seeds and the recorded tensors only: tiny_gated's weights alone
would be 2.1 MB as float32, against the 500 KB a fixture may have.  gated_tiny.npz therefore stands for its model only while
cbas_amd.weights.synth_encoder_weights(VIT_TINY_GATED, enc_seed) stays bit-stable; a change to that generator shows as a failure of
tests/test_gated_mlp_host.py::test_float64_restatement_against_the_transformers_rows (CPU), and this script then has to be run again.
Needs transformers; the tests that read the fixtures do not.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import sys
from dataclasses import replace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from cbas_amd import config as C  # noqa: E402
from cbas_amd import weights as W  # noqa: E402
from cbas_amd import synth  # noqa: E402

ENC_SEED = 1234
# one layer at the ViT-H+ width: the D = 1280 LayerNorm / GEMM paths at a size a test can afford
W1280 = replace(C.VIT_H16PLUS, num_hidden_layers=1, image_size=32)


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def hf_gated(cfg: C.ViTConfig, weights):
    from transformers import DINOv3ViTConfig, DINOv3ViTModel
    hcfg = DINOv3ViTConfig(hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                           num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                           num_register_tokens=cfg.num_register_tokens, patch_size=cfg.patch_size, image_size=cfg.image_size,
                           layer_norm_eps=cfg.layer_norm_eps, rope_theta=cfg.rope_theta, use_gated_mlp=cfg.use_gated_mlp,
                           hidden_act=cfg.hidden_act)
    hcfg._attn_implementation = "eager"
    m = DINOv3ViTModel(hcfg).eval()
    assert type(m.model.layer[0].mlp).__name__ == "DINOv3ViTGatedMLP" if hasattr(m, "model") else True
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in weights.items()}, strict=True)
    return m


def _pixels(frames):
    g = torch.from_numpy(frames[:, :, :, 1] / 255.0).float()           # cbas.py:431
    return g.unsqueeze(1).repeat(1, 3, 1, 1)                             # cbas.py:675


def g_tiny(out):
    """tiny_gated: 2 frames at 64 x 64 and 2 at 48 x 80; per layer the MLP's activation product
    silu(gate_proj(x)) * up_proj(x) (the tensor the fused GEMM stores), each layer's output, and row 0."""
    cfg = C.VIT_TINY_GATED
    w = W.synth_encoder_weights(cfg, ENC_SEED)
    m = hf_gated(cfg, w)
    res = {"enc_seed": ENC_SEED}      # the weights are 2.1 MB as float32: the seed stands for them, as in the larger fixtures
    for tag, (H, W_), seed in (("a", (64, 64), 61), ("b", (48, 80), 62)):
        frames = synth.cage_frames(seed, 2, H, W_)
        acts, hooks = [], []
        for layer in m.model.layer if hasattr(m, "model") else m.layer:
            hooks.append(layer.mlp.down_proj.register_forward_pre_hook(lambda mod, args: acts.append(args[0].detach().numpy().copy())))
        with torch.no_grad():
            o = m(_pixels(frames), output_hidden_states=True)
        for h in hooks:
            h.remove()
        res.update({f"{tag}_height": H, f"{tag}_width": W_, f"{tag}_seed": seed, f"{tag}_frames_sha": sha(frames),
                    f"{tag}_cls": o.last_hidden_state[:, 0].numpy()})
        for i in range(cfg.num_hidden_layers):
            res[f"{tag}_act{i}"] = acts[i]
            res[f"{tag}_layer{i}"] = o.hidden_states[i + 1].numpy()
    np.savez_compressed(os.path.join(out, "gated_tiny.npz"), **res)
    print("gated_tiny", {k: v.shape for k, v in res.items() if isinstance(v, np.ndarray) and v.ndim > 1})


def _cls_only(out, name, cfg, n, H, W_, seed):
    m = hf_gated(cfg, W.synth_encoder_weights(cfg, ENC_SEED))
    frames = synth.cage_frames(seed, n, H, W_)
    with torch.no_grad():
        cls = m(_pixels(frames)).last_hidden_state[:, 0].numpy()
    np.savez_compressed(os.path.join(out, name), cls=cls.astype(np.float32), n=n, height=H, width=W_, frame_seed=seed,
                        enc_seed=ENC_SEED, frames_sha=sha(frames))
    print(name, cls.shape, float(np.abs(cls).max()))


def g_splus(out):
    _cls_only(out, "gated_vits16plus.npz", C.VIT_S16PLUS, 2, 224, 224, 63)


def g_w1280(out):
    _cls_only(out, "gated_w1280.npz", W1280, 2, 32, 32, 64)


ALL = {"tiny": g_tiny, "splus": g_splus, "w1280": g_w1280}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for k, fn in ALL.items():
        if a.only and k not in a.only.split(","):
            continue
        fn(a.out)
