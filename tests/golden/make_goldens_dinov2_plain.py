"""Generate the plain-DINOv2 golden vectors (model_type "dinov2": no register tokens, position embedding resampled WITHOUT
antialiasing) under tests/golden/ by running the REFERENCE's arithmetic: transformers' Dinov2Model in fp32 with eager attention
on the CPU, and the reference's own DinoEncoder wrapper + infer_file (backend/cbas.py:650-677).

    python tests/golden/make_goldens_dinov2_plain.py [--only tiny,b14,tables,e2e] [--out DIR] [--reference DIR]

Weights, frames and the table fixture's input grid come from the counter-based generators (cbas_amd.weights / cbas_amd.synth),
so the fixtures hold recorded outputs only.  Needs transformers (and, for b14 / e2e, the reference checkout); the tests that
read the fixtures need neither.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_goldens as MG  # noqa: E402  (sets up sys.path, torch, the h5 / decord fakes)
from make_goldens import ENC_SEED, HEAD_SEED, BEHAVIORS, sha, import_reference, ref_head  # noqa: E402

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from cbas_amd import config as C  # noqa: E402
from cbas_amd import weights as W  # noqa: E402
from cbas_amd import synth  # noqa: E402

TABLE_SEED, TABLE_GRID, TABLE_DIM = 77, 37, 16
TABLE_SIZES = ((16, 16), (18, 18), (18, 20), (40, 40))
MIN_MARGIN = 1e-3         # the e2e clip's smallest reference top-2 margin must be at least this (else: next frame seed)


def hf_dinov2_plain(cfg: C.ViTConfig, weights):
    from transformers import Dinov2Config, Dinov2Model
    hcfg = Dinov2Config(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, mlp_ratio=cfg.intermediate_size // cfg.hidden_size,
                        image_size=cfg.image_size, patch_size=cfg.patch_size, layer_norm_eps=cfg.layer_norm_eps, qkv_bias=True)
    hcfg._attn_implementation = "eager"
    m = Dinov2Model(hcfg).eval()
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in weights.items()}, strict=True)
    return m


def _green(frames):
    return torch.from_numpy(frames[:, :, :, 1] / 255.0).float()           # cbas.py:431


def g_tiny(out):
    """Tiny plain DINOv2 (5 x 5 stored grid, patch 14): 2 frames at 56 x 84 (4 x 6 patches: both axes resampled, by different
    matrices) and 2 at the native 70 x 70 (the skip branch).  Taps: the position table interpolate_pos_encoding returns (cls row
    included), the embeddings, each layer's output and last_hidden_state."""
    cfg = C.DINOV2_TINY
    m = hf_dinov2_plain(cfg, W.synth_encoder_weights(cfg, ENC_SEED))
    res = {}
    for tag, (H, W_), seed in (("r", (56, 84), 41), ("n", (70, 70), 42)):
        frames = synth.cage_frames(seed, 2, H, W_)
        px = _green(frames).unsqueeze(1).repeat(1, 3, 1, 1)
        with torch.no_grad():
            o = m(px, output_hidden_states=True)
            dummy = torch.zeros(1, 1 + (H // cfg.patch_size) * (W_ // cfg.patch_size), cfg.hidden_size)
            pos = m.embeddings.interpolate_pos_encoding(dummy, H, W_)[0]
        res.update({f"{tag}_height": H, f"{tag}_width": W_, f"{tag}_seed": seed, f"{tag}_frames_sha": sha(frames),
                    f"{tag}_pos": pos.numpy(), f"{tag}_emb": o.hidden_states[0].numpy(), f"{tag}_layer0": o.hidden_states[1].numpy(),
                    f"{tag}_layer1": o.hidden_states[2].numpy(), f"{tag}_last": o.last_hidden_state.numpy()})
    np.savez_compressed(os.path.join(out, "dinov2_tiny.npz"), **res)
    print("dinov2_tiny", {k: v.shape for k, v in res.items() if isinstance(v, np.ndarray) and v.ndim > 1})


def g_b14(out):
    """ViT-B/14 ("facebook/dinov2-base" shape) row 0: 4 frames at 224^2 (16 x 16: downsample), 2 at CBAS's standard 256^2
    (18 x 18) through the reference's own DinoEncoder wrapper, 2 at 252 x 280 (18 x 20: a different matrix per axis), 2 at 518^2
    (37 x 37: the stored table)."""
    cfg = C.DINOV2_B14
    m = hf_dinov2_plain(cfg, W.synth_encoder_weights(cfg, ENC_SEED))
    cbas, _ = import_reference()
    res = {}
    with tempfile.TemporaryDirectory() as td:
        m.save_pretrained(td)
        enc = cbas.DinoEncoder(td, device="cpu")               # reference wrapper, AutoModel -> Dinov2Model
        assert type(enc.model).__name__ == "Dinov2Model", type(enc.model)
        for tag, n, (H, W_), seed, wrapper in (("r224", 4, (224, 224), 51, False), ("r256", 2, (256, 256), 52, True),
                                               ("r252x280", 2, (252, 280), 53, False), ("r518", 2, (518, 518), 54, False)):
            frames = synth.cage_frames(seed, n, H, W_)
            g = _green(frames)
            with torch.no_grad():
                if wrapper:
                    row0 = enc(g.unsqueeze(1)).squeeze(1).numpy()
                else:
                    row0 = torch.cat([m(g[i:i + 2].unsqueeze(1).repeat(1, 3, 1, 1)).last_hidden_state[:, 0]
                                      for i in range(0, n, 2)]).numpy()
            res.update({f"{tag}_cls": row0, f"{tag}_n": n, f"{tag}_height": H, f"{tag}_width": W_, f"{tag}_seed": seed,
                        f"{tag}_frames_sha": sha(frames)})
    np.savez_compressed(os.path.join(out, "dinov2_b14.npz"), **res)
    print("dinov2_b14", {k: v.shape for k, v in res.items() if isinstance(v, np.ndarray) and v.ndim > 1})


def table_grid() -> np.ndarray:
    """The table fixture's input: a seeded (37 * 37, 16) grid (the tests regenerate it)."""
    return W.synth_normal(TABLE_SEED, "pos_table_grid", (TABLE_GRID * TABLE_GRID, TABLE_DIM), 0.3)


def g_tables(out):
    """F.interpolate(size=, mode="bicubic", align_corners=False) - exactly HF modeling_dinov2.py:86-91 - of a seeded 37 x 37 x 16
    grid to 16^2, 18^2, 18 x 20 and 40^2 (an upsample): checks the table builder on the CPU."""
    src = torch.from_numpy(table_grid()).reshape(1, TABLE_GRID, TABLE_GRID, TABLE_DIM).permute(0, 3, 1, 2)
    res = {"grid_sha": sha(table_grid()), "seed": TABLE_SEED, "grid": TABLE_GRID, "dim": TABLE_DIM}
    for nh, nw in TABLE_SIZES:
        t = F.interpolate(src.to(torch.float32), size=(nh, nw), mode="bicubic", align_corners=False)
        res[f"t{nh}x{nw}"] = t.permute(0, 2, 3, 1).reshape(nh * nw, TABLE_DIM).numpy()
    np.savez_compressed(os.path.join(out, "dinov2_pos_tables.npz"), **res)
    print("dinov2_pos_tables", {k: v.shape for k, v in res.items() if isinstance(v, np.ndarray) and v.ndim > 1})


def g_e2e(out, n=256, first_seed=8):
    """Plain DINOv2 ViT-B/14 end to end through the reference's OWN DinoEncoder (loaded from a save_pretrained directory): n frames
    at 256^2 (18 x 18 patches, T = 325) in 8-frame calls -> f16 -> the reference's infer_file with the C = 9 head.  The label
    test on the fixture is only meaningful when the reference itself is not near a tie: the frame seed is advanced until the
    clip's smallest top-2 probability margin is >= MIN_MARGIN, and that margin is stored."""
    cbas, classifier_head = import_reference()
    cfg = C.DINOV2_B14
    w = W.synth_encoder_weights(cfg, ENC_SEED)
    os.replace = MG._real_replace
    with tempfile.TemporaryDirectory() as td:
        hf_dinov2_plain(cfg, w).save_pretrained(td)
        enc = cbas.DinoEncoder(td, device="cpu")
        hcfg = C.HeadConfig(in_features=768)
        hm = ref_head(classifier_head, hcfg, W.synth_head_weights(hcfg, HEAD_SEED))
        for seed in range(first_seed, first_seed + 6):
            frames = synth.cage_frames(seed, n, 256, 256)
            g = _green(frames)
            with torch.no_grad():
                cls = torch.cat([enc(g[i:i + 8].unsqueeze(1)).squeeze(1) for i in range(0, n, 8)]).numpy()     # cbas.py:435-436
            p = os.path.join(td, f"e2e{seed}_cls.h5")
            with MG._FakeH5File(p, "w") as f:
                d = f.create_dataset("cls", shape=(n, 768), dtype="f2")
                d[:] = cls
                cls16 = d[:].copy()
            o = cbas.infer_file(p, hm, "gold", BEHAVIORS, 31, device=torch.device("cpu"), temperature=1.0)
            import pandas as pd
            probs = pd.read_csv(o).to_numpy(dtype=np.float64).astype(np.float32)
            top2 = np.sort(probs.astype(np.float64), axis=1)[:, -2:]
            margin = float((top2[:, 1] - top2[:, 0]).min())
            labels = probs.argmax(1)
            print(f"e2e dinov2_b14 seed {seed}: labels {np.bincount(labels, minlength=9)}, transitions "
                  f"{int((labels[1:] != labels[:-1]).sum())}, smallest top-2 margins {np.sort(top2[:, 1] - top2[:, 0])[:6]}")
            if margin >= MIN_MARGIN and len(set(labels.tolist())) >= 2:
                break
        else:
            raise SystemExit("no frame seed gave a clip whose smallest reference margin is >= MIN_MARGIN")
    np.savez_compressed(os.path.join(out, "e2e_dinov2_b14.npz"), cls_every8=cls[::8].astype(np.float32), cls_f16=cls16,
                        probs=probs, labels=labels, frames_sha=sha(frames), frame_seed=seed, n=n, hw=256, min_margin=margin)


ALL = {"tables": g_tables, "tiny": g_tiny, "b14": g_b14, "e2e": g_e2e}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--reference", default=None, help="the reference checkout (default: make_goldens.REF)")
    a = ap.parse_args()
    if a.reference:
        MG.REF = a.reference
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for k, fn in ALL.items():
        if a.only and k not in a.only.split(","):
            continue
        fn(a.out)
