"""Generate the DINOv3 ConvNeXt golden vectors under tests/golden/ by running the REFERENCE's arithmetic: transformers'
DINOv3ConvNextModel in fp32 on the CPU (what the reference's DinoEncoder runs through AutoModel, backend/cbas.py:650-677).

    python tests/golden/make_goldens_convnext.py [--only tiny,t,e2e,config] [--out DIR]

Weights and frames come from the counter-based generators (cbas_amd.weights / cbas_amd.synth), so the fixtures hold outputs
only.  Needs transformers (and, for e2e, the reference checkout); the tests that read the fixtures need neither.
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

from cbas_amd import config as C  # noqa: E402
from cbas_amd import weights as W  # noqa: E402
from cbas_amd import synth  # noqa: E402


def hf_convnext(cfg: C.ConvNextConfig, weights):
    from transformers import DINOv3ConvNextConfig, DINOv3ConvNextModel
    hcfg = DINOv3ConvNextConfig(hidden_sizes=list(cfg.hidden_sizes), depths=list(cfg.depths), layer_norm_eps=cfg.layer_norm_eps,
                                image_size=cfg.image_size)
    m = DINOv3ConvNextModel(hcfg).eval()
    sd = {k: torch.from_numpy(v.copy()) for k, v in weights.items()}
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return m


def _green(frames):
    return torch.from_numpy(frames[:, :, :, 1] / 255.0).float()           # cbas.py:431


def g_tiny(out):
    """Tiny ConvNeXt with the stem output and every stage's output - kernel-by-kernel bring-up."""
    cfg = C.CONVNEXT_TINY
    m = hf_convnext(cfg, W.synth_convnext_weights(cfg, ENC_SEED))
    res = {"n": 3}
    for tag, (H, W_) in (("a", (64, 64)), ("b", (72, 88))):
        frames = synth.cage_frames(21, 3, H, W_)
        px = _green(frames).unsqueeze(1).repeat(1, 3, 1, 1)
        with torch.no_grad():
            stem = m.model.stages[0].downsample_layers[1](m.model.stages[0].downsample_layers[0](px))
            o = m(px, output_hidden_states=True)
        cl = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()     # noqa: E731  channels-last rows (f, y, x)
        res.update({f"{tag}_height": H, f"{tag}_width": W_, f"{tag}_frames_sha": sha(frames), f"{tag}_stem": cl(stem),
                    f"{tag}_row0": o.last_hidden_state[:, 0].numpy()})
        for i, hs in enumerate(o.hidden_states[-4:]):
            res[f"{tag}_stage{i}"] = cl(hs)
    np.savez_compressed(os.path.join(out, "convnext_tiny.npz"), frame_seed=21, **res)
    print("convnext_tiny", {k: v.shape for k, v in res.items() if isinstance(v, np.ndarray) and v.ndim > 1})


def g_t(out):
    """ConvNeXt-T row 0: 4 frames at 224^2, 4 at 256^2, 2 at 250 x 250 (odd grids at stage 3)."""
    cfg = C.CONVNEXT_T
    m = hf_convnext(cfg, W.synth_convnext_weights(cfg, ENC_SEED))
    res = {}
    for tag, n, S, seed in (("r224", 4, 224, 31), ("r256", 4, 256, 32), ("r250", 2, 250, 33)):
        frames = synth.cage_frames(seed, n, S, S)
        with torch.no_grad():
            row0 = m(_green(frames).unsqueeze(1).repeat(1, 3, 1, 1)).last_hidden_state[:, 0].numpy()
        res.update({f"{tag}_cls": row0, f"{tag}_n": n, f"{tag}_size": S, f"{tag}_seed": seed, f"{tag}_frames_sha": sha(frames)})
    np.savez_compressed(os.path.join(out, "convnext_t.npz"), **res)
    print("convnext_t", {k: v.shape for k, v in res.items() if isinstance(v, np.ndarray) and v.ndim > 1})


def g_e2e(out):
    """ConvNeXt-T end to end through the reference's OWN DinoEncoder (loaded from a save_pretrained directory): 512 frames at
    256^2 in 8-frame calls -> f16 -> the reference's infer_file with the C = 9 head."""
    cbas, classifier_head = import_reference()
    cfg = C.CONVNEXT_T
    w = W.synth_convnext_weights(cfg, ENC_SEED)
    n, S, seed = 512, 256, 5
    frames = synth.cage_frames(seed, n, S, S)
    os.replace = MG._real_replace
    with tempfile.TemporaryDirectory() as td:
        hf_convnext(cfg, w).save_pretrained(td)
        enc = cbas.DinoEncoder(td, device="cpu")
        g = _green(frames)
        with torch.no_grad():
            cls = torch.cat([enc(g[i:i + 8].unsqueeze(1)).squeeze(1) for i in range(0, n, 8)]).numpy()     # cbas.py:435-436
        hcfg = C.HeadConfig(in_features=768)
        hm = ref_head(classifier_head, hcfg, W.synth_head_weights(hcfg, HEAD_SEED))
        p = os.path.join(td, "e2e_cls.h5")
        with MG._FakeH5File(p, "w") as f:
            d = f.create_dataset("cls", shape=(n, 768), dtype="f2")
            d[:] = cls
            cls16 = d[:].copy()
        o = cbas.infer_file(p, hm, "gold", BEHAVIORS, 31, device=torch.device("cpu"), temperature=1.0)
        import pandas as pd
        probs = pd.read_csv(o).to_numpy(dtype=np.float64).astype(np.float32)
    np.savez_compressed(os.path.join(out, "e2e_convnext_t.npz"), cls_every8=cls[::8].astype(np.float32), cls_f16=cls16,
                        probs=probs, labels=probs.argmax(1), frames_sha=sha(frames), frame_seed=seed, n=n, height=S, width=S)
    top2 = np.sort(probs, axis=1)[:, -2:]
    print("e2e convnext_t labels", np.bincount(probs.argmax(1), minlength=9), "smallest top-2 margins",
          np.sort(top2[:, 1] - top2[:, 0])[:6])


def g_config(out):
    """The HF config.json of ConvNeXt-T (settings only) and the state-dict key list, for the CPU tests."""
    from transformers import DINOv3ConvNextConfig, DINOv3ConvNextModel
    hc = DINOv3ConvNextConfig()
    with open(os.path.join(out, "convnext_t_config.json"), "w") as f:
        f.write(hc.to_json_string())
    sd = DINOv3ConvNextModel(hc).state_dict()
    with open(os.path.join(out, "convnext_t_keys.txt"), "w") as f:
        for k, v in sd.items():
            f.write(f"{k} {','.join(str(s) for s in v.shape)}\n")


ALL = {"config": g_config, "tiny": g_tiny, "t": g_t, "e2e": g_e2e}

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
