"""What each fp8 plan of precision 2 costs and buys (DESIGN.md "fp8 plans"; written to profiles/fp8_plans.json).

For precision 0, precision 2 (plan "all") and every other named plan, on ViT-B/16 with the synthetic weights of the tests:

  * frames/s at batch 128, 224 x 224, device-resident uint8 frames (scripts/quick_perf.py's loop), the modes ALTERNATING inside
    one process - round r times every mode once, the figure is the median over the rounds;
  * CLS relative error against the fp32 goldens (tests/golden/vitb16_224_noise.npz, vitb16_256.npz; the tests' 3 frames);
  * on the long end-to-end clip (tests/golden/e2e_vitb16_long.npz, 2 048 frames, the fixture's head): labels that differ from
    the fp16 mode's and from the reference's, and how many of those sit at a reference top-2 margin under 1e-2 (near ties);
  * optionally (--study) the label study of scripts/fp8_label_study.py through heads trained on the device.

    python scripts/fp8_plan_table.py [--rounds 7] [--iters 10] [--study] [--json profiles/fp8_plans.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cbas_amd import config as C, weights as W, synth  # noqa: E402
from cbas_amd.encoder import DinoEncoder  # noqa: E402
from cbas_amd.head import ClassifierLSTMDeltas  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def modes():
    out = [("precision 0", {"precision": 0})]
    out += [(f"plan {n}", {"precision": 2, "fp8_plan": n}) for n in C.FP8_PLANS]
    return out


def throughput(cfg, w, batch, hw, rounds, iters):
    encs = [(name, DinoEncoder.from_weights(cfg, w, "cuda", max_batch=batch, max_frame=(hw, hw), **kw)) for name, kw in modes()]
    fr = torch.from_numpy(synth.noise_frames(0, batch, hw, hw)[:, :, :, 1].copy()).cuda()
    fps = {name: [] for name, _ in encs}
    for name, enc in encs:
        for _ in range(3):
            enc.encode_u8(fr, want_f32=False)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, enc in encs:
            t0 = time.perf_counter()
            for _ in range(iters):
                enc.encode_u8(fr, want_f32=False)
            torch.cuda.synchronize()
            fps[name].append(batch * iters / (time.perf_counter() - t0))
    for _, enc in encs:
        enc.close()
    return {name: {"frames_per_s_median": float(np.median(v)), "frames_per_s_min": float(min(v)), "frames_per_s_max": float(max(v))}
            for name, v in fps.items()}


def cls_errors(cfg, w):
    out = {}
    for gold, hw in (("vitb16_224_noise", 224), ("vitb16_256", 256)):
        g = np.load(os.path.join(GOLD, gold + ".npz"))
        mk = synth.noise_frames if str(g["kind"]) == "noise" else synth.cage_frames
        fd = torch.from_numpy(mk(int(g["frame_seed"]), int(g["n"]), hw, hw)[:3]).cuda()
        ref = g["cls"][:3].astype(np.float64)
        for name, kw in modes():
            enc = DinoEncoder.from_weights(cfg, w, "cuda", max_batch=8, max_frame=(hw, hw), **kw)
            got = enc.encode_u8(fd)[1].cpu().numpy().astype(np.float64)
            enc.close()
            out.setdefault(name, {})[gold] = float((np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)).max())
    return out


def long_clip(cfg, w):
    g = np.load(os.path.join(GOLD, "e2e_vitb16_long.npz"))
    n = int(g["n"])
    fr = synth.cage_frames(int(g["frame_seed"]), n, 224, 224)
    head = ClassifierLSTMDeltas(768, 9)
    head.load_state_dict(W.synth_head_weights(C.HeadConfig(in_features=768), 4321))
    head.to("cuda")
    ref = g["probs"].astype(np.float64)
    srt = np.sort(ref, axis=1)
    margin = srt[:, -1] - srt[:, -2]
    labels, out = {}, {}
    for name, kw in modes():
        enc = DinoEncoder.from_weights(cfg, w, "cuda", max_batch=128, max_frame=(224, 224), **kw)
        c16 = torch.cat([enc.encode_u8(torch.from_numpy(fr[i:i + 128]).cuda(), want_f32=False)[0] for i in range(0, n, 128)])
        enc.close()
        labels[name] = head.infer_clip(c16, 1.0).cpu().numpy().argmax(1)
    head.close()
    l16 = labels["precision 0"]
    for name, lab in labels.items():
        f16, fref = lab != l16, lab != ref.argmax(1)
        out[name] = {"frames": n, "labels_differing_from_fp16_mode": int(f16.sum()), "agreement_with_fp16_mode": float(1.0 - f16.mean()),
                     "labels_differing_from_reference": int(fref.sum()), "flip_rate_vs_reference": float(fref.mean()),
                     "flips_at_reference_margin_under_1e-2": int((fref & (margin < 1e-2)).sum()),
                     "flips_at_reference_margin_over_1e-2": int((fref & (margin >= 1e-2)).sum())}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--study", action="store_true")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "fp8_plans.json"))
    a = ap.parse_args()
    cfg = C.NAMED_VIT["vitb16"]
    w = W.synth_encoder_weights(cfg, 1234)
    rec = {"model": "vitb16", "weights": "synthetic (seed 1234)", "batch": a.batch, "rounds": a.rounds, "iters_per_round": a.iters,
           "throughput_224": throughput(cfg, w, a.batch, 224, a.rounds, a.iters), "cls_rel_err_vs_fp32_golden": cls_errors(cfg, w),
           "e2e_vitb16_long": long_clip(cfg, w)}
    if a.study:
        import fp8_label_study as S
        rec["label_study"] = S.study("vitb16", 224, n_classes=6, epochs=30, plans=("mlp", "mlp_qkv", "up", "down", 2), verbose=True)
    p0 = rec["throughput_224"]["precision 0"]["frames_per_s_median"]
    print(f"{'mode':14s} {'frames/s':>9s} {'x fp16':>7s} {'CLS err 224':>12s} {'CLS err 256':>12s} {'flips vs ref':>13s} {'near ties':>10s} {'vs fp16 mode':>13s}")
    for name, _ in modes():
        t, e, l = rec["throughput_224"][name], rec["cls_rel_err_vs_fp32_golden"][name], rec["e2e_vitb16_long"][name]
        print(f"{name:14s} {t['frames_per_s_median']:9.0f} {t['frames_per_s_median'] / p0:7.3f} {e['vitb16_224_noise']:12.3e} "
              f"{e['vitb16_256']:12.3e} {l['labels_differing_from_reference']:13d} {l['flips_at_reference_margin_under_1e-2']:10d} "
              f"{l['labels_differing_from_fp16_mode']:13d}")
    with open(a.json, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.json)
