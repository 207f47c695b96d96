"""DINOv3 ConvNeXt-T frame rate, pinned host -> host (cbas_enc_submit_u8_host / cbas_enc_wait over the three slots), 256^2,
batch 64, precisions 3 and 4; one JSON line: frames/s, GFLOP/frame, achieved TFLOP/s against the fp32 MFMA peak (p3) and the
fp16 peak (p4, algorithmic FLOPs), and the row-0 gate against tests/golden/convnext_t.npz.

    python scripts/convnext_rate.py [--steps 20] [--warmup 3] [--batch 64] [--size 256] [--timeout 600]
"""
import argparse
import faulthandler
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbas_amd import config as C, weights as W, synth  # noqa: E402
from cbas_amd.encoder import DinoEncoder  # noqa: E402

PEAK_TF = {3: 157.3, 4: 2516.6}          # MI355X dense fp32 MFMA / fp16 MFMA peak, TFLOP/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--timeout", type=float, default=600.0)
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.timeout, exit=True)         # watchdog: a hung step ends the process
    cfg = C.CONVNEXT_T
    w = W.synth_convnext_weights(cfg, 1234)
    gold = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "convnext_t.npz"))
    S, B = a.size, a.batch
    frames = torch.from_numpy(synth.cage_frames(32, B, S, S)[:, :, :, 1].copy()).pin_memory().numpy()
    gflop = cfg.flops_per_frame(S, S) / 1e9
    res = {"model": "dinov3_convnext_t", "size": S, "batch": B, "steps": a.steps, "gflop_per_frame": round(gflop, 3)}
    for prec in (3, 4):
        enc = DinoEncoder.from_weights(cfg, w, "cuda", max_batch=B, max_frame=(S, S), precision=prec)
        try:
            gf = synth.cage_frames(int(gold["r256_seed"]), int(gold["r256_n"]), 256, 256)
            _, c32 = enc.encode_u8(torch.from_numpy(gf).cuda())
            torch.cuda.synchronize()
            d, r = c32.cpu().numpy().astype(np.float64), gold["r256_cls"].astype(np.float64)
            rel = float((np.linalg.norm(d - r, axis=1) / np.linalg.norm(r, axis=1)).max())

            def run(k):
                for i in range(k):
                    s = i % 3
                    if i >= 3:
                        enc.wait(s)
                    enc.submit_host(s, frames)
                for i in range(max(0, k - 3), k):
                    enc.wait(i % 3)
            run(a.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(a.steps)
            dt = time.perf_counter() - t0
            fps = a.steps * B / dt
            res[f"p{prec}"] = {"frames_per_s": round(fps, 1), "ms_per_batch": round(dt / a.steps * 1e3, 3),
                               "tflops": round(fps * gflop / 1e3, 2), "frac_of_peak": round(fps * gflop / 1e3 / PEAK_TF[prec], 4),
                               "cls_rel_max_vs_ref": rel, "cls_gate_5e-6": rel < 5e-6}
        finally:
            enc.close()
    faulthandler.cancel_dump_traceback_later()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
