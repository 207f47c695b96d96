"""Gated-MLP DINOv3 frame rates and the cost of the fused gate | up epilogue, on one MI355X; one JSON document
(profiles/gated_mlp.json).

* Frame rates: vits16plus and vith16plus at 224^2, batch 64, precisions 0 and 4, device frames -> device rows through
  encode_u8 (the rate of the encoder's launch sequence alone); vits16 and vitl16 from the same run, for scale.  Each figure is
  the median of --repeats timed blocks of --steps batches after --warmup batches, with the spread (min, max) beside it.
* The epilogue: one ViT-S+ up-projection launch (M = 64 x 201, K = 384, N = 3072) with EPI_SWIGLU (1536 columns stored) and
  the same shape with EPI_GELU (3072 columns stored), through cbas_debug_gemm_bench, interleaved A B A B so that clock drift
  falls on both alike; median and spread of --repeats blocks of --iters launches.

    python scripts/gated_rate.py [--steps 10] [--warmup 3] [--repeats 5] [--iters 200] [--models ...] [--out FILE]
"""
import argparse
import ctypes as C
import faulthandler
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbas_amd import _lib, config as cfgs, weights as W, synth  # noqa: E402
from cbas_amd.encoder import DinoEncoder  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def frame_rate(name, precision, a):
    cfg = cfgs.NAMED_VIT[name]
    enc = DinoEncoder.from_weights(cfg, W.synth_encoder_weights(cfg, 1234), "cuda", max_batch=a.batch, max_frame=(a.size, a.size),
                                   precision=precision)
    try:
        frames = torch.from_numpy(synth.cage_frames(32, a.batch, a.size, a.size)).cuda()
        for _ in range(a.warmup):
            enc.encode_u8(frames, want_f32=False)
        torch.cuda.synchronize()
        fps = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                enc.encode_u8(frames, want_f32=False)
            torch.cuda.synchronize()
            fps.append(a.steps * a.batch / (time.perf_counter() - t0))
        try:
            enc.check_finite()
            finite = True
        except RuntimeError:                                         # synthetic weights may leave a mode's range: the rate still stands
            finite = False
        gflop = cfg.flops_per_frame(a.size, a.size) / 1e9
        s = spread(fps)
        return {"frames_per_s": {k: (round(v, 1) if k != "n" else v) for k, v in s.items()}, "gflop_per_frame": round(gflop, 3),
                "tflops": round(s["median"] * gflop / 1e3, 1), "rows_finite": finite}
    finally:
        enc.close()


def epilogue_cost(a):
    _lib.require_debug("cbas_debug_gemm_bench")
    lib = _lib.load()
    M, K, N = 64 * 201, 384, 3072

    def ms(code):
        t, cs = C.c_float(), C.c_ulonglong()
        rc = lib.cbas_debug_gemm_bench(M, N, K, code, a.iters, C.byref(t), C.byref(cs))
        if rc:
            raise RuntimeError(lib.cbas_last_error().decode())
        return t.value * 1e3                                         # microseconds per launch
    ms(0), ms(3000)                                                  # warm both code objects and the clocks
    gelu, swiglu = [], []
    for _ in range(a.repeats):
        gelu.append(ms(0))
        swiglu.append(ms(3000))
    g, s = spread(gelu), spread(swiglu)
    return {"shape": {"M": M, "K": K, "N": N}, "iters_per_block": a.iters, "gelu_us": g, "swiglu_us": s,
            "swiglu_over_gelu": round(s["median"] / g["median"], 4),
            "gelu_spread_frac": round((g["max"] - g["min"]) / g["median"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--models", default="vits16plus,vith16plus,vits16,vitl16")
    ap.add_argument("--precisions", default="0,4")
    ap.add_argument("--timeout", type=float, default=500.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    faulthandler.dump_traceback_later(a.timeout, exit=True)         # watchdog: a hung step ends the process
    res = {"device": torch.cuda.get_device_name(0), "size": a.size, "batch": a.batch, "steps": a.steps, "warmup": a.warmup,
           "path": "encode_u8: device frames -> device fp16 rows", "models": {}}
    res["up_projection_epilogue"] = epilogue_cost(a)
    for name in a.models.split(","):
        res["models"][name] = {f"p{p}": frame_rate(name, int(p), a) for p in a.precisions.split(",")}
    faulthandler.cancel_dump_traceback_later()
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
