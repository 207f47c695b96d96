#!/usr/bin/env python3
"""What a CLS attention map costs beside the forward it rides on.

ViT-B/16 at 224 x 224, batch 64, frames resident on the device, precisions 0 and 4.  Per precision, in one process and one
library, each a pass of PASSES calls timed with HIP events on the caller's stream, the median of REPEATS passes after a warm-up:
  * ``encode_u8``                          - the comparison point
  * ``cls_attention``                      - map only
  * ``cls_attention(per_head=True)``       - map and the (n, NH, T) rows
and the map kernel's own time from the library's per-kernel events (category "other" of ``profile_read``), per call.
Every sample is kept; the spread of the encode_u8 samples is the noise the two differences have to be read against.

    python scripts/attention_map_rate.py [--out profiles/attention_maps.json]
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbas_amd import config as C, synth, weights as W  # noqa: E402
from cbas_amd.encoder import DinoEncoder  # noqa: E402

BATCH, HW, PASSES, REPEATS = 64, 224, 10, 5


def pass_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(PASSES):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / PASSES


def median_of(fn):
    pass_ms(fn)                                                # warm-up
    samples = [pass_ms(fn) for _ in range(REPEATS)]
    return {"median_ms": statistics.median(samples), "samples_ms": samples}


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    cfg = C.VIT_B16
    weights = W.synth_encoder_weights(cfg, 1234)
    frames = torch.from_numpy(synth.cage_frames(3, BATCH, HW, HW)).cuda()
    res = {"model": "vitb16", "batch": BATCH, "frame": [HW, HW], "passes_per_sample": PASSES, "repeats": REPEATS,
           "device": torch.cuda.get_device_name(0), "precisions": {}}
    for precision in (0, 4):
        enc = DinoEncoder.from_weights(cfg, weights, "cuda", max_batch=BATCH, max_frame=(HW, HW), precision=precision)
        try:
            r = {"encode_u8": median_of(lambda: enc.encode_u8(frames)),
                 "cls_attention_map": median_of(lambda: enc.cls_attention(frames)),
                 "cls_attention_per_head": median_of(lambda: enc.cls_attention(frames, per_head=True))}
            r["encode_u8_again"] = median_of(lambda: enc.encode_u8(frames))       # the same measurement at the end: drift
            base = r["encode_u8"]["median_ms"]
            for k in ("cls_attention_map", "cls_attention_per_head", "encode_u8_again"):
                r[k]["ratio_to_encode_u8"] = r[k]["median_ms"] / base
            for name, per_head in (("kernel_map_only", False), ("kernel_per_head", True)):
                enc.profile(True)
                for _ in range(PASSES):
                    enc.cls_attention(frames, per_head=per_head)
                prof = enc.profile_read(reset=True)
                enc.profile(False)
                r[name] = {"ms_per_call": prof["other"]["ms"] / prof["other"]["launches"], "launches": prof["other"]["launches"],
                           "forward_ms_per_call_with_events": sum(v["ms"] for v in prof.values()) / PASSES}
            res["precisions"][str(precision)] = r
            print(f"precision {precision}: encode_u8 {base:.3f} ms, +map {r['cls_attention_map']['median_ms']:.3f} ms "
                  f"(x{r['cls_attention_map']['ratio_to_encode_u8']:.4f}), +map+heads {r['cls_attention_per_head']['median_ms']:.3f} ms "
                  f"(x{r['cls_attention_per_head']['ratio_to_encode_u8']:.4f}), encode_u8 again x{r['encode_u8_again']['ratio_to_encode_u8']:.4f}; "
                  f"kernel {r['kernel_map_only']['ms_per_call'] * 1e3:.1f} us / {r['kernel_per_head']['ms_per_call'] * 1e3:.1f} us")
        finally:
            enc.close()
    text = json.dumps(res, indent=1)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
