"""What the per-layer outputs cost: hidden_states (raw and normed), cls_attention(layer="all") and attention_rollout beside the
calls they extend, ViT-B/16 at 256 x 256, batch 64, precisions 0 and 4.  Medians of five timings with HIP events on the caller's
stream, after two warm-up calls, all on one handle per precision so that the baselines share its clocks.

    python scripts/encoder_layers_rate.py [--out profiles/encoder_layers.json] [--batch 64] [--size 256]

The two rollout kernels are timed through the library's own per-category events (cbas_enc_profile: category "other" holds the
per-layer copies, the CLS map kernel and both rollout kernels; the row gather is not bracketed).  A rollout with start_layer = L
launches kernel 1 once and kernel 2 never, so its "other" time is one layer of kernel 1; the full rollout launches kernel 1 L
times and kernel 2 L - 1 times, so kernel 2 per layer = (other_full - L x kernel 1) / (L - 1).  Each is a median of five.  FLOP/s
of each is given against the fp32 vector pipe's peak taken as CUs x 4 SIMDs x 16 lanes x 2 (fma) x 2 (dual issue) x 2.4 GHz - the
data sheet's 157.3 TFLOP/s at 256 CUs; the clock is assumed, not read.  The extra bytes the raw copies write are reported with the
time difference of two END-TO-END medians (hidden_states - hidden_state); a bandwidth is derived only where that difference
exceeds the spread of the baseline's own samples.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cbas_amd import config as C, synth, weights as W  # noqa: E402
from cbas_amd.encoder import DinoEncoder  # noqa: E402


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "encoder_layers.json"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    cfg = C.VIT_B16
    n, S = a.batch, a.size
    T, D, L, NH = cfg.num_tokens(S, S), cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads
    weights = W.synth_encoder_weights(cfg, 1234)
    frames = torch.from_numpy(synth.cage_frames(5, n, S, S)).cuda()
    res = {"model": "vit_b16 (synthetic weights)", "batch": n, "size": S, "tokens": T, "reps": 5, "precisions": {}}
    for precision in (0, 4):
        enc = DinoEncoder.from_weights(cfg, weights, "cuda", max_batch=n, max_frame=(S, S), precision=precision)
        try:
            r = {}
            for name, fn in (("hidden_state", lambda: enc.hidden_state(frames)),
                             ("hidden_states_raw_all", lambda: enc.hidden_states(frames)),
                             ("hidden_states_normed_all", lambda: enc.hidden_states(frames, norm=True)),
                             ("cls_attention", lambda: enc.cls_attention(frames)),
                             ("cls_attention_all", lambda: enc.cls_attention(frames, layer="all")),
                             ("attention_rollout", lambda: enc.attention_rollout(frames))):
                med, all_ms = timed(fn)
                r[name] = {"median_ms": med, "ms": all_ms}
            copied = (L + 1) * n * T * D * 4
            base = r["hidden_state"]["ms"]
            extra_ms, spread_ms = r["hidden_states_raw_all"]["median_ms"] - r["hidden_state"]["median_ms"], max(base) - min(base)
            r["hidden_states_raw_all"].update({
                "bytes_written": copied, "extra_ms_difference_of_end_to_end_medians": extra_ms, "baseline_spread_ms": spread_ms,
                "copy_GBps_read_plus_write_from_that_difference": 2 * copied / (extra_ms * 1e-3) / 1e9 if extra_ms > spread_ms else None})

            def other_ms(start):
                ms, launches = [], 0
                for _ in range(5):
                    enc.profile(True)
                    enc.attention_rollout(frames, start_layer=start)
                    torch.cuda.synchronize()
                    o = enc.profile_read().get("other", {})
                    enc.profile(False)
                    ms.append(float(o.get("ms") or 0.0))
                    launches = int(o.get("launches") or 0)
                return statistics.median(ms), ms, launches

            enc.attention_rollout(frames)
            k1_ms, k1_all, k1_n = other_ms(L)
            full_ms, full_all, full_n = other_ms(1)
            k2_ms = (full_ms - L * k1_ms) / (L - 1)
            k1_flop, k2_flop = 2.0 * n * T * T * D, 2.0 * n * T * T * T      # per layer; kernel 1: the scores only, no softmax
            from cbas_amd import _lib
            peak = _lib.device_info(0)[1] * 4 * 16 * 2 * 2 * 2.4e9
            r["rollout_kernels"] = {"kernel1_ms_per_layer": k1_ms, "kernel1_samples_ms": k1_all, "kernel1_launches": k1_n,
                                    "both_ms_per_call": full_ms, "both_samples_ms": full_all, "both_launches": full_n,
                                    "kernel2_ms_per_layer_derived": k2_ms, "kernel1_flop_per_layer": k1_flop, "kernel2_flop_per_layer": k2_flop,
                                    "kernel1_TFLOPs": k1_flop / (k1_ms * 1e-3) / 1e12, "kernel2_TFLOPs": k2_flop / (k2_ms * 1e-3) / 1e12,
                                    "fp32_vector_peak_TFLOPs_assumed_2.4GHz": peak / 1e12}
            res["precisions"][str(precision)] = r
            print(precision, json.dumps({k: v.get("median_ms", v) if isinstance(v, dict) else v for k, v in r.items()}, default=str))
        finally:
            enc.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
