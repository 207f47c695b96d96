#!/usr/bin/env python3
"""What every token's final hidden state costs beside the CLS row.

ViT-B/16 at 224 x 224, batch 64, frames and rows resident on the device.  Per precision (0 and 4), in one process and one
library, three calls ALTERNATED pass by pass - a pass is PASSES calls timed with HIP events on the caller's stream - and the
median of REPEATS passes of each after a warm-up, every sample kept:
  * ``hidden_state``                             - the (n, T, D) fp32 image
  * ``encode_u8`` with the last layer unpruned   - the same forward with the CLS tail: the difference is the all-row final norm
  * ``encode_u8`` (pruned, the default)          - what unpruning costs
and, in precision 3 (plain fp32 rows in and out of every LayerNorm), the bandwidth of the two row kernels from the library's
per-kernel events (category "layernorm" of ``profile_read``), medians of REPEATS profiled passes of the same two calls alternated:
  * ``layernorm_f32`` over all M = n T rows: the 24 launches of an unpruned ``encode_u8`` (its CLS norm is not in the category)
  * ``launch_final_norm_rows``: the category's total in ``hidden_state`` minus that of ``encode_u8`` unpruned in the same repeat
Both move M D 4 bytes in and M D 4 bytes out.

    python scripts/hidden_state_rate.py [--out profiles/hidden_state.json]
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


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    cfg = C.VIT_B16
    weights = W.synth_encoder_weights(cfg, 1234)
    frames = torch.from_numpy(synth.cage_frames(3, BATCH, HW, HW)).cuda()
    T, D, L = cfg.num_tokens(HW, HW), cfg.hidden_size, cfg.num_hidden_layers
    res = {"model": "vitb16", "batch": BATCH, "frame": [HW, HW], "tokens": T, "passes_per_sample": PASSES, "repeats": REPEATS,
           "device": torch.cuda.get_device_name(0), "precisions": {}}

    def variants(enc):
        def unpruned():
            enc.set_prune_last_layer(False)
            enc.encode_u8(frames)
            enc.set_prune_last_layer(True)
        return {"hidden_state": lambda: enc.hidden_state(frames), "encode_u8_unpruned": unpruned, "encode_u8": lambda: enc.encode_u8(frames)}

    for precision in (0, 4):
        enc = DinoEncoder.from_weights(cfg, weights, "cuda", max_batch=BATCH, max_frame=(HW, HW), precision=precision)
        try:
            fns = variants(enc)
            samples = {k: [] for k in fns}
            for k, fn in fns.items():
                pass_ms(fn)                                        # warm-up
            for _ in range(REPEATS):
                for k, fn in fns.items():
                    samples[k].append(pass_ms(fn))
            r = {k: {"median_ms": statistics.median(v), "samples_ms": v} for k, v in samples.items()}
            for k in ("hidden_state", "encode_u8_unpruned"):
                r[k]["ratio_to_encode_u8"] = r[k]["median_ms"] / r["encode_u8"]["median_ms"]
            res["precisions"][str(precision)] = r
            print(f"precision {precision}: hidden_state {r['hidden_state']['median_ms']:.3f} ms, encode_u8 unpruned "
                  f"{r['encode_u8_unpruned']['median_ms']:.3f} ms, encode_u8 {r['encode_u8']['median_ms']:.3f} ms per batch of {BATCH}")
        finally:
            enc.close()

    enc = DinoEncoder.from_weights(cfg, weights, "cuda", max_batch=BATCH, max_frame=(HW, HW), precision=3)
    try:
        fns = variants(enc)

        def layernorm_ms(fn):
            enc.profile(True)
            for _ in range(PASSES):
                fn()
            prof = enc.profile_read(reset=True)
            enc.profile(False)
            return prof["layernorm"]["ms"] / PASSES, prof["layernorm"]["launches"] // PASSES

        for k in ("hidden_state", "encode_u8_unpruned"):
            layernorm_ms(fns[k])                                   # warm-up
        ln, rows = [], []
        for _ in range(REPEATS):
            all_ms, launches = layernorm_ms(fns["encode_u8_unpruned"])
            assert launches == 2 * L, launches
            tok_ms, launches = layernorm_ms(fns["hidden_state"])
            assert launches == 2 * L + 1, launches
            ln.append(all_ms / (2 * L))
            rows.append(tok_ms - all_ms)
        nbytes = 2.0 * BATCH * T * D * 4
        gbs = lambda ms: nbytes / (ms * 1e-3) / 1e9                # noqa: E731
        res["row_kernels_precision_3"] = {
            "rows": BATCH * T, "width": D, "bytes_per_launch": nbytes,
            "layernorm_f32": {"median_us": statistics.median(ln) * 1e3, "samples_us": [v * 1e3 for v in ln],
                              "GBps": gbs(statistics.median(ln)), "GBps_samples": [gbs(v) for v in ln]},
            "final_norm_rows": {"median_us": statistics.median(rows) * 1e3, "samples_us": [v * 1e3 for v in rows],
                                "GBps": gbs(statistics.median(rows)), "GBps_samples": [gbs(v) for v in rows]}}
        k = res["row_kernels_precision_3"]
        print(f"rows {BATCH * T} x {D}: layernorm_f32 {k['layernorm_f32']['median_us']:.1f} us ({k['layernorm_f32']['GBps']:.0f} GB/s), "
              f"final_norm_rows {k['final_norm_rows']['median_us']:.1f} us ({k['final_norm_rows']['GBps']:.0f} GB/s)")
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
