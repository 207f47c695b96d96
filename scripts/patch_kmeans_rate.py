#!/usr/bin/env python3
"""What clustering patch features costs on the device, beside the host route it replaces.

ViT-B/16 at 256 x 256 (T = 261 tokens, 256 patches), batch 64, precision 4, frames resident on the device, k = 4 and 16, both scopes
("frame": 64 problems of 256 rows; "batch": one problem of 16 384 rows).  Each figure is timed between two
``torch.cuda.synchronize()`` calls, the median of REPEATS after one warm-up call, every sample kept:
  * ``hidden_state``      the (n, T, D) fp32 rows alone
  * ``patch_clusters``    the same forward, then seeding, KMEANS_DEFAULT_ITERS rounds and the assignment on the device
  * a round               cbas_patch_kmeans_fit on resident rows with 16 and with 48 rounds: (t48 - t16) / 32 is one round (the pass
                          over the rows and the update), free of the seeding and of launch warm-up
  * bandwidth             the bytes a round moves over that time: the rows once (M D 4), the centroids once per chunk of 64 rows,
                          the chunk sums written by the pass and read by the update
  * the host route        ``hidden_state(frames).cpu()``, then tests/patch_kmeans_ref.py's float64 Lloyd from the device's own seeds
                          for the same number of rounds and its assignment - ONE sample, no warm-up (it takes seconds)

Per-kernel times come from a run of this script under ``rocprofv3 --kernel-trace --stats`` (a run of its own: ``--profile-pass``
makes two fits of 16 rounds per case and writes nothing).

    python scripts/patch_kmeans_rate.py [--out profiles/patch_kmeans.json] [--no-host] [--profile-pass]
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import patch_kmeans_ref as R  # noqa: E402
from cbas_amd import _lib, config as C, synth, weights as W  # noqa: E402
from cbas_amd.encoder import KMEANS_DEFAULT_ITERS, DinoEncoder, token_grid  # noqa: E402

BATCH, HW, KS, REPEATS, PRECISION = 64, 256, (4, 16), 5, 4
ROUNDS_A, ROUNDS_B = 16, 48


def timed_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def sample(fn):
    fn()                                                     # warm-up
    s = [timed_ms(fn) for _ in range(REPEATS)]
    return {"median_ms": statistics.median(s), "samples_ms": s}


def raw_fit(lib, tokens, P0, k, scope, iters):
    n, T, D = tokens.shape
    sc = _lib.PCA_BATCH if scope == "batch" else _lib.PCA_FRAME
    nb = 1 if scope == "batch" else n
    need = int(lib.cbas_patch_kmeans_workspace_bytes(n, T, P0, D, k, sc))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    cent = torch.empty(nb, k, D, device="cuda")
    counts, init = torch.empty(nb, k, dtype=torch.int32, device="cuda"), torch.empty(nb, k, dtype=torch.int32, device="cuda")
    inertia = torch.empty(nb, iters + 1, device="cuda")

    def run():
        _lib.check(lib.cbas_patch_kmeans_fit(tokens.data_ptr(), n, T, P0, D, D, k, sc, iters, 1, cent.data_ptr(), counts.data_ptr(),
                                             inertia.data_ptr(), init.data_ptr(), ws.data_ptr(), need, None), "cbas_patch_kmeans_fit")
    return run


def host_route(enc, frames, scope, P0, init_index, iters):
    rows = enc.hidden_state(frames).cpu().numpy()[:, P0:]                              # (n, P, D)
    out = []
    for b, X in enumerate([rows.reshape(-1, rows.shape[2])] if scope == "batch" else rows):
        out.append(R.lloyd(R.working_rows(X, 1), list(init_index[b]), iters)["labels"])
    return out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    cfg = C.VIT_B16
    lib = _lib.load()
    enc = DinoEncoder.from_weights(cfg, W.synth_encoder_weights(cfg, 1234), "cuda", max_batch=BATCH, max_frame=(HW, HW), precision=PRECISION)
    frames = torch.from_numpy(synth.cage_frames(3, BATCH, HW, HW)).cuda()
    nh, nw, P0 = token_grid(cfg, HW, HW)
    D, P = cfg.hidden_size, nh * nw
    tokens = enc.hidden_state(frames)
    if "--profile-pass" in sys.argv:
        # for a run under rocprofv3 --kernel-trace --stats: per case one warm-up fit and one fit of ROUNDS_A rounds, nothing written
        for k in KS:
            for scope in ("frame", "batch"):
                run = raw_fit(lib, tokens, P0, k, scope, ROUNDS_A)
                run()
                torch.cuda.synchronize()
                run()
                torch.cuda.synchronize()
        enc.close()
        return
    res = {"model": "vitb16", "batch": BATCH, "frame": [HW, HW], "patches": P, "dim": D, "iters": KMEANS_DEFAULT_ITERS, "chunk": R.CHUNK,
           "precision": PRECISION, "repeats": REPEATS, "device": torch.cuda.get_device_name(0),
           "hidden_state": sample(lambda: enc.hidden_state(frames)), "cases": {}}
    hs = res["hidden_state"]["median_ms"]
    for k in KS:
        for scope in ("frame", "batch"):
            dev = sample(lambda: enc.patch_clusters(frames, k, scope))
            ta, tb = sample(raw_fit(lib, tokens, P0, k, scope, ROUNDS_A)), sample(raw_fit(lib, tokens, P0, k, scope, ROUNDS_B))
            round_us = (tb["median_ms"] - ta["median_ms"]) / (ROUNDS_B - ROUNDS_A) * 1e3
            M, nb = (BATCH * P, 1) if scope == "batch" else (P, BATCH)
            chunks = nb * -(-M // R.CHUNK)
            row_bytes, all_bytes = BATCH * P * D * 4, BATCH * P * D * 4 + 3 * chunks * k * D * 4
            case = {"patch_clusters": dev, "device_share_ms": dev["median_ms"] - hs, f"fit_{ROUNDS_A}_rounds": ta, f"fit_{ROUNDS_B}_rounds": tb,
                    "round_us": round_us, "row_bytes": row_bytes, "round_bytes": all_bytes, "rows_GBps": row_bytes / round_us / 1e3,
                    "round_GBps": all_bytes / round_us / 1e3}
            line = (f"[k {k} {scope}] hidden_state {hs:.2f} ms; patch_clusters {dev['median_ms']:.2f} ms (clustering {dev['median_ms'] - hs:.2f}); "
                    f"a round {round_us:.1f} us = {case['rows_GBps']:.0f} GB/s of rows, {case['round_GBps']:.0f} GB/s of all bytes")
            if "--no-host" not in sys.argv:
                _, cl = enc.patch_clusters(frames, k, scope)
                init = cl.init_index.cpu().numpy()
                host_ms = timed_ms(lambda: host_route(enc, frames, scope, P0, init, KMEANS_DEFAULT_ITERS))
                case.update(host_route_ms=host_ms, host_share_ms=host_ms - hs, host_over_device=(host_ms - hs) / max(dev["median_ms"] - hs, 1e-9))
                line += f"; host route {host_ms:.0f} ms"
            res["cases"][f"k{k}_{scope}"] = case
            print(line, flush=True)
    enc.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({c: {k: v for k, v in r.items() if not isinstance(v, dict)} for c, r in res["cases"].items()}))


if __name__ == "__main__":
    main()
