#!/usr/bin/env python3
"""What a patch-feature PCA costs on the device, beside the host route it replaces.

ViT-B/16 at 256 x 256 (T = 261 tokens, 256 patches), batch 64, k = 3, precision 4, frames resident on the device.  For each scope
("frame": 64 problems of 256 rows; "batch": one problem of 16 384 rows) three things are timed, each between two
``torch.cuda.synchronize()`` calls, the median of REPEATS after one warm-up call, every sample kept:
  * ``hidden_state``                the (n, T, D) fp32 rows alone
  * ``patch_pca``                   the same forward, then fit and projection on the device (cbas_patch_pca_fit / _project)
  * the host route                  ``hidden_state(frames).cpu()``, then float64 mean, covariance, ``numpy.linalg.eigh`` and the
                                    projection on the host (per frame, or once for the batch)
The device route's own share is ``patch_pca`` minus ``hidden_state``; the host route's is its total minus ``hidden_state``.
Per-kernel times come from a run of this script under ``rocprofv3 --kernel-trace --stats`` (a run of its own: ``--profile-pass``
makes one ``patch_pca`` call per scope after a warm-up and writes nothing).

    python scripts/patch_pca_rate.py [--out profiles/patch_pca.json] [--profile-pass]
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cbas_amd import config as C, synth, weights as W  # noqa: E402
from cbas_amd.encoder import PCA_DEFAULT_ITERS, DinoEncoder, token_grid  # noqa: E402

BATCH, HW, K, REPEATS, PRECISION = 64, 256, 3, 5, 4


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


def host_route(enc, frames, scope, P0):
    rows = enc.hidden_state(frames).cpu().numpy()[:, P0:].astype(np.float64)          # (n, P, D)
    out = []
    for X in ([rows.reshape(-1, rows.shape[2])] if scope == "batch" else rows):
        Xc = X - X.mean(axis=0)
        w, V = np.linalg.eigh(Xc.T @ Xc / (X.shape[0] - 1))
        out.append(Xc @ V[:, ::-1][:, :K])
    return out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    cfg = C.VIT_B16
    enc = DinoEncoder.from_weights(cfg, W.synth_encoder_weights(cfg, 1234), "cuda", max_batch=BATCH, max_frame=(HW, HW), precision=PRECISION)
    frames = torch.from_numpy(synth.cage_frames(3, BATCH, HW, HW)).cuda()
    nh, nw, P0 = token_grid(cfg, HW, HW)
    if "--profile-pass" in sys.argv:
        for scope in ("frame", "batch"):
            enc.patch_pca(frames, K, scope)
            torch.cuda.synchronize()
            enc.patch_pca(frames, K, scope)
            torch.cuda.synchronize()
        enc.close()
        return
    res = {"model": "vitb16", "batch": BATCH, "frame": [HW, HW], "patches": nh * nw, "dim": cfg.hidden_size, "components": K,
           "iters": PCA_DEFAULT_ITERS, "precision": PRECISION, "repeats": REPEATS, "device": torch.cuda.get_device_name(0),
           "hidden_state": sample(lambda: enc.hidden_state(frames)), "scopes": {}}
    hs = res["hidden_state"]["median_ms"]
    for scope in ("frame", "batch"):
        dev = sample(lambda: enc.patch_pca(frames, K, scope))
        host = sample(lambda: host_route(enc, frames, scope, P0))
        res["scopes"][scope] = {"patch_pca": dev, "host_route": host, "device_share_ms": dev["median_ms"] - hs,
                                "host_share_ms": host["median_ms"] - hs,
                                "host_over_device": (host["median_ms"] - hs) / max(dev["median_ms"] - hs, 1e-9)}
        print(f"[{scope}] hidden_state {hs:.2f} ms; patch_pca {dev['median_ms']:.2f} ms (fit + project {dev['median_ms'] - hs:.2f}); "
              f"host route {host['median_ms']:.2f} ms ({host['median_ms'] - hs:.2f} after the forward)")
    enc.close()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({s: {k: v for k, v in r.items() if k.endswith("_ms") or k == "host_over_device"} for s, r in res["scopes"].items()}))


if __name__ == "__main__":
    main()
