"""The rate of the motif HMM's two passes and of a whole EM round -> profiles/rows_hmm.json.

Random fp16 rows, D = 768, N = 180 000 and 2 000 000, C = 9, 16 and 64 unit means, kappa = 10; clips of 18 000 frames; medians of
five synchronised calls after a warm-up.

  * the emissions     cbasx_rows_emissions (probs and lognorm)
  * the sums          cbasx_rows_weighted_sums on the gamma of the round
  * the copy          a device copy of the same row bytes: the floor for one read of the rows and as many bytes written
  * the torch route   fp16 matmul in slabs of 65 536 rows + softmax, and gamma.T @ X in the same slabs (rows normalised per slab)
  * the round         emissions, cbasx_hmm_posteriors, sums: each call, and the three together with the small update
  * the host route    float64 numpy of both passes on the 180 000 frames - ONE sample

    python scripts/rows_hmm_rate.py [--out profiles/rows_hmm.json] [--no-host]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cbas_amd import _lib, bouts, motif_hmm  # noqa: E402

D, CLIP, SLAB, KAPPA = 768, 18_000, 65_536, 10.0


def timed_ms(fn, reps=5, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "samples": reps}


def torch_emissions(rows, means16, kappa):
    out = []
    for a in range(0, rows.shape[0], SLAB):
        x = rows[a:a + SLAB]
        rn = x.float().norm(dim=1, keepdim=True).clamp_min(1e-30).reciprocal()
        out.append(torch.softmax(kappa * rn * (x @ means16.T).float(), dim=1))
    return torch.cat(out)


def torch_sums(rows, gamma):
    acc = torch.zeros((gamma.shape[1], rows.shape[1]), dtype=torch.float32, device=rows.device)
    for a in range(0, rows.shape[0], SLAB):
        x = rows[a:a + SLAB].float()
        x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-30)
        acc += gamma[a:a + SLAB].T @ x
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_hmm.json"))
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.load()
    result = {"dim": D, "kappa": KAPPA, "clip": CLIP, "device": _lib.device_info(0)[0], "cases": []}
    for N in (180_000, 2_000_000):
        g = torch.Generator(device=dev).manual_seed(N)
        rows = torch.randn((N, D), generator=g, device=dev).to(torch.float16).contiguous()
        other = torch.empty_like(rows)
        copy = timed_ms(lambda: other.copy_(rows))
        del other
        firsts = np.arange(0, N, CLIP, dtype=np.int64)
        table = torch.from_numpy(np.stack([firsts, np.minimum(CLIP, N - firsts)], axis=1)).to(dev)
        for C in (9, 16, 64):
            means = torch.nn.functional.normalize(torch.randn((C, D), generator=g, device=dev), dim=1).contiguous()
            means16 = means.to(torch.float16)
            A = torch.from_numpy(bouts.sticky_transitions(C, mean_duration=40, as_probs=True)).to(dev)
            prior = torch.full((C,), 1.0 / C, dtype=torch.float64, device=dev)
            ws = torch.empty(_lib.workspace_bytes("cbasx_rows_weighted_sums_workspace_bytes", N, D, C), dtype=torch.uint8, device=dev)
            entry = {"N": N, "C": C, "row_bytes": N * D * 2, "device_copy_same_row_bytes": copy, "sums_workspace_bytes": int(ws.numel())}
            probs, _ = motif_hmm.device_emissions(rows, means, KAPPA)
            gamma = bouts.device_posteriors(probs, table, A)[0].contiguous()
            entry["emissions"] = timed_ms(lambda: motif_hmm.device_emissions(rows, means, KAPPA))
            entry["weighted_sums"] = timed_ms(lambda: motif_hmm.device_weighted_sums(rows, gamma, True, ws))
            entry["posteriors"] = timed_ms(lambda: bouts.device_posteriors(probs, table, A))
            entry["torch_emissions"] = timed_ms(lambda: torch_emissions(rows, means16, KAPPA))
            entry["torch_sums"] = timed_ms(lambda: torch_sums(rows, gamma))

            def em_round():
                p, _ = motif_hmm.device_emissions(rows, means, KAPPA)
                gm, Xi, Pi, _, _ = bouts.device_posteriors(p, table, A)
                s, m = motif_hmm.device_weighted_sums(rows, gm, True, ws)
                return motif_hmm.em_update(means, s, m, Xi, Pi, prior, 1.0, False)
            entry["em_round"] = timed_ms(em_round)
            for key in ("emissions", "weighted_sums", "torch_emissions", "torch_sums", "em_round"):
                entry[key]["over_copy"] = entry[key]["median_ms"] / copy["median_ms"]
            entry["emissions"]["torch_over_kernel"] = entry["torch_emissions"]["median_ms"] / entry["emissions"]["median_ms"]
            entry["weighted_sums"]["torch_over_kernel"] = entry["torch_sums"]["median_ms"] / entry["weighted_sums"]["median_ms"]
            entry["weighted_sums"]["tflops"] = 2.0 * N * C * D / (entry["weighted_sums"]["median_ms"] * 1e-3) / 1e12
            if N == 180_000 and not a.no_host:
                x, mu, gm = rows.cpu().numpy(), means.cpu().numpy(), gamma.cpu().numpy()
                t0 = time.perf_counter()
                motif_hmm.emissions_host(x, mu, KAPPA)
                t1 = time.perf_counter()
                motif_hmm.weighted_sums_host(x, gm)
                entry["numpy_host_float64"] = {"emissions_ms": (t1 - t0) * 1e3, "weighted_sums_ms": (time.perf_counter() - t1) * 1e3, "samples": 1}
            result["cases"].append(entry)
            print(json.dumps(entry), flush=True)
            del probs, gamma, ws
        del rows
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
