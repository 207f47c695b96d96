"""The rate of the k-means over resident CLS rows -> profiles/rows_kmeans.json.

D = 768 fp16 rows resident on the device, N = 180 000 and 2 000 000, k = 8, 16 and 64; medians of five synchronised calls after a warm-up.

  * a round               cbas_rows_kmeans_fit from given centroids with 2 and with 6 rounds: (t6 - t2) / 4 is one round (pass, sums, update)
  * seeding               the fit with 0 rounds from seeds minus the fit with 0 rounds from given centroids
  * the whole fit         20 rounds from seeds
  * ``assign``            cbas_rows_kmeans_assign alone: one pass
  * a device copy         of the same row bytes: the floor for one read
  * the torch route       fp16 matmul against the centroids in row slabs, argmax, index_add_ - one round, with its scratch bytes
  * the host route        float64 numpy (tests/rows_kmeans_ref.py), one round, at the smaller N only - ONE sample, no warm-up

    python scripts/rows_kmeans_rate.py [--out profiles/rows_kmeans.json] [--no-host]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rows_kmeans_ref as R  # noqa: E402

from cbas_amd import _lib  # noqa: E402

D = 768
SLAB = 1 << 16


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


def fitter(rows, k):
    lib = _lib.load()
    n = rows.shape[0]
    need = int(lib.cbas_rows_kmeans_workspace_bytes(n, D, k))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    cent = torch.empty((k, D), device="cuda")
    counts = torch.empty(k, dtype=torch.int64, device="cuda")
    inertia = torch.empty(32, device="cuda")
    seeds = torch.empty(k, dtype=torch.int64, device="cuda")
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    dist2 = torch.empty(n, device="cuda")

    def fit(iters, init=None):
        _lib.check(lib.cbas_rows_kmeans_fit(rows.data_ptr(), n, D, D, k, iters, 1, None if init is None else init.data_ptr(), cent.data_ptr(),
                                            counts.data_ptr(), inertia.data_ptr(), seeds.data_ptr(), labels.data_ptr(), dist2.data_ptr(),
                                            ws.data_ptr(), need, None), "cbas_rows_kmeans_fit")

    def assign():
        _lib.check(lib.cbas_rows_kmeans_assign(rows.data_ptr(), n, D, D, k, 1, cent.data_ptr(), labels.data_ptr(), dist2.data_ptr(), None),
                   "cbas_rows_kmeans_assign")
    return fit, assign, cent, need


def torch_round(rows, cent):
    """One Lloyd round in torch: cosine scores in fp16, argmax, sums by index_add_.  Returns the scratch bytes."""
    n, k = rows.shape[0], cent.shape[0]
    c16 = cent.to(torch.float16)
    half = 0.5 * (cent * cent).sum(dim=1)
    sums = torch.zeros((k, D), device="cuda")
    counts = torch.zeros(k, device="cuda")
    scratch = 0
    for a in range(0, n, SLAB):
        x = rows[a:a + SLAB]
        u = torch.nn.functional.normalize(x.float(), dim=1)
        score = (u.to(torch.float16) @ c16.T).float() - half
        lab = score.argmax(dim=1)
        sums.index_add_(0, lab, u)
        counts.index_add_(0, lab, torch.ones_like(lab, dtype=torch.float32))
        scratch = max(scratch, u.numel() * 6 + score.numel() * 6 + lab.numel() * 12)
    return sums / counts.clamp(min=1)[:, None], scratch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_kmeans.json"))
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--rows", type=int, nargs="+", default=[180_000, 2_000_000])
    ap.add_argument("--clusters", type=int, nargs="+", default=[8, 16, 64])
    a = ap.parse_args()
    res = {"dim": D, "segment": R.SEGMENT, "tile": R.TILE, "device": torch.cuda.get_device_name(0), "cases": []}
    gen = torch.Generator(device="cuda").manual_seed(1)
    for n in a.rows:
        proto = torch.randn((64, D), device="cuda", generator=gen)
        group = torch.randint(0, 64, (n,), device="cuda", generator=gen)
        rows = (proto[group] + 0.5 * torch.randn((n, D), device="cuda", generator=gen)).to(torch.float16)
        del group
        row_bytes = n * D * 2
        other = torch.empty_like(rows)
        copy = timed_ms(lambda: other.copy_(rows))
        del other
        for k in a.clusters:
            fit, assign, cent, need = fitter(rows, k)
            fit(0)
            start = cent.clone()
            t_seeded0, t_init0 = timed_ms(lambda: fit(0)), timed_ms(lambda: fit(0, start))
            t2, t6 = timed_ms(lambda: fit(2, start)), timed_ms(lambda: fit(6, start))
            whole = timed_ms(lambda: fit(20), reps=3)
            t_assign = timed_ms(assign)
            round_ms = (t6["median_ms"] - t2["median_ms"]) / 4
            scratch = torch_round(rows, start)[1]
            t_torch = timed_ms(lambda: torch_round(rows, start))
            case = {"rows": n, "clusters": k, "row_bytes": row_bytes, "workspace_bytes": need, "device_copy": copy, "fit_0_seeded": t_seeded0,
                    "fit_0_init": t_init0, "fit_2_init": t2, "fit_6_init": t6, "fit_20_seeded": whole, "assign": t_assign, "round_ms": round_ms,
                    "seeding_ms": t_seeded0["median_ms"] - t_init0["median_ms"], "round_over_copy": round_ms / copy["median_ms"],
                    "round_GBps_of_rows": row_bytes / round_ms / 1e6, "torch_round": t_torch, "torch_scratch_bytes": scratch,
                    "torch_over_round": t_torch["median_ms"] / round_ms}
            if not a.no_host and n <= 200_000:
                x = rows.cpu().numpy()
                t0 = time.perf_counter()
                lab, _, _ = R.assign(x, start.cpu().numpy(), 1)
                R.update(x, lab, start.cpu().numpy(), 1)
                case["host_float64_round_ms"] = (time.perf_counter() - t0) * 1e3
            res["cases"].append(case)
            print(f"[N {n} k {k}] round {round_ms:.3f} ms = {case['round_over_copy']:.2f} x the copy ({copy['median_ms']:.3f} ms); assign "
                  f"{t_assign['median_ms']:.3f} ms; seeding {case['seeding_ms']:.2f} ms; fit(20) {whole['median_ms']:.1f} ms; torch round "
                  f"{t_torch['median_ms']:.3f} ms ({scratch / 1e6:.0f} MB scratch); host {case.get('host_float64_round_ms', float('nan')):.0f} ms",
                  flush=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        del rows
        torch.cuda.empty_cache()
    print(json.dumps({"out": a.out, "cases": len(res["cases"])}))


if __name__ == "__main__":
    main()
