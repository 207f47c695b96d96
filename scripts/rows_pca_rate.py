"""The rate of the PCA over resident CLS rows -> profiles/rows_pca.json.

D = 768 fp16 rows resident on the device, N = 180 000 and 2 000 000, k = 3 and 8; medians of five synchronised calls after a warm-up.

  * the fit               cbas_rows_pca_fit with 64 rounds of the solver, and with 1: (t64 - t1) / 63 is one round, t1 minus one round the
                          mean and the covariance together
  * its kernels           one fit under torch.profiler, the device time summed per kernel: mean, covariance, reduce, solver apart
                          (absent from the JSON when the profiler reports no kernels)
  * ``project``           cbas_rows_pca_project alone, with the residual: one pass (two reads of a row with normalize)
  * a device copy         of the same row bytes: the floor for one read
  * the torch route       centred fp32 slabs, X.T @ X accumulated, torch.linalg.eigh, matmul for the scores - with its scratch bytes
  * the host route        float64 numpy (tests/rows_pca_ref.py) at the smaller N only - ONE sample, no warm-up
The covariance's work is the upper triangle of 128 x 128 tiles: 2 * N * 128 * 128 * T (T + 1) / 2 FLOP, T = D / 128; PEAK_TF is the fp32
matrix pipe's 157 TFLOP/s.

    python scripts/rows_pca_rate.py [--out profiles/rows_pca.json] [--no-host]
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
import rows_pca_ref as R  # noqa: E402

from cbas_amd import _lib  # noqa: E402

D = 768
SLAB = 1 << 16
PEAK_TF = 157.0


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
    need = int(lib.cbas_rows_pca_workspace_bytes(n, D, k))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    mean, comp = torch.empty(D, device="cuda"), torch.empty((k, D), device="cuda")
    eig, tv = torch.empty(k, device="cuda"), torch.empty(1, device="cuda")
    scores, resid = torch.empty((n, k), device="cuda"), torch.empty(n, device="cuda")

    def fit(iters):
        _lib.check(lib.cbas_rows_pca_fit(rows.data_ptr(), n, D, D, k, iters, 1, mean.data_ptr(), comp.data_ptr(), eig.data_ptr(), tv.data_ptr(),
                                         ws.data_ptr(), need, None), "cbas_rows_pca_fit")

    def project():
        _lib.check(lib.cbas_rows_pca_project(rows.data_ptr(), n, D, D, k, 1, mean.data_ptr(), comp.data_ptr(), None, scores.data_ptr(),
                                             resid.data_ptr(), None), "cbas_rows_pca_project")
    return fit, project, (mean, comp, eig), need


def kernel_times_ms(fn):
    """Device time per kernel family of one call, from torch.profiler; None when it sees no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        fam = {"rows_rn": "rn", "fp_mean": "mean", "fp_cov_kernel": "covariance", "fp_cov_reduce": "reduce", "pca_": "solver"}
        out = {}
        for ev in prof.key_averages():
            for key, name in fam.items():
                if key in ev.key:
                    us = getattr(ev, "device_time_total", None)
                    us = getattr(ev, "cuda_time_total", 0.0) if us is None else us
                    out[name] = out.get(name, 0.0) + us / 1e3
                    break
        return out or None
    except Exception as e:                                       # a measurement aid: the wall-clock numbers stand without it
        print(f"torch.profiler gave no kernel times: {e}", flush=True)
        return None


def torch_route(rows, k):
    """The same map in torch: unit rows and centring in fp32 slabs, X.T @ X accumulated, eigh, a matmul for the scores."""
    n = rows.shape[0]
    total = torch.zeros(D, device="cuda")
    for a in range(0, n, SLAB):
        total += torch.nn.functional.normalize(rows[a:a + SLAB].float(), dim=1).sum(dim=0)
    mean = total / n
    cov = torch.zeros((D, D), device="cuda")
    for a in range(0, n, SLAB):
        x = torch.nn.functional.normalize(rows[a:a + SLAB].float(), dim=1) - mean
        cov += x.T @ x
    cov /= n - 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    w, v = torch.linalg.eigh(cov)
    torch.cuda.synchronize()
    t_eigh = (time.perf_counter() - t0) * 1e3
    comp = v[:, -k:].flip(1).T.contiguous()
    t0 = time.perf_counter()
    scores = torch.empty((n, k), device="cuda")
    for a in range(0, n, SLAB):
        scores[a:a + SLAB] = (torch.nn.functional.normalize(rows[a:a + SLAB].float(), dim=1) - mean) @ comp.T
    torch.cuda.synchronize()
    t_proj = (time.perf_counter() - t0) * 1e3
    return t_eigh, t_proj, w.flip(0)[:k], min(SLAB, n) * D * 8 + D * D * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_pca.json"))
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--rows", type=int, nargs="+", default=[180_000, 2_000_000])
    ap.add_argument("--components", type=int, nargs="+", default=[3, 8])
    a = ap.parse_args()
    res = {"dim": D, "chunk": R.CHUNK, "max_parts": R.MAX_PARTS, "peak_tflops": PEAK_TF, "device": torch.cuda.get_device_name(0), "cases": []}
    gen = torch.Generator(device="cuda").manual_seed(1)
    tiles = D // 128
    for n in a.rows:
        proto = torch.randn((64, D), device="cuda", generator=gen)
        group = torch.randint(0, 64, (n,), device="cuda", generator=gen)
        rows = (proto[group] + 0.5 * torch.randn((n, D), device="cuda", generator=gen)).to(torch.float16)
        del group
        row_bytes = n * D * 2
        other = torch.empty_like(rows)
        copy = timed_ms(lambda: other.copy_(rows))
        del other
        flop = 2.0 * n * 128 * 128 * tiles * (tiles + 1) / 2
        for k in a.components:
            fit, project, (mean, comp, eig), need = fitter(rows, k)
            t64, t1 = timed_ms(lambda: fit(64)), timed_ms(lambda: fit(1))
            kernels = kernel_times_ms(lambda: fit(64))
            t_proj = timed_ms(project)
            round_ms = (t64["median_ms"] - t1["median_ms"]) / 63
            meancov_ms = t1["median_ms"] - round_ms
            torch_route(rows, k)
            t0 = time.perf_counter()
            t_eigh, t_tproj, w_torch, scratch = torch_route(rows, k)
            t_torch_all = (time.perf_counter() - t0) * 1e3
            case = {"rows": n, "components": k, "row_bytes": row_bytes, "workspace_bytes": need, "partition": list(R.partition(n)), "device_copy": copy,
                    "fit_64": t64, "fit_1": t1, "solver_round_ms": round_ms, "solver_64_ms": 64 * round_ms, "mean_and_covariance_ms": meancov_ms,
                    "kernels_ms": kernels, "project": t_proj, "project_over_copy": t_proj["median_ms"] / copy["median_ms"],
                    "covariance_flop": flop, "torch_fit_ms": t_torch_all - t_tproj, "torch_eigh_ms": t_eigh, "torch_project_ms": t_tproj,
                    "torch_scratch_bytes": scratch, "eigenvalue_rel_diff_vs_torch": float(((eig - w_torch).abs() / w_torch.abs()).max())}
            cov_ms = kernels.get("covariance") if kernels else None
            if cov_ms:
                case["covariance_tflops"] = flop / cov_ms / 1e9
                case["covariance_of_peak"] = case["covariance_tflops"] / PEAK_TF
            if not a.no_host and n <= 200_000:
                x = rows.cpu().numpy()
                t0 = time.perf_counter()
                ref = R.fit(x, k, 1)
                R.project(x, 1, ref["mean"], ref["components"])
                case["host_float64_ms"] = (time.perf_counter() - t0) * 1e3
            res["cases"].append(case)
            print(f"[N {n} k {k}] fit(64) {t64['median_ms']:.2f} ms: mean + covariance {meancov_ms:.2f} ms, solver {64 * round_ms:.2f} ms; kernels {kernels}; "
                  f"project {t_proj['median_ms']:.3f} ms = {case['project_over_copy']:.2f} x the copy ({copy['median_ms']:.3f} ms); torch fit "
                  f"{case['torch_fit_ms']:.1f} ms (eigh {t_eigh:.1f}), project {t_tproj:.2f} ms; host {case.get('host_float64_ms', float('nan')):.0f} ms",
                  flush=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        del rows
        torch.cuda.empty_cache()
    print(json.dumps({"out": a.out, "cases": len(res["cases"])}))


if __name__ == "__main__":
    main()
