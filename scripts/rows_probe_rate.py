"""The rate of the linear probe over resident CLS rows -> profiles/rows_probe.json.

Medians of five synchronised calls after one warm-up, D = 768, l2 = 1e-4, balanced-style sample weights:
  * an iteration          cbas_rows_probe_fit from given weights with 10 and with 50 steps: (t50 - t10) / 40 is one step (forward pass,
                          loss sums, gradient, update); the call's fixed part (checks, one synchronisation, closing pass) cancels
  * a fit                 1000 steps from zeros, the whole call
  * ``predict``           cbas_rows_probe_predict over 180 000 and 2 000 000 rows
  * a device copy         of the same row bytes, beside each
  * the torch route       the same iteration on the same device: fp32 normalised rows (made once, outside the timing), ``matmul``,
                          ``log_softmax``, the gradient as a second ``matmul``, the same Nesterov update; and predict as
                          ``softmax(normalize(x.float()) @ W.T + b)``
Nothing here is asserted anywhere: these are new paths without an earlier time.

    python scripts/rows_probe_rate.py [--out profiles/rows_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cbas_amd import _lib  # noqa: E402

D = 768
L2 = 1e-4
SEGMENT, TILE = 1024, 128


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


def planted(n, C, gen):
    proto = torch.randn((C, D), device="cuda", generator=gen)
    y = torch.randint(0, C, (n,), device="cuda", generator=gen)
    rows = (proto[y] + 1.0 * torch.randn((n, D), device="cuda", generator=gen)).to(torch.float16)
    return rows, y.to(torch.int32)


def fitter(rows, y, omega, C):
    lib = _lib.load()
    n = rows.shape[0]
    need = int(lib.cbas_rows_probe_workspace_bytes(n, D, C))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    W, b, loss = torch.empty((C, D), device="cuda"), torch.empty(C, device="cuda"), torch.empty(1001, device="cuda")

    def fit(iters, W0=None, b0=None):
        _lib.check(lib.cbas_rows_probe_fit(rows.data_ptr(), n, D, D, y.data_ptr(), omega.data_ptr(), C, L2, iters,
                                           None if W0 is None else W0.data_ptr(), None if b0 is None else b0.data_ptr(), W.data_ptr(), b.data_ptr(),
                                           loss.data_ptr(), ws.data_ptr(), need, None), "cbas_rows_probe_fit")
    return fit, W, b, loss, need


def predictor(rows, W, b):
    lib = _lib.load()
    n, C = rows.shape[0], W.shape[0]
    probs = torch.empty((n, C), device="cuda")

    def run():
        _lib.check(lib.cbas_rows_probe_predict(rows.data_ptr(), n, D, D, W.data_ptr(), b.data_ptr(), C, probs.data_ptr(), None, None),
                   "cbas_rows_probe_predict")
    return run, probs


def torch_fit(u, y64, omega, C, iters):
    """The same iteration in torch on fp32 unit rows u: returns (W, b)."""
    Lc = 1.0 + L2
    sq = (L2 / Lc) ** 0.5
    beta, inv_l = (1.0 - sq) / (1.0 + sq), 1.0 / Lc
    W, b = torch.zeros((C, D), device="cuda"), torch.zeros(C, device="cuda")
    vW, vb = W.clone(), b.clone()
    inv_om = 1.0 / omega.sum()
    onehot = torch.nn.functional.one_hot(y64, C).float()
    for _ in range(iters):
        p = torch.softmax(u @ vW.T + vb, dim=1)
        r = (p - onehot) * omega[:, None]
        gW, gb = (r.T @ u) * inv_om + L2 * vW, r.sum(dim=0) * inv_om + L2 * vb
        nW, nb = vW - inv_l * gW, vb - inv_l * gb
        vW, vb = nW + beta * (nW - W), nb + beta * (nb - b)
        W, b = nW, nb
    return W, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_probe.json"))
    ap.add_argument("--train", type=int, nargs="+", default=[1024, 8192, 65536])
    ap.add_argument("--classes", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--rows", type=int, nargs="+", default=[180_000, 2_000_000])
    a = ap.parse_args()
    res = {"dim": D, "l2": L2, "segment": SEGMENT, "tile": TILE, "device": torch.cuda.get_device_name(0), "fit": [], "predict": []}
    gen = torch.Generator(device="cuda").manual_seed(1)
    for M in a.train:
        for C in a.classes:
            rows, y = planted(M, C, gen)
            y64 = y.long()
            count = torch.bincount(y64, minlength=C).float()
            omega = (M / (C * count.clamp(min=1)))[y64].contiguous()
            other = torch.empty_like(rows)
            copy = timed_ms(lambda: other.copy_(rows))
            fit, W, b, loss, need = fitter(rows, y, omega, C)
            fit(10)
            W0, b0 = W.clone(), b.clone()
            t10, t50 = timed_ms(lambda: fit(10, W0, b0)), timed_ms(lambda: fit(50, W0, b0))
            whole = timed_ms(lambda: fit(1000), reps=5)
            dev_loss = float(loss[1000])
            step_ms = (t50["median_ms"] - t10["median_ms"]) / 40
            u = torch.nn.functional.normalize(rows.float(), dim=1)
            tt10, tt50 = timed_ms(lambda: torch_fit(u, y64, omega, C, 10)), timed_ms(lambda: torch_fit(u, y64, omega, C, 50))
            torch_whole = timed_ms(lambda: torch_fit(u, y64, omega, C, 1000), reps=5)
            Wt, bt = torch_fit(u, y64, omega, C, 1000)
            torch_step = (tt50["median_ms"] - tt10["median_ms"]) / 40
            case = {"train_rows": M, "classes": C, "row_bytes": M * D * 2, "workspace_bytes": need, "device_copy": copy, "fit_10": t10, "fit_50": t50,
                    "fit_1000": whole, "step_ms": step_ms, "step_over_copy": step_ms / copy["median_ms"], "loss_after_1000": dev_loss,
                    "torch_fit_10": tt10, "torch_fit_50": tt50, "torch_fit_1000": torch_whole, "torch_step_ms": torch_step,
                    "torch_over_step": torch_step / step_ms, "torch_fit_over_fit": torch_whole["median_ms"] / whole["median_ms"],
                    "max_weight_difference_to_torch": float((Wt - W).abs().max())}
            res["fit"].append(case)
            print(f"[M {M} C {C}] step {step_ms * 1e3:.1f} us ({case['step_over_copy']:.1f} x the copy of {copy['median_ms'] * 1e3:.1f} us); fit(1000) "
                  f"{whole['median_ms']:.1f} ms; torch step {torch_step * 1e3:.1f} us, fit(1000) {torch_whole['median_ms']:.1f} ms; max |W - W_torch| "
                  f"{case['max_weight_difference_to_torch']:.2e}", flush=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
            del rows, other, u
    for n in a.rows:
        for C in a.classes:
            rows, _ = planted(n, C, gen)
            other = torch.empty_like(rows)
            copy = timed_ms(lambda: other.copy_(rows))
            del other
            W = (0.1 * torch.randn((C, D), device="cuda", generator=gen)).contiguous()
            b = torch.zeros(C, device="cuda")
            run, probs = predictor(rows, W, b)
            t = timed_ms(run)
            tt = timed_ms(lambda: torch.softmax(torch.nn.functional.normalize(rows.float(), dim=1) @ W.T + b, dim=1))
            ref = torch.softmax(torch.nn.functional.normalize(rows.float(), dim=1) @ W.T + b, dim=1)
            case = {"rows": n, "classes": C, "row_bytes": n * D * 2, "device_copy": copy, "predict": t, "predict_over_copy": t["median_ms"] / copy["median_ms"],
                    "predict_GBps_of_rows": n * D * 2 / t["median_ms"] / 1e6, "torch_predict": tt, "torch_over_predict": tt["median_ms"] / t["median_ms"],
                    "max_difference_to_torch": float((ref - probs).abs().max())}
            res["predict"].append(case)
            print(f"[N {n} C {C}] predict {t['median_ms']:.3f} ms = {case['predict_over_copy']:.2f} x the copy ({copy['median_ms']:.3f} ms); torch "
                  f"{tt['median_ms']:.3f} ms", flush=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
            del rows, ref, probs
            torch.cuda.empty_cache()
    print(json.dumps({"out": a.out, "fit": len(res["fit"]), "predict": len(res["predict"])}))


if __name__ == "__main__":
    main()
