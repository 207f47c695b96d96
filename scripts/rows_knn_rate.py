#!/usr/bin/env python3
"""What labelling every resident frame from its nearest labelled frames costs on the device, beside what a user would write without it.

D = 768 fp16 rows resident on the device, k = 20, T = 0.07, C = 8; N = 180 000 and N = 2 000 000 store rows against banks of
M = 1 024, 8 192 and 65 536 labelled rows.  Each figure is timed between two ``torch.cuda.synchronize()`` calls, the median of REPEATS
after one warm-up call, every sample kept, all in this one process:
  * ``cbas_rows_knn``   the whole call: label check and reciprocal norms (one stream synchronisation), then the fused pass.  Its
                        FLOP/s are 2 N M D over the time, set against the 2.5 PFLOP/s dense fp16 peak of the MI355X
  * the torch route     row slabs of an fp16 ``matmul`` against the normalised bank (a slab's similarities are at most 512 MB), then
                        ``topk``, ``exp`` and ``index_add_``; when its warm-up call takes over 5 s, one sample instead of REPEATS
  * a device copy       ``dst.copy_(rows)`` of the same row bytes

    python scripts/rows_knn_rate.py [--out profiles/rows_knn.json]
"""
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cbas_amd import _lib, knn  # noqa: E402

D, K, T, C, REPEATS = 768, 20, 0.07, 8, 5
NS = (180_000, 2_000_000)
MS = (1024, 8192, 65536)
PEAK_F16 = 2.5e15


def timed_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def sample(fn, slow_ms=None):
    warm = timed_ms(fn)
    s = [timed_ms(fn) for _ in range(1 if slow_ms is not None and warm > slow_ms else REPEATS)]
    return {"median_ms": statistics.median(s), "samples_ms": s}


def make_rows(n):
    """Random fp16 rows that drift slowly (neighbouring frames alike, as video is), made on the device in blocks."""
    g = torch.Generator(device="cuda").manual_seed(n)
    rows = torch.empty((n, D), dtype=torch.float16, device="cuda")
    base = torch.randn(D, device="cuda", generator=g)
    for a in range(0, n, 1 << 16):
        b = min(n, a + (1 << 16))
        step = torch.randn((b - a, D), device="cuda", generator=g) * 0.05
        walk = base + torch.cumsum(step, 0)
        rows[a:b] = (walk + 0.3 * torch.randn((b - a, D), device="cuda", generator=g)).half()
        base = walk[-1] * 0.9
    return rows


def knn_call(lib, rows, bank, labels):
    n, M = rows.shape[0], bank.shape[0]
    need = int(lib.cbas_rows_knn_workspace_bytes(n, M, K))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    probs = torch.empty((n, C), device="cuda")

    def run():
        _lib.check(lib.cbas_rows_knn(rows.data_ptr(), n, D, D, bank.data_ptr(), M, D, labels.data_ptr(), None, None, C, None, K, T, probs.data_ptr(),
                                     None, None, None, ws.data_ptr(), need, None), "cbas_rows_knn")
    return run, probs


def torch_route(rows, bank, labels):
    n, M = rows.shape[0], bank.shape[0]
    bn = torch.nn.functional.normalize(bank.float(), dim=1).half()
    lab = labels.long()
    probs = torch.zeros((n, C), device="cuda")
    slab = max(1, min(n, (1 << 28) // M))
    for a in range(0, n, slab):
        x = rows[a:a + slab]
        s = (x @ bn.T).float() / x.float().norm(dim=1, keepdim=True).clamp_min(1e-30)
        top = torch.topk(s, min(K, M), dim=1)
        w = torch.exp((top.values - top.values[:, :1]) / T)
        at = (torch.arange(a, a + x.shape[0], device="cuda")[:, None] * C + lab[top.indices]).reshape(-1)
        probs.view(-1).index_add_(0, at, w.reshape(-1))
    return probs / probs.sum(dim=1, keepdim=True)


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lib = _lib.load()
    res = {"dim": D, "k": K, "temperature": T, "classes": C, "repeats": REPEATS, "tile": knn.TILE, "block": knn.BLOCK, "peak_f16_flops": PEAK_F16,
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for n in NS:
        rows = make_rows(n)
        row_bytes = n * D * 2
        dst = torch.empty_like(rows)
        copy = sample(lambda: dst.copy_(rows))
        del dst
        for M in MS:
            pick = torch.arange(M, device="cuda") * (n // M) + 3
            bank = rows[pick].contiguous()
            labels = (torch.arange(M, device="cuda") * C // M).int()
            run, probs = knn_call(lib, rows, bank, labels)
            dev = sample(run)
            flops = 2.0 * n * M * D
            tr = sample(lambda: torch_route(rows, bank, labels), slow_ms=5000.0)
            run()
            agree = float((probs.argmax(1) == torch_route(rows, bank, labels).argmax(1)).float().mean())
            case = {"rows": n, "bank": M, "row_bytes": row_bytes, "flop": flops, "cbas_rows_knn": dev, "knn_TFLOPs": flops / dev["median_ms"] / 1e9,
                    "knn_of_f16_peak": flops / (dev["median_ms"] * 1e-3) / PEAK_F16, "torch_route": tr,
                    "torch_over_knn": tr["median_ms"] / dev["median_ms"], "top1_agreement_with_torch": agree, "device_copy": copy}
            res["cases"][f"N{n}_M{M}"] = case
            print(f"[N {n} M {M}] cbas_rows_knn {dev['median_ms']:.3f} ms = {case['knn_TFLOPs']:.0f} TFLOP/s ({100 * case['knn_of_f16_peak']:.1f} % of "
                  f"peak); torch route {tr['median_ms']:.3f} ms ({case['torch_over_knn']:.2f} x); copy {copy['median_ms']:.3f} ms; top-1 agree "
                  f"{agree:.4f}", flush=True)
            if out_path:                                       # after every case: a partial file survives a time limit
                with open(out_path, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")
        del rows
        torch.cuda.empty_cache()
    print(json.dumps({c: {k: v for k, v in r.items() if not isinstance(v, dict)} for c, r in res["cases"].items()}))


if __name__ == "__main__":
    main()
