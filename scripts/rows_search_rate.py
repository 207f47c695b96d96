#!/usr/bin/env python3
"""What searching resident CLS rows costs on the device, beside what a user would write without it.

D = 768 fp16 rows resident on the device; N = 180 000 (ten clips of 18 000 frames: half an hour at 10 fps each) and N = 2 000 000;
Q = 1 and Q = 16 queries; k = 20, min_gap = 15.  Each figure is timed between two ``torch.cuda.synchronize()`` calls, the median
of REPEATS after one warm-up call, every sample kept, all in this one process:
  * ``cbas_rows_search``  the whole call: clip-table check (one stream synchronisation), scores, peaks, merge
  * the score pass        the call with every row masked and min_gap = 0 costs the same scores but the cheapest selection, and the
                          selection alone cannot be called; so the split is taken from per-kernel times instead: run this script under
                          ``rocprofv3 --kernel-trace --stats`` with ``--profile-pass`` (a run of its own; nothing is written)
  * ``torch.topk``        ``topk((rows.float() @ F.normalize(q).T) / rows.float().norm(dim=1), k)``: no gap rule - the lower bound of what a
                          user would write; it materialises the fp32 copy of the rows
  * the host route        the rows copied out, float64 numpy cosines and tests/rows_search_ref.select - ONE sample, no warm-up
  * a device copy         ``dst.copy_(rows)`` of the same row bytes: the bandwidth ceiling of reading the rows once (and writing them)
GB/s figures are row bytes (N D 2) over the time named.

    python scripts/rows_search_rate.py [--out profiles/rows_search.json] [--no-host] [--profile-pass]
    python scripts/rows_search_rate.py --out profiles/rows_search.json --merge-trace KERNEL_TRACE.csv      # adds the per-kernel times
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
import rows_search_ref as R  # noqa: E402
from cbas_amd import _lib  # noqa: E402

D, K, GAP, REPEATS = 768, 20, 15, 5
CASES = [(180_000, 10), (2_000_000, 10)]                     # (rows, clips)
QS = (1, 16)


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


def search_call(lib, rows, q, table, k=K, gap=GAP):
    n, Q = rows.shape[0], q.shape[0]
    need = int(lib.cbas_rows_search_workspace_bytes(n, Q, k))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    trace = torch.empty((Q, n), device="cuda")
    index = torch.empty((Q, k), dtype=torch.int64, device="cuda")
    score = torch.empty((Q, k), device="cuda")

    def run():
        _lib.check(lib.cbas_rows_search(rows.data_ptr(), n, D, D, q.data_ptr(), Q, table.data_ptr(), table.shape[0], None, gap, 0, 0.0, k,
                                        trace.data_ptr(), index.data_ptr(), score.data_ptr(), ws.data_ptr(), need, None), "cbas_rows_search")
    return run, trace, index, score


def torch_route(rows, q):
    x = rows.float()
    s = (x @ torch.nn.functional.normalize(q, dim=1).T) / x.norm(dim=1, keepdim=True).clamp_min(1e-30)
    return torch.topk(s.T, K, dim=1)


def host_route(rows, q, table):
    trace = R.scores64(rows.cpu().numpy(), q.cpu().numpy()).astype(np.float32)
    return R.select(trace, table, None, GAP, None, K)


def merge_trace(json_path, csv_path):
    """Add the per-kernel times of a ``--profile-pass`` run under ``rocprofv3 --kernel-trace`` to the cases of ``json_path``: the pass
    makes two calls per case in the order of CASES x QS, the second call's kernels are kept.  Needs no device."""
    import csv
    with open(csv_path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "rs_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], None
    for r in rows:
        if "rs_clip_fill" in r["Kernel_Name"]:                   # the first kernel of every call
            cur = []
            calls.append(cur)
        cur.append((r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    names = [f"N{n}_Q{Q}" for n, _ in CASES for Q in QS]
    assert len(calls) == 2 * len(names), (len(calls), len(names))
    with open(json_path) as f:
        res = json.load(f)
    for name, call in zip(names, calls[1::2]):
        case = res["cases"][name]
        us = {}
        for kernel, t in call:
            short = next(s for s in ("rs_clip_fill", "rs_clip_check", "rs_qnorm", "rs_score", "rs_peaks", "rs_merge") if s in kernel)
            us[short] = us.get(short, 0.0) + t
        select_us = us["rs_peaks"] + us.get("rs_merge", 0.0)
        case["kernel_us"] = us
        case["score_kernel_GBps"] = case["row_bytes"] / us["rs_score"] / 1e3
        case["selection_us"] = select_us
        case["selection_GBps_of_rows"] = case["row_bytes"] / select_us / 1e3
        print(f"[{name}] score kernel {us['rs_score']:.1f} us = {case['score_kernel_GBps']:.0f} GB/s of rows; selection {select_us:.1f} us; "
              f"clip table {us['rs_clip_fill'] + us['rs_clip_check']:.1f} us")
    with open(json_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if "--merge-trace" in sys.argv:
        return merge_trace(out_path, sys.argv[sys.argv.index("--merge-trace") + 1])
    lib = _lib.load()
    res = {"dim": D, "k": K, "min_gap": GAP, "repeats": REPEATS, "chunk": R.CHUNK, "device": torch.cuda.get_device_name(0), "cases": {}}
    for n, clips in CASES:
        rows = make_rows(n)
        per = n // clips
        table_host = [(c * per, per if c < clips - 1 else n - c * per) for c in range(clips)]
        table = torch.tensor(table_host, dtype=torch.int64, device="cuda")
        row_bytes = n * D * 2
        for Q in QS:
            q = rows[torch.arange(Q, device="cuda") * (n // Q) + 7].float().contiguous()
            run, trace, index, score = search_call(lib, rows, q, table)
            if "--profile-pass" in sys.argv:
                run()
                torch.cuda.synchronize()
                run()
                torch.cuda.synchronize()
                continue
            dev = sample(run)
            dst = torch.empty_like(rows)
            copy = sample(lambda: dst.copy_(rows))
            del dst
            tk = sample(lambda: torch_route(rows, q))
            case = {"rows": n, "clips": clips, "queries": Q, "row_bytes": row_bytes, "cbas_rows_search": dev,
                    "search_GBps": row_bytes / dev["median_ms"] / 1e6, "device_copy": copy, "copy_GBps": row_bytes / copy["median_ms"] / 1e6,
                    "torch_topk": tk, "torch_over_search": tk["median_ms"] / dev["median_ms"]}
            line = (f"[N {n} Q {Q}] cbas_rows_search {dev['median_ms']:.3f} ms = {case['search_GBps']:.0f} GB/s of rows; copy "
                    f"{copy['median_ms']:.3f} ms = {case['copy_GBps']:.0f} GB/s; torch.topk route {tk['median_ms']:.3f} ms")
            if "--no-host" not in sys.argv and n <= 200_000:
                host_ms = timed_ms(lambda: host_route(rows, q, table_host))
                want = host_route(rows, q, table_host)
                run()
                torch.cuda.synchronize()
                agree = float((index.cpu().numpy() == want[0]).mean())      # float64 scores may order near-ties differently
                case.update(host_route_ms=host_ms, host_over_search=host_ms / dev["median_ms"], host_index_agreement=agree)
                line += f"; host route {host_ms:.0f} ms (indices agree {agree:.3f})"
            res["cases"][f"N{n}_Q{Q}"] = case
            print(line, flush=True)
        del rows
        torch.cuda.empty_cache()
    if "--profile-pass" in sys.argv:
        return
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({c: {k: v for k, v in r.items() if not isinstance(v, dict)} for c, r in res["cases"].items()}))


if __name__ == "__main__":
    main()
