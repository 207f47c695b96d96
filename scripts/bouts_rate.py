"""The rate of the Viterbi decode -> profiles/bouts.json.

2 000 000 frames of random probabilities as 111 clips of 18 000 frames (the last one shorter) and as one clip, C = 9, 16, 64,
sticky transitions with a mean bout of 40 frames; medians of five synchronised calls after a warm-up.

  * the decode        cbasx_viterbi_decode on scores that are already there (it synchronises once itself, to read its refusals)
  * the scores        cbasx_viterbi_scores, beside a device copy of the same probability bytes: the floor for one read
  * the host route    bouts.viterbi_host (numpy) on the first 100 000 frames - ONE sample, no warm-up; scale by 20 for the store
  * the torch route   a per-step loop of torch calls on the device (max and argmax over (C, C)) on the same 100 000 frames, forward pass
                      only - ONE sample after a 1 000-step warm-up

    python scripts/bouts_rate.py [--out profiles/bouts.json] [--no-host]
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

from cbas_amd import _lib, bouts  # noqa: E402

N, CLIP, SLICE = 2_000_000, 18_000, 100_000


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


def once_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def torch_forward(scores, A):
    """The forward pass as a loop of torch calls: what a user without the kernel would write on the device."""
    d = scores[0].to(torch.int64)
    A = A.to(torch.int64)
    bp = torch.empty(scores.shape, dtype=torch.uint8, device=scores.device)
    for t in range(1, scores.shape[0]):
        m, arg = (d[:, None] + A).max(dim=0)
        bp[t] = arg
        d = m + scores[t]
    return d, bp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bouts.json"))
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    lib, dev = _lib.load(), torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    firsts = np.arange(0, N, CLIP, dtype=np.int64)
    stores = {"111_clips_of_18000": np.stack([firsts, np.minimum(CLIP, N - firsts)], axis=1), "one_clip": np.array([[0, N]], np.int64)}
    result = {"frames": N, "chunk": bouts.CHUNK, "device": _lib.device_info(0)[0], "cases": []}
    for C in (9, 16, 64):
        g = torch.Generator(device=dev).manual_seed(C)
        probs = torch.softmax(3.0 * torch.randn((N, C), generator=g, device=dev), dim=1).contiguous()
        scores = torch.empty((N, C), dtype=torch.int32, device=dev)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        copy = torch.empty_like(probs)
        A = torch.from_numpy(bouts.sticky_transitions(C, mean_duration=40)).to(dev)
        t_scores = timed_ms(lambda: _lib.check(lib.cbasx_viterbi_scores(probs.data_ptr(), N, C, scores.data_ptr(), flags.data_ptr(), stream), "scores"))
        t_copy = timed_ms(lambda: copy.copy_(probs))
        entry = {"C": C, "scores": t_scores, "device_copy_same_bytes": t_copy, "stores": {}}
        for name, table in stores.items():
            table_dev = torch.from_numpy(table).to(dev)
            need = int(lib.cbasx_viterbi_workspace_bytes(N, len(table), C))
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            labels = torch.empty(N, dtype=torch.int32, device=dev)
            clip_score = torch.empty(len(table), dtype=torch.int64, device=dev)
            t = timed_ms(lambda: _lib.check(lib.cbasx_viterbi_decode(scores.data_ptr(), N, table_dev.data_ptr(), len(table), C, A.data_ptr(), None,
                                                                     labels.data_ptr(), clip_score.data_ptr(), ws.data_ptr(), need, stream), "decode"))
            t["workspace_bytes"] = need
            t["frames_per_s"] = N / (t["median_ms"] * 1e-3)
            entry["stores"][name] = t
            del ws
        small = scores[:SLICE].contiguous()
        torch_forward(small[:1000], A)
        entry["torch_loop_forward_only"] = {"frames": SLICE, "ms": once_ms(lambda: torch_forward(small, A)), "samples": 1}
        if not a.no_host:
            host, A_host = small.cpu().numpy(), A.cpu().numpy()
            t0 = time.perf_counter()
            bouts.viterbi_host(host, [(0, SLICE)], A_host)
            entry["numpy_host"] = {"frames": SLICE, "ms": (time.perf_counter() - t0) * 1e3, "samples": 1}
        result["cases"].append(entry)
        print(json.dumps(entry), flush=True)
        del probs, scores, copy
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
