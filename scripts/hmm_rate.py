"""The rate of the forward-backward pass -> profiles/hmm.json.

2 000 000 frames of random probabilities as 111 clips of 18 000 frames (the last one shorter) and as one clip, C = 9, 16, 64,
sticky transitions with a mean bout of 40 frames; medians of five synchronised calls after a warm-up.

  * the posteriors    cbasx_hmm_posteriors with and without the sums (xi / pi / loglik NULL); it synchronises once itself, to read
                      its refusals
  * the decode        cbasx_viterbi_decode of the same shape, on scores that are already there
  * the copy          a device copy of the same probability bytes: the floor for one read and one write
  * the host route    bouts.posteriors_host (numpy, float64) on the first 100 000 frames - ONE sample, no warm-up
  * the torch route   a per-step loop of torch calls on the device, forward and backward recursion without the counts, on the same
                      100 000 frames - ONE sample after a 1 000-step warm-up

    python scripts/hmm_rate.py [--out profiles/hmm.json] [--no-host]
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


def torch_forward_backward(probs, A):
    """Both recursions as loops of torch calls: what a user without the kernel would write on the device."""
    T, C = probs.shape
    b = probs.clamp(min=2.0 ** -32)
    alpha = torch.empty_like(b)
    a = b[0] / C
    alpha[0] = a / a.sum()
    for t in range(1, T):
        a = (alpha[t - 1] @ A) * b[t]
        alpha[t] = a / a.sum()
    beta = torch.ones(C, device=probs.device)
    gamma = torch.empty_like(b)
    gamma[T - 1] = alpha[T - 1]
    for t in range(T - 2, -1, -1):
        beta = A @ (b[t + 1] * beta)
        beta = beta / beta.max()
        g = alpha[t] * beta
        gamma[t] = g / g.sum()
    return gamma


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmm.json"))
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    lib, dev = _lib.load(), torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    firsts = np.arange(0, N, CLIP, dtype=np.int64)
    stores = {"111_clips_of_18000": np.stack([firsts, np.minimum(CLIP, N - firsts)], axis=1), "one_clip": np.array([[0, N]], np.int64)}
    result = {"frames": N, "chunk": bouts.HMM_CHUNK, "device": _lib.device_info(0)[0], "cases": []}
    for C in (9, 16, 64):
        g = torch.Generator(device=dev).manual_seed(C)
        probs = torch.softmax(3.0 * torch.randn((N, C), generator=g, device=dev), dim=1).contiguous()
        gamma = torch.empty_like(probs)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        A = torch.from_numpy(bouts.sticky_transitions(C, mean_duration=40, as_probs=True)).to(dev)
        A_scores = torch.from_numpy(bouts.sticky_transitions(C, mean_duration=40)).to(dev)
        entry = {"C": C, "device_copy_same_bytes": timed_ms(lambda: gamma.copy_(probs)), "stores": {}}
        scores = torch.empty((N, C), dtype=torch.int32, device=dev)
        _lib.check(lib.cbasx_viterbi_scores(probs.data_ptr(), N, C, scores.data_ptr(), flags.data_ptr(), stream), "scores")
        for name, table in stores.items():
            table_dev = torch.from_numpy(table).to(dev)
            need = int(lib.cbasx_hmm_workspace_bytes(N, len(table), C))
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            xi = torch.empty((C, C), dtype=torch.float64, device=dev)
            pi = torch.empty(C, dtype=torch.float64, device=dev)
            loglik = torch.empty(len(table), dtype=torch.float64, device=dev)

            def call(sums):
                _lib.check(lib.cbasx_hmm_posteriors(probs.data_ptr(), N, table_dev.data_ptr(), len(table), C, A.data_ptr(), None, gamma.data_ptr(),
                                                    xi.data_ptr() if sums else None, pi.data_ptr() if sums else None,
                                                    loglik.data_ptr() if sums else None, flags.data_ptr(), ws.data_ptr(), need, stream), "posteriors")
            case = {"workspace_bytes": need}
            for key, sums in (("gamma_and_sums", True), ("gamma_only", False)):
                t = timed_ms(lambda: call(sums))
                t["frames_per_s"] = N / (t["median_ms"] * 1e-3)
                case[key] = t
            call(True)
            case["loglik_bits_total"] = float(loglik.sum())
            del ws
            need = int(lib.cbasx_viterbi_workspace_bytes(N, len(table), C))
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            labels = torch.empty(N, dtype=torch.int32, device=dev)
            t = timed_ms(lambda: _lib.check(lib.cbasx_viterbi_decode(scores.data_ptr(), N, table_dev.data_ptr(), len(table), C, A_scores.data_ptr(), None,
                                                                     labels.data_ptr(), None, ws.data_ptr(), need, stream), "decode"))
            t["frames_per_s"] = N / (t["median_ms"] * 1e-3)
            case["viterbi_decode_same_shape"] = t
            entry["stores"][name] = case
            del ws, labels
        del scores
        small = probs[:SLICE].contiguous()
        torch_forward_backward(small[:1000], A)
        entry["torch_loop"] = {"frames": SLICE, "ms": once_ms(lambda: torch_forward_backward(small, A)), "samples": 1}
        if not a.no_host:
            host, A_host = small.cpu().numpy(), A.cpu().numpy()
            t0 = time.perf_counter()
            bouts.posteriors_host(host, [(0, SLICE)], A_host)
            entry["numpy_host_float64"] = {"frames": SLICE, "ms": (time.perf_counter() - t0) * 1e3, "samples": 1}
        result["cases"].append(entry)
        print(json.dumps(entry), flush=True)
        del probs, gamma
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
