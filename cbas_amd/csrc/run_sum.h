// The one summation of per-frame confidences over a run of frames: head_report_kernels.hip (cbas_disagreement_runs) and
// head_post_kernels.hip (cbas_label_runs) both report a run's mean confidence through it, so equal runs give equal bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Called by all 64 lanes of a wave.  Lane l adds conf[first + l], conf[first + l + 64], ... up to `last` in ascending order in
// float64; a fixed butterfly combines the 64 partial sums (a + b == b + a: every lane returns the same bits).  `last < first`
// gives 0.  No atomics: the value depends on the run alone.
__device__ __forceinline__ double run_conf_sum(const float* __restrict__ conf, int64_t first, int64_t last, int lane) {
    double sum = 0.0;
    for (int64_t f = first + lane; f <= last; f += 64) sum += (double)conf[f];
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    return sum;
}
