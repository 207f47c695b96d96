// The reciprocal norm of a resident fp16 row, written once: rows_search.hip, rows_knn.hip, rows_kmeans.hip, rows_probe.hip and
// rows_pca.hip all include this file, so the same row has the same rn in each.  s = (l0 + l1) + (l2 + l3) in fp32, l_j the fmaf
// chain, from 0, of x_d^2 over the columns d with (d % 32) / 8 = j, ascending; rn = fp32(1 / sqrt((double)s)), 0 when s = 0.
#pragma once
#include "common.h"

static __device__ __forceinline__ float rows_rn(float s) { return s > 0.f ? (float)(1.0 / sqrt((double)s)) : 0.f; }

// l_j continued over the 8 halves a lane of column group j holds of one 32-column block
static __device__ __forceinline__ float rows_ss8(const f16x8 h, float ss) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = (float)h[e];
        ss = fmaf(v, v, ss);
    }
    return ss;
}

// rn of every row: 4 lanes a row, lane j the chain l_j.  grid (ceil(4 n / 256)), 256 threads
static __global__ __launch_bounds__(256) void rows_rn_kernel(const uint16_t* __restrict__ x, int64_t n, int D, int64_t ld, float* __restrict__ rn) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, row = gid >> 2;
    const int kr = (int)(gid & 3);
    float ss = 0.f;
    if (row < n) {
        const uint16_t* const p = x + row * ld + 8 * kr;
        for (int c = 0; c < (D >> 5); ++c) ss = rows_ss8(__builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(p + 32 * c)), ss);
    }
    ss += __shfl_xor(ss, 1, 64);                     // (l0 + l1) and (l2 + l3), then their sum: the same bits in all four
    ss += __shfl_xor(ss, 2, 64);
    if (row < n && kr == 0) rn[row] = rows_rn(ss);
}
