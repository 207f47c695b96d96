// The two LayerNorm row forms of the encoder, each written once: every kernel that normalises a row includes this file, so the
// CLS path (final_norm_cls_kernel, cnx_pool_ln_kernel) and the all-token path (tokens_out.hip) give the same bits for the same row.
// One wave owns one row: lane l holds the 4-column groups l, l + 64, ... (NV of them); EXEC must be full at the call (wave_sum_dpp).
#pragma once
#include "common.h"

// ViT rows (vit_kernels.hip): loads the row, two-pass statistics in registers.
// Returns rstd: 0 when the variance overflowed fp32, NaN when the row holds a NaN / infinity (the range checks of the callers read it).
template <int NV>
static __device__ __forceinline__ float ln_row(const float* __restrict__ xr, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, int D, float eps, int lane, f32x4 (&y)[NV]) {
    const int nvec = D >> 2;
    f32x4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        v[k] = (idx < nvec) ? reinterpret_cast<const f32x4*>(xr)[idx] : f32x4{0.f, 0.f, 0.f, 0.f};
        s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
    }
    const float mean = wave_sum_dpp(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        if (idx < nvec) {
            const f32x4 d = v[k] - mean;
            q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum_dpp(q) / (float)D + eps);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        if (idx < nvec) {
            const f32x4 g = reinterpret_cast<const f32x4*>(gamma)[idx];
            const f32x4 bb = reinterpret_cast<const f32x4*>(beta)[idx];
            y[k] = (v[k] - mean) * rstd * g + bb;
        }
    }
    return rstd;
}

// ConvNeXt rows (convnext_f32.hip): the caller holds the row (a pixel, a window, a pooled mean).
// LayerNorm of one row held as NV f32x4 per lane (groups lane + 64 k < C / 4), the reference's two-pass form; returns rstd
// (0 when the variance overflowed fp32, NaN for a non-finite row)
template <int NV>
static __device__ __forceinline__ float cnx_ln(f32x4 (&v)[NV], int C, float eps, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, int lane) {
    const int nvec = C >> 2;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k)
        if (lane + 64 * k < nvec) s += add_np(add_np(v[k][0], v[k][1]), add_np(v[k][2], v[k][3]));
    const float mean = wave_sum_dpp(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        if (lane + 64 * k < nvec) {
#pragma clang fp contract(off)
            const f32x4 d = v[k] - mean;
            const f32x4 sq = d * d;
            q += add_np(add_np(sq[0], sq[1]), add_np(sq[2], sq[3]));
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum_dpp(q) / (float)C + eps);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        if (idx < nvec) {
#pragma clang fp contract(off)
            const f32x4 g = reinterpret_cast<const f32x4*>(gamma)[idx];
            const f32x4 b = reinterpret_cast<const f32x4*>(beta)[idx];
            v[k] = (v[k] - mean) * rstd * g + b;
        }
    }
    return rstd;
}
