// DINOv3 ConvNeXt encoders (transformers models/dinov3_convnext, "[cx]" = modeling_dinov3_convnext.py) in precision 3 and 4:
// the element-wise and spatial steps the ViT does not have.  Every contraction of the model that is a matrix product (the
// 4x4 / stride-4 stem, the 2x2 / stride-2 downsamples, pointwise_conv1 / pointwise_conv2) runs on the ViT's fp32 GEMMs
// (vit_f32.hip; in precision 4 the split-operand forms), so these kernels are the GEMMs' producers and the model's tail:
//
//   cnx_stem_im2col_kernel   green plane (u8: px / 255.0 in double, then float; or f32) -> A [pixels][32]: the 4 x 4 patch at
//                            k = 4 i + j, k >= 16 zero.  The 3 identical input channels are folded into the packed weight
//                            exactly as the ViT's patch weight is (summed in double, rounded once)             [cx] stage 0
//   cnx_ln_rows_kernel       channels-first LayerNorm after the stem, in place on the residual stream          [cx] stage 0
//   cnx_downsample_kernel    LayerNorm of each of the 4 input pixels of a 2 x 2 / stride-2 window, written as one A row of
//                            K = 4 C ([kh][kw][c] order; the weight is repacked to match at create)           [cx] stages 1-3
//   cnx_dwconv_ln_kernel     depthwise 7 x 7 (pad 3, groups = C) + bias, then LayerNorm(C): pointwise_conv1's A operand
//   cnx_pool_ln_kernel       AdaptiveAvgPool2d(1) + the final LayerNorm, row 0 only; counts non-finite rows as
//                            final_norm_cls_kernel does (the range check of precision 4)
//
// Activations are channels-last fp32 rows (frame, y, x) with a row stride ld >= C (the residual stream is padded to a multiple
// of 128 columns so that every GEMM's N meets the 128-column tile; the padding columns stay zero).  One wave owns one pixel
// row: lane l holds the 4-channel groups l, l + 64, ... (NV of them), and LayerNorm is two-pass in registers like
// layernorm_f32_kernel.  In precision 4 the producers write their GEMM operand in the split hi | lo tile format
// (vit32_epilogue.h store_split4) at scale 1.
#include "kernels.h"
#include "vit32_epilogue.h"
#include "row_norm.h"

namespace {

// one thread = one output pixel of the stem: 16 pixels in, 32 floats out (plain or split)
template <typename SRC>
__global__ void cnx_stem_im2col_kernel(const SRC* __restrict__ frames, int n, int64_t frame_stride, int64_t row_stride,
                                       int64_t pixel_stride, int ho, int wo, float* __restrict__ A, int split) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= (int64_t)n * ho * wo) return;
    const int ox = (int)(m % wo);
    const int64_t t = m / wo;
    const int oy = (int)(t % ho);
    const int b = (int)(t / ho);
    const SRC* src = frames + b * frame_stride + (int64_t)(4 * oy) * row_stride + (int64_t)(4 * ox) * pixel_stride;
    float* dst = A + m * 32;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const SRC px = src[(int64_t)q * row_stride + (int64_t)e * pixel_stride];
                if (sizeof(SRC) == 1) v[e] = (float)((double)px / 255.0);     // numpy: uint8 / 255.0 -> float64; .float()
                else v[e] = (float)px;
            }
        }
        if (split) store_split4(dst, q * 4, v, 1.0f);
        else reinterpret_cast<f32x4*>(dst)[q] = v;
    }
}

template <int NV>
__global__ __launch_bounds__(256) void cnx_ln_rows_kernel(float* __restrict__ x, int64_t ld, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int64_t M, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float* xr = x + row * ld;
    const int nvec = C >> 2;
    f32x4 v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        v[k] = idx < nvec ? reinterpret_cast<const f32x4*>(xr)[idx] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    cnx_ln<NV>(v, C, eps, gamma, beta, lane);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        if (idx < nvec) reinterpret_cast<f32x4*>(xr)[idx] = v[k];
    }
}

// one wave = one of the 4 input pixels (q = 2 kh + kw) of output pixel m; output rows of n x ho x wo pixels, K = 4 C
template <int NV>
__global__ __launch_bounds__(256) void cnx_downsample_kernel(const float* __restrict__ x, int64_t ldx, int hi, int wi, int n, int ho,
                                                             int wo, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             int C, float eps, float* __restrict__ A, int split) {
    const int lane = threadIdx.x & 63;
    const int q = threadIdx.x >> 6;
    const int64_t m = blockIdx.x;
    if (m >= (int64_t)n * ho * wo) return;
    const int ox = (int)(m % wo);
    const int64_t t = m / wo;
    const int oy = (int)(t % ho);
    const int b = (int)(t / ho);
    const int iy = 2 * oy + (q >> 1), ix = 2 * ox + (q & 1);      // odd hi / wi: the last row / column is never read
    const float* xr = x + (((int64_t)b * hi + iy) * wi + ix) * ldx;
    const int nvec = C >> 2;
    f32x4 v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        v[k] = idx < nvec ? reinterpret_cast<const f32x4*>(xr)[idx] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    cnx_ln<NV>(v, C, eps, gamma, beta, lane);
    float* dst = A + m * 4 * C;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        if (idx < nvec) {
            if (split) store_split4(dst, q * C + idx * 4, v[k], 1.0f);
            else reinterpret_cast<f32x4*>(dst + q * C)[idx] = v[k];
        }
    }
}

// Depthwise 7 x 7 + bias + LayerNorm.  A workgroup = 4 waves = 4 consecutive pixels of one image row; the 7 x (4 + 6) input
// window of a channel group is read once per wave from L1 / L2 with 16-byte loads along the channels (taps outside the frame are
// skipped - the zero padding; frames never bleed into each other).  wt: the taps repacked tap-major, [49][C].
template <int NV>
__global__ __launch_bounds__(256) void cnx_dwconv_ln_kernel(const float* __restrict__ x, int64_t ld, int n, int hh, int ww,
                                                            const float* __restrict__ wt, const float* __restrict__ bias,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, int C,
                                                            float eps, float* __restrict__ A, int split) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= (int64_t)n * hh * ww) return;
    const int px = (int)(m % ww);
    const int64_t t = m / ww;
    const int py = (int)(t % hh);
    const int64_t fbase = (t / hh) * hh * ww;                  // first pixel of the frame
    const int nvec = C >> 2;
    const int y0 = py - 3 < 0 ? 0 : py - 3, y1 = py + 3 >= hh ? hh - 1 : py + 3;
    const int x0 = px - 3 < 0 ? 0 : px - 3, x1 = px + 3 >= ww ? ww - 1 : px + 3;
    f32x4 v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (idx < nvec) {
            for (int yy = y0; yy <= y1; ++yy) {
                const float* xrow = x + (fbase + (int64_t)yy * ww) * ld + idx * 4;
                const float* wrow = wt + (size_t)((yy - py + 3) * 7) * C + idx * 4;
                for (int xx = x0; xx <= x1; ++xx) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(xrow + (int64_t)xx * ld);
                    const f32x4 w = *reinterpret_cast<const f32x4*>(wrow + (size_t)(xx - px + 3) * C);
                    acc = __builtin_elementwise_fma(w, a, acc);
                }
            }
            acc = acc + reinterpret_cast<const f32x4*>(bias)[idx];
        }
        v[k] = acc;
    }
    cnx_ln<NV>(v, C, eps, gamma, beta, lane);
    float* dst = A + m * C;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        if (idx < nvec) {
            if (split) store_split4(dst, idx * 4, v[k], 1.0f);
            else reinterpret_cast<f32x4*>(dst)[idx] = v[k];
        }
    }
}

// One workgroup per frame: wave w sums pixels w, w + 4, ... in order; wave 0 adds the four partial sums in order, divides by
// the pixel count (the mean of AdaptiveAvgPool2d(1)) and applies the final LayerNorm.  Per frame only: batch-invariant.
template <int NV>
__global__ __launch_bounds__(256) void cnx_pool_ln_kernel(const float* __restrict__ x, int64_t ld, int hw, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int C, float eps, float* __restrict__ cls_f32,
                                                          f16* __restrict__ cls_f16, unsigned* __restrict__ nonfinite) {
    __shared__ f32x4 part[4][NV * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const int nvec = C >> 2;
    const float* xf = x + (int64_t)b * hw * ld;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        if (idx < nvec)
            for (int p = wave; p < hw; p += 4) s = s + reinterpret_cast<const f32x4*>(xf + (int64_t)p * ld)[idx];
        part[wave][idx] = s;
    }
    __syncthreads();
    if (wave) return;
    f32x4 v[NV];
    const float inv = (float)hw;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        v[k] = (((part[0][idx] + part[1][idx]) + part[2][idx]) + part[3][idx]) / inv;
    }
    const float rstd = cnx_ln<NV>(v, C, eps, gamma, beta, lane);
    if (nonfinite) {
        bool bad = !(rstd > 0.f);          // an overflowed variance gives rstd = 0 and a finite row (beta)
#pragma unroll
        for (int k = 0; k < NV; ++k)
            if (lane + 64 * k < nvec) {
                const f32x4 a = __builtin_elementwise_abs(v[k]);
                bad |= !(a[0] <= 3.0e38f && a[1] <= 3.0e38f && a[2] <= 3.0e38f && a[3] <= 3.0e38f);
            }
        if (__ballot(bad) && lane == 0) atomicAdd(nonfinite, 1u);
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        if (idx < nvec) {
            if (cls_f32) reinterpret_cast<f32x4*>(cls_f32 + (size_t)b * C)[idx] = v[k];
            if (cls_f16) {
                f16x4 h = {(f16)v[k][0], (f16)v[k][1], (f16)v[k][2], (f16)v[k][3]};   // round-to-nearest-even, as h5py's f4->f2 cast
                reinterpret_cast<f16x4*>(cls_f16 + (size_t)b * C)[idx] = h;
            }
        }
    }
}

#define CNX_NV_SWITCH(nv, KERNEL, ...)                                                     \
    switch (nv) {                                                                          \
        case 1: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break;                         \
        case 2: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break;                         \
        case 3: hipLaunchKernelGGL(KERNEL<3>, __VA_ARGS__); break;                         \
        case 4: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break;                         \
        case 5: hipLaunchKernelGGL(KERNEL<5>, __VA_ARGS__); break;                         \
        case 6: hipLaunchKernelGGL(KERNEL<6>, __VA_ARGS__); break;                         \
        default: return -1;                                                                \
    }

inline int cnx_nv(int C) { return (C / 4 + 63) / 64; }
inline int cnx_ok(int C) { return C > 0 && C % 32 == 0 && C <= 1536; }

}  // namespace

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -2)

int launch_cnx_stem_im2col_u8(const uint8_t* frames, int n, int height, int width, int64_t frame_stride, int64_t row_stride,
                              int64_t pixel_stride, float* A, int split, hipStream_t stream) {
    const int ho = height / 4, wo = width / 4;
    const int64_t total = (int64_t)n * ho * wo;
    if (n <= 0 || height < 4 || width < 4 || frame_stride <= 0 || row_stride <= 0 || pixel_stride <= 0) return -1;
    hipLaunchKernelGGL(cnx_stem_im2col_kernel<uint8_t>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, frames, n,
                       frame_stride, row_stride, pixel_stride, ho, wo, A, split);
    return CHECK_LAUNCH();
}

int launch_cnx_stem_im2col_f32(const float* frames, int n, int height, int width, float* A, int split, hipStream_t stream) {
    const int ho = height / 4, wo = width / 4;
    const int64_t total = (int64_t)n * ho * wo;
    if (n <= 0 || height < 4 || width < 4) return -1;
    hipLaunchKernelGGL(cnx_stem_im2col_kernel<float>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, frames, n,
                       (int64_t)height * width, (int64_t)width, (int64_t)1, ho, wo, A, split);
    return CHECK_LAUNCH();
}

int launch_cnx_ln_rows(float* x, int64_t ld, const float* gamma, const float* beta, int64_t M, int C, float eps, hipStream_t stream) {
    if (!cnx_ok(C) || ld < C || M <= 0) return -1;
    CNX_NV_SWITCH(cnx_nv(C), cnx_ln_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, x, ld, gamma, beta, M, C, eps);
    return CHECK_LAUNCH();
}

int launch_cnx_downsample(const float* x, int64_t ldx, int n, int hi, int wi, const float* gamma, const float* beta, int C, float eps,
                          float* A, int split, hipStream_t stream) {
    const int ho = hi / 2, wo = wi / 2;
    const int64_t M = (int64_t)n * ho * wo;
    if (!cnx_ok(C) || ldx < C || n <= 0 || hi < 2 || wi < 2 || M > 0x7fffffff) return -1;
    CNX_NV_SWITCH(cnx_nv(C), cnx_downsample_kernel, dim3((unsigned)M), dim3(256), 0, stream, x, ldx, hi, wi, n, ho, wo, gamma, beta, C,
                  eps, A, split);
    return CHECK_LAUNCH();
}

int launch_cnx_dwconv_ln(const float* x, int64_t ld, int n, int hh, int ww, const float* wt, const float* bias, const float* gamma,
                         const float* beta, int C, float eps, float* A, int split, hipStream_t stream) {
    const int64_t M = (int64_t)n * hh * ww;
    if (!cnx_ok(C) || ld < C || n <= 0 || hh <= 0 || ww <= 0) return -1;
    CNX_NV_SWITCH(cnx_nv(C), cnx_dwconv_ln_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, x, ld, n, hh, ww, wt, bias, gamma,
                  beta, C, eps, A, split);
    return CHECK_LAUNCH();
}

int launch_cnx_pool_ln(const float* x, int64_t ld, int n, int hw, const float* gamma, const float* beta, int C, float eps,
                       float* cls_f32, f16* cls_f16, unsigned* nonfinite, hipStream_t stream) {
    if (!cnx_ok(C) || ld < C || n <= 0 || hw <= 0) return -1;
    CNX_NV_SWITCH(cnx_nv(C), cnx_pool_ln_kernel, dim3((unsigned)n), dim3(256), 0, stream, x, ld, hw, gamma, beta, C, eps, cls_f32,
                  cls_f16, nonfinite);
    return CHECK_LAUNCH();
}
