// Every token's final hidden state (transformers' last_hidden_state) and patch similarity maps.  The forward keeps the fp32
// residual stream of every token in HBM until its last layer; the CLS path normalises row 0 of each frame only
// (final_norm_cls_kernel, cnx_pool_ln_kernel).  These kernels write the whole (n, T, D) image instead:
//
//   final_norm_rows_kernel    ViT: out[r] = LayerNorm(x[r]) for all M = n T rows                            [tf]:540
//   copy_rows_kernel          ViT: out[r] = x[r], the raw rows of any layer (transformers' hidden_states[l])
//   cnx_token_rows_kernel     ConvNeXt: out[b][0] = LayerNorm(mean over the hw pixels), out[b][1 + p] = LayerNorm(x[b][p])
//                             (DINOv3ConvNextModel.forward: pool, concatenate, then ONE LayerNorm over every row)
//   token_similarity_kernel   map[b][p] = cos(out[b][q_b], out[b][P0 + p]) over the patch rows
//
// All three are bandwidth-bound row kernels: one wave per row, lane l holds the 4-column groups l, l + 64, ..., fp32 rows are
// read and written as 16-byte vectors (fp16 rows: 8 bytes per lane, 512 contiguous bytes per wave instruction).  The rows are
// normalised by ln_row / cnx_ln of row_norm.h - the code the CLS kernels run - and the pooled mean is summed in
// cnx_pool_ln_kernel's order, so row 0 of every frame has the bits the CLS path gives.  A row that comes out non-finite (or whose
// variance overflowed) adds one to `nonfinite`: one per ROW here, where the CLS kernels count one per frame.
#include "kernels.h"
#include "row_norm.h"

namespace {

// the range check of final_norm_cls_kernel on a normalised row
template <int NV>
__device__ __forceinline__ void count_nonfinite(float rstd, const f32x4 (&y)[NV], int nvec, int lane, unsigned* __restrict__ nonfinite) {
    if (!nonfinite) return;
    bool bad = !(rstd > 0.f);
#pragma unroll
    for (int k = 0; k < NV; ++k)
        if (lane + 64 * k < nvec) {
            const f32x4 a = __builtin_elementwise_abs(y[k]);
            bad |= !(a[0] <= 3.0e38f && a[1] <= 3.0e38f && a[2] <= 3.0e38f && a[3] <= 3.0e38f);
        }
    if (__ballot(bad) && lane == 0) atomicAdd(nonfinite, 1u);
}

template <int NV>
__device__ __forceinline__ void store_row(const f32x4 (&y)[NV], float* __restrict__ o32, f16* __restrict__ o16, int nvec, int lane) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        if (idx < nvec) {
            if (o32) reinterpret_cast<f32x4*>(o32)[idx] = y[k];
            if (o16) {
                f16x4 h = {(f16)y[k][0], (f16)y[k][1], (f16)y[k][2], (f16)y[k][3]};   // round-to-nearest-even, as the CLS rows
                reinterpret_cast<f16x4*>(o16)[idx] = h;
            }
        }
    }
}

template <int NV>
__global__ __launch_bounds__(256) void final_norm_rows_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* __restrict__ out_f32,
                                                              f16* __restrict__ out_f16, int64_t ld_out, int64_t M, int D, float eps,
                                                              unsigned* __restrict__ nonfinite) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    f32x4 y[NV];
    const float rstd = ln_row<NV>(x + row * ldx, gamma, beta, D, eps, lane, y);
    count_nonfinite<NV>(rstd, y, D >> 2, lane, nonfinite);
    store_row<NV>(y, out_f32 ? out_f32 + row * ld_out : nullptr, out_f16 ? out_f16 + row * ld_out : nullptr, D >> 2, lane);
}

// The raw rows of the residual stream (transformers' hidden_states[l]: no LayerNorm): one wave per row, 16-byte loads, the same
// stores and the same range check on the values themselves.
__global__ __launch_bounds__(256) void copy_rows_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ out_f32,
                                                        f16* __restrict__ out_f16, int64_t ld_out, int64_t M, int D,
                                                        unsigned* __restrict__ nonfinite) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + row * ldx;
    float* o32 = out_f32 ? out_f32 + row * ld_out : nullptr;
    f16* o16 = out_f16 ? out_f16 + row * ld_out : nullptr;
    bool bad = false;
    for (int idx = lane; idx < (D >> 2); idx += 64) {
        const f32x4 v = reinterpret_cast<const f32x4*>(xr)[idx];
        const f32x4 a = __builtin_elementwise_abs(v);
        bad |= !(a[0] <= 3.0e38f && a[1] <= 3.0e38f && a[2] <= 3.0e38f && a[3] <= 3.0e38f);
        if (o32) reinterpret_cast<f32x4*>(o32)[idx] = v;
        if (o16) {
            f16x4 hv = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};      // round-to-nearest-even
            reinterpret_cast<f16x4*>(o16)[idx] = hv;
        }
    }
    if (nonfinite && __ballot(bad) && lane == 0) atomicAdd(nonfinite, 1u);
}

// grid (1 + ceil(hw / 4), n).  Block 0 of a frame is cnx_pool_ln_kernel's workgroup (wave w sums pixels w, w + 4, ... in order;
// wave 0 adds the four partial sums in order and divides by hw) and writes row 0; every other block normalises four pixels.
template <int NV>
__global__ __launch_bounds__(256) void cnx_token_rows_kernel(const float* __restrict__ x, int64_t ld, int hw, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, int C, float eps, float* __restrict__ out_f32,
                                                             f16* __restrict__ out_f16, int64_t ld_out, unsigned* __restrict__ nonfinite) {
    __shared__ f32x4 part[4][NV * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int nvec = C >> 2;
    const float* xf = x + (int64_t)b * hw * ld;
    f32x4 v[NV];
    int64_t row = (int64_t)b * (hw + 1);                       // of the output image
    if (blockIdx.x == 0) {
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
        const float inv = (float)hw;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int idx = lane + 64 * k;
            v[k] = (((part[0][idx] + part[1][idx]) + part[2][idx]) + part[3][idx]) / inv;
        }
    } else {
        const int p = (blockIdx.x - 1) * 4 + wave;
        if (p >= hw) return;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int idx = lane + 64 * k;
            v[k] = idx < nvec ? reinterpret_cast<const f32x4*>(xf + (int64_t)p * ld)[idx] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        row += 1 + p;
    }
    const float rstd = cnx_ln<NV>(v, C, eps, gamma, beta, lane);
    count_nonfinite<NV>(rstd, v, nvec, lane, nonfinite);
    store_row<NV>(v, out_f32 ? out_f32 + row * ld_out : nullptr, out_f16 ? out_f16 + row * ld_out : nullptr, nvec, lane);
}

__device__ __forceinline__ f32x4 load4(const float* r, int idx) { return reinterpret_cast<const f32x4*>(r)[idx]; }
__device__ __forceinline__ f32x4 load4(const f16* r, int idx) {
    const f16x4 h = reinterpret_cast<const f16x4*>(r)[idx];
    return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}

// grid (ceil(P / 4), n): one wave per patch row.  Three fp32 sums per row (q . p, q . q, p . p), each a lane's fmaf chain over its
// columns in ascending order, then the wave's xor tree: the order is fixed, a frame's map depends on nothing but its own rows.
template <typename E>
__global__ __launch_bounds__(256) void token_similarity_kernel(const E* __restrict__ tok, int64_t ld, int T, int D, int P0,
                                                               const int* __restrict__ query_idx, float* __restrict__ map) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.y, P = T - P0;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    int q = query_idx ? query_idx[b] : 0;
    q = q < 0 ? 0 : (q >= T ? T - 1 : q);                     // never a read outside the frame
    const E* const qr = tok + ((int64_t)b * T + q) * ld;
    const E* const pr = tok + ((int64_t)b * T + P0 + p) * ld;
    float qp = 0.f, qq = 0.f, pp = 0.f;
    for (int idx = lane; idx < (D >> 2); idx += 64) {
        const f32x4 a = load4(qr, idx), c = load4(pr, idx);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            qp = fmaf(a[e], c[e], qp);
            qq = fmaf(a[e], a[e], qq);
            pp = fmaf(c[e], c[e], pp);
        }
    }
    qp = wave_sum(qp);
    qq = wave_sum(qq);
    pp = wave_sum(pp);
    const float den = sqrtf(qq) * sqrtf(pp);
    if (lane == 0) map[(int64_t)b * P + p] = den == 0.f ? 0.f : qp / den;      // a zero row has no direction: 0, not NaN
}

#define TOK_NV_SWITCH(nv, KERNEL, ...)                                 \
    switch (nv) {                                                      \
        case 1: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break;     \
        case 2: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break;     \
        case 3: hipLaunchKernelGGL(KERNEL<3>, __VA_ARGS__); break;     \
        case 4: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break;     \
        case 5: hipLaunchKernelGGL(KERNEL<5>, __VA_ARGS__); break;     \
        case 6: hipLaunchKernelGGL(KERNEL<6>, __VA_ARGS__); break;     \
        default: return -1;                                            \
    }

// rows of ld elements behind p, read or written as 16-byte (fp32) / 8-byte (fp16) vectors
bool rows_ok(const void* p, int64_t ld, int width, size_t elem) {
    return !p || (ld >= width && ld % 4 == 0 && (uintptr_t)p % (4 * elem) == 0);
}

}  // namespace

int launch_final_norm_rows(const float* x, int64_t ldx, const float* gamma, const float* beta, float* out_f32, f16* out_f16,
                           int64_t ld_out, int64_t M, int D, float eps, unsigned* nonfinite, hipStream_t stream) {
    if (!x || !gamma || !beta || (!out_f32 && !out_f16) || M <= 0 || (M + 3) / 4 > 0x7fffffff || D <= 0 || D % 4 || D > 1280 ||
        !rows_ok(x, ldx, D, 4) || !rows_ok(out_f32, ld_out, D, 4) || !rows_ok(out_f16, ld_out, D, 2))
        return -1;
    TOK_NV_SWITCH((D / 4 + 63) / 64, final_norm_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, x, ldx, gamma, beta,
                  out_f32, out_f16, ld_out, M, D, eps, nonfinite);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_copy_rows(const float* x, int64_t ldx, float* out_f32, f16* out_f16, int64_t ld_out, int64_t M, int D, unsigned* nonfinite,
                     hipStream_t stream) {
    if (!x || (!out_f32 && !out_f16) || M <= 0 || (M + 3) / 4 > 0x7fffffff || D <= 0 || D % 4 || !rows_ok(x, ldx, D, 4) ||
        !rows_ok(out_f32, ld_out, D, 4) || !rows_ok(out_f16, ld_out, D, 2))
        return -1;
    hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, x, ldx, out_f32, out_f16, ld_out, M, D, nonfinite);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_cnx_token_rows(const float* x, int64_t ld, int n, int hw, const float* gamma, const float* beta, int C, float eps,
                          float* out_f32, f16* out_f16, int64_t ld_out, unsigned* nonfinite, hipStream_t stream) {
    if (!x || !gamma || !beta || (!out_f32 && !out_f16) || n <= 0 || n > 65535 || hw <= 0 || C <= 0 || C % 32 || C > 1536 ||
        !rows_ok(x, ld, C, 4) || !rows_ok(out_f32, ld_out, C, 4) || !rows_ok(out_f16, ld_out, C, 2))
        return -1;
    TOK_NV_SWITCH((C / 4 + 63) / 64, cnx_token_rows_kernel, dim3(1u + (unsigned)((hw + 3) / 4), (unsigned)n), dim3(256), 0, stream, x, ld,
                  hw, gamma, beta, C, eps, out_f32, out_f16, ld_out, nonfinite);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <typename E>
int launch_token_similarity(const E* tokens, int64_t ld, int n, int T, int D, int P0, const int* query_idx, float* map,
                            hipStream_t stream) {
    if (!tokens || !map || n <= 0 || n > 65535 || P0 < 0 || T <= P0 || D <= 0 || D % 4 || !rows_ok(tokens, ld, D, sizeof(E)))
        return -1;
    hipLaunchKernelGGL(token_similarity_kernel<E>, dim3((unsigned)((T - P0 + 3) / 4), (unsigned)n), dim3(256), 0, stream, tokens, ld, T, D,
                       P0, query_idx, map);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
template int launch_token_similarity<float>(const float*, int64_t, int, int, int, int, const int*, float*, hipStream_t);
template int launch_token_similarity<f16>(const f16*, int64_t, int, int, int, int, const int*, float*, hipStream_t);
