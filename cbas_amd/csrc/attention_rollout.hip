// Attention rollout (Abnar and Zuidema, "Quantifying attention flow in transformers"): what the whole network looks at, from
// the head-averaged attention of EVERY query row of every layer.  The fused attention kernels never store probabilities; the
// kernels here recompute them from the q | k | v image a layer's q|k|v GEMM leaves in HBM, before the next layer reuses it.
//
//   attention_mean_kernel   A[b,i,t] = (1 / NH) sum_{h ascending} softmax_t(q[b,i,h,:] . K[b,t,h,:])           (T x T per frame)
//                           with blend: A^ = 0.5 A + 0.5 I, the rollout's residual mix (x 0.5 is exact, the diagonal rounds once)
//   rollout_step_kernel     R' = A^ R per frame, T x T by T x T
//   rollout_row_kernel      out[b,p] = R[b, query_b, NP + p]: the query row's patch columns
//
// Everything is fp32 on the vector pipe, every sum has a fixed order and there are no atomics; a frame's result depends on
// nothing but its own rows.
//   score:   one thread per key token holds that key's 64 values in registers and runs ONE fmaf chain in ascending d against each
//            of the workgroup's QB query rows (broadcast reads of q from LDS): K is fetched once per QB rows
//   softmax: one wave per query row; lane i owns tokens i, i + 64, ... in ascending order (max, then exp and sum), then the
//            wave's xor tree 32 .. 1: a term passes through at most ceil(T / 64) + 6 additions
//   mean:    the owning lane adds head h's p to its token's LDS slot, h ascending; x (1 / NH) at the end
//   step:    out[i][j] = fmaf chain over k ascending of A^[i][k] R[k][j]; 64 x 64 tiles, edges masked (operands zero-filled)
// LDS of the first kernel is sized by the launch: QB (64 + 2 T) floats, QB the largest of 16, 8, 4, 2, 1 that fits the 64 KiB a
// launch gets without a function attribute; T beyond QB = 1 (about 8 100 tokens) is refused.
#include "kernels.h"
#include "attn_loaders.h"

namespace {

constexpr int AM_THREADS = 256, AM_WAVES = AM_THREADS / 64;
constexpr size_t AM_LDS_MAX = (size_t)ATTENTION_MEAN_LDS_BYTES;

template <typename L>
__global__ __launch_bounds__(AM_THREADS) void attention_mean_kernel(const typename L::elem* __restrict__ q, int64_t ldq,
                                                                    const typename L::elem* __restrict__ K, int64_t ldk, int T, int NH,
                                                                    int QB, float inv_nh, int blend, float* __restrict__ out) {
    extern __shared__ float am_lds[];
    float* const ql = am_lds;                      // [QB][64] one head of the block's queries
    float* const sc = am_lds + QB * 64;            // [QB][T] scores, then exp(s - max)
    float* const acc = sc + (size_t)QB * T;        // [QB][T] head sums of p
    const int b = blockIdx.y, i0 = blockIdx.x * QB, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = min(QB, T - i0);                // query rows of this block that exist
    const typename L::elem* const qb = q + ((int64_t)b * T + i0) * ldq;
    const typename L::elem* const Kb = K + (int64_t)b * T * ldk;

    for (int h = 0; h < NH; ++h) {
        // stage the queries: 8 threads per row, 8 values each (rows past the frame's end: zeros, never read back)
        for (int e = tid; e < QB * 8; e += AM_THREADS) {
            const int r = e >> 3, l = e & 7;
            float v[8];
            if (r < nq) L::load8(qb + (int64_t)r * ldq + 64 * h, l, v);
            else
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) ql[r * 64 + 8 * l + j] = v[j];
        }
        __syncthreads();
        for (int t = tid; t < T; t += AM_THREADS) {
            float kv[64];
#pragma unroll
            for (int l = 0; l < 8; ++l) {
                float v[8];
                L::load8(Kb + (int64_t)t * ldk + 64 * h, l, v);
#pragma unroll
                for (int j = 0; j < 8; ++j) kv[8 * l + j] = v[j];
            }
            for (int r = 0; r < nq; ++r) {
                const f32x4* const qr = reinterpret_cast<const f32x4*>(ql + r * 64);
                float s = 0.f;
#pragma unroll
                for (int d4 = 0; d4 < 16; ++d4) {
                    const f32x4 qv = qr[d4];
                    s = fmaf(qv[0], kv[4 * d4], s);
                    s = fmaf(qv[1], kv[4 * d4 + 1], s);
                    s = fmaf(qv[2], kv[4 * d4 + 2], s);
                    s = fmaf(qv[3], kv[4 * d4 + 3], s);
                }
                sc[(size_t)r * T + t] = s * L::SCORE_SCALE;
            }
        }
        __syncthreads();
        for (int r = wave; r < nq; r += AM_WAVES) {
            float* const s = sc + (size_t)r * T;
            float* const a = acc + (size_t)r * T;
            float m = -INFINITY;
            for (int t = lane; t < T; t += 64) m = fmaxf(m, s[t]);
            m = wave_max(m);
            float sum = 0.f;
            for (int t = lane; t < T; t += 64) {
                const float e = expf(s[t] - m);
                s[t] = e;                                          // its own slot
                sum += e;
            }
            sum = wave_sum(sum);
            for (int t = lane; t < T; t += 64) {
                const float p = s[t] / sum;
                a[t] = h == 0 ? p : a[t] + p;
            }
        }
        __syncthreads();                                           // ql and sc are rewritten by the next head
    }
    for (int r = wave; r < nq; r += AM_WAVES) {
        const float* const a = acc + (size_t)r * T;
        float* const o = out + ((int64_t)b * T + i0 + r) * T;
        for (int t = lane; t < T; t += 64) {
            const float v = a[t] * inv_nh;
            o[t] = blend ? 0.5f * v + (t == i0 + r ? 0.5f : 0.f) : v;
        }
    }
}

// 64 x 64 output tile per workgroup, 4 x 4 per thread, K in steps of 16 through LDS.  Out-of-range operand elements are staged as
// zeros, so every output's chain runs over k = 0 .. T - 1 (+ zero terms) in ascending order whatever the tile.
constexpr int RS_TILE = 64, RS_K = 16;
__global__ __launch_bounds__(256) void rollout_step_kernel(const float* __restrict__ A, const float* __restrict__ R,
                                                           float* __restrict__ out, int T) {
    __shared__ float As[RS_K][RS_TILE + 4];       // [k][i]
    __shared__ float Rs[RS_K][RS_TILE + 4];       // [k][j]
    const int b = blockIdx.z, i0 = blockIdx.y * RS_TILE, j0 = blockIdx.x * RS_TILE, tid = threadIdx.x;
    const float* const Ab = A + (int64_t)b * T * T;
    const float* const Rb = R + (int64_t)b * T * T;
    const int ti = (tid >> 4) * 4, tj = (tid & 15) * 4;
    float c[4][4];
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int x = 0; x < 4; ++x) c[y][x] = 0.f;
    for (int k0 = 0; k0 < T; k0 += RS_K) {
        for (int e = tid; e < RS_TILE * RS_K; e += 256) {
            const int ai = e / RS_K, ak = e % RS_K;               // A: consecutive threads walk k (contiguous in memory)
            As[ak][ai] = (i0 + ai < T && k0 + ak < T) ? Ab[(int64_t)(i0 + ai) * T + k0 + ak] : 0.f;
            const int rk = e / RS_TILE, rj = e % RS_TILE;         // R: consecutive threads walk j
            Rs[rk][rj] = (k0 + rk < T && j0 + rj < T) ? Rb[(int64_t)(k0 + rk) * T + j0 + rj] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < RS_K; ++k) {
            float a[4], r[4];
#pragma unroll
            for (int y = 0; y < 4; ++y) a[y] = As[k][ti + y];
#pragma unroll
            for (int x = 0; x < 4; ++x) r[x] = Rs[k][tj + x];
#pragma unroll
            for (int y = 0; y < 4; ++y)
#pragma unroll
                for (int x = 0; x < 4; ++x) c[y][x] = fmaf(a[y], r[x], c[y][x]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int x = 0; x < 4; ++x)
            if (i0 + ti + y < T && j0 + tj + x < T) out[(int64_t)b * T * T + (int64_t)(i0 + ti + y) * T + j0 + tj + x] = c[y][x];
}

__global__ __launch_bounds__(256) void rollout_row_kernel(const float* __restrict__ R, int T, int NP, const int* __restrict__ query_idx,
                                                          float* __restrict__ out) {
    const int b = blockIdx.y, P = T - NP;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    int qi = query_idx ? query_idx[b] : 0;
    qi = qi < 0 ? 0 : (qi >= T ? T - 1 : qi);                      // never a read outside the frame
    out[(int64_t)b * P + p] = R[(int64_t)b * T * T + (int64_t)qi * T + NP + p];
}

template <typename L>
int launch_mean_form(const typename L::elem* q, int64_t ldq, const typename L::elem* K, int64_t ldk, int n, int T, int NH, int blend,
                     float* out, hipStream_t stream) {
    const int QB = attention_mean_rows_per_block(T);
    if (QB <= 0) return -1;
    const size_t lds = (size_t)QB * (64 + 2 * (size_t)T) * sizeof(float);
    hipLaunchKernelGGL(attention_mean_kernel<L>, dim3((unsigned)((T + QB - 1) / QB), (unsigned)n), dim3(AM_THREADS), lds, stream, q, ldq, K,
                       ldk, T, NH, QB, 1.0f / (float)NH, blend, out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

int attention_mean_rows_per_block(int64_t T) {
    if (T <= 0) return 0;
    for (int QB = 16; QB >= 1; QB >>= 1)
        if ((size_t)QB * (64 + 2 * (size_t)T) * sizeof(float) <= AM_LDS_MAX) return QB;
    return 0;
}

template <typename E>
int launch_attention_mean(const E* q, int64_t ldq, const E* K, int64_t ldk, int n, int T, int NH, int split, int blend, float* out,
                          hipStream_t stream) {
    constexpr int per16 = 16 / (int)sizeof(E);         // every 8-value load is 16-byte aligned
    if (!q || !K || !out || n <= 0 || n > 65535 || NH <= 0 || T <= 0 || ldq % per16 || ldk % per16 || ldq < (int64_t)NH * 64 ||
        ldk < (int64_t)NH * 64 || ((uintptr_t)q | (uintptr_t)K) % 16 || (uintptr_t)out % 4)
        return -1;
    if constexpr (sizeof(E) == 2) {
        if (split) return -1;
        return launch_mean_form<LoadF16>(q, ldq, K, ldk, n, T, NH, blend, out, stream);
    } else {
        return split ? launch_mean_form<LoadSplit>(q, ldq, K, ldk, n, T, NH, blend, out, stream)
                     : launch_mean_form<LoadF32>(q, ldq, K, ldk, n, T, NH, blend, out, stream);
    }
}
template int launch_attention_mean<f16>(const f16*, int64_t, const f16*, int64_t, int, int, int, int, int, float*, hipStream_t);
template int launch_attention_mean<float>(const float*, int64_t, const float*, int64_t, int, int, int, int, int, float*, hipStream_t);

int launch_rollout_step(const float* A, const float* R, float* out, int n, int T, hipStream_t stream) {
    if (!A || !R || !out || out == A || out == R || n <= 0 || n > 65535 || T <= 0 || (T + RS_TILE - 1) / RS_TILE > 65535) return -1;
    const unsigned g = (unsigned)((T + RS_TILE - 1) / RS_TILE);
    hipLaunchKernelGGL(rollout_step_kernel, dim3(g, g, (unsigned)n), dim3(256), 0, stream, A, R, out, T);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_rollout_row(const float* R, int n, int T, int NP, const int* query_idx, float* out, hipStream_t stream) {
    if (!R || !out || n <= 0 || n > 65535 || NP <= 0 || T <= NP) return -1;
    hipLaunchKernelGGL(rollout_row_kernel, dim3((unsigned)((T - NP + 255) / 256), (unsigned)n), dim3(256), 0, stream, R, T, NP, query_idx, out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
