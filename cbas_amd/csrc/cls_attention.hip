// CLS attention maps: the last layer's softmax row of the CLS query over every token, per head, and its head mean over the
// patch tokens (what the reference's compare_encoders.py:36-49 takes from output_attentions=True).  The fused attention kernels
// never store probabilities; this kernel recomputes that one row per head from the two buffers the pruned last layer leaves
// behind - the CLS queries (bias added, x 1/8) and K of every token (RoPE applied) - and touches nothing else.
//
//     s[b,h,t] = sum_{j<64} q[b, 64 h + j] K[b T + t, 64 h + j]
//     p[b,h,t] = exp(s - max_t s) / sum_t exp(s - max_t s)                 over all T tokens, prefix included
//     map[b,i] = (1 / NH) sum_{h ascending} p[b,h,NP + i]                  i < P = T - NP
//
// One workgroup per frame walks the heads in ascending order, so the map needs no scratch sized by the batch and a frame's
// result depends on nothing but its own q and K rows.  Everything is fp32 and the order of every sum is fixed:
//   score:   8 lanes per token, lane l owns d = 8 l .. 8 l + 7: an fmaf chain in ascending d, then the xor tree 1, 2, 4
//   max/sum: thread i owns tokens i, i + 1024, ... in ascending order, then the wave's xor tree 32 .. 1, then the same tree over
//            the 16 wave results read back from LDS
//   map:     thread i adds head h's p to its own tokens' LDS slots, h ascending; x (1 / NH) at the end
// No atomics.  LDS: T scores + P map sums (dynamic: no T is baked in; the launcher refuses what does not fit the 64 KiB a launch
// gets without a per-device function attribute - T up to about 8 000 tokens, a 1 400 x 1 400 frame at patch 16).
#include "kernels.h"
#include "attn_loaders.h"

namespace {

constexpr int CA_THREADS = 1024, CA_WAVES = CA_THREADS / 64, CA_LPT = 8;      // lanes per token
constexpr size_t CA_LDS_MAX = (size_t)CLS_ATTENTION_LDS_BYTES;      // dynamic bytes; the rest is the static reduction buffer and slack

// max / sum over the workgroup, every thread gets the result: wave tree, then the same tree over the wave results
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* red, int tid) {
    v = MAX ? wave_max(v) : wave_sum(v);
    __syncthreads();                                   // the previous use of red is over
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float r = (tid & 63) < CA_WAVES ? red[tid & 63] : (MAX ? -INFINITY : 0.f);
    return MAX ? wave_max(r) : wave_sum(r);
}

template <typename L>
__global__ __launch_bounds__(CA_THREADS) void cls_attention_kernel(const typename L::elem* __restrict__ q, int64_t ldq,
                                                                   const typename L::elem* __restrict__ K, int64_t ldk, int T, int NH,
                                                                   int NP, float inv_nh, float* __restrict__ heads_out,
                                                                   float* __restrict__ map_out) {
    extern __shared__ float ca_lds[];
    __shared__ float red[CA_WAVES];
    float* const sc = ca_lds;              // [T] scores, then exp(s - max)
    float* const acc = ca_lds + T;         // [P] head sums of p
    const int b = blockIdx.x, tid = threadIdx.x, P = T - NP;
    const int l = tid & (CA_LPT - 1), g = tid / CA_LPT;
    const typename L::elem* const qb = q + (int64_t)b * ldq;
    const typename L::elem* const Kb = K + (int64_t)b * T * ldk;
    // slot t - NP belongs to the thread that owns token t (tid, tid + 1024, ...): zeroed, accumulated and read by that thread alone
    if (map_out)
        for (int t = tid + NP; t < T; t += CA_THREADS) acc[t - NP] = 0.f;

    for (int h = 0; h < NH; ++h) {
        float qv[8];
        L::load8(qb + 64 * h, l, qv);
        for (int t = g; t < T; t += CA_THREADS / CA_LPT) {
            float kv[8];
            L::load8(Kb + (int64_t)t * ldk + 64 * h, l, kv);
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) s = fmaf(qv[e], kv[e], s);
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            s += __shfl_xor(s, 4, 64);
            if (l == 0) sc[t] = s * L::SCORE_SCALE;
        }
        __syncthreads();
        float m = -INFINITY;
        for (int t = tid; t < T; t += CA_THREADS) m = fmaxf(m, sc[t]);
        m = block_reduce<true>(m, red, tid);
        float sum = 0.f;
        for (int t = tid; t < T; t += CA_THREADS) {
            const float e = expf(sc[t] - m);
            sc[t] = e;                                               // its own slot: no other thread reads it
            sum += e;
        }
        sum = block_reduce<false>(sum, red, tid);
        for (int t = tid; t < T; t += CA_THREADS) {
            const float p = sc[t] / sum;
            if (heads_out) heads_out[((int64_t)b * NH + h) * T + t] = p;
            if (map_out && t >= NP) acc[t - NP] += p;
        }
        __syncthreads();                                             // sc is rewritten by the next head's scores
    }
    if (map_out)
        for (int t = tid + NP; t < T; t += CA_THREADS) map_out[(int64_t)b * P + t - NP] = acc[t - NP] * inv_nh;
}

template <typename L>
int launch_form(const typename L::elem* q, int64_t ldq, const typename L::elem* K, int64_t ldk, int n, int T, int NH, int NP,
                float* heads_out, float* map_out, hipStream_t stream) {
    const size_t lds = (size_t)(2 * T - NP) * sizeof(float);
    if (lds > CA_LDS_MAX) return -1;
    hipLaunchKernelGGL(cls_attention_kernel<L>, dim3(n), dim3(CA_THREADS), lds, stream, q, ldq, K, ldk, T, NH, NP,
                       1.0f / (float)NH, heads_out, map_out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

template <typename E>
int launch_cls_attention(const E* q, int64_t ldq, const E* K, int64_t ldk, int n, int T, int NH, int NP, int split,
                         float* heads_out, float* map_out, hipStream_t stream) {
    constexpr int per16 = 16 / (int)sizeof(E);         // every 8-value load is 16-byte aligned
    if (!q || !K || (!heads_out && !map_out) || n <= 0 || NH <= 0 || NP <= 0 || T < NP || ldq % per16 || ldk % per16 ||
        ldq < (int64_t)NH * 64 || ldk < (int64_t)NH * 64 || ((uintptr_t)q | (uintptr_t)K) % 16)
        return -1;
    if constexpr (sizeof(E) == 2) {
        if (split) return -1;
        return launch_form<LoadF16>(q, ldq, K, ldk, n, T, NH, NP, heads_out, map_out, stream);
    } else {
        return split ? launch_form<LoadSplit>(q, ldq, K, ldk, n, T, NH, NP, heads_out, map_out, stream)
                     : launch_form<LoadF32>(q, ldq, K, ldk, n, T, NH, NP, heads_out, map_out, stream);
    }
}
template int launch_cls_attention<f16>(const f16*, int64_t, const f16*, int64_t, int, int, int, int, int, float*, float*, hipStream_t);
template int launch_cls_attention<float>(const float*, int64_t, const float*, int64_t, int, int, int, int, int, float*, float*, hipStream_t);
