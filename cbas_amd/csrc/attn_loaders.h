// The three storage forms of one head's 64 values of q or K that the attention-probability kernels read (cls_attention.hip,
// attention_rollout.hip): what the q|k|v GEMM of each operand family leaves in HBM.
#pragma once
#include "kernels.h"
#include "vit32_epilogue.h"

// the 8 values d = 8 l .. 8 l + 7 of one head (64 values at `head`) as floats, by storage form
struct LoadF16 {       // fp16 [64]
    typedef f16 elem;
    static __device__ __forceinline__ void load8(const f16* head, int l, float (&v)[8]) {
        const f16x8 x = *reinterpret_cast<const f16x8*>(head + 8 * l);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)x[e];
    }
    static constexpr float SCORE_SCALE = 1.f;
};
struct LoadF32 {       // fp32 [64]
    typedef float elem;
    static __device__ __forceinline__ void load8(const float* head, int l, float (&v)[8]) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(head + 8 * l), b = *reinterpret_cast<const f32x4*>(head + 8 * l + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
    }
    static constexpr float SCORE_SCALE = 1.f;
};
struct LoadSplit {     // precision 4: [hi: 64 x fp16 | lo: 64 x fp16] in the 64 float slots (store_head_split4), q x ATT_QS, K x ATT_KS
    typedef float elem;
    static __device__ __forceinline__ void load8(const float* head, int l, float (&v)[8]) {
        const f16* h16 = reinterpret_cast<const f16*>(head);
        const f16x8 hi = *reinterpret_cast<const f16x8*>(h16 + 8 * l), lo = *reinterpret_cast<const f16x8*>(h16 + 64 + 8 * l);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)hi[e] + (float)lo[e];
    }
    static constexpr float SCORE_SCALE = 1.f / (ATT_QS * ATT_KS);       // a power of two: exact
};
