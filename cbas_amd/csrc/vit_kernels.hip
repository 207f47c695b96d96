// ViT kernels other than the GEMM: frame ingest (im2col of the green plane), LayerNorm, fused
// multi-head attention, final CLS LayerNorm, weight packing.  gfx950 only.
//
// Reference arithmetic replaced:
//   ingest        backend/cbas.py:431 (green/255), :674 (gray -> 3 identical channels, folded into
//                 the patch weights by pack_patch_weight), [tf]:82-83 (Conv2d k=s=16 as im2col), :86-89 (prefix tokens)
//   layernorm     [tf]:404,410 (norm1/norm2), :540 (final norm; only the CLS row is needed, cbas.py:677)
//   attention     [tf]:210-234 (softmax(q k^T * 64^-0.5) v), heads split/merge :311-313,:330
#include <stdlib.h>
#include "kernels.h"
#include "row_norm.h"

namespace {

// ---------------------------------------------------------------------------------------------
// ingest
// ---------------------------------------------------------------------------------------------
// One thread = one patch row of `ps` pixels (ps = 16 for DINOv3, 14 for DINOv2).  A[m][i*16 + j],
// m = b*P + py*nw + px; the K layout always has 16x16 slots per patch: slots with i >= ps or j >= ps
// stay zero (rows i >= ps are never written; the buffer is zeroed at allocation) and the packed
// patch weights are zero there too.
__global__ void im2col_u8_kernel(const uint8_t* __restrict__ frames, int n, int height, int width,
                                 int64_t frame_stride, int64_t row_stride, int64_t pixel_stride,
                                 f16* __restrict__ A, int nh, int nw, int ps) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)n * nh * ps * nw;
    if (gid >= total) return;
    const int px = gid % nw;
    const int64_t t1 = gid / nw;
    const int y = t1 % (nh * ps);
    const int b = t1 / (nh * ps);
    const int py = y / ps, i = y - py * ps;
    const uint8_t* src = frames + b * frame_stride + (int64_t)y * row_stride + (int64_t)px * ps * pixel_stride;
    f16x8 lo, hi;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        lo[j] = (f16)(float)src[j * pixel_stride];                       // ps >= 14 > 8
        hi[j] = (j + 8 < ps) ? (f16)(float)src[(j + 8) * pixel_stride] : (f16)0.f;
    }
    f16* dst = A + ((int64_t)b * nh * nw + (int64_t)py * nw + px) * 256 + i * 16;
    *reinterpret_cast<f16x8*>(dst) = lo;
    *reinterpret_cast<f16x8*>(dst + 8) = hi;
}

// float input: K = 512, columns [0,256) hold fp16(x), [256,512) hold fp16(x - fp16(x)).
__global__ void im2col_f32_kernel(const float* __restrict__ frames, int n, int height, int width,
                                  f16* __restrict__ A, int nh, int nw, int ps) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)n * nh * ps * nw;
    if (gid >= total) return;
    const int px = gid % nw;
    const int64_t t1 = gid / nw;
    const int y = t1 % (nh * ps);
    const int b = t1 / (nh * ps);
    const int py = y / ps, i = y - py * ps;
    const float* src = frames + ((int64_t)b * height + y) * width + px * ps;
    f16* dst = A + ((int64_t)b * nh * nw + (int64_t)py * nw + px) * 512 + i * 16;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        f16x8 h, l;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = (half * 8 + j < ps) ? src[half * 8 + j] : 0.f;
            const f16 hv = (f16)v;
            h[j] = hv;
            l[j] = (f16)(v - (float)hv);
        }
        *reinterpret_cast<f16x8*>(dst + half * 8) = h;
        *reinterpret_cast<f16x8*>(dst + 256 + half * 8) = l;
    }
}

__global__ void write_prefix_kernel(float* __restrict__ x, const float* __restrict__ prefix, int n,
                                    int n_prefix, int D, int T) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per = (int64_t)n_prefix * (D / 4);
    if (gid >= (int64_t)n * per) return;
    const int b = gid / per;
    const int rem = gid - (int64_t)b * per;
    const int r = rem / (D / 4), c = rem - r * (D / 4);
    reinterpret_cast<f32x4*>(x + ((int64_t)b * T + r) * D)[c] = reinterpret_cast<const f32x4*>(prefix + (int64_t)r * D)[c];
}

// ---------------------------------------------------------------------------------------------
// LayerNorm: one wave per row, two-pass statistics in registers (matches the reference's
// mean / biased-variance formulation), fp32 in, fp16 out.  The row itself is ln_row (row_norm.h).
// ---------------------------------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(256) void layernorm_f16_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, f16* __restrict__ out,
                                                            int M, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    f32x4 y[NV];
    ln_row<NV>(x + (size_t)row * ldx, gamma, beta, D, eps, lane, y);
    const int nvec = D >> 2;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        if (idx < nvec) {
            f16x4 h = {(f16)y[k][0], (f16)y[k][1], (f16)y[k][2], (f16)y[k][3]};
            reinterpret_cast<f16x4*>(out + (size_t)row * D)[idx] = h;
        }
    }
}

// LayerNorm with an MX-fp8 result (precision 2): lane `l` of vector k holds columns 4*(l + 64k) .. +3, so a 32-column
// scale block is 8 consecutive lanes and a 128-column K-tile half a wave.  out_sc: [D/128][sc_ld] dwords, byte b of
// dword (kt, row) = E8M0 scale of columns kt*128 + 32b .. +31 (the layout GemmParams::A_sc documents).
template <int NV>
__global__ __launch_bounds__(256) void layernorm_f8_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, uint8_t* __restrict__ out8,
                                                           uint32_t* __restrict__ out_sc, int sc_ld, int M, int D, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    f32x4 y[NV];
    ln_row<NV>(x + (size_t)row * ldx, gamma, beta, D, eps, lane, y);
    const int nvec = D >> 2;
    uint8_t* sc_bytes = reinterpret_cast<uint8_t*>(out_sc);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        const bool on = idx < nvec;
        float a = on ? fmaxf(fmaxf(fabsf(y[k][0]), fabsf(y[k][1])), fmaxf(fabsf(y[k][2]), fabsf(y[k][3]))) : 0.f;
        a = fmaxf(a, __shfl_xor(a, 1, 64));
        a = fmaxf(a, __shfl_xor(a, 2, 64));
        a = fmaxf(a, __shfl_xor(a, 4, 64));
        const int sb = mx_scale_byte(a);
        const float inv = mx_inv_scale(sb);
        if (on) {
            reinterpret_cast<unsigned*>(out8 + (size_t)row * D)[idx] =
                cvt4_e4m3(y[k][0] * inv, y[k][1] * inv, y[k][2] * inv, y[k][3] * inv);
            if ((lane & 7) == 0) {
                const int col = idx * 4, kt = col >> 7, b = (col & 127) >> 5;
                sc_bytes[((size_t)kt * sc_ld + row) * 4 + b] = (uint8_t)sb;
            }
        }
    }
}

// LayerNorm fold, first layer: what EPI_RESID_LN leaves behind for the later ones.  One wave per row; vector k of a lane
// (columns 4 (lane + 64 k) .. +3) lies in 256-column block k, so a block's statistics are one wave reduction each:
// the sum, then the sum of squares about the block mean.
template <int NV>
__global__ __launch_bounds__(256) void ln_stats_x16_kernel(const float* __restrict__ x, f16* __restrict__ x16,
                                                           float2* __restrict__ ln_out, int ln_ld, int M, int D) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * D);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const f32x4 v = xr[lane + 64 * k];
        const float bs = wave_sum((v[0] + v[1]) + (v[2] + v[3]));
        const f32x4 d = v - bs * (1.0f / 256.0f);
        const float bq = wave_sum((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]));
        const f32x4 c = __builtin_elementwise_max(__builtin_elementwise_min(v, f32x4{65504.f, 65504.f, 65504.f, 65504.f}),
                                                  f32x4{-65504.f, -65504.f, -65504.f, -65504.f});
        const f16x4 h = {(f16)c[0], (f16)c[1], (f16)c[2], (f16)c[3]};
        reinterpret_cast<f16x4*>(x16 + (size_t)row * D)[lane + 64 * k] = h;
        if (lane == 0) ln_out[(size_t)k * ln_ld + row] = float2{bs, bq};
    }
}

// LayerNorm fold, create time.  One 256-thread block per output row n:
//   Wf[n][k] = fp16(gamma[k] W[n][k]);  colsum[n] = sum_k float(Wf[n][k]);  biasf[n] = b[n] + sum_k beta[k] W[n][k]
// colsum is taken over the ROUNDED weights: rstd (acc - mean colsum) then cancels the mean exactly as the MFMA saw it.
__global__ __launch_bounds__(256) void fold_ln_weight_kernel(const float* __restrict__ W, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ b,
                                                             f16* __restrict__ Wf, float* __restrict__ colsum,
                                                             float* __restrict__ biasf, int K) {
    __shared__ float red[2][4];
    const int n = blockIdx.x, tid = threadIdx.x;
    float cs = 0.f, bs = 0.f;
    for (int k = tid; k < K; k += 256) {
        const float w = W[(size_t)n * K + k];
        const f16 wf = (f16)(gamma[k] * w);
        Wf[(size_t)n * K + k] = wf;
        cs += (float)wf;
        bs = fmaf(beta[k], w, bs);
    }
    cs = wave_sum(cs);
    bs = wave_sum(bs);
    if ((tid & 63) == 0) { red[0][tid >> 6] = cs; red[1][tid >> 6] = bs; }
    __syncthreads();
    if (tid == 0) {
        colsum[n] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        biasf[n] = b[n] + ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
    }
}

template <int NV>
__global__ __launch_bounds__(256) void final_norm_cls_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* __restrict__ cls_f32,
                                                             f16* __restrict__ cls_f16, int n, int T, int D, float eps,
                                                             unsigned* __restrict__ nonfinite) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n) return;
    f32x4 y[NV];
    const float rstd = ln_row<NV>(x + (size_t)b * T * D, gamma, beta, D, eps, lane, y);
    const int nvec = D >> 2;
    // A non-finite value anywhere in the encoder reaches the CLS row (every query attends to every key): one test per
    // frame here watches the whole forward pass.  The reference's fp32 arithmetic has no range limit; the split-fp16 operands
    // of precision 4 (|x| scale < 65 504, vit32_epilogue.h) and the fp16 activations of precision 0 do - a violation is
    // counted and turned into CBAS_ERANGE at the next wait instead of NaN rows in a `_cls.h5`.
    // A finite value whose square overflows the variance gives rstd = 0 and a finite row (beta): counted through rstd.
    if (nonfinite) {
        bool bad = !(rstd > 0.f);
#pragma unroll
        for (int k = 0; k < NV; ++k)
            if (lane + 64 * k < nvec) {
                const f32x4 a = __builtin_elementwise_abs(y[k]);
                bad |= !(a[0] <= 3.0e38f && a[1] <= 3.0e38f && a[2] <= 3.0e38f && a[3] <= 3.0e38f);
            }
        if (__ballot(bad) && lane == 0) atomicAdd(nonfinite, 1u);
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int idx = lane + 64 * k;
        if (idx < nvec) {
            if (cls_f32) reinterpret_cast<f32x4*>(cls_f32 + (size_t)b * D)[idx] = y[k];
            if (cls_f16) {
                f16x4 h = {(f16)y[k][0], (f16)y[k][1], (f16)y[k][2], (f16)y[k][3]};   // round-to-nearest-even, as h5py's f4->f2 cast
                reinterpret_cast<f16x4*>(cls_f16 + (size_t)b * D)[idx] = h;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Attention: one workgroup per (frame, head).  K and V of the head (T x 64 fp16 each) live in LDS;
// each wave takes 16-query tiles.  S^T = K Q^T is computed with the key on the MFMA row so that a
// lane holds, for ONE query, 4 keys per key tile: the softmax reductions are in-lane plus two
// cross-lane steps, and the probabilities are already laid out as the B operand of the P.V MFMA.
// V is read through ds_read_b64_tr_b16 (hardware transpose) as the A operand, giving O^T with 4
// consecutive head dims per lane (one 8-byte store per tile).
// ---------------------------------------------------------------------------------------------
// max of three without the canonicalising v_max_f32 x,x that hipcc puts in front of fmaxf on MFMA outputs (one extra
// VALU instruction per score in kernels that are VALU-bound: PMC in DESIGN.md); no NaNs occur here
__device__ __forceinline__ float max3_raw(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

__device__ __forceinline__ int k_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int v_off(int row, int col) {   // col in halves
    return row * 128 + ((((col >> 4) ^ ((row >> 1) & 3))) << 5) + ((col & 15) << 1);
}

// Store one query's 64 context values of head `hd` as MX-fp8.  A lane holds dims 16*dt + 4*g + r (dt, r = 0..3) of
// ONE query, the four lanes g = 0..3 with equal (lane & 15) share the query: a 32-dim scale block is dt in {2b, 2b+1}
// over those four lanes.  The head's 64 dims are blocks (hd & 1) * 2 + {0, 1} of K-tile hd >> 1.
__device__ __forceinline__ void attn_store_f8(const f32x4 (&o)[4], float inv, uint8_t* out8, uint32_t* out_sc, int sc_ld,
                                              size_t row, bool valid, int D, int hd, int g) {
    int sb[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        float a = 0.f;
#pragma unroll
        for (int dt = 2 * b; dt < 2 * b + 2; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) a = fmaxf(a, fabsf(o[dt][r] * inv));
        a = xor16_max(a);
        a = xor32_max(a);
        sb[b] = mx_scale_byte(a);
    }
    if (!valid) return;
    uint8_t* orow = out8 + row * D + hd * 64 + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const float m = inv * mx_inv_scale(sb[dt >> 1]);
        *reinterpret_cast<unsigned*>(orow + 16 * dt) = cvt4_e4m3(o[dt][0] * m, o[dt][1] * m, o[dt][2] * m, o[dt][3] * m);
    }
    if (g == 0)
        *reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(out_sc) + ((size_t)(hd >> 1) * sc_ld + row) * 4 + (hd & 1) * 2) =
            (uint16_t)(sb[0] | (sb[1] << 8));
}

// NKT = key tiles held in LDS (even); NV = tiles that contain at least one real key when that is known
// at compile time (T in ((NV-1)*16, NV*16]), 0 = decide per element at run time.  With NV fixed only the
// ONE partial tile is masked (4 compares per lane, once) and fully padded tiles cost no MFMA; the
// run-time form costs a compare+select per score because hipcc if-converts the tail test.
// SPLIT = 2 (the exact-T instantiations, full-frame mode): a (frame, head) pair is handled by TWO workgroups of 4
// waves, one per half of the query tiles; both stage the pair's K and V.  With K + V = 52 KiB at T = 201 three such
// workgroups share a CU, so 64 x 12 x 2 = 1 536 workgroups are exactly two full rounds over 256 CUs (one 7-wave
// workgroup per pair was 1.5 rounds at two per CU), and the staging of one workgroup runs under the math of its
// neighbours.  Workgroups b and b + 8 land on the same XCD (round-robin dispatch): the two halves of a pair are placed
// 8 apart so the second K/V fetch hits that XCD's L2.
// K and V are staged by 16-byte LDS-DMA (global_load_lds), all pieces in flight at once and no VGPR round trip; the
// swizzles of the two images are applied on the SOURCE address (the LDS side of the DMA is lane-linear), rows past T
// re-read row T-1 (finite values: their scores are masked, their probabilities exactly 0).
template <int NKT, int NV, int SPLIT>
#ifndef CBAS_ATTN_MIN_WAVES
#define CBAS_ATTN_MIN_WAVES 4      // waves per SIMD the resident kernel is compiled for (6 = 80 VGPRs = three 7-wave workgroups per CU at T = 201: spills, 24.8 us vs 23.4)
#endif
__global__ __launch_bounds__(SPLIT == 2 ? 256 : 512, (SPLIT == 2 ? (NKT > 14 ? 2 : 3) : (NKT > 14 ? 2 : CBAS_ATTN_MIN_WAVES)))
void attention_kernel(const f16* __restrict__ qkv, const f16* __restrict__ q_cls, void* __restrict__ out_v,
                      uint32_t* __restrict__ out_sc, int sc_ld, int T, int D, int n_heads, int n_pairs) {
    f16* __restrict__ out = reinterpret_cast<f16*>(out_v);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NQK = NV ? NV : NKT;                 // key tiles that need S = K Q^T
    constexpr int NG = NV ? (NV + 1) / 2 : NKT / 2;    // 32-key groups that need P.V
    // LDS: the V image first, then K, NQK tiles each.  With NV odd the last P.V group reads one V tile more than is
    // held: that read lands on the first K tile - finite values, multiplied by probabilities that are exactly 0.
    // (T = 201: 2 x 13 tiles = 52 KiB instead of 2 x 14 = 56, which is what lets three workgroups share a CU.)
    constexpr int ROWS = NQK * 16;
    char* Vs = smem;
    char* Ks = smem + ROWS * 128;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    int pair = blockIdx.x, half = 0;
    if (SPLIT == 2) {
        pair = ((int)blockIdx.x >> 4) * 8 + ((int)blockIdx.x & 7);
        half = ((int)blockIdx.x >> 3) & 1;
        if (pair >= n_pairs) return;                   // grid is padded to a multiple of 16
    }
    const int b = pair / n_heads, hd = pair - b * n_heads;
    const size_t ld = (size_t)3 * D;
    const f16* qbase = qkv + (size_t)b * T * ld + hd * 64;
    const f16* kbase = qbase + D;
    const f16* vbase = qbase + 2 * D;
    const int g = lane >> 4, li = lane & 15;
    // CLS-query mode (last layer): one query per frame, read from the compact q_cls [n][D]; all 16 query
    // slots of the tile carry that row (each MFMA column depends on its own query only), slot 0 is stored
    const int nq = q_cls ? 1 : T;
    const f16* qsrc = q_cls ? q_cls + (size_t)b * D + hd * 64 : qbase;
    const size_t qld = q_cls ? 0 : ld;
    const int nqt_all = (nq + 15) >> 4;
    const int q_per = SPLIT == 2 ? (nqt_all + 1) / 2 : nqt_all;         // query tiles of this workgroup: [qt0, nqt)
    const int qt0 = half * q_per;
    const int nqt = qt0 + q_per < nqt_all ? qt0 + q_per : nqt_all;

    auto load_q = [&](int qt, f16x8 (&qf)[2]) {
        const int q = qt * 16 + li;
        const int qrow = q < nq ? q : nq - 1;
        qf[0] = *reinterpret_cast<const f16x8*>(qsrc + (size_t)qrow * qld + g * 8);
        qf[1] = *reinterpret_cast<const f16x8*>(qsrc + (size_t)qrow * qld + 32 + g * 8);
    };
    // Q of this wave's first tile is fetched before the K/V staging so its latency hides under it
    f16x8 qf[2] = {};
    int qt = qt0 + wave;
    if (qt < nqt) load_q(qt, qf);

    {   // K / V staging: 1 KiB pieces (8 rows x 128 B) by LDS-DMA, piece p of each image to waves p mod nwaves
        const int pr = lane >> 3, pos = lane & 7;
        for (int p = wave; p < ROWS / 8; p += nwaves) {
            const int r = p * 8 + pr;
            const int rs = r < T ? r : T - 1;
            const int kc = pos ^ ((r >> 1) & 7);                                   // k_off: chunk c sits at position c ^ swz
            const int vc = (((pos >> 1) ^ ((r >> 1) & 3)) << 1) | (pos & 1);       // v_off: 32-byte granules swizzled
            __builtin_amdgcn_global_load_lds(GLB_PTR(kbase + (size_t)rs * ld + kc * 8), LDS_PTR(Ks + p * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(GLB_PTR(vbase + (size_t)rs * ld + vc * 8), LDS_PTR(Vs + p * 1024), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // Per-lane base addresses: the swizzles depend on (row & 15) / (row & 7) only, tile strides are
    // multiples of 16 rows, so every fragment read below is base + compile-time immediate.
    const char* kb0 = Ks + k_off(li, g);               // + kt*2048 for key tile kt, k-half 0
    const char* kb1 = Ks + k_off(li, 4 + g);           //                             k-half 1
    const char* vb[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) vb[dt] = Vs + v_off(4 * g + (li >> 2), 16 * dt + 4 * (li & 3));   // + s2*4096 (+2048)
    float tail_bias[4];                                // 0 / -inf for the single partial tile (NV fixed)
#pragma unroll
    for (int r = 0; r < 4; ++r) tail_bias[r] = (NV && (NV - 1) * 16 + 4 * g + r >= T) ? -INFINITY : 0.f;

    for (; qt < nqt; qt += nwaves) {
        const int q = qt * 16 + li;

        // ---- S^T = K Q^T, two key tiles (4 fragment reads, 4 MFMAs) per group; the scheduling
        // barriers keep the compiler from hoisting every fragment read (4 VGPRs each) up front
        f32x4 s[NQK];
#pragma unroll
        for (int grp = 0; grp < (NQK + 1) / 2; ++grp) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int kt = 2 * grp + u;
                if (kt >= NQK) continue;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                if (NV && kt == NV - 1) acc = f32x4{tail_bias[0], tail_bias[1], tail_bias[2], tail_bias[3]};
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(kb0 + kt * 2048), qf[0], acc, 0, 0, 0);
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(kb1 + kt * 2048), qf[1], acc, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // s[kt][r] = S[q][key = kt*16 + 4g + r]   (q already carries the 1/8 scale)
        if (qt + nwaves < nqt) load_q(qt + nwaves, qf);          // Q is dead from here on: the next tile's rows load under the softmax and P.V
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NQK; ++kt) {
            if (!NV) {                                             // run-time tail: per-element select
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kt * 16 + 4 * g + r >= T) s[kt][r] = -INFINITY;
            }
            mx = max3_raw(mx, s[kt][0], s[kt][1]);
            mx = max3_raw(mx, s[kt][2], s[kt][3]);
        }
        mx = xor16_max(mx);
        mx = xor32_max(mx);
        const float m2 = mx * 1.4426950408889634f;
        float sum = 0.f;
        f16x8 pf[NG];                                                // P^T packed as the B operand of P.V
#pragma unroll
        for (int grp = 0; grp < NG; ++grp) {
            f32x4 e0, e1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                e0[r] = __builtin_amdgcn_exp2f(fmaf(s[2 * grp][r], 1.4426950408889634f, -m2));
                if (2 * grp + 1 < NQK) e1[r] = __builtin_amdgcn_exp2f(fmaf(s[2 * grp + 1 < NQK ? 2 * grp + 1 : 0][r], 1.4426950408889634f, -m2));
            }
            sum += ((e0[0] + e0[1]) + (e0[2] + e0[3])) + ((e1[0] + e1[1]) + (e1[2] + e1[3]));
            pf[grp] = f16x8{(f16)e0[0], (f16)e0[1], (f16)e0[2], (f16)e0[3], (f16)e1[0], (f16)e1[1], (f16)e1[2], (f16)e1[3]};
        }
        sum = xor16_add(sum);
        sum = xor32_add(sum);

        // ---- O^T = V^T P^T: V through the hardware-transposing LDS read, 8 reads + 4 MFMAs per group
        f32x4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s2 = 0; s2 < NG; ++s2) {
            f16x8 vf[4];
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) s16x4*)(vb[dt] + s2 * 4096));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) s16x4*)(vb[dt] + s2 * 4096 + 2048));
                union { struct { s16x4 a, b; } s; f16x8 v; } u;
                u.s.a = lo; u.s.b = hi;
                vf[dt] = u.v;
            }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[dt], pf[s2], o[dt], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (out_sc) {                                   // MX-fp8 context (wave-uniform branch; full-frame mode only)
            attn_store_f8(o, 1.0f / sum, reinterpret_cast<uint8_t*>(out_v), out_sc, sc_ld, (size_t)b * T + q, q < nq, D, hd, g);
        } else if (q < nq) {
            const float inv = 1.0f / sum;
            f16* orow = out + (q_cls ? (size_t)b : (size_t)b * T + q) * D + hd * 64 + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const f32x4 w = o[dt] * inv;
                f16x4 hv = {(f16)w[0], (f16)w[1], (f16)w[2], (f16)w[3]};
                *reinterpret_cast<f16x4*>(orow + 16 * dt) = hv;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Streaming variant for long token sequences (T > 288, e.g. ViT-L/16 at 518x518: T = 1029), where
// K and V of one head (2 x 132 KB) no longer fit the LDS: one workgroup = 8 waves = 128 queries of
// one (frame, head); keys stream through a double-buffered 64-key LDS block with an online softmax
// (running max m, partial sums l, O rescaled by exp2((m_old - m_new) log2e) per block).  Same
// S^T = K Q^T / P^T-as-B-operand / transposing-read-of-V layout as the resident kernel: a lane's
// accumulators all belong to ONE query, so the rescale is a per-lane scalar.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 2) void attention_stream_kernel(const f16* __restrict__ qkv, const f16* __restrict__ q_cls,
                                                                  void* __restrict__ out_v, uint32_t* __restrict__ out_sc, int sc_ld,
                                                                  int T, int D, int n_heads) {
    f16* __restrict__ out = reinterpret_cast<f16*>(out_v);
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * 64 * 128];    // [buf][K|V][64 keys][128 B]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / n_heads, hd = blockIdx.x - b * n_heads;
    const size_t ld = (size_t)3 * D;
    const f16* qbase = qkv + (size_t)b * T * ld + hd * 64;
    const f16* kbase = qbase + D;
    const f16* vbase = qbase + 2 * D;
    const int g = lane >> 4, li = lane & 15;
    const int nkb = (T + 63) >> 6;
    const int q = (blockIdx.y * 8 + wave) * 16 + li;
    const int nq = q_cls ? 1 : T;                              // CLS-query mode: see attention_kernel
    const bool wave_active = (blockIdx.y * 8 + wave) * 16 < nq;   // wave-uniform; idle waves still stage K/V
    const int qrow = q < nq ? q : nq - 1;
    const f16* qsrc = q_cls ? q_cls + (size_t)b * D + hd * 64 : qbase + (size_t)qrow * ld;
    f16x8 qf[2];
    qf[0] = *reinterpret_cast<const f16x8*>(qsrc + g * 8);
    qf[1] = *reinterpret_cast<const f16x8*>(qsrc + 32 + g * 8);

    const int sr = tid >> 3, sc = tid & 7;                     // staging: one 16-byte chunk of K and of V per thread
    auto load_blk = [&](int kb, f16x8& kv, f16x8& vv) {
        const int r = kb * 64 + sr;
        kv = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        vv = kv;
        if (r < T) {
            kv = *reinterpret_cast<const f16x8*>(kbase + (size_t)r * ld + sc * 8);
            vv = *reinterpret_cast<const f16x8*>(vbase + (size_t)r * ld + sc * 8);
        }
    };
    auto store_blk = [&](int buf, const f16x8& kv, const f16x8& vv) {
        char* Kb = smem + buf * 16384;
        *reinterpret_cast<f16x8*>(Kb + k_off(sr, sc)) = kv;
        *reinterpret_cast<f16x8*>(Kb + 8192 + v_off(sr, sc * 8)) = vv;
    };
    f16x8 kv, vv;
    load_blk(0, kv, vv);
    store_blk(0, kv, vv);
    __syncthreads();

    float m = -INFINITY, l = 0.f;                              // m: shared by the 4 lane groups of a query; l: per-lane partial
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kb = 0; kb < nkb; ++kb) {
        if (kb + 1 < nkb) load_blk(kb + 1, kv, vv);
        const char* Ks = smem + (kb & 1) * 16384;
        const char* Vs = Ks + 8192;
        if (wave_active) {
        f32x4 s[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(Ks + k_off(kt * 16 + li, g)), qf[0], acc, 0, 0, 0);
            s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(Ks + k_off(kt * 16 + li, 4 + g)), qf[1], acc, 0, 0, 0);
        }
        float bm = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (kb * 64 + kt * 16 + 16 > T) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kb * 64 + kt * 16 + 4 * g + r >= T) s[kt][r] = -INFINITY;
            }
            bm = fmaxf(bm, fmaxf(fmaxf(s[kt][0], s[kt][1]), fmaxf(s[kt][2], s[kt][3])));
        }
        bm = xor16_max(bm);
        bm = xor32_max(bm);
        const float m_new = fmaxf(m, bm);                      // finite: block 0 always holds key 0
        const float alpha = __builtin_amdgcn_exp2f((m - m_new) * 1.4426950408889634f);
        const float m2 = m_new * 1.4426950408889634f;
        m = m_new;
        float bs = 0.f;
        f16x8 pf[2];
#pragma unroll
        for (int grp = 0; grp < 2; ++grp) {
            f32x4 e0, e1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                e0[r] = __builtin_amdgcn_exp2f(fmaf(s[2 * grp][r], 1.4426950408889634f, -m2));
                e1[r] = __builtin_amdgcn_exp2f(fmaf(s[2 * grp + 1][r], 1.4426950408889634f, -m2));
            }
            bs += ((e0[0] + e0[1]) + (e0[2] + e0[3])) + ((e1[0] + e1[1]) + (e1[2] + e1[3]));
            pf[grp] = f16x8{(f16)e0[0], (f16)e0[1], (f16)e0[2], (f16)e0[3], (f16)e1[0], (f16)e1[1], (f16)e1[2], (f16)e1[3]};
        }
        l = l * alpha + bs;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = o[dt] * alpha;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const int krow = 32 * s2 + 4 * g + (li >> 2);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const int col = 16 * dt + 4 * (li & 3);
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) s16x4*)(Vs + v_off(krow, col)));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) s16x4*)(Vs + v_off(krow + 16, col)));
                union { struct { s16x4 a, b; } s; f16x8 v; } u;
                u.s.a = lo; u.s.b = hi;
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(u.v, pf[s2], o[dt], 0, 0, 0);
            }
        }
        }
        if (kb + 1 < nkb) store_blk((kb + 1) & 1, kv, vv);
        __syncthreads();
    }
    l = xor16_add(l);
    l = xor32_add(l);
    if (out_sc) {
        if (wave_active) attn_store_f8(o, 1.0f / l, reinterpret_cast<uint8_t*>(out_v), out_sc, sc_ld, (size_t)b * T + q, q < nq, D, hd, g);
    } else if (q < nq) {
        const float inv = 1.0f / l;
        f16* orow = out + (q_cls ? (size_t)b : (size_t)b * T + q) * D + hd * 64 + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const f32x4 w = o[dt] * inv;
            f16x4 hv = {(f16)w[0], (f16)w[1], (f16)w[2], (f16)w[3]};
            *reinterpret_cast<f16x4*>(orow + 16 * dt) = hv;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Streaming variant, second form (r2): the same per-wave arithmetic with KT key tiles (16*KT keys) per block, K/V
// blocks staged by 16-byte LDS-DMA into a 2-deep ring (no VGPR round trip, no LDS-write pass) and ONE raw barrier
// per block: iteration kb waits for its own pieces of block kb (vmcnt(0): they were issued one iteration earlier),
// joins the barrier (every wave's pieces have landed AND every wave is done reading the other buffer), issues block
// kb+1 into that other buffer and computes on block kb.  Twice the keys per block halve the barriers and the online
// softmax rescales and double the independent MFMA chains in flight (the kernel is dependency-bound: PMC in DESIGN.md).
// Rows past T re-read row T-1 (finite; their scores are masked to -inf before the max).
// ---------------------------------------------------------------------------------------------
template <int KT, bool RS>
__global__ __launch_bounds__(512, KT <= 4 ? 6 : 2) void attention_stream2_kernel(const f16* __restrict__ qkv, const f16* __restrict__ q_cls,
                                                                   void* __restrict__ out_v, uint32_t* __restrict__ out_sc, int sc_ld,
                                                                   int T, int D, int n_heads) {
    constexpr int KB = KT * 16;                                  // keys per block
    constexpr int BLK = KB * 128;                                // bytes of one K (or V) block image
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * BLK];   // [buf][K | V][KB keys][128 B]
    f16* __restrict__ out = reinterpret_cast<f16*>(out_v);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / n_heads, hd = blockIdx.x - b * n_heads;
    const size_t ld = (size_t)3 * D;
    const f16* qbase = qkv + (size_t)b * T * ld + hd * 64;
    const f16* kbase = qbase + D;
    const f16* vbase = qbase + 2 * D;
    const int g = lane >> 4, li = lane & 15;
    const int nkb = (T + KB - 1) / KB;
    const int q = (blockIdx.y * 8 + wave) * 16 + li;
    const int nq = q_cls ? 1 : T;                              // CLS-query mode: see attention_kernel
    const bool wave_active = (blockIdx.y * 8 + wave) * 16 < nq;   // wave-uniform; idle waves still stage K/V
    const int qrow = q < nq ? q : nq - 1;
    const f16* qsrc = q_cls ? q_cls + (size_t)b * D + hd * 64 : qbase + (size_t)qrow * ld;
    f16x8 qf[2];
    qf[0] = *reinterpret_cast<const f16x8*>(qsrc + g * 8);
    qf[1] = *reinterpret_cast<const f16x8*>(qsrc + 32 + g * 8);

    // staging: KB/8 pieces of 1 KiB per image, piece p to wave p mod 8 (KT = 8: two K and two V pieces per wave)
    const int pr = lane >> 3, pos = lane & 7;
    auto stage = [&](int kb) {
        char* Kd = smem + (kb & 1) * 2 * BLK;
        char* Vd = Kd + BLK;
#pragma unroll
        for (int s2 = 0; s2 < KB / 64; ++s2) {
            const int p = wave + 8 * s2;
            const int r = p * 8 + pr;                            // row within the block
            int gr = kb * KB + r;
            gr = gr < T ? gr : T - 1;
            const int kc = pos ^ ((r >> 1) & 7);
            const int vc = (((pos >> 1) ^ ((r >> 1) & 3)) << 1) | (pos & 1);
            __builtin_amdgcn_global_load_lds(GLB_PTR(kbase + (size_t)gr * ld + kc * 8), LDS_PTR(Kd + p * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(GLB_PTR(vbase + (size_t)gr * ld + vc * 8), LDS_PTR(Vd + p * 1024), 16, 0, 0);
        }
    };
    stage(0);

    // The row sum l rides on a fifth P.V MFMA per key group against an all-ones "V" tile: every row of that product is
    // sum_k P[k][query], so lane (g, li) holds the running sum of ITS query four times over - no adds per score, no
    // cross-lane reduction at the end, and the sum is taken over the same fp16-rounded probabilities that multiply V.
    // (This kernel is VALU-bound: 9 -> 4 VALU instructions per score in r2, the add was one of the four.)
    // RS = false: the sum is kept in fp32 on the VALU (r2 form).  Measured at ViT-L/518 batch 32, same device: see DESIGN.md.
    float m = -INFINITY, l = 0.f;
    f32x4 ol = {0.f, 0.f, 0.f, 0.f};
    const f16x8 ones = {(f16)1.f, (f16)1.f, (f16)1.f, (f16)1.f, (f16)1.f, (f16)1.f, (f16)1.f, (f16)1.f};
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kb = 0; kb < nkb; ++kb) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // this wave's pieces of block kb
        __builtin_amdgcn_s_barrier();                            // everyone's; and buffer (kb+1)&1 is free
        if (kb + 1 < nkb) stage(kb + 1);
        const char* Ks = smem + (kb & 1) * 2 * BLK;
        const char* Vs = Ks + BLK;
        if (wave_active) {
            f32x4 s[KT];
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(Ks + k_off(kt * 16 + li, g)), qf[0], acc, 0, 0, 0);
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(Ks + k_off(kt * 16 + li, 4 + g)), qf[1], acc, 0, 0, 0);
            }
            if (kb == nkb - 1) {                                 // only the last block can hold keys past T (scalar branch)
                const int k0 = kb * KB + 4 * g;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (k0 + kt * 16 + r >= T) s[kt][r] = -INFINITY;
            }
            float bm = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                bm = max3_raw(bm, s[kt][0], s[kt][1]);
                bm = max3_raw(bm, s[kt][2], s[kt][3]);
            }
            bm = xor16_max(bm);
            bm = xor32_max(bm);
            const float m_new = fmaxf(m, bm);                    // finite: block 0 always holds key 0
            const float alpha = __builtin_amdgcn_exp2f((m - m_new) * 1.4426950408889634f);
            const float m2 = m_new * 1.4426950408889634f;
            m = m_new;
            float bs = 0.f;
            f16x8 pf[KT / 2];
#pragma unroll
            for (int grp = 0; grp < KT / 2; ++grp) {
                f32x4 e0, e1;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    e0[r] = __builtin_amdgcn_exp2f(fmaf(s[2 * grp][r], 1.4426950408889634f, -m2));
                    e1[r] = __builtin_amdgcn_exp2f(fmaf(s[2 * grp + 1][r], 1.4426950408889634f, -m2));
                }
                // add_np: the same sums in the same order, not paired into v_pk_add_f32 with cross-half selection (common.h)
                if (!RS) bs += add_np(add_np(add_np(e0[0], e0[1]), add_np(e0[2], e0[3])), add_np(add_np(e1[0], e1[1]), add_np(e1[2], e1[3])));
                pf[grp] = f16x8{(f16)e0[0], (f16)e0[1], (f16)e0[2], (f16)e0[3], (f16)e1[0], (f16)e1[1], (f16)e1[2], (f16)e1[3]};
            }
            if (RS) ol = ol * alpha;
            else l = l * alpha + bs;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt] = o[dt] * alpha;
#pragma unroll
            for (int s2 = 0; s2 < KT / 2; ++s2) {
                const int krow = 32 * s2 + 4 * g + (li >> 2);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const int col = 16 * dt + 4 * (li & 3);
                    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) s16x4*)(Vs + v_off(krow, col)));
                    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) s16x4*)(Vs + v_off(krow + 16, col)));
                    union { struct { s16x4 a, b; } s; f16x8 v; } u;
                    u.s.a = lo; u.s.b = hi;
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(u.v, pf[s2], o[dt], 0, 0, 0);
                }
                if (RS) ol = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, pf[s2], ol, 0, 0, 0);
            }
        }
    }
    if (RS) {
        l = ol[0];
    } else {
        l = xor16_add(l);
        l = xor32_add(l);
    }
    if (out_sc) {
        if (wave_active) attn_store_f8(o, 1.0f / l, reinterpret_cast<uint8_t*>(out_v), out_sc, sc_ld, (size_t)b * T + q, q < nq, D, hd, g);
    } else if (q < nq) {
        const float inv = 1.0f / l;
        f16* orow = out + (q_cls ? (size_t)b : (size_t)b * T + q) * D + hd * 64 + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const f32x4 w = o[dt] * inv;
            f16x4 hv = {(f16)w[0], (f16)w[1], (f16)w[2], (f16)w[3]};
            *reinterpret_cast<f16x4*>(orow + 16 * dt) = hv;
        }
    }
}

template <int NKT, int NV, int SPLIT>
int launch_attention_t(const f16* qkv, const f16* q_cls, void* out, uint32_t* out_sc, int sc_ld, int n, int T, int D, int n_heads,
                       hipStream_t stream) {
    constexpr int lds = (NV ? NV : NKT) * 16 * 128 * 2;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_kernel<NKT, NV, SPLIT>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
            return -2;
        attr_set = true;
    }
    if (SPLIT == 2) {                            // two 4-wave workgroups per (frame, head), grid padded to 16
        const int pairs = n * n_heads;
        hipLaunchKernelGGL((attention_kernel<NKT, NV, 2>), dim3(((pairs + 7) / 8) * 16), dim3(256), lds, stream, qkv, q_cls, out,
                           out_sc, sc_ld, T, D, n_heads, pairs);
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    // at most 8 waves (a 1024-thread bound caps the kernel at 128 VGPRs and it spills); the fewest waves that keep
    // every wave equally loaded: T = 201 -> 13 tiles -> 7 waves x 2, T = 261 -> 17 tiles -> 6 waves x 3
    constexpr int maxw = 8;                  // measured: 13 waves x 1 tile (35 us) loses to 7 waves x 2 tiles (29.6 us) at T = 201
    const int nqt = (T + 15) / 16, rounds = (nqt + maxw - 1) / maxw;
    static const int waves_env = [] { const char* e = getenv("CBAS_ATTN_WAVES"); return e ? atoi(e) : 0; }();      // experiments
    int nwaves = q_cls ? 4 : (nqt + rounds - 1) / rounds;             // CLS mode: one query tile, 4 waves stage K/V
    if (!q_cls && waves_env > 0 && waves_env <= 8) nwaves = waves_env;
    hipLaunchKernelGGL((attention_kernel<NKT, NV, 1>), dim3(n * n_heads), dim3(64 * nwaves), lds, stream, qkv, q_cls, out, out_sc,
                       sc_ld, T, D, n_heads, n * n_heads);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---------------------------------------------------------------------------------------------
// weight packing (runs once at create)
// ---------------------------------------------------------------------------------------------
__global__ void convert_f16_kernel(const float* __restrict__ src, f16* __restrict__ hi, f16* __restrict__ lo, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = src[i];
    const f16 h = (f16)v;
    hi[i] = h;
    if (lo) lo[i] = (f16)(v - (float)h);
}

// gated MLP: out row r of [2F][K] = gate row 32 (r / 64) + r % 64 when r % 64 < 32, else up row 32 (r / 64) + r % 64 - 32
// (EPI_SWIGLU, kernels.h); n = 2 F K elements
__global__ void interleave_gate_up_kernel(const float* __restrict__ gate, const float* __restrict__ up, float* __restrict__ out,
                                          int64_t n, int K) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t r = i / K;
    const int k = (int)(i - r * K), in = (int)(r & 63);
    const int64_t src = ((r >> 6) * 32 + (in & 31)) * K + k;
    out[i] = in < 32 ? gate[src] : up[src];
}

// One thread per 32-element block of a [N][K] weight: E8M0 scale (no clipping) + 32 e4m3 bytes.
__global__ void pack_fp8_weight_kernel(const float* __restrict__ src, uint8_t* __restrict__ w8, uint32_t* __restrict__ sc,
                                       int N, int K, int n_total, int n0) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int kb_per_row = K / 32;
    if (gid >= (int64_t)N * kb_per_row) return;
    const int n = (int)(gid / kb_per_row), kb = (int)(gid - (int64_t)n * kb_per_row);
    const float* p = src + (size_t)n * K + kb * 32;
    f32x4 v[8];
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = reinterpret_cast<const f32x4*>(p)[i];
        a = fmaxf(a, fmaxf(fmaxf(fabsf(v[i][0]), fabsf(v[i][1])), fmaxf(fabsf(v[i][2]), fabsf(v[i][3]))));
    }
    const int sb = mx_scale_byte(a);
    const float inv = mx_inv_scale(sb);
    unsigned* o = reinterpret_cast<unsigned*>(w8 + (size_t)n * K + kb * 32);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = cvt4_e4m3(v[i][0] * inv, v[i][1] * inv, v[i][2] * inv, v[i][3] * inv);
    reinterpret_cast<uint8_t*>(sc)[((size_t)(kb >> 2) * n_total + n0 + n) * 4 + (kb & 3)] = (uint8_t)sb;
}

// w: (D,3,ps,ps).  hi/lo: (D,256) with the 16x16 slot layout (zero where i >= ps or j >= ps);
// hi2/lo2: (D,512) = [W' | W'] for the float-input path (fp16(x) | residual share W')
__global__ void pack_patch_weight_kernel(const float* __restrict__ w, f16* __restrict__ hi, f16* __restrict__ lo,
                                         f16* __restrict__ hi2, f16* __restrict__ lo2, int D, int ps) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;     // over D*256
    if (idx >= D * 256) return;
    const int d = idx >> 8, k = idx & 255, i = k >> 4, j = k & 15;
    float v = 0.f;
    if (i < ps && j < ps) {
        const float* base = w + (size_t)d * 3 * ps * ps + i * ps + j;
        v = (base[0] + base[ps * ps]) + base[2 * ps * ps];     // sum over the 3 identical input channels
    }
    const f16 h = (f16)v;
    const f16 l = (f16)(v - (float)h);
    hi[idx] = h;
    hi2[d * 512 + k] = h;
    hi2[d * 512 + 256 + k] = h;
    if (lo) { lo[idx] = l; lo2[d * 512 + k] = l; lo2[d * 512 + 256 + k] = l; }
}

}  // namespace

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -2)

// what every ingest launcher refuses (-1): a null pointer, no frame, a patch size without a 16 x 16 slot layout, a frame smaller
// than one patch, no prefix row, rows of x that are no whole 16-byte vectors, a T that does not hold the frame's rows
bool im2col_args_ok(const void* frames, const void* A, const float* x, const float* prefix_tokens, int n, int height, int width,
                    int n_prefix, int D, int T, int ps) {
    if (!frames || !A || !x || !prefix_tokens || n <= 0 || (ps != 14 && ps != 16) || height < ps || width < ps) return false;
    return n_prefix >= 1 && D > 0 && D % 4 == 0 && (int64_t)T >= (int64_t)(height / ps) * (width / ps) + n_prefix;
}

int launch_im2col_u8(const uint8_t* frames, int n, int height, int width, int64_t frame_stride,
                     int64_t row_stride, int64_t pixel_stride, f16* A, float* x, const float* prefix_tokens,
                     int n_prefix, int D, int T, int ps, hipStream_t stream) {
    // strides as cbas_enc_submit_u8_host accepts them (a frame stride of 0 reads one frame n times)
    if (!im2col_args_ok(frames, A, x, prefix_tokens, n, height, width, n_prefix, D, T, ps) || frame_stride < 0 || row_stride < 0 ||
        pixel_stride < 1)
        return -1;
    const int nh = height / ps, nw = width / ps;
    const int64_t total = (int64_t)n * nh * ps * nw;
    hipLaunchKernelGGL(im2col_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, frames, n,
                       height, width, frame_stride, row_stride, pixel_stride, A, nh, nw, ps);
    const int64_t tp = (int64_t)n * n_prefix * (D / 4);
    hipLaunchKernelGGL(write_prefix_kernel, dim3((unsigned)((tp + 255) / 256)), dim3(256), 0, stream, x, prefix_tokens,
                       n, n_prefix, D, T);
    return CHECK_LAUNCH();
}

int launch_im2col_f32(const float* frames, int n, int height, int width, f16* A, float* x,
                      const float* prefix_tokens, int n_prefix, int D, int T, int ps, hipStream_t stream) {
    if (!im2col_args_ok(frames, A, x, prefix_tokens, n, height, width, n_prefix, D, T, ps)) return -1;
    const int nh = height / ps, nw = width / ps;
    const int64_t total = (int64_t)n * nh * ps * nw;
    hipLaunchKernelGGL(im2col_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, frames, n,
                       height, width, A, nh, nw, ps);
    const int64_t tp = (int64_t)n * n_prefix * (D / 4);
    hipLaunchKernelGGL(write_prefix_kernel, dim3((unsigned)((tp + 255) / 256)), dim3(256), 0, stream, x, prefix_tokens,
                       n, n_prefix, D, T);
    return CHECK_LAUNCH();
}

int launch_layernorm_f16(const float* x, int64_t ldx, const float* gamma, const float* beta, f16* out, int M, int D,
                         float eps, hipStream_t stream) {
    if (M <= 0 || D <= 0 || D % 4 || ldx < D) return -1;     // rows are read as 16-byte vectors
    const int nv = (D / 4 + 63) / 64;
    const dim3 grid((M + 3) / 4), block(256);
    switch (nv) {
        case 1: hipLaunchKernelGGL(layernorm_f16_kernel<1>, grid, block, 0, stream, x, ldx, gamma, beta, out, M, D, eps); break;
        case 2: hipLaunchKernelGGL(layernorm_f16_kernel<2>, grid, block, 0, stream, x, ldx, gamma, beta, out, M, D, eps); break;
        case 3: hipLaunchKernelGGL(layernorm_f16_kernel<3>, grid, block, 0, stream, x, ldx, gamma, beta, out, M, D, eps); break;
        case 4: hipLaunchKernelGGL(layernorm_f16_kernel<4>, grid, block, 0, stream, x, ldx, gamma, beta, out, M, D, eps); break;
        case 5: hipLaunchKernelGGL(layernorm_f16_kernel<5>, grid, block, 0, stream, x, ldx, gamma, beta, out, M, D, eps); break;      // D = 1280 (ViT-H+)
        default: return -1;
    }
    return CHECK_LAUNCH();
}

int launch_ln_stats_x16(const float* x, f16* x16, float2* ln_out, int ln_ld, int M, int D, hipStream_t stream) {
    if (D % 256 || D > 1024) return -1;
    const dim3 grid((M + 3) / 4), block(256);
    switch (D / 256) {
        case 1: hipLaunchKernelGGL(ln_stats_x16_kernel<1>, grid, block, 0, stream, x, x16, ln_out, ln_ld, M, D); break;
        case 2: hipLaunchKernelGGL(ln_stats_x16_kernel<2>, grid, block, 0, stream, x, x16, ln_out, ln_ld, M, D); break;
        case 3: hipLaunchKernelGGL(ln_stats_x16_kernel<3>, grid, block, 0, stream, x, x16, ln_out, ln_ld, M, D); break;
        default: hipLaunchKernelGGL(ln_stats_x16_kernel<4>, grid, block, 0, stream, x, x16, ln_out, ln_ld, M, D); break;
    }
    return CHECK_LAUNCH();
}

int launch_fold_ln_weight(const float* W, const float* gamma, const float* beta, const float* b, f16* Wf, float* colsum,
                          float* biasf, int N, int K, hipStream_t stream) {
    hipLaunchKernelGGL(fold_ln_weight_kernel, dim3(N), dim3(256), 0, stream, W, gamma, beta, b, Wf, colsum, biasf, K);
    return CHECK_LAUNCH();
}

int launch_layernorm_f8(const float* x, int64_t ldx, const float* gamma, const float* beta, uint8_t* out8,
                        uint32_t* out_sc, int sc_ld, int M, int D, float eps, hipStream_t stream) {
    // precision 2 runs D = 256 .. 1024 (cbas_enc_create refuses other handles; the fp8 GEMMs take K-tiles of 128 in pairs)
    if (D % 128 || D < 256 || D > 1024 || M <= 0 || ldx < D || sc_ld < M) return -1;
    const int nv = (D / 4 + 63) / 64;
    const dim3 grid((M + 3) / 4), block(256);
    switch (nv) {
        case 1: hipLaunchKernelGGL(layernorm_f8_kernel<1>, grid, block, 0, stream, x, ldx, gamma, beta, out8, out_sc, sc_ld, M, D, eps); break;      // D = 256
        case 2: hipLaunchKernelGGL(layernorm_f8_kernel<2>, grid, block, 0, stream, x, ldx, gamma, beta, out8, out_sc, sc_ld, M, D, eps); break;
        case 3: hipLaunchKernelGGL(layernorm_f8_kernel<3>, grid, block, 0, stream, x, ldx, gamma, beta, out8, out_sc, sc_ld, M, D, eps); break;
        case 4: hipLaunchKernelGGL(layernorm_f8_kernel<4>, grid, block, 0, stream, x, ldx, gamma, beta, out8, out_sc, sc_ld, M, D, eps); break;
        default: return -1;
    }
    return CHECK_LAUNCH();
}

int launch_final_norm_cls(const float* x, const float* gamma, const float* beta, float* cls_f32,
                          f16* cls_f16, int n, int T, int D, float eps, hipStream_t stream, unsigned* nonfinite) {
    if (n <= 0 || T <= 0 || D <= 0 || D % 4) return -1;
    const int nv = (D / 4 + 63) / 64;
    const dim3 grid((n + 3) / 4), block(256);
    switch (nv) {
        case 1: hipLaunchKernelGGL(final_norm_cls_kernel<1>, grid, block, 0, stream, x, gamma, beta, cls_f32, cls_f16, n, T, D, eps, nonfinite); break;
        case 2: hipLaunchKernelGGL(final_norm_cls_kernel<2>, grid, block, 0, stream, x, gamma, beta, cls_f32, cls_f16, n, T, D, eps, nonfinite); break;
        case 3: hipLaunchKernelGGL(final_norm_cls_kernel<3>, grid, block, 0, stream, x, gamma, beta, cls_f32, cls_f16, n, T, D, eps, nonfinite); break;
        case 4: hipLaunchKernelGGL(final_norm_cls_kernel<4>, grid, block, 0, stream, x, gamma, beta, cls_f32, cls_f16, n, T, D, eps, nonfinite); break;
        case 5: hipLaunchKernelGGL(final_norm_cls_kernel<5>, grid, block, 0, stream, x, gamma, beta, cls_f32, cls_f16, n, T, D, eps, nonfinite); break;      // D = 1280 (ViT-H+)
        default: return -1;
    }
    return CHECK_LAUNCH();
}

int launch_attention(const f16* qkv, const f16* q_cls, void* out, uint32_t* out_sc, int sc_ld, int n, int T, int D, int n_heads,
                     hipStream_t stream) {
    if (q_cls && out_sc) return -1;                 // the CLS tail of the last layer stays fp16
    const int nkt = (T + 15) / 16;
    // exact-tile-count instantiations for the sequence lengths CBAS produces: 224x224 /16 -> T = 201 (13 tiles),
    // 256x256 /16 and 224x224 /14 -> T = 261 (17 tiles); everything else takes the run-time-masked form
    static const int split_env = [] { const char* e = getenv("CBAS_ATTN_SPLIT"); return e ? atoi(e) : 1; }();    // experiments
    const bool split = split_env == 2 && !q_cls;
    if (nkt == 13) return split ? launch_attention_t<14, 13, 2>(qkv, q_cls, out, out_sc, sc_ld, n, T, D, n_heads, stream)
                                : launch_attention_t<14, 13, 1>(qkv, q_cls, out, out_sc, sc_ld, n, T, D, n_heads, stream);
    if (nkt == 17) return split ? launch_attention_t<18, 17, 2>(qkv, q_cls, out, out_sc, sc_ld, n, T, D, n_heads, stream)
                                : launch_attention_t<18, 17, 1>(qkv, q_cls, out, out_sc, sc_ld, n, T, D, n_heads, stream);
    if (nkt <= 2) return launch_attention_t<2, 0, 1>(qkv, q_cls, out, out_sc, sc_ld, n, T, D, n_heads, stream);
    if (nkt <= 6) return launch_attention_t<6, 0, 1>(qkv, q_cls, out, out_sc, sc_ld, n, T, D, n_heads, stream);
    if (nkt <= 14) return launch_attention_t<14, 0, 1>(qkv, q_cls, out, out_sc, sc_ld, n, T, D, n_heads, stream);
    if (nkt <= 18) return launch_attention_t<18, 0, 1>(qkv, q_cls, out, out_sc, sc_ld, n, T, D, n_heads, stream);
    // T > 288: K/V no longer fit the LDS -> streaming kernel, 128 queries per workgroup
    const int nqb = q_cls ? 1 : ((T + 15) / 16 + 7) / 8;
    // default: 64-key blocks (KT = 4: 74 VGPRs, 32 KiB of LDS -> three workgroups per CU; 217 us at ViT-L/518 batch 32);
    // CBAS_ATTN_STREAM=2: 128-key blocks (two workgroups per CU, 235 us); 1: the first form
    static const int stream_env = [] { const char* e = getenv("CBAS_ATTN_STREAM"); return e ? atoi(e) : 3; }();
    if (stream_env == 2) {
        hipLaunchKernelGGL((attention_stream2_kernel<8, false>), dim3(n * n_heads, nqb), dim3(512), 0, stream, qkv, q_cls, out, out_sc, sc_ld, T, D,
                           n_heads);
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    if (stream_env == 4) {                      // experiment: row sum on a fifth P.V MFMA against an all-ones tile
        hipLaunchKernelGGL((attention_stream2_kernel<4, true>), dim3(n * n_heads, nqb), dim3(512), 0, stream, qkv, q_cls, out, out_sc, sc_ld, T, D,
                           n_heads);
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    if (stream_env == 3) {
        hipLaunchKernelGGL((attention_stream2_kernel<4, false>), dim3(n * n_heads, nqb), dim3(512), 0, stream, qkv, q_cls, out, out_sc, sc_ld, T, D,
                           n_heads);
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    hipLaunchKernelGGL(attention_stream_kernel, dim3(n * n_heads, nqb), dim3(512), 0, stream, qkv, q_cls, out, out_sc, sc_ld, T, D, n_heads);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_interleave_gate_up(const float* gate, const float* up, float* out, int64_t F, int K, hipStream_t stream) {
    if (F <= 0 || F % 32 || K <= 0) return -1;
    const int64_t n = 2 * F * K;
    hipLaunchKernelGGL(interleave_gate_up_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, gate, up, out, n, K);
    return CHECK_LAUNCH();
}

int launch_convert_f16(const float* src, f16* hi, f16* lo, int64_t n, hipStream_t stream) {
    if (!src || !hi || n <= 0) return -1;
    hipLaunchKernelGGL(convert_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, hi, lo, n);
    return CHECK_LAUNCH();
}

int launch_pack_fp8_weight(const float* src, uint8_t* w8, uint32_t* sc, int N, int K, int n_total, int n0, hipStream_t stream) {
    if (N <= 0 || K % 128) return -1;
    const int64_t blocks = (int64_t)N * (K / 32);
    hipLaunchKernelGGL(pack_fp8_weight_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, stream, src, w8, sc, N, K,
                       n_total, n0);
    return CHECK_LAUNCH();
}

int launch_pack_patch_weight(const float* w, f16* hi, f16* lo, f16* hi2, f16* lo2, int D, int ps, hipStream_t stream) {
    // lo and lo2 are NULL together (the kernel tests lo alone); D * 512 elements are indexed in 32 bits
    if (!w || !hi || !hi2 || (lo == nullptr) != (lo2 == nullptr) || D <= 0 || D > (1 << 22) || (ps != 14 && ps != 16)) return -1;
    hipLaunchKernelGGL(pack_patch_weight_kernel, dim3((D * 256 + 255) / 256), dim3(256), 0, stream, w, hi, lo, hi2, lo2, D, ps);
    return CHECK_LAUNCH();
}
