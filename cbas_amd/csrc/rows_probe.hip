// A linear probe on resident CLS rows: cbas_rows_probe_workspace_bytes / cbas_rows_probe_fit /
// cbas_rows_probe_predict of include/cbas_mi355x.h, kernels and entry points in one file.  rows (N, D) fp16 with row stride ld,
// weights (C, D) fp32, bias (C) fp32.  The working row of a row x is always u = fl(x * rn), rn the reciprocal norm of rows_rn.h; no
// normalised copy is written, rn is applied where the row is used.
//
//   rows_rn_kernel     (rows_rn.h) rn of every training row, for the gradient
//   rp_check_kernel    a label outside [0, C) or a weight that is negative or not finite sets a flag, read back before the iteration
//   rp_rowsum_kernel   one workgroup per SEGMENT of RP_SEG rows: one fp32 chain over the segment's values in ascending row order (the
//                      sample weights once, the rows' loss terms every pass)
//   rp_omega_kernel    Omega = the segments' sums in ascending order; a flag when it is not a positive finite number
//   rp_forward_kernel  THE PASS, rkm_score_kernel's: a workgroup owns RP_TILE = 128 rows, wave w the two 16-row tiles 32 w .. 32 w + 31;
//                      the weights come through LDS in chunks of RP_KC = 64 columns of all (at most 64) classes, two buffers, the
//                      next chunk's global loads in flight under this chunk's MFMAs (v_mfma_f32_16x16x4_f32, exact products).
//                      x . w_c = chain0 + chain1 (cbas_rows_search's dot), z_c = fmaf(rn, x . w_c, b_c).  After the MFMAs the 16
//                      lanes fc = 0 .. 15 of a lane group hold one row's logits, lane fc the classes fc, 16 + fc, ..:
//                        mx  = the largest logit (a maximum has no order)
//                        e_c = expf(z_c - mx);  S = the lane's e_c added in ascending c, then the xor tree 1, 2, 4, 8 over the lanes
//                        p_c = e_c / S;  lse = mx + logf(S)
//                      PREDICT writes p and, unless NULL, z.  TRAIN writes r_c = fl(omega * (p_c - [c = y])) and the row's loss term
//                      fl(omega * (lse - z_y)), and workgroup 0 the squared norms |w_c|^2 (one fmaf chain, from 0, over d ascending)
//                      and |b|^2 (one chain over c ascending) of the weights it ran on.  A tile belongs to one wave from its first
//                      column to its last: neither the grid, nor N, nor where the row lies enters a sum.
//   rp_grad_kernel     one workgroup per SEGMENT and slab of 256 columns, wave w the columns 64 w .. 64 w + 63 of the slab: G_seg (C,
//                      D) = sum_m r_m (x) u_m on the fp32 matrix pipe, the MFMA's k dimension running over the segment's rows: every
//                      element is ONE fmaf chain, from 0, over the rows in ascending order.  u = fl(x * rn) is formed in registers.
//                      The bias column (u = 1: a plain fp32 sum of r in ascending row order) is wave 0's of slab 0.
//   rp_step_kernel     per element: the segments' partials added in ascending order, * (1 / Omega), + l2 v (one fmaf); then
//                      w' = fmaf(-1/L, g, v), v' = fmaf(beta, w' - w, w').  Thread 0: the loss of the weights the pass ran on.
// No atomics anywhere.
#include "kernels.h"
#include "rows_api.h"
#include "rows_rn.h"

#include <cmath>

namespace {

constexpr int RP_THREADS = 256;
constexpr int RP_TILE = 128;                         // rows a workgroup of the pass owns (tests/rows_probe_ref.py: TILE)
constexpr int RP_RT = 2;                             // 16-row tiles per wave
constexpr int RP_KC = 64;                            // columns per staged chunk of the weights
constexpr int RP_CLD = RP_KC + 4;                    // floats between the staged weight rows
constexpr int RP_SEG = CBAS_ROWS_PROBE_SEGMENT;
constexpr int RP_SLAB = 256;                         // columns per workgroup of the gradient: 64 a wave
constexpr int RP_MAX_C = 64, RP_MAX_D = 1536;
constexpr int64_t RP_MAX_M = 4194304;
constexpr int RP_NORMS = 80;                         // floats: |w_c|^2 of 64 classes, then |b|^2

struct RpPass {
    const uint16_t* rows;
    int64_t N;
    int D;
    int64_t ld;
    const float* w;                                  // (C, D)
    const float* b;                                  // (C)
    int C;
    float* probs;                                    // predict: (N, C);  train: NULL
    float* logits;                                   // predict: (N, C) or NULL
    const int32_t* label;                            // train: (N)
    const float* omega;                              // train: (N) or NULL = ones
    float* r;                                        // train: (N, C)
    float* ell;                                      // train: (N)
    float* norms;                                    // train: RP_NORMS floats
};

__global__ __launch_bounds__(RP_THREADS) void rp_check_kernel(const int32_t* __restrict__ label, const float* __restrict__ omega, int64_t M, int C,
                                                              unsigned* __restrict__ flags) {
    const int64_t m = (int64_t)blockIdx.x * RP_THREADS + threadIdx.x;
    if (m >= M) return;
    if ((unsigned)label[m] >= (unsigned)C) flags[0] = 1u;
    if (omega) {
        const float o = omega[m];
        if (!(o >= 0.f) || !(o <= 3.402823466e38f)) flags[1] = 1u;
    }
}

// grid (segments), 256 threads: out[seg] = the chain, from 0, over the segment's values in ascending row order; vals == NULL: ones
__global__ __launch_bounds__(RP_THREADS) void rp_rowsum_kernel(const float* __restrict__ vals, int64_t M, float* __restrict__ out) {
    __shared__ float sv[RP_SEG];
    const int64_t m0 = (int64_t)blockIdx.x * RP_SEG;
    const int n = (int)(M - m0 < RP_SEG ? M - m0 : RP_SEG);
    for (int i = threadIdx.x; i < n; i += RP_THREADS) sv[i] = vals ? vals[m0 + i] : 1.f;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) s = __fadd_rn(s, sv[i]);
        out[blockIdx.x] = s;
    }
}

// grid (1), 1 thread
__global__ void rp_omega_kernel(const float* __restrict__ pomega, int64_t nseg, float* __restrict__ omega, unsigned* __restrict__ flags) {
    float s = 0.f;
    for (int64_t g = 0; g < nseg; ++g) s = __fadd_rn(s, pomega[g]);
    omega[0] = s;
    if (!(s > 0.f) || !(s <= 3.402823466e38f)) flags[2] = 1u;
}

// grid (ceil(N / RP_TILE)), 256 threads, LDS 2 x 16 NG x RP_CLD floats + 16 NG
template <int NG, bool TRAIN>
__global__ __launch_bounds__(RP_THREADS) void rp_forward_kernel(RpPass a) {
    __shared__ __attribute__((aligned(16))) float sc[2][16 * NG * RP_CLD];
    __shared__ float sb[16 * NG];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fc = lane & 15, kr = lane >> 4;
    const int nb = a.D >> 5, nch = (a.D + RP_KC - 1) / RP_KC;
    const int64_t m0 = (int64_t)blockIdx.x * RP_TILE + 32 * wave;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const uint4 zero16 = {0u, 0u, 0u, 0u};

    const uint16_t* p[RP_RT];
    bool valid[RP_RT];
#pragma unroll
    for (int t = 0; t < RP_RT; ++t) {
        const int64_t m = m0 + 16 * t + fc;
        valid[t] = m < a.N;                                      // a row past the end is read as zeros and never written
        p[t] = a.rows + (valid[t] ? m : 0) * a.ld + 8 * kr;
    }
    // the 16-byte pieces of a chunk this thread stages: piece v is class (v 256 + tid) / 16, columns 4 ((v 256 + tid) % 16) .. + 3
    auto fetch_c = [&](int ch, f32x4 (&c)[NG]) {
#pragma unroll
        for (int v = 0; v < NG; ++v) {
            const int idx = v * RP_THREADS + tid, j = idx >> 4, col = ch * RP_KC + 4 * (idx & 15);
            c[v] = (j < a.C && col < a.D) ? *reinterpret_cast<const f32x4*>(a.w + (int64_t)j * a.D + col) : zero;
        }
    };
    auto stage_c = [&](float* buf, const f32x4 (&c)[NG]) {
#pragma unroll
        for (int v = 0; v < NG; ++v) {
            const int idx = v * RP_THREADS + tid;
            *reinterpret_cast<f32x4*>(buf + (idx >> 4) * RP_CLD + 4 * (idx & 15)) = c[v];
        }
    };
    auto fetch_x = [&](int ch, uint4 (&x)[RP_RT][2]) {
#pragma unroll
        for (int t = 0; t < RP_RT; ++t)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int c = 2 * ch + i;
                x[t][i] = (valid[t] && c < nb) ? *reinterpret_cast<const uint4*>(p[t] + 32 * c) : zero16;
            }
    };

    f32x4 cpre[NG];
    uint4 xb[RP_RT][2], xn[RP_RT][2];
    fetch_c(0, cpre);
    fetch_x(0, xb);
    if (tid < 16 * NG) sb[tid] = tid < a.C ? a.b[tid] : 0.f;
    stage_c(sc[0], cpre);
    __syncthreads();

    f32x4 acc[RP_RT][NG][2];
    float ss[RP_RT];
#pragma unroll
    for (int t = 0; t < RP_RT; ++t) {
        ss[t] = 0.f;
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[t][g][0] = acc[t][g][1] = zero;
    }
    float wn = 0.f;                                              // train, thread c < 16 NG of workgroup 0: |w_c|^2, one chain over d ascending
    const bool norms = TRAIN && blockIdx.x == 0 && tid < 16 * NG;

    for (int ch = 0; ch < nch; ++ch) {
        const bool more = ch + 1 < nch;
        if (more) {
            fetch_c(ch + 1, cpre);
            fetch_x(ch + 1, xn);
        }
        const float* const buf = sc[ch & 1];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (2 * ch + i < nb) {                               // block c = 2 ch + i: c % 2 = i
                f32x4 qa[NG], qv[NG];
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    const float* const qb = buf + (16 * g + fc) * RP_CLD + 32 * i + 8 * kr;
                    qa[g] = *reinterpret_cast<const f32x4*>(qb);
                    qv[g] = *reinterpret_cast<const f32x4*>(qb + 4);
                }
#pragma unroll
                for (int t = 0; t < RP_RT; ++t) {
                    const f16x8 h = __builtin_bit_cast(f16x8, xb[t][i]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float x = (float)h[e];
                        ss[t] = fmaf(x, x, ss[t]);
#pragma unroll
                        for (int g = 0; g < NG; ++g)
                            acc[t][g][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, e < 4 ? qa[g][e] : qv[g][e - 4], acc[t][g][i], 0, 0, 0);
                    }
                }
            }
        }
        if (norms) {
            const int w = a.D - ch * RP_KC < RP_KC ? a.D - ch * RP_KC : RP_KC;
            for (int d = 0; d < w; ++d) wn = fmaf(buf[tid * RP_CLD + d], buf[tid * RP_CLD + d], wn);
        }
        if (more) stage_c(sc[(ch & 1) ^ 1], cpre);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < RP_RT; ++t)
#pragma unroll
            for (int i = 0; i < 2; ++i) xb[t][i] = xn[t][i];
    }
    if (TRAIN && blockIdx.x == 0) {
        if (tid < 64) a.norms[tid] = tid < a.C ? wn : 0.f;       // NG < 4: the threads past 16 NG kept wn = 0
        if (tid == 64) {
            float bn = 0.f;
            for (int c = 0; c < a.C; ++c) bn = fmaf(sb[c], sb[c], bn);
            a.norms[64] = bn;
        }
    }
    float bl[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) bl[g] = sb[16 * g + fc];
    const float ninf = -__builtin_inff();

#pragma unroll
    for (int t = 0; t < RP_RT; ++t) {
        float s = ss[t];
        s += __shfl_xor(s, 16, 64);                              // (l0 + l1) and (l2 + l3), then their sum: the same bits in all four
        s += __shfl_xor(s, 32, 64);
        const float rn = rows_rn(s);
        // acc[t][g][.][e]: row 4 kr + e of the tile against class 16 g + fc; that row's rn sits in lane 4 kr + e
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float rn_row = __shfl(rn, 4 * kr + e, 64);
            const int64_t m = m0 + 16 * t + 4 * kr + e;
            const bool live = m < a.N;
            float z[NG], ex[NG];
            float mx = ninf;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                z[g] = 16 * g + fc < a.C ? fmaf(rn_row, __fadd_rn(acc[t][g][0][e], acc[t][g][1][e]), bl[g]) : ninf;
                mx = fmaxf(mx, z[g]);
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            float S = 0.f;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                ex[g] = 16 * g + fc < a.C ? expf(__fsub_rn(z[g], mx)) : 0.f;
                S = g == 0 ? ex[0] : __fadd_rn(S, ex[g]);
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) S = __fadd_rn(S, __shfl_xor(S, o, 64));   // a + b = b + a: the same bits in all sixteen
            if constexpr (TRAIN) {
                const int y = live ? a.label[m] : 0;
                const float om = (live && a.omega) ? a.omega[m] : 1.f;
                float zy = ninf;
#pragma unroll
                for (int g = 0; g < NG; ++g) zy = (16 * g + fc == y) ? z[g] : zy;
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) zy = fmaxf(zy, __shfl_xor(zy, o, 64));
                if (live) {
#pragma unroll
                    for (int g = 0; g < NG; ++g) {
                        const int c = 16 * g + fc;
                        if (c < a.C) {
                            const float pc = __fdiv_rn(ex[g], S);
                            a.r[m * a.C + c] = __fmul_rn(om, c == y ? __fsub_rn(pc, 1.f) : pc);
                        }
                    }
                    if (fc == 0) a.ell[m] = __fmul_rn(om, __fsub_rn(__fadd_rn(mx, logf(S)), zy));
                }
            } else {
                if (live) {
#pragma unroll
                    for (int g = 0; g < NG; ++g) {
                        const int c = 16 * g + fc;
                        if (c < a.C) {
                            a.probs[m * a.C + c] = __fdiv_rn(ex[g], S);
                            if (a.logits) a.logits[m * a.C + c] = z[g];
                        }
                    }
                }
            }
        }
    }
}

// grid (segments, ceil(D / RP_SLAB)), 256 threads.  Lane (fc, kr) of wave w holds, of the four rows 4 i + kr of a step, the four
// columns d0 + 4 fc .. + 3 (B operands of four MFMAs: column tile j is the columns d0 + 4 fc + j) and the classes 16 g + fc of r (the A
// operands); acc[g][j][e] is class 16 g + 4 kr + e, column d0 + 4 fc + j.
template <int NG>
__global__ __launch_bounds__(RP_THREADS) void rp_grad_kernel(const uint16_t* __restrict__ rows, int64_t M, int D, int64_t ld,
                                                             const float* __restrict__ rn, const float* __restrict__ r, int C,
                                                             float* __restrict__ pG, float* __restrict__ pb) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fc = lane & 15, kr = lane >> 4;
    const int64_t seg = blockIdx.x, m0 = seg * RP_SEG, m1 = m0 + RP_SEG < M ? m0 + RP_SEG : M;
    const int d0 = blockIdx.y * RP_SLAB + 64 * wave;
    if (d0 >= D) return;                                         // the whole wave
    const bool mine = d0 + 4 * fc < D;                           // D is a multiple of 32: the last wave may own 32 columns only
    const bool bias = blockIdx.y == 0 && wave == 0;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[NG][4], accb[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        accb[g] = zero;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[g][j] = zero;
    }
    const uint16_t* const px = rows + d0 + 4 * fc;
    for (int64_t mb = m0; mb < m1; mb += 16) {
        uint2 x[4];
        float sc[4], rr[4][NG];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t m = mb + 4 * i + kr;
            const bool ok = m < m1;                              // past the segment's end: zeros, fmaf(0, 0, acc) = acc
            x[i] = (ok && mine) ? *reinterpret_cast<const uint2*>(px + m * ld) : make_uint2(0u, 0u);
            sc[i] = ok ? rn[m] : 0.f;
#pragma unroll
            for (int g = 0; g < NG; ++g) rr[i][g] = (ok && 16 * g + fc < C) ? r[m * C + 16 * g + fc] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f16x4 h = __builtin_bit_cast(f16x4, x[i]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float u = __fmul_rn((float)h[j], sc[i]);
#pragma unroll
                for (int g = 0; g < NG; ++g) acc[g][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(rr[i][g], u, acc[g][j], 0, 0, 0);
            }
            if (bias) {
#pragma unroll
                for (int g = 0; g < NG; ++g) accb[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(rr[i][g], 1.f, accb[g], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 16 * g + 4 * kr + e;
            if (c >= C) continue;
            const f32x4 out = {acc[g][0][e], acc[g][1][e], acc[g][2][e], acc[g][3][e]};
            if (mine) *reinterpret_cast<f32x4*>(pG + (seg * C + c) * D + d0 + 4 * fc) = out;
            if (bias && fc == 0) pb[seg * 64 + c] = accb[g][e];
        }
}

struct RpStep {
    const float* pG;                                 // (nseg, C, D)
    const float* pb;                                 // (nseg, 64)
    const float* ploss;                              // (nseg)
    const float* omega;                              // Omega
    const float* norms;                              // RP_NORMS
    int64_t nseg;
    int C, D;
    float l2, inv_l, beta;
    int update;                                      // 0: the loss only
    float* w;                                        // C D weights, then 64 floats of bias
    float* v;
    float* loss;
};

// grid (ceil((C D + C) / 256)), 256 threads
__global__ __launch_bounds__(RP_THREADS) void rp_step_kernel(RpStep a) {
    const int idx = blockIdx.x * RP_THREADS + threadIdx.x, CD = a.C * a.D;
    const float omega = a.omega[0];
    if (idx == 0) {
        float s = 0.f;
        for (int64_t g = 0; g < a.nseg; ++g) s = __fadd_rn(s, a.ploss[g]);
        float reg = 0.f;
        for (int c = 0; c < a.C; ++c) reg = __fadd_rn(reg, a.norms[c]);
        reg = __fadd_rn(reg, a.norms[64]);
        a.loss[0] = fmaf(__fmul_rn(0.5f, a.l2), reg, __fdiv_rn(s, omega));
    }
    if (!a.update || idx >= CD + a.C) return;
    const float* ps;
    int64_t stride;
    if (idx < CD) { ps = a.pG + idx; stride = CD; } else { ps = a.pb + (idx - CD); stride = 64; }
    float s = ps[0];
#pragma unroll 8
    for (int64_t g = 1; g < a.nseg; ++g) s = __fadd_rn(s, ps[g * stride]);
    const float v = a.v[idx], w = a.w[idx];
    const float grad = fmaf(a.l2, v, __fmul_rn(s, __fdiv_rn(1.f, omega)));
    const float wn = fmaf(-a.inv_l, grad, v);
    a.w[idx] = wn;
    a.v[idx] = fmaf(a.beta, __fsub_rn(wn, w), wn);
}

// byte offsets into the workspace, each a multiple of 16
struct RpLayout {
    int64_t nseg;
    int64_t flags, omega, w, v, norms, rn, ell, r, pG, pb, ploss, pomega, total;
};

// the checks the entry points share; 0, or CBAS_EINVAL with the message set
int rp_shape(const char* what, int32_t dim, int32_t C) {
    if (rows_width_ok(what, "dim", dim, RP_MAX_D) != CBAS_OK) return CBAS_EINVAL;
    if (C < 2 || C > RP_MAX_C) return cbas_fail(CBAS_EINVAL, "%s: n_classes = %d (2 .. %d)", what, C, RP_MAX_C);
    return CBAS_OK;
}

int rp_layout(const char* what, int64_t M, int32_t dim, int32_t C, RpLayout* L) {
    if (M < 1 || M > RP_MAX_M) return cbas_fail(CBAS_EINVAL, "%s: n_train = %lld (1 .. %lld)", what, (long long)M, (long long)RP_MAX_M);
    if (rp_shape(what, dim, C) != CBAS_OK) return CBAS_EINVAL;
    L->nseg = (M + RP_SEG - 1) / RP_SEG;
    RowsTake take;
    L->flags = take(16);
    L->omega = take(16);
    L->w = take(((int64_t)C * dim + 64) * 4);
    L->v = take(((int64_t)C * dim + 64) * 4);
    L->norms = take(RP_NORMS * 4);
    L->rn = take(M * 4);
    L->ell = take(M * 4);
    L->r = take(M * C * 4);
    L->pG = take(L->nseg * C * dim * 4);
    L->pb = take(L->nseg * 64 * 4);
    L->ploss = take(L->nseg * 4);
    L->pomega = take(L->nseg * 4);
    L->total = take.at;
    return CBAS_OK;
}

template <bool TRAIN>
int rp_pass(const RpPass& a, hipStream_t st) {
    const dim3 grid((unsigned)((a.N + RP_TILE - 1) / RP_TILE)), wg(RP_THREADS);
    switch ((a.C + 15) / 16) {
        case 1: hipLaunchKernelGGL((rp_forward_kernel<1, TRAIN>), grid, wg, 0, st, a); break;
        case 2: hipLaunchKernelGGL((rp_forward_kernel<2, TRAIN>), grid, wg, 0, st, a); break;
        case 3: hipLaunchKernelGGL((rp_forward_kernel<3, TRAIN>), grid, wg, 0, st, a); break;
        default: hipLaunchKernelGGL((rp_forward_kernel<4, TRAIN>), grid, wg, 0, st, a); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int rp_grad(const uint16_t* rows, int64_t M, int D, int64_t ld, const float* rn, const float* r, int C, int64_t nseg, float* pG, float* pb,
            hipStream_t st) {
    const dim3 grid((unsigned)nseg, (unsigned)((D + RP_SLAB - 1) / RP_SLAB)), wg(RP_THREADS);
    switch ((C + 15) / 16) {
        case 1: hipLaunchKernelGGL(rp_grad_kernel<1>, grid, wg, 0, st, rows, M, D, ld, rn, r, C, pG, pb); break;
        case 2: hipLaunchKernelGGL(rp_grad_kernel<2>, grid, wg, 0, st, rows, M, D, ld, rn, r, C, pG, pb); break;
        case 3: hipLaunchKernelGGL(rp_grad_kernel<3>, grid, wg, 0, st, rows, M, D, ld, rn, r, C, pG, pb); break;
        default: hipLaunchKernelGGL(rp_grad_kernel<4>, grid, wg, 0, st, rows, M, D, ld, rn, r, C, pG, pb); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

extern "C" int64_t cbas_rows_probe_workspace_bytes(int64_t n_train, int32_t dim, int32_t n_classes) {
    RpLayout L;
    if (rp_layout("cbas_rows_probe_workspace_bytes", n_train, dim, n_classes, &L) != CBAS_OK) return CBAS_EINVAL;
    return L.total;
}

extern "C" int cbas_rows_probe_fit(const void* train_f16_dev, int64_t n_train, int32_t dim, int64_t ld, const int32_t* label_dev,
                                   const float* sample_weight_dev, int32_t n_classes, float l2, int32_t iters, const float* init_weights_dev,
                                   const float* init_bias_dev, float* weights_dev, float* bias_dev, float* loss_dev, void* workspace_dev,
                                   int64_t workspace_bytes, void* stream) {
    const char* const what = "cbas_rows_probe_fit";
    RpLayout L;
    if (rp_layout(what, n_train, dim, n_classes, &L) != CBAS_OK) return CBAS_EINVAL;
    if (rows_ld_ok(what, "ld", ld, "dim", dim) != CBAS_OK) return CBAS_EINVAL;
    if (iters < 0) return cbas_fail(CBAS_EINVAL, "%s: iters = %d (at least 0)", what, iters);
    if (!(l2 > 0.f) || !(l2 <= 3.402823466e38f)) return cbas_fail(CBAS_EINVAL, "%s: l2 = %g (finite and greater than 0)", what, (double)l2);
    if (!train_f16_dev || !label_dev || !weights_dev || !bias_dev || !loss_dev || !workspace_dev)
        return cbas_fail(CBAS_EINVAL, "%s: a NULL pointer (only sample_weight, init_weights and init_bias may be NULL)", what);
    if (((uintptr_t)train_f16_dev | (uintptr_t)init_weights_dev | (uintptr_t)weights_dev | (uintptr_t)workspace_dev) % 16)
        return cbas_fail(CBAS_EINVAL, "%s: rows, weights and workspace must be 16-byte aligned", what);
    if (((uintptr_t)label_dev | (uintptr_t)sample_weight_dev | (uintptr_t)init_bias_dev | (uintptr_t)bias_dev | (uintptr_t)loss_dev) % 4)
        return cbas_fail(CBAS_EINVAL, "%s: label, sample_weight, bias and loss must be 4-byte aligned", what);
    if (workspace_bytes < L.total)
        return cbas_fail(CBAS_EINVAL, "%s: workspace of %lld bytes, %lld needed (cbas_rows_probe_workspace_bytes)", what,
                         (long long)workspace_bytes, (long long)L.total);
    if (cbas_use_device_of(train_f16_dev) != CBAS_OK) return CBAS_EHIP;
    hipStream_t st = (hipStream_t)stream;
    const uint16_t* const rows = (const uint16_t*)train_f16_dev;
    const int64_t M = n_train;
    const int C = n_classes, D = dim, CD = C * D;
    char* const ws = (char*)workspace_dev;
    unsigned* const flags = (unsigned*)(ws + L.flags);
    float* const omega = (float*)(ws + L.omega);
    float* const w = (float*)(ws + L.w);
    float* const v = (float*)(ws + L.v);
    float* const norms = (float*)(ws + L.norms);
    float* const rn = (float*)(ws + L.rn);
    float* const ell = (float*)(ws + L.ell);
    float* const r = (float*)(ws + L.r);
    float* const pG = (float*)(ws + L.pG);
    float* const pb = (float*)(ws + L.pb);
    float* const ploss = (float*)(ws + L.ploss);
    float* const pomega = (float*)(ws + L.pomega);
    const dim3 wg(RP_THREADS);
    const unsigned nseg = (unsigned)L.nseg;

    // the labels and the weights, before anything is indexed or scaled with one; the reciprocal norms and Omega meanwhile
    HIP_TRY(hipMemsetAsync(flags, 0, 16, st));
    hipLaunchKernelGGL(rp_check_kernel, dim3((unsigned)((M + RP_THREADS - 1) / RP_THREADS)), wg, 0, st, label_dev, sample_weight_dev, M, C, flags);
    hipLaunchKernelGGL(rows_rn_kernel, dim3((unsigned)((M * 4 + RP_THREADS - 1) / RP_THREADS)), wg, 0, st, rows, M, D, ld, rn);
    hipLaunchKernelGGL(rp_rowsum_kernel, dim3(nseg), wg, 0, st, sample_weight_dev, M, pomega);
    hipLaunchKernelGGL(rp_omega_kernel, dim3(1), dim3(1), 0, st, (const float*)pomega, L.nseg, omega, flags);
    HIP_TRY(hipGetLastError());
    unsigned bad[4] = {0u, 0u, 0u, 0u};
    HIP_TRY(hipMemcpyAsync(bad, flags, sizeof(bad), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad[0]) return cbas_fail(CBAS_EINVAL, "%s: a label lies outside [0, n_classes = %d)", what, C);
    if (bad[1]) return cbas_fail(CBAS_EINVAL, "%s: a sample weight is negative or not finite", what);
    if (bad[2]) return cbas_fail(CBAS_EINVAL, "%s: the sample weights add up to 0 (or overflow): Omega must be a positive number", what);

    // L = 1 + l2, q = l2 / L, beta = (1 - sqrt q) / (1 + sqrt q): in double, rounded once
    const double Ld = 1.0 + (double)l2, sq = std::sqrt((double)l2 / Ld);
    const float inv_l = (float)(1.0 / Ld), beta = (float)((1.0 - sq) / (1.0 + sq));

    // w_0, and v_0 = w_0 (w_{-1} = w_0: a fit continued from given weights starts without momentum)
    if (init_weights_dev) HIP_TRY(hipMemcpyAsync(w, init_weights_dev, (size_t)CD * 4, hipMemcpyDeviceToDevice, st));
    else HIP_TRY(hipMemsetAsync(w, 0, (size_t)CD * 4, st));
    HIP_TRY(hipMemsetAsync(w + CD, 0, 64 * 4, st));
    if (init_bias_dev) HIP_TRY(hipMemcpyAsync(w + CD, init_bias_dev, (size_t)C * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(v, w, (size_t)(CD + 64) * 4, hipMemcpyDeviceToDevice, st));

    RpPass pass{rows, M, D, ld, v, v + CD, C, nullptr, nullptr, label_dev, sample_weight_dev, r, ell, norms};
    RpStep step{pG, pb, ploss, omega, norms, L.nseg, C, D, l2, inv_l, beta, 1, w, v, loss_dev};
    const dim3 step_grid((unsigned)((CD + C + RP_THREADS - 1) / RP_THREADS));
    for (int t = 0; t < iters; ++t) {
        LAUNCH_TRY(rp_pass<true>(pass, st));
        hipLaunchKernelGGL(rp_rowsum_kernel, dim3(nseg), wg, 0, st, (const float*)ell, M, ploss);
        LAUNCH_TRY(rp_grad(rows, M, D, ld, rn, r, C, L.nseg, pG, pb, st));
        step.loss = loss_dev + t;
        hipLaunchKernelGGL(rp_step_kernel, step_grid, wg, 0, st, step);
    }
    // the closing pass: F at the weights returned
    pass.w = w;
    pass.b = w + CD;
    LAUNCH_TRY(rp_pass<true>(pass, st));
    hipLaunchKernelGGL(rp_rowsum_kernel, dim3(nseg), wg, 0, st, (const float*)ell, M, ploss);
    step.update = 0;
    step.loss = loss_dev + iters;
    hipLaunchKernelGGL(rp_step_kernel, dim3(1), wg, 0, st, step);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(weights_dev, w, (size_t)CD * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(bias_dev, w + CD, (size_t)C * 4, hipMemcpyDeviceToDevice, st));
    return CBAS_OK;
}

extern "C" int cbas_rows_probe_predict(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, const float* weights_dev,
                                       const float* bias_dev, int32_t n_classes, float* probs_dev, float* logits_dev, void* stream) {
    const char* const what = "cbas_rows_probe_predict";
    if (n_rows < 0 || (n_rows + RP_TILE - 1) / RP_TILE > 0x7fffffff)
        return cbas_fail(CBAS_EINVAL, "%s: n_rows = %lld (0 .. %lld)", what, (long long)n_rows, (long long)0x7fffffff * RP_TILE);
    if (rp_shape(what, dim, n_classes) != CBAS_OK) return CBAS_EINVAL;
    if (rows_ld_ok(what, "ld", ld, "dim", dim) != CBAS_OK) return CBAS_EINVAL;
    if (n_rows == 0) return CBAS_OK;
    if (!rows_f16_dev || !weights_dev || !bias_dev || !probs_dev) return cbas_fail(CBAS_EINVAL, "%s: a NULL pointer (only logits may be NULL)", what);
    if (((uintptr_t)rows_f16_dev | (uintptr_t)weights_dev) % 16) return cbas_fail(CBAS_EINVAL, "%s: rows and weights must be 16-byte aligned", what);
    if (((uintptr_t)bias_dev | (uintptr_t)probs_dev | (uintptr_t)logits_dev) % 4)
        return cbas_fail(CBAS_EINVAL, "%s: bias, probs and logits must be 4-byte aligned", what);
    if (cbas_use_device_of(rows_f16_dev) != CBAS_OK) return CBAS_EHIP;
    const RpPass pass{(const uint16_t*)rows_f16_dev, n_rows, dim, ld, weights_dev, bias_dev, n_classes, probs_dev, logits_dev, nullptr, nullptr,
                      nullptr, nullptr, nullptr};
    LAUNCH_TRY(rp_pass<false>(pass, (hipStream_t)stream));
    return CBAS_OK;
}
