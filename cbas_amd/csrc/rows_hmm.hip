// The two passes over resident CLS rows that close the motif HMM's loop: cbasx_rows_emissions and
// cbasx_rows_weighted_sums_workspace_bytes / cbasx_rows_weighted_sums of include/cbas_mi355x_ext.h, kernels and entry points in one
// file.  rows (N, D) fp16 with row stride ld.  The working row u of a row x is x widened (normalize = 0) or fl(x * rn), rn the
// reciprocal norm of rows_rn.h (normalize = 1); no normalised copy is written, rn is applied where the row is used.
//
//   rhm_emit_kernel   THE E STEP'S PASS, built as rkm_score_kernel of rows_kmeans.hip: a workgroup owns RHM_TILE = 128 rows, wave w the
//                     two 16-row tiles 32 w .. 32 w + 31; the means come through LDS in chunks of RHM_KC = 64 columns of all (at most 64)
//                     states, two buffers, the next chunk's global loads in flight under this chunk's v_mfma_f32_16x16x4_f32.
//                     THE ORDER OF THE SUMS, a function of D alone:
//                       x . mu_j = chain0 + chain1; chain p = the fp32 fmaf chain, from 0, over the columns d with (d / 32) % 2 = p,
//                                  ordered by (d / 32, d % 8, (d % 32) / 8) ascending (cbas_rows_search's dot)
//                       s = (l0 + l1) + (l2 + l3), rows_rn.h
//                     z_j = fmaf(kappa, fl(rn * x . mu_j), logw_j) (rn = 1 without normalize); m = max_j z_j; e_j = expf(z_j - m);
//                     S = the sum of e_j: lane f of 16 adds its states f, 16 + f, 32 + f, 48 + f in ascending order, then the xor tree
//                     1, 2, 4, 8 over the 16 lanes; probs_j = e_j / S (one correctly rounded division);
//                     lognorm = fl(fl(m + logf(S)) * log2(e)).  A tile belongs to one wave from its first column to its last: neither
//                     the grid, nor N, nor where the row lies enters a sum.
//   rhm_sum_kernel    THE M STEP'S PASS: sums = W^T U on the fp32 matrix pipe.  The rows are dealt to PARTS of rpp consecutive rows
//                     (rhm_parts: a function of n_rows alone, at most RHM_MAX_PARTS parts of a multiple of 64 rows).  A workgroup owns
//                     one part and one group of 128 SL columns per wave-column (SL = 4, 2, 1, 1 slabs for NG = ceil(C / 16) = 1, 2, 3, 4),
//                     all C states.  A part's 16-row blocks go to the four waves in turn (block b to wave b % 4); a wave walks its blocks
//                     in ascending order, four MFMA steps of four rows a block: ONE fp32 chain per (state, column) and wave, rows
//                     ascending.  Lane (fc, kr) loads the 8 halves 8 fc .. 8 fc + 7 of row 4 s + kr of the slab: 256 contiguous bytes
//                     per row; MFMA i of 8 takes column 8 fc + i.  rn of the block's 16 rows is the chain of rows_rn.h over the whole
//                     row (read once more, from the caches), u = fl(x * rn) formed in registers.  mass rides the same chain: one more
//                     MFMA per step against a column of ones.  The four waves' results are added ((w0 + w1) + w2) + w3 through LDS.
//   rhm_reduce_kernel sums[c][d] = the parts in ascending order, added in float64; mass likewise
// No atomics anywhere.
#include "kernels.h"
#include "rows_api.h"
#include "rows_rn.h"
#include "../../include/cbas_mi355x_ext.h"

namespace {

constexpr int RHM_THREADS = 256;
constexpr int RHM_TILE = 128;                        // rows a workgroup of the emissions pass owns
constexpr int RHM_RT = 2;                            // 16-row tiles per wave
constexpr int RHM_KC = 64;                           // columns per staged chunk of the means
constexpr int RHM_CLD = RHM_KC + 4;                  // floats between the staged means
constexpr int RHM_MAX_C = CBASX_ROWS_HMM_MAX_STATES, RHM_MAX_D = CBASX_ROWS_HMM_MAX_DIM;
constexpr int RHM_MAX_PARTS = CBASX_ROWS_HMM_MAX_PARTS;
constexpr int RHM_PART_ROWS = CBASX_ROWS_HMM_PART_ROWS;      // a part is a multiple of this many rows: 16 per wave and round
constexpr int RHM_SLAB = 128;                        // columns a wave loads of a row at once: 16 lanes x 8 halves
constexpr float RHM_LOG2E = 1.44269504088896340736f;

static_assert(RHM_PART_ROWS == 64, "a round of a part is 16 rows for each of the four waves");

struct RhmEmit {
    const uint16_t* rows;
    int64_t N;
    int D;
    int64_t ld;
    const float* means;
    const float* logw;
    int C, normalize;
    float kappa;
    float* probs;
    float* lognorm;
};

// grid (ceil(N / RHM_TILE)), 256 threads, LDS 2 x 16 NG x RHM_CLD floats
template <int NG>
__global__ __launch_bounds__(RHM_THREADS) void rhm_emit_kernel(RhmEmit a) {
    __shared__ __attribute__((aligned(16))) float sc[2][16 * NG * RHM_CLD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fc = lane & 15, kr = lane >> 4;
    const int nb = a.D >> 5, nch = (a.D + RHM_KC - 1) / RHM_KC;
    const int64_t m0 = (int64_t)blockIdx.x * RHM_TILE + 32 * wave;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const uint4 zero16 = {0u, 0u, 0u, 0u};

    const uint16_t* p[RHM_RT];
    bool valid[RHM_RT];
#pragma unroll
    for (int t = 0; t < RHM_RT; ++t) {
        const int64_t m = m0 + 16 * t + fc;
        valid[t] = m < a.N;                                      // a row past the end is read as zeros and never written
        p[t] = a.rows + (valid[t] ? m : 0) * a.ld + 8 * kr;
    }
    // the 16-byte pieces of a chunk this thread stages: piece v is state (v 256 + tid) / 16, columns 4 ((v 256 + tid) % 16) .. + 3
    auto fetch_c = [&](int ch, f32x4 (&c)[NG]) {
#pragma unroll
        for (int v = 0; v < NG; ++v) {
            const int idx = v * RHM_THREADS + tid, j = idx >> 4, col = ch * RHM_KC + 4 * (idx & 15);
            c[v] = (j < a.C && col < a.D) ? *reinterpret_cast<const f32x4*>(a.means + (int64_t)j * a.D + col) : zero;
        }
    };
    auto stage_c = [&](float* buf, const f32x4 (&c)[NG]) {
#pragma unroll
        for (int v = 0; v < NG; ++v) {
            const int idx = v * RHM_THREADS + tid;
            *reinterpret_cast<f32x4*>(buf + (idx >> 4) * RHM_CLD + 4 * (idx & 15)) = c[v];
        }
    };
    auto fetch_x = [&](int ch, uint4 (&x)[RHM_RT][2]) {
#pragma unroll
        for (int t = 0; t < RHM_RT; ++t)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int c = 2 * ch + i;
                x[t][i] = (valid[t] && c < nb) ? *reinterpret_cast<const uint4*>(p[t] + 32 * c) : zero16;
            }
    };

    f32x4 cpre[NG];
    uint4 xb[RHM_RT][2], xn[RHM_RT][2];
    fetch_c(0, cpre);
    fetch_x(0, xb);
    stage_c(sc[0], cpre);
    __syncthreads();

    f32x4 acc[RHM_RT][NG][2];
    float ss[RHM_RT];
#pragma unroll
    for (int t = 0; t < RHM_RT; ++t) {
        ss[t] = 0.f;
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[t][g][0] = acc[t][g][1] = zero;
    }

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
                    const float* const qb = buf + (16 * g + fc) * RHM_CLD + 32 * i + 8 * kr;
                    qa[g] = *reinterpret_cast<const f32x4*>(qb);
                    qv[g] = *reinterpret_cast<const f32x4*>(qb + 4);
                }
#pragma unroll
                for (int t = 0; t < RHM_RT; ++t) {
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
        if (more) stage_c(sc[(ch & 1) ^ 1], cpre);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < RHM_RT; ++t)
#pragma unroll
            for (int i = 0; i < 2; ++i) xb[t][i] = xn[t][i];
    }
    float lw[NG];                                                // log-weight of state 16 g + fc
#pragma unroll
    for (int g = 0; g < NG; ++g) lw[g] = (a.logw && 16 * g + fc < a.C) ? a.logw[16 * g + fc] : 0.f;

#pragma unroll
    for (int t = 0; t < RHM_RT; ++t) {
        float s = ss[t];
        s += __shfl_xor(s, 16, 64);                              // (l0 + l1) and (l2 + l3), then their sum: the same bits in all four
        s += __shfl_xor(s, 32, 64);
        const float rn = a.normalize ? rows_rn(s) : 1.f;
        // acc[t][g][.][e]: row 4 kr + e of the tile against state 16 g + fc; that row's rn sits in lane 4 kr + e
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float rn_row = __shfl(rn, 4 * kr + e, 64);
            float z[NG];
            float top = -__builtin_inff();
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const float cosj = __fmul_rn(rn_row, __fadd_rn(acc[t][g][0][e], acc[t][g][1][e]));
                z[g] = 16 * g + fc < a.C ? fmaf(a.kappa, cosj, lw[g]) : -__builtin_inff();
                top = fmaxf(top, z[g]);
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) top = fmaxf(top, __shfl_xor(top, o, 64));
            float ex[NG];
            float sum = 0.f;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                ex[g] = 16 * g + fc < a.C ? expf(__fsub_rn(z[g], top)) : 0.f;
                sum = __fadd_rn(sum, ex[g]);
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) sum = __fadd_rn(sum, __shfl_xor(sum, o, 64));      // both partners add the same pair: the same bits in all 16
            const int64_t m = m0 + 16 * t + 4 * kr + e;
            if (m < a.N) {
#pragma unroll
                for (int g = 0; g < NG; ++g)
                    if (16 * g + fc < a.C) a.probs[m * a.C + 16 * g + fc] = __fdiv_rn(ex[g], sum);
                if (a.lognorm && fc == 0) a.lognorm[m] = __fmul_rn(__fadd_rn(top, logf(sum)), RHM_LOG2E);
            }
        }
    }
}

// ---- the weighted sums -----------------------------------------------------------------------------------------------------------
struct RhmSum {
    const uint16_t* rows;
    int64_t N;
    int D;
    int64_t ld;
    const float* w;
    int C, normalize;
    int64_t rpp;                                                 // rows per part
    float* psum;                                                 // (parts, C, D)
    float* pmass;                                                // (parts, 64)
};

template <int NG>
struct RhmShape {
    static constexpr int SL = NG == 1 ? 4 : NG == 2 ? 2 : 1;     // 128-column slabs per wave: 32 NG SL accumulator registers
    static constexpr int REGS = NG * SL * 8 + NG;                // f32x4 a lane holds: the sums and the mass
};

// grid (ceil(D / (128 SL)), parts), 256 threads, LDS REGS x 64 f32x4
template <int NG>
__global__ __launch_bounds__(RHM_THREADS) void rhm_sum_kernel(RhmSum a) {
    constexpr int SL = RhmShape<NG>::SL, REGS = RhmShape<NG>::REGS;
    __shared__ f32x4 red[REGS * 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fc = lane & 15, kr = lane >> 4;
    const int nb = a.D >> 5;
    const int col0 = blockIdx.x * (RHM_SLAB * SL) + 8 * fc;      // this lane's 8 columns of slab 0
    const bool with_mass = blockIdx.x == 0;
    const int64_t part = blockIdx.y, pm0 = part * a.rpp, pm1 = pm0 + a.rpp < a.N ? pm0 + a.rpp : a.N;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const uint4 zero16 = {0u, 0u, 0u, 0u};

    f32x4 acc[NG][SL * 8], accm[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        accm[g] = zero;
#pragma unroll
        for (int i = 0; i < SL * 8; ++i) acc[g][i] = zero;
    }

    // block b of the part: rows pm0 + 16 b .. + 15; step s of it: rows 4 s .. 4 s + 3, this lane row 4 s + kr
    auto fetch = [&](int64_t t0, uint4 (&x)[4][SL], float (&w)[4][NG]) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int64_t m = t0 + 4 * s + kr;
            const bool ok = m < pm1;                             // a row past the part is read as zeros, weights and all
#pragma unroll
            for (int sl = 0; sl < SL; ++sl)
                x[s][sl] = (ok && col0 + RHM_SLAB * sl < a.D) ? *reinterpret_cast<const uint4*>(a.rows + m * a.ld + col0 + RHM_SLAB * sl) : zero16;
#pragma unroll
            for (int g = 0; g < NG; ++g) w[s][g] = (ok && 16 * g + fc < a.C) ? a.w[m * a.C + 16 * g + fc] : 0.f;
        }
    };
    // rn of row t0 + fc in lane (fc, .): rows_rn.h's chain over the whole row
    auto block_rn = [&](int64_t t0) {
        if (!a.normalize) return 1.f;
        const int64_t m = t0 + fc;
        float ss = 0.f;
        if (m < pm1) {
            const uint16_t* const p = a.rows + m * a.ld + 8 * kr;
            for (int c = 0; c < nb; ++c) ss = rows_ss8(__builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(p + 32 * c)), ss);
        }
        ss += __shfl_xor(ss, 16, 64);                            // (l0 + l1) and (l2 + l3), then their sum: the same bits in all four
        ss += __shfl_xor(ss, 32, 64);
        return rows_rn(ss);
    };

    uint4 xb[4][SL], xn[4][SL];
    float wb[4][NG], wn[4][NG];
    int64_t t0 = pm0 + 16 * wave;
    if (t0 < pm1) fetch(t0, xb, wb);
    for (; t0 < pm1; t0 += 64) {
        const bool more = t0 + 64 < pm1;
        if (more) fetch(t0 + 64, xn, wn);
        const float rn = block_rn(t0);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float rn_row = __shfl(rn, 4 * s + kr, 64);     // lane 4 s + kr holds rn of row 4 s + kr of the block
            if (with_mass) {
#pragma unroll
                for (int g = 0; g < NG; ++g) accm[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[s][g], 1.f, accm[g], 0, 0, 0);
            }
#pragma unroll
            for (int sl = 0; sl < SL; ++sl) {
                const f16x8 h = __builtin_bit_cast(f16x8, xb[s][sl]);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float u = (float)h[i];
                    if (a.normalize) u = __fmul_rn(u, rn_row);
#pragma unroll
                    for (int g = 0; g < NG; ++g)
                        acc[g][sl * 8 + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[s][g], u, acc[g][sl * 8 + i], 0, 0, 0);
                }
            }
        }
        if (more) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int sl = 0; sl < SL; ++sl) xb[s][sl] = xn[s][sl];
#pragma unroll
                for (int g = 0; g < NG; ++g) wb[s][g] = wn[s][g];
            }
        }
    }

    // ((w0 + w1) + w2) + w3: wave w hands its registers over, wave 0 adds them
    for (int w = 1; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
#pragma unroll
                for (int i = 0; i < SL * 8; ++i) red[(g * SL * 8 + i) * 64 + lane] = acc[g][i];
                red[(NG * SL * 8 + g) * 64 + lane] = accm[g];
            }
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
#pragma unroll
                for (int i = 0; i < SL * 8; ++i) {
                    const f32x4 o = red[(g * SL * 8 + i) * 64 + lane];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[g][i][e] = __fadd_rn(acc[g][i][e], o[e]);
                }
                const f32x4 o = red[(NG * SL * 8 + g) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) accm[g][e] = __fadd_rn(accm[g][e], o[e]);
            }
        }
        __syncthreads();
    }
    if (wave != 0) return;
    // acc[g][8 sl + i][e]: state 16 g + 4 kr + e, column col0 + 128 sl + i
    float* const out = a.psum + part * a.C * a.D;
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 16 * g + 4 * kr + e;
            if (c >= a.C) continue;
#pragma unroll
            for (int sl = 0; sl < SL; ++sl) {
                const int col = col0 + RHM_SLAB * sl;
                if (col >= a.D) continue;
                const f32x4 lo = {acc[g][sl * 8 + 0][e], acc[g][sl * 8 + 1][e], acc[g][sl * 8 + 2][e], acc[g][sl * 8 + 3][e]};
                const f32x4 hi = {acc[g][sl * 8 + 4][e], acc[g][sl * 8 + 5][e], acc[g][sl * 8 + 6][e], acc[g][sl * 8 + 7][e]};
                *reinterpret_cast<f32x4*>(out + (int64_t)c * a.D + col) = lo;
                *reinterpret_cast<f32x4*>(out + (int64_t)c * a.D + col + 4) = hi;
            }
            if (with_mass && fc == 0) a.pmass[part * 64 + c] = accm[g][e];
        }
}

// grid (ceil((C D + C) / 256)), 256 threads: element idx < C D of the sums, then the C masses
__global__ __launch_bounds__(RHM_THREADS) void rhm_reduce_kernel(const float* __restrict__ psum, const float* __restrict__ pmass, int64_t nparts,
                                                                 int C, int D, double* __restrict__ sums, double* __restrict__ mass) {
    const int64_t idx = (int64_t)blockIdx.x * RHM_THREADS + threadIdx.x, cd = (int64_t)C * D;
    if (idx >= cd + C) return;
    double s = 0.0;
    if (idx < cd) {
        for (int64_t p = 0; p < nparts; ++p) s += (double)psum[p * cd + idx];
        sums[idx] = s;
    } else {
        for (int64_t p = 0; p < nparts; ++p) s += (double)pmass[p * 64 + (idx - cd)];
        mass[idx - cd] = s;
    }
}

// the parts of n_rows rows: a function of n_rows alone
struct RhmParts {
    int64_t rpp, nparts;
};

RhmParts rhm_parts(int64_t n_rows) {
    RhmParts P;
    const int64_t per = (n_rows + RHM_MAX_PARTS - 1) / RHM_MAX_PARTS;
    P.rpp = (per + RHM_PART_ROWS - 1) / RHM_PART_ROWS * RHM_PART_ROWS;
    if (P.rpp < RHM_PART_ROWS) P.rpp = RHM_PART_ROWS;
    P.nparts = (n_rows + P.rpp - 1) / P.rpp;
    return P;
}

struct RhmLayout {
    RhmParts parts;
    int64_t psum, pmass, total;
};

// the checks both entry points share; 0, or CBAS_EINVAL with the message set
int rhm_shape(const char* what, int64_t n_rows, int32_t dim, int64_t ld, int32_t C, int32_t normalize) {
    if (n_rows < 0 || (n_rows + RHM_TILE - 1) / RHM_TILE > 0x7fffffff)
        return cbas_fail(CBAS_EINVAL, "%s: n_rows = %lld (0 .. %lld)", what, (long long)n_rows, (long long)0x7fffffff * RHM_TILE);
    if (rows_width_ok(what, "dim", dim, RHM_MAX_D) != CBAS_OK) return CBAS_EINVAL;
    if (C < 1 || C > RHM_MAX_C) return cbas_fail(CBAS_EINVAL, "%s: C = %d states (1 .. %d)", what, C, RHM_MAX_C);
    if (rows_ld_ok(what, "ld", ld, "dim", dim) != CBAS_OK) return CBAS_EINVAL;
    if (normalize != 0 && normalize != 1) return cbas_fail(CBAS_EINVAL, "%s: normalize = %d (0 or 1)", what, normalize);
    return CBAS_OK;
}

void rhm_layout(int64_t n_rows, int32_t dim, int32_t C, RhmLayout* L) {
    L->parts = rhm_parts(n_rows);
    const int64_t blocks = L->parts.nparts > 0 ? L->parts.nparts : 1;      // never an empty workspace
    RowsTake take;
    L->psum = take(blocks * C * dim * 4);
    L->pmass = take(blocks * 64 * 4);
    L->total = take.at;
}

}  // namespace

extern "C" int cbasx_rows_emissions(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, int32_t C, int32_t normalize,
                                    const float* means_dev, float kappa, const float* log_weights_dev, float* probs_dev, float* lognorm_dev,
                                    void* stream) {
    const char* const what = "cbasx_rows_emissions";
    if (rhm_shape(what, n_rows, dim, ld, C, normalize) != CBAS_OK) return CBAS_EINVAL;
    if (!(kappa >= 0.f) || kappa > 3.0e38f) return cbas_fail(CBAS_EINVAL, "%s: kappa = %g (finite and at least 0)", what, (double)kappa);
    if (!rows_f16_dev || !means_dev || !probs_dev) return cbas_fail(CBAS_EINVAL, "%s: a NULL pointer (only log_weights and lognorm may be NULL)", what);
    if (((uintptr_t)rows_f16_dev | (uintptr_t)means_dev) % 16) return cbas_fail(CBAS_EINVAL, "%s: rows and means must be 16-byte aligned", what);
    if (((uintptr_t)log_weights_dev | (uintptr_t)probs_dev | (uintptr_t)lognorm_dev) % 4)
        return cbas_fail(CBAS_EINVAL, "%s: log_weights, probs and lognorm must be 4-byte aligned", what);
    if (n_rows == 0) return CBAS_OK;
    if (cbas_use_device_of(rows_f16_dev) != CBAS_OK) return CBAS_EHIP;
    const RhmEmit a{(const uint16_t*)rows_f16_dev, n_rows, dim, ld, means_dev, log_weights_dev, C, normalize, kappa, probs_dev, lognorm_dev};
    const dim3 grid((unsigned)((n_rows + RHM_TILE - 1) / RHM_TILE)), wg(RHM_THREADS);
    hipStream_t st = (hipStream_t)stream;
    switch ((C + 15) / 16) {
        case 1: hipLaunchKernelGGL(rhm_emit_kernel<1>, grid, wg, 0, st, a); break;
        case 2: hipLaunchKernelGGL(rhm_emit_kernel<2>, grid, wg, 0, st, a); break;
        case 3: hipLaunchKernelGGL(rhm_emit_kernel<3>, grid, wg, 0, st, a); break;
        default: hipLaunchKernelGGL(rhm_emit_kernel<4>, grid, wg, 0, st, a); break;
    }
    HIP_TRY(hipGetLastError());
    return CBAS_OK;
}

extern "C" int64_t cbasx_rows_weighted_sums_workspace_bytes(int64_t n_rows, int32_t dim, int32_t C) {
    if (rhm_shape("cbasx_rows_weighted_sums_workspace_bytes", n_rows, dim, dim, C, 0) != CBAS_OK) return CBAS_EINVAL;
    RhmLayout L;
    rhm_layout(n_rows, dim, C, &L);
    return L.total;
}

extern "C" int cbasx_rows_weighted_sums(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, int32_t C, int32_t normalize,
                                        const float* weights_dev, double* sums_dev, double* mass_dev, void* workspace_dev,
                                        int64_t workspace_bytes, void* stream) {
    const char* const what = "cbasx_rows_weighted_sums";
    if (rhm_shape(what, n_rows, dim, ld, C, normalize) != CBAS_OK) return CBAS_EINVAL;
    if (!rows_f16_dev || !weights_dev || !sums_dev || !mass_dev || !workspace_dev) return cbas_fail(CBAS_EINVAL, "%s: a NULL pointer", what);
    if (((uintptr_t)rows_f16_dev | (uintptr_t)workspace_dev) % 16) return cbas_fail(CBAS_EINVAL, "%s: rows and workspace must be 16-byte aligned", what);
    if ((uintptr_t)weights_dev % 4 || ((uintptr_t)sums_dev | (uintptr_t)mass_dev) % 8)
        return cbas_fail(CBAS_EINVAL, "%s: weights must be 4-byte aligned, sums and mass 8-byte aligned", what);
    RhmLayout L;
    rhm_layout(n_rows, dim, C, &L);
    if (workspace_bytes < L.total)
        return cbas_fail(CBAS_EINVAL, "%s: workspace of %lld bytes, %lld needed (cbasx_rows_weighted_sums_workspace_bytes)", what,
                         (long long)workspace_bytes, (long long)L.total);
    if (cbas_use_device_of(rows_f16_dev) != CBAS_OK) return CBAS_EHIP;
    hipStream_t st = (hipStream_t)stream;
    char* const ws = (char*)workspace_dev;
    float* const psum = (float*)(ws + L.psum);
    float* const pmass = (float*)(ws + L.pmass);
    const RhmSum a{(const uint16_t*)rows_f16_dev, n_rows, dim, ld, weights_dev, C, normalize, L.parts.rpp, psum, pmass};
    const unsigned nparts = (unsigned)L.parts.nparts;
    const dim3 wg(RHM_THREADS);
    auto groups = [&](int sl) { return dim3((unsigned)((dim + RHM_SLAB * sl - 1) / (RHM_SLAB * sl)), nparts); };
    if (nparts > 0) {
        switch ((C + 15) / 16) {
            case 1: hipLaunchKernelGGL(rhm_sum_kernel<1>, groups(RhmShape<1>::SL), wg, 0, st, a); break;
            case 2: hipLaunchKernelGGL(rhm_sum_kernel<2>, groups(RhmShape<2>::SL), wg, 0, st, a); break;
            case 3: hipLaunchKernelGGL(rhm_sum_kernel<3>, groups(RhmShape<3>::SL), wg, 0, st, a); break;
            default: hipLaunchKernelGGL(rhm_sum_kernel<4>, groups(RhmShape<4>::SL), wg, 0, st, a); break;
        }
    }
    hipLaunchKernelGGL(rhm_reduce_kernel, dim3((unsigned)(((int64_t)C * dim + C + RHM_THREADS - 1) / RHM_THREADS)), wg, 0, st, (const float*)psum,
                       (const float*)pmass, L.parts.nparts, C, dim, sums_dev, mass_dev);
    HIP_TRY(hipGetLastError());
    return CBAS_OK;
}
