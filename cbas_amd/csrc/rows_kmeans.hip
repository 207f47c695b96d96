// k-means over resident CLS rows: cbas_rows_kmeans_workspace_bytes / cbas_rows_kmeans_fit /
// cbas_rows_kmeans_assign of include/cbas_mi355x.h, kernels and entry points in one file.  rows (N, D) fp16 with row stride ld,
// centroids (k, D) fp32.  The working row u of a row x is x widened (normalize = 0) or fl(x * rn), rn the reciprocal norm of
// rows_rn.h (normalize = 1); no normalised copy is written, rn is applied where the row is used.
//
//   rows_rn_kernel        (rows_rn.h) rn of every row, for the seeding and the sums
//   rkm_seed_dist_kernel  d(m) = sum_d (u_md - t_d)^2 against the target t (the mean, then the newest seed): one wave per row, lane l
//                         the fmaf chain over the columns d with (d / 8) % 64 = l, ascending, then the xor tree 32, 16, .., 1;
//                         mind(m) = min(mind(m), d(m)); the largest mind of the block's 64 rows and its lowest row
//   rkm_seed_pick_kernel  the largest over the blocks, ties to the lowest row; writes the seed (a u row) and its index
//   rkm_score_kernel      THE PASS.  A workgroup owns RKM_TILE = 128 rows, wave w the two 16-row tiles 32 w .. 32 w + 31.  The
//                         centroids come through LDS by COLUMNS: chunks of RKM_KC = 64 columns of all (at most 64) centroids, two
//                         buffers, the next chunk's global loads (rows and centroids) in flight under this chunk's MFMAs - 128 NG
//                         v_mfma_f32_16x16x4_f32 a wave and barrier, NG = ceil(k / 16).  Lane (fc, kr) holds the 8 halves
//                         d = 32 c + 8 kr .. + 7 of row fc of a tile and widens them (exact); products are exact.
//                         THE ORDER OF THE SUMS, a function of D alone:
//                           x . c_j = chain0 + chain1; chain p = the fp32 fmaf chain, from 0, over the columns d with (d / 32) % 2 = p,
//                                     ordered by (d / 32, d % 8, (d % 32) / 8) ascending (cbas_rows_search's dot)
//                           s = (l0 + l1) + (l2 + l3), rows_rn.h;  |c_j|^2 = one fmaf chain, from 0, over d ascending; h_j = 0.5 |c_j|^2
//                         score_j = fmaf(rn, x . c_j, -h_j); the largest wins, ties to the lowest j; dist2 = max(0, fmaf(-2, score,
//                         |u|^2)), |u|^2 = s, or 1 (0 for a zero row) with normalize.  A tile belongs to one wave from its first
//                         column to its last: neither the grid, nor N, nor where the row lies enters a sum.
//   rkm_sum_kernel        one workgroup per SEGMENT of RKM_SEG = 4096 rows and slab of 512 columns: thread t owns two columns and
//                         adds u to its row's cluster in LDS, rows in ascending order (one fp32 add a row); the segment's counts and
//                         its inertia (one fp32 chain over the rows, ascending).  labels == NULL: everything into cluster 0 (the mean)
//   rkm_update_kernel     centroid = (segment sums added in ascending order) / (float)count, an empty cluster untouched; the round's
//                         inertia = the segments' in ascending order
//   rkm_finish_kernel     final counts and inertia, clusters by descending count (ties: seeding order)
//   rkm_remap_kernel      the last assignment in the output numbering
// No atomics anywhere.
#include "kernels.h"
#include "rows_api.h"
#include "rows_rn.h"

namespace {

constexpr int RKM_THREADS = 256;
constexpr int RKM_TILE = 128;                        // rows a workgroup of the pass owns (tests/rows_kmeans_ref.py: TILE)
constexpr int RKM_RT = 2;                            // 16-row tiles per wave
constexpr int RKM_KC = 64;                           // columns per staged chunk of the centroids
constexpr int RKM_CLD = RKM_KC + 4;                  // floats between the staged centroids
constexpr int RKM_SEG = CBAS_ROWS_KMEANS_SEGMENT;
constexpr int RKM_SLAB = 2 * RKM_THREADS;            // columns per workgroup of the sums
constexpr int RKM_SEED_ROWS = 64;                    // rows per workgroup of the seeding distances
constexpr int RKM_MAX_K = 64, RKM_MAX_D = 1536;

struct RkmPass {
    const uint16_t* rows;
    int64_t N;
    int D;
    int64_t ld;
    const float* cent;
    int k, normalize;
    int32_t* labels;
    float* dist2;
};

// grid (ceil(N / RKM_TILE)), 256 threads, LDS 2 x 16 NG x RKM_CLD floats + 64
template <int NG>
__global__ __launch_bounds__(RKM_THREADS) void rkm_score_kernel(RkmPass a) {
    __shared__ __attribute__((aligned(16))) float sc[2][16 * NG * RKM_CLD];
    __shared__ float hn[16 * NG];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fc = lane & 15, kr = lane >> 4;
    const int nb = a.D >> 5, nch = (a.D + RKM_KC - 1) / RKM_KC;
    const int64_t m0 = (int64_t)blockIdx.x * RKM_TILE + 32 * wave;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const uint4 zero16 = {0u, 0u, 0u, 0u};

    const uint16_t* p[RKM_RT];
    bool valid[RKM_RT];
#pragma unroll
    for (int t = 0; t < RKM_RT; ++t) {
        const int64_t m = m0 + 16 * t + fc;
        valid[t] = m < a.N;                                      // a row past the end is read as zeros and never written
        p[t] = a.rows + (valid[t] ? m : 0) * a.ld + 8 * kr;
    }
    // the 16-byte pieces of a chunk this thread stages: piece v is centroid (v 256 + tid) / 16, columns 4 ((v 256 + tid) % 16) .. + 3
    auto fetch_c = [&](int ch, f32x4 (&c)[NG]) {
#pragma unroll
        for (int v = 0; v < NG; ++v) {
            const int idx = v * RKM_THREADS + tid, j = idx >> 4, col = ch * RKM_KC + 4 * (idx & 15);
            c[v] = (j < a.k && col < a.D) ? *reinterpret_cast<const f32x4*>(a.cent + (int64_t)j * a.D + col) : zero;
        }
    };
    auto stage_c = [&](float* buf, const f32x4 (&c)[NG]) {
#pragma unroll
        for (int v = 0; v < NG; ++v) {
            const int idx = v * RKM_THREADS + tid;
            *reinterpret_cast<f32x4*>(buf + (idx >> 4) * RKM_CLD + 4 * (idx & 15)) = c[v];
        }
    };
    auto fetch_x = [&](int ch, uint4 (&x)[RKM_RT][2]) {
#pragma unroll
        for (int t = 0; t < RKM_RT; ++t)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int c = 2 * ch + i;
                x[t][i] = (valid[t] && c < nb) ? *reinterpret_cast<const uint4*>(p[t] + 32 * c) : zero16;
            }
    };

    f32x4 cpre[NG];
    uint4 xb[RKM_RT][2], xn[RKM_RT][2];
    fetch_c(0, cpre);
    fetch_x(0, xb);
    stage_c(sc[0], cpre);
    __syncthreads();

    f32x4 acc[RKM_RT][NG][2];
    float ss[RKM_RT];
#pragma unroll
    for (int t = 0; t < RKM_RT; ++t) {
        ss[t] = 0.f;
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[t][g][0] = acc[t][g][1] = zero;
    }
    float cn = 0.f;                                              // thread j < 16 NG: |c_j|^2, one chain over the columns in ascending order

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
                    const float* const qb = buf + (16 * g + fc) * RKM_CLD + 32 * i + 8 * kr;
                    qa[g] = *reinterpret_cast<const f32x4*>(qb);
                    qv[g] = *reinterpret_cast<const f32x4*>(qb + 4);
                }
#pragma unroll
                for (int t = 0; t < RKM_RT; ++t) {
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
        if (tid < 16 * NG) {
            const int w = a.D - ch * RKM_KC < RKM_KC ? a.D - ch * RKM_KC : RKM_KC;
            for (int d = 0; d < w; ++d) cn = fmaf(buf[tid * RKM_CLD + d], buf[tid * RKM_CLD + d], cn);
        }
        if (more) stage_c(sc[(ch & 1) ^ 1], cpre);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < RKM_RT; ++t)
#pragma unroll
            for (int i = 0; i < 2; ++i) xb[t][i] = xn[t][i];
    }
    if (tid < 16 * NG) hn[tid] = tid < a.k ? 0.5f * cn : __builtin_inff();
    __syncthreads();
    float hl[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) hl[g] = hn[16 * g + fc];

#pragma unroll
    for (int t = 0; t < RKM_RT; ++t) {
        float s = ss[t];
        s += __shfl_xor(s, 16, 64);                              // (l0 + l1) and (l2 + l3), then their sum: the same bits in all four
        s += __shfl_xor(s, 32, 64);
        const float rn = a.normalize ? rows_rn(s) : 1.f;
        const float un2 = a.normalize ? (s > 0.f ? 1.f : 0.f) : s;
        // acc[t][g][.][e]: row 4 kr + e of the tile against centroid 16 g + fc; that row's rn sits in lane 4 kr + e
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float rn_row = __shfl(rn, 4 * kr + e, 64), un2_row = __shfl(un2, 4 * kr + e, 64);
            float best = -__builtin_inff();
            int bj = 0x7fffffff;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const float sj = fmaf(rn_row, acc[t][g][0][e] + acc[t][g][1][e], -hl[g]);
                if (sj > best) { best = sj; bj = 16 * g + fc; } // ascending j within the lane: the first of equal scores is kept
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const float ov = __shfl_xor(best, o, 64);
                const int oj = __shfl_xor(bj, o, 64);
                if (ov > best || (ov == best && oj < bj)) { best = ov; bj = oj; }
            }
            const int64_t m = m0 + 16 * t + 4 * kr + e;
            if (fc == e && m < a.N) {
                a.labels[m] = bj;
                if (a.dist2) a.dist2[m] = fmaxf(0.f, fmaf(-2.f, best, un2_row));
            }
        }
    }
}

// ---- seeding -------------------------------------------------------------------------------------------------------------------
// grid (ceil(N / 64)), 256 threads: wave w takes rows 16 w .. 16 w + 15 of the block in ascending order.  rn == NULL: u = x
__global__ __launch_bounds__(RKM_THREADS) void rkm_seed_dist_kernel(const uint16_t* __restrict__ rows, int64_t N, int D, int64_t ld,
                                                                    const float* __restrict__ rn, const float* __restrict__ target, int first,
                                                                    float* __restrict__ mind, float* __restrict__ bestv,
                                                                    int64_t* __restrict__ besti) {
    __shared__ float sv[4];
    __shared__ int64_t si[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * RKM_SEED_ROWS + wave * 16;
    float bv = -1.f;
    int64_t bi = 0x7fffffffffffffffll;
    for (int i = 0; i < 16; ++i) {
        const int64_t m = m0 + i;
        if (m >= N) break;
        const float scale = rn ? rn[m] : 1.f;
        float acc = 0.f;
        for (int g = lane; g < (D >> 3); g += 64) {
            const f16x8 h = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(rows + m * ld + 8 * g));
            const f32x4 t0 = *reinterpret_cast<const f32x4*>(target + 8 * g), t1 = *reinterpret_cast<const f32x4*>(target + 8 * g + 4);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float diff = __fsub_rn(__fmul_rn((float)h[e], scale), e < 4 ? t0[e] : t1[e - 4]);
                acc = fmaf(diff, diff, acc);
            }
        }
        float v = wave_sum(acc);
        if (!first) v = fminf(mind[m], v);
        if (lane == 0) mind[m] = v;
        if (v > bv) { bv = v; bi = m; }                          // ascending rows: the first of equal values is kept
    }
    if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (sv[w] > bv) { bv = sv[w]; bi = si[w]; }
        bestv[blockIdx.x] = bv;
        besti[blockIdx.x] = bi;
    }
}

// grid (1), 256 threads
__global__ __launch_bounds__(RKM_THREADS) void rkm_seed_pick_kernel(const uint16_t* __restrict__ rows, int64_t N, int D, int64_t ld,
                                                                    const float* __restrict__ rn, const float* __restrict__ bestv,
                                                                    const int64_t* __restrict__ besti, int64_t nblk, int j,
                                                                    float* __restrict__ cur, int64_t* __restrict__ init_index) {
    __shared__ float sv[4];
    __shared__ int64_t si[4];
    const int tid = threadIdx.x;
    float bv = -2.f;
    int64_t bi = 0x7fffffffffffffffll;
    for (int64_t c = tid; c < nblk; c += RKM_THREADS) {
        const float v = bestv[c];
        const int64_t i = besti[c];
        if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int64_t oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { sv[tid >> 6] = bv; si[tid >> 6] = bi; }
    __syncthreads();
    bv = sv[0];
    bi = si[0];
    for (int w = 1; w < 4; ++w)
        if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
    if (bi < 0 || bi >= N) bi = 0;                               // rows of NaN only: no comparison held
    const float scale = rn ? rn[bi] : 1.f;
    const _Float16* const p = reinterpret_cast<const _Float16*>(rows) + bi * ld;
    for (int d = tid; d < D; d += RKM_THREADS) cur[(int64_t)j * D + d] = __fmul_rn((float)p[d], scale);
    if (tid == 0) init_index[j] = bi;
}

// ---- the sums ------------------------------------------------------------------------------------------------------------------
// grid (segments, ceil(D / 512)) - or (segments, 1) with psum == NULL: counts and inertia only -, 256 threads, LDS k x 512 floats + 64
// ints.  rn == NULL: u = x.  labels == NULL: cluster 0.  dist2 == NULL: no inertia.
__global__ __launch_bounds__(RKM_THREADS) void rkm_sum_kernel(const uint16_t* __restrict__ rows, int64_t N, int D, int64_t ld,
                                                              const float* __restrict__ rn, const int32_t* __restrict__ labels,
                                                              const float* __restrict__ dist2, int k, float* __restrict__ psum,
                                                              int32_t* __restrict__ pcount, float* __restrict__ pinertia) {
    extern __shared__ __attribute__((aligned(16))) float rkm_lds[];
    int* const cnt = reinterpret_cast<int*>(rkm_lds);            // [64]
    float* const acc = rkm_lds + 64;                             // [k][RKM_SLAB]: thread t touches columns 2 t, 2 t + 1 only
    const int tid = threadIdx.x;
    const int64_t seg = blockIdx.x, m0 = seg * RKM_SEG, m1 = m0 + RKM_SEG < N ? m0 + RKM_SEG : N;
    const int c0 = blockIdx.y * RKM_SLAB + 2 * tid;
    const bool sums = psum != nullptr, active = sums && c0 < D;
    const bool stats = blockIdx.y == 0;
    if (tid < 64) cnt[tid] = 0;
    if (sums)
        for (int j = 0; j < k; ++j) *reinterpret_cast<float2*>(acc + j * RKM_SLAB + 2 * tid) = make_float2(0.f, 0.f);
    __syncthreads();
    float inertia = 0.f;
    for (int64_t mb = m0; mb < m1; mb += 8) {
        int lab[8];
        float r[8], d2[8];
        unsigned x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t m = mb + i;
            const bool ok = m < m1;
            lab[i] = ok ? (labels ? labels[m] : 0) : -1;
            r[i] = (ok && rn) ? rn[m] : 1.f;
            d2[i] = (ok && stats && dist2) ? dist2[m] : 0.f;
            x[i] = (ok && active) ? *reinterpret_cast<const unsigned*>(rows + m * ld + c0) : 0u;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if ((unsigned)lab[i] >= (unsigned)k) continue;       // past the segment's end (a label is the pass's own: always in range)
            inertia += d2[i];
            if (stats && tid == 0) cnt[lab[i]] += 1;
            if (active) {
                const f16x2 h = __builtin_bit_cast(f16x2, x[i]);
                float2* const at = reinterpret_cast<float2*>(acc + lab[i] * RKM_SLAB + 2 * tid);
                float2 v = *at;
                v.x += __fmul_rn((float)h[0], r[i]);
                v.y += __fmul_rn((float)h[1], r[i]);
                *at = v;
            }
        }
    }
    if (active)
        for (int j = 0; j < k; ++j)
            *reinterpret_cast<float2*>(psum + (seg * k + j) * D + c0) = *reinterpret_cast<const float2*>(acc + j * RKM_SLAB + 2 * tid);
    if (!stats) return;
    __syncthreads();                                             // thread 0's last counts
    if (tid == 0) pinertia[seg] = inertia;
    if (tid < 64) pcount[seg * 64 + tid] = cnt[tid];
}

// grid (ceil(D / 64)), 64 threads: the column mean from the one-cluster sums
__global__ void rkm_mean_kernel(const float* __restrict__ psum, int64_t nseg, int D, float rows, float* __restrict__ mean) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= D) return;
    float s = 0.f;
    for (int64_t g = 0; g < nseg; ++g) s += psum[g * D + c];
    mean[c] = s / rows;
}

// grid (ceil(D / 64), k), 64 threads
__global__ void rkm_update_kernel(const float* __restrict__ psum, const int32_t* __restrict__ pcount, const float* __restrict__ pinertia,
                                  int64_t nseg, int D, int k, float* __restrict__ cur, float* __restrict__ inertia_out) {
    const int c = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
    if (blockIdx.x == 0 && j == 0 && threadIdx.x == 0) {
        float s = 0.f;
        for (int64_t g = 0; g < nseg; ++g) s += pinertia[g];
        inertia_out[0] = s;
    }
    if (c >= D) return;
    int64_t count = 0;
    for (int64_t g = 0; g < nseg; ++g) count += pcount[g * 64 + j];
    if (count == 0) return;                                      // an empty cluster keeps its centroid
    const float* const ps = psum + (int64_t)j * D + c;
    float s = ps[0];
#pragma unroll 8
    for (int64_t g = 1; g < nseg; ++g) s += ps[g * k * D];
    cur[(int64_t)j * D + c] = s / (float)count;
}

// grid (1), 256 threads: order (64 int32) = the seeding position of output cluster r, -1 past k; pos its inverse
__global__ __launch_bounds__(RKM_THREADS) void rkm_finish_kernel(const int32_t* __restrict__ pcount, const float* __restrict__ pinertia,
                                                                 int64_t nseg, int D, int k, const float* __restrict__ cur,
                                                                 float* __restrict__ inertia_out, float* __restrict__ centroids,
                                                                 int64_t* __restrict__ counts, int32_t* __restrict__ order,
                                                                 int32_t* __restrict__ pos) {
    __shared__ int64_t cn[64];
    __shared__ int ord[64];
    const int tid = threadIdx.x;
    if (tid < k) {
        int64_t count = 0;
        for (int64_t g = 0; g < nseg; ++g) count += pcount[g * 64 + tid];
        cn[tid] = count;
    }
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int64_t g = 0; g < nseg; ++g) s += pinertia[g];
        inertia_out[0] = s;
        for (int j = 0; j < k; ++j) ord[j] = j;                  // insertion sort: descending count, equal counts keep their order
        for (int j = 1; j < k; ++j) {
            const int oj = ord[j];
            int i = j - 1;
            while (i >= 0 && cn[ord[i]] < cn[oj]) { ord[i + 1] = ord[i]; --i; }
            ord[i + 1] = oj;
        }
        for (int j = 0; j < 64; ++j) order[j] = j < k ? ord[j] : -1;
        for (int j = 0; j < 64; ++j) pos[j] = -1;
        for (int j = 0; j < k; ++j) {
            pos[ord[j]] = j;
            counts[j] = cn[ord[j]];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < k * D; idx += RKM_THREADS) {
        const int j = idx / D, d = idx - j * D;
        centroids[idx] = cur[(int64_t)ord[j] * D + d];
    }
}

__global__ __launch_bounds__(RKM_THREADS) void rkm_remap_kernel(const int32_t* __restrict__ labels, const float* __restrict__ dist2,
                                                                const int32_t* __restrict__ pos, int64_t N, int32_t* __restrict__ labels_out,
                                                                float* __restrict__ dist2_out) {
    const int64_t m = (int64_t)blockIdx.x * RKM_THREADS + threadIdx.x;
    if (m >= N) return;
    if (labels_out) labels_out[m] = pos[labels[m] & 63];
    if (dist2_out) dist2_out[m] = dist2[m];
}

// byte offsets into the workspace, each a multiple of 16
struct RkmLayout {
    int64_t nseg, nblk;
    int64_t cur, order, pos, mean, rn, labels, dist2, mind, bestv, besti, psum, pcount, pinertia, total;
};

// the checks the three entry points share; 0, or CBAS_EINVAL with the message set
int rkm_layout(const char* what, int64_t n_rows, int32_t dim, int32_t k, bool fit, RkmLayout* L) {
    if (n_rows < 1 || (n_rows + RKM_SEED_ROWS - 1) / RKM_SEED_ROWS > 0x7fffffff)
        return cbas_fail(CBAS_EINVAL, "%s: n_rows = %lld (1 .. %lld)", what, (long long)n_rows, (long long)0x7fffffff * RKM_SEED_ROWS);
    if (rows_width_ok(what, "dim", dim, RKM_MAX_D) != CBAS_OK) return CBAS_EINVAL;
    if (k < 2 || k > RKM_MAX_K) return cbas_fail(CBAS_EINVAL, "%s: k = %d clusters (2 .. %d)", what, k, RKM_MAX_K);
    if (fit && k > n_rows) return cbas_fail(CBAS_EINVAL, "%s: k = %d clusters of %lld rows", what, k, (long long)n_rows);
    L->nseg = (n_rows + RKM_SEG - 1) / RKM_SEG;
    L->nblk = (n_rows + RKM_SEED_ROWS - 1) / RKM_SEED_ROWS;
    RowsTake take;
    L->cur = take((int64_t)k * dim * 4);
    L->order = take(64 * 4);
    L->pos = take(64 * 4);
    L->mean = take((int64_t)dim * 4);
    L->rn = take(n_rows * 4);
    L->labels = take(n_rows * 4);
    L->dist2 = take(n_rows * 4);
    L->mind = take(n_rows * 4);
    L->bestv = take(L->nblk * 4);
    L->besti = take(L->nblk * 8);
    L->psum = take(L->nseg * k * dim * 4);
    L->pcount = take(L->nseg * 64 * 4);
    L->pinertia = take(L->nseg * 4);
    L->total = take.at;
    return CBAS_OK;
}

int rkm_rows_ok(const char* what, const void* rows, int32_t dim, int64_t ld, int32_t normalize) {
    if (rows_ld_ok(what, "ld", ld, "dim", dim) != CBAS_OK) return CBAS_EINVAL;
    if (normalize != 0 && normalize != 1) return cbas_fail(CBAS_EINVAL, "%s: normalize = %d (0 or 1)", what, normalize);
    if (!rows) return cbas_fail(CBAS_EINVAL, "%s: a NULL pointer", what);
    return CBAS_OK;
}

int rkm_pass(const RkmPass& a, hipStream_t st) {
    const dim3 grid((unsigned)((a.N + RKM_TILE - 1) / RKM_TILE)), wg(RKM_THREADS);
    switch ((a.k + 15) / 16) {
        case 1: hipLaunchKernelGGL(rkm_score_kernel<1>, grid, wg, 0, st, a); break;
        case 2: hipLaunchKernelGGL(rkm_score_kernel<2>, grid, wg, 0, st, a); break;
        case 3: hipLaunchKernelGGL(rkm_score_kernel<3>, grid, wg, 0, st, a); break;
        default: hipLaunchKernelGGL(rkm_score_kernel<4>, grid, wg, 0, st, a); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

extern "C" int64_t cbas_rows_kmeans_workspace_bytes(int64_t n_rows, int32_t dim, int32_t k) {
    RkmLayout L;
    if (rkm_layout("cbas_rows_kmeans_workspace_bytes", n_rows, dim, k, true, &L) != CBAS_OK) return CBAS_EINVAL;
    return L.total;
}

extern "C" int cbas_rows_kmeans_fit(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, int32_t k, int32_t iters, int32_t normalize,
                                    const float* init_centroids_dev, float* centroids_dev, int64_t* counts_dev, float* inertia_dev,
                                    int64_t* init_index_dev, int32_t* labels_dev, float* dist2_dev, void* workspace_dev, int64_t workspace_bytes,
                                    void* stream) {
    const char* const what = "cbas_rows_kmeans_fit";
    RkmLayout L;
    if (rkm_layout(what, n_rows, dim, k, true, &L) != CBAS_OK) return CBAS_EINVAL;
    if (rkm_rows_ok(what, rows_f16_dev, dim, ld, normalize) != CBAS_OK) return CBAS_EINVAL;
    if (iters < 0) return cbas_fail(CBAS_EINVAL, "%s: iters = %d (at least 0)", what, iters);
    if (!centroids_dev || !counts_dev || !inertia_dev || !init_index_dev || !workspace_dev)
        return cbas_fail(CBAS_EINVAL, "%s: a NULL pointer (only init_centroids, labels and dist2 may be NULL)", what);
    if (((uintptr_t)rows_f16_dev | (uintptr_t)init_centroids_dev | (uintptr_t)centroids_dev | (uintptr_t)workspace_dev) % 16)
        return cbas_fail(CBAS_EINVAL, "%s: rows, centroids and workspace must be 16-byte aligned", what);
    if (((uintptr_t)counts_dev | (uintptr_t)init_index_dev) % 8 || ((uintptr_t)inertia_dev | (uintptr_t)labels_dev | (uintptr_t)dist2_dev) % 4)
        return cbas_fail(CBAS_EINVAL, "%s: counts and init_index must be 8-byte aligned, inertia, labels and dist2 4-byte aligned", what);
    if (workspace_bytes < L.total)
        return cbas_fail(CBAS_EINVAL, "%s: workspace of %lld bytes, %lld needed (cbas_rows_kmeans_workspace_bytes)", what,
                         (long long)workspace_bytes, (long long)L.total);
    if (cbas_use_device_of(rows_f16_dev) != CBAS_OK) return CBAS_EHIP;
    hipStream_t st = (hipStream_t)stream;
    const uint16_t* const rows = (const uint16_t*)rows_f16_dev;
    char* const ws = (char*)workspace_dev;
    float* const cur = (float*)(ws + L.cur);
    int32_t* const order = (int32_t*)(ws + L.order);
    int32_t* const pos = (int32_t*)(ws + L.pos);
    float* const mean = (float*)(ws + L.mean);
    float* const rn = normalize ? (float*)(ws + L.rn) : nullptr;
    int32_t* const labels = (int32_t*)(ws + L.labels);
    float* const dist2 = (float*)(ws + L.dist2);
    float* const mind = (float*)(ws + L.mind);
    float* const bestv = (float*)(ws + L.bestv);
    int64_t* const besti = (int64_t*)(ws + L.besti);
    float* const psum = (float*)(ws + L.psum);
    int32_t* const pcount = (int32_t*)(ws + L.pcount);
    float* const pinertia = (float*)(ws + L.pinertia);
    const dim3 wg(RKM_THREADS);
    const unsigned nseg = (unsigned)L.nseg, slabs = (unsigned)((dim + RKM_SLAB - 1) / RKM_SLAB);
    const size_t sum_lds = (size_t)(64 + (size_t)k * RKM_SLAB) * 4;
    if (rows_lds_opt_in(&rkm_sum_kernel, sum_lds) != CBAS_OK) return CBAS_EHIP;

    if (normalize)
        hipLaunchKernelGGL(rows_rn_kernel, dim3((unsigned)((n_rows * 4 + RKM_THREADS - 1) / RKM_THREADS)), wg, 0, st, rows, n_rows, dim, ld, rn);
    if (init_centroids_dev) {
        HIP_TRY(hipMemcpyAsync(cur, init_centroids_dev, (size_t)k * dim * 4, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemsetAsync(init_index_dev, 0xff, (size_t)k * 8, st));
    } else {
        // the column mean: the sums of one cluster that holds every row
        hipLaunchKernelGGL(rkm_sum_kernel, dim3(nseg, slabs), wg, (size_t)(64 + RKM_SLAB) * 4, st, rows, n_rows, dim, ld, (const float*)rn,
                           (const int32_t*)nullptr, (const float*)nullptr, 1, psum, pcount, pinertia);
        hipLaunchKernelGGL(rkm_mean_kernel, dim3((dim + 63) / 64), dim3(64), 0, st, (const float*)psum, L.nseg, dim, (float)n_rows, mean);
        for (int j = 0; j < k; ++j) {
            // j = 1 starts the running minimum over the seeds: what step 0 left in mind is the distance to the mean
            hipLaunchKernelGGL(rkm_seed_dist_kernel, dim3((unsigned)L.nblk), wg, 0, st, rows, n_rows, dim, ld, (const float*)rn,
                               j == 0 ? (const float*)mean : (const float*)(cur + (int64_t)(j - 1) * dim), j <= 1 ? 1 : 0, mind, bestv, besti);
            hipLaunchKernelGGL(rkm_seed_pick_kernel, dim3(1), wg, 0, st, rows, n_rows, dim, ld, (const float*)rn, (const float*)bestv,
                               (const int64_t*)besti, L.nblk, j, cur, init_index_dev);
        }
    }
    HIP_TRY(hipGetLastError());
    const RkmPass pass{rows, n_rows, dim, ld, cur, k, normalize, labels, dist2};
    for (int t = 0; t <= iters; ++t) {
        LAUNCH_TRY(rkm_pass(pass, st));
        const bool last = t == iters;
        hipLaunchKernelGGL(rkm_sum_kernel, dim3(nseg, last ? 1u : slabs), wg, last ? (size_t)64 * 4 : sum_lds, st, rows, n_rows, dim, ld,
                           (const float*)rn, (const int32_t*)labels, (const float*)dist2, k, last ? (float*)nullptr : psum, pcount, pinertia);
        if (!last)
            hipLaunchKernelGGL(rkm_update_kernel, dim3((dim + 63) / 64, k), dim3(64), 0, st, (const float*)psum, (const int32_t*)pcount,
                               (const float*)pinertia, L.nseg, dim, k, cur, inertia_dev + t);
    }
    hipLaunchKernelGGL(rkm_finish_kernel, dim3(1), wg, 0, st, (const int32_t*)pcount, (const float*)pinertia, L.nseg, dim, k, (const float*)cur,
                       inertia_dev + iters, centroids_dev, counts_dev, order, pos);
    if (labels_dev || dist2_dev)
        hipLaunchKernelGGL(rkm_remap_kernel, dim3((unsigned)((n_rows + RKM_THREADS - 1) / RKM_THREADS)), wg, 0, st, (const int32_t*)labels,
                           (const float*)dist2, (const int32_t*)pos, n_rows, labels_dev, dist2_dev);
    HIP_TRY(hipGetLastError());
    return CBAS_OK;
}

extern "C" int cbas_rows_kmeans_assign(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, int32_t k, int32_t normalize,
                                       const float* centroids_dev, int32_t* labels_dev, float* dist2_dev, void* stream) {
    const char* const what = "cbas_rows_kmeans_assign";
    RkmLayout L;
    if (rkm_layout(what, n_rows, dim, k, false, &L) != CBAS_OK) return CBAS_EINVAL;      // fewer rows than centroids is fine here
    if (rkm_rows_ok(what, rows_f16_dev, dim, ld, normalize) != CBAS_OK) return CBAS_EINVAL;
    if (!centroids_dev || !labels_dev) return cbas_fail(CBAS_EINVAL, "%s: a NULL pointer (only dist2 may be NULL)", what);
    if (((uintptr_t)rows_f16_dev | (uintptr_t)centroids_dev) % 16) return cbas_fail(CBAS_EINVAL, "%s: rows and centroids must be 16-byte aligned", what);
    if (((uintptr_t)labels_dev | (uintptr_t)dist2_dev) % 4) return cbas_fail(CBAS_EINVAL, "%s: labels and dist2 must be 4-byte aligned", what);
    if (cbas_use_device_of(rows_f16_dev) != CBAS_OK) return CBAS_EHIP;
    const RkmPass pass{(const uint16_t*)rows_f16_dev, n_rows, dim, ld, centroids_dev, k, normalize, labels_dev, dist2_dev};
    LAUNCH_TRY(rkm_pass(pass, (hipStream_t)stream));
    return CBAS_OK;
}
