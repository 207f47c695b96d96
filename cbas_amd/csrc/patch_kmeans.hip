// k-means of patch features on the device: farthest-point seeding, Lloyd rounds, assignment.  Rows and
// problems are patch_pca.hip's: n frames of T fp32 rows of D floats (row stride ld), the first n_prefix rows of a frame skipped;
// FRAME scope is n problems of M = P rows, BATCH scope one problem of M = n P rows, the problem a grid dimension of every kernel.
// The working row u of a row x is x itself, or with `normalize` fl(x * rn), rn = fp32(1 / sqrt(sum x^2)) with the sum in fp64
// (rn = 0 for a zero row); no normalised copy is written, rn is applied where the row is used.
//
//   km_rownorm_kernel    rn of every row (seeding only): one wave per row
//   km_mean_*            the column mean of u: thread per column, KMEANS_CHUNK rows each in ascending order, chunks in order
//   km_seed_dist_kernel  d(m) = sum_d (u_md - t_d)^2 against the target t (the mean, then the newest seed): one wave per row, lane
//                        l the fmaf chain over d = l, l + 64, ..., then the xor tree; mind(m) = min(mind(m), d(m)); the chunk's
//                        largest mind and its lowest row
//   km_seed_pick_kernel  the largest over the chunks, ties to the lowest row; writes the seed and its index
//   km_pass_kernel       THE ROUND.  One workgroup per chunk of KMEANS_CHUNK rows, the k centroids resident in LDS, 16 rows at a
//                        time: x . c_j for 16 rows x 16 centroids on v_mfma_f32_16x16x4_f32 (the 16-column tiles of D dealt round
//                        robin to the four waves, the four partial dots added in wave order), score_j = fmaf(rn, x . c_j,
//                        -|c_j|^2 / 2), the largest score wins (ties: the lowest j), dist2 = max(0, |u|^2 - 2 score).  The rows
//                        stay in registers; a second matrix product sums[j][d] += w[m][j] x[m][d], w = rn for the row's cluster
//                        and 0 elsewhere, adds them to the chunk's k x D sums in ascending row order (adding 0 x changes no sum)
//   km_update_kernel     centroid = (chunk sums in ascending order) / count, an empty cluster untouched; the round's inertia
//   km_finish_kernel     final counts and inertia, clusters by descending count (ties: seeding order)
// No atomics; every sum has a fixed order that does not depend on how many problems a launch carries.
#include "kernels.h"

namespace {

constexpr int KM_THREADS = 256;
constexpr int KM_TILE = 16;                          // rows per matrix tile
constexpr int KM_CPAD = 4;                           // LDS centroid rows are D + 4 floats apart
constexpr int KM_XT_LD = 20;                         // floats per row of a wave's 16 x 16 transposition tile
constexpr int KM_FIXED_LDS = 16 + 4 * 256 + 2 * 64 + 4 * 16 + 4 * KM_TILE * KM_XT_LD;      // floats after the centroids

__device__ __forceinline__ const float* km_row(const PcaRows& r, int prob, int64_t m) {
    const int64_t f = (int64_t)prob * r.frames_per_problem + m / r.P;
    return r.x + (f * r.T + r.n_prefix + (m % r.P)) * r.ld;
}
__device__ __forceinline__ float km_scale(double ss, int normalize) {
    return normalize ? (ss > 0.0 ? (float)(1.0 / sqrt(ss)) : 0.f) : 1.f;
}
// LDS traffic between the lanes of ONE wave: the hardware runs a wave's LDS instructions in order; this keeps the compiler from
// moving them across
__device__ __forceinline__ void km_wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- seeding -------------------------------------------------------------------------------------------------------------------
// grid (ceil(M / 4), problems), 256 threads: one wave per row
__global__ __launch_bounds__(KM_THREADS) void km_rownorm_kernel(PcaRows r, int D, int normalize, float* __restrict__ rn) {
    const int lane = threadIdx.x & 63, prob = blockIdx.y;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= r.M) return;
    const float* const p = km_row(r, prob, m);
    double ss = 0.0;
    for (int d = lane; d < D; d += 64) ss = fma((double)p[d], (double)p[d], ss);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if (lane == 0) rn[(int64_t)prob * r.M + m] = km_scale(ss, normalize);
}

// grid (ceil(D / 64), chunks, problems), 64 threads
__global__ void km_mean_stage1_kernel(PcaRows r, int D, int64_t nch, const float* __restrict__ rn, float* __restrict__ tmp) {
    const int c = blockIdx.x * 64 + threadIdx.x, prob = blockIdx.z;
    const int64_t ch = blockIdx.y;
    if (c >= D) return;
    const int64_t m0 = ch * KMEANS_CHUNK, m1 = m0 + KMEANS_CHUNK < r.M ? m0 + KMEANS_CHUNK : r.M;
    float s = 0.f;
    for (int64_t m = m0; m < m1; ++m) s += __fmul_rn(km_row(r, prob, m)[c], rn[(int64_t)prob * r.M + m]);
    tmp[((int64_t)prob * nch + ch) * D + c] = s;
}
// grid (ceil(D / 64), problems), 64 threads
__global__ void km_mean_stage2_kernel(const float* __restrict__ tmp, int D, int64_t nch, float rows, float* __restrict__ mean) {
    const int c = blockIdx.x * 64 + threadIdx.x, prob = blockIdx.y;
    if (c >= D) return;
    float s = 0.f;
    for (int64_t ch = 0; ch < nch; ++ch) s += tmp[((int64_t)prob * nch + ch) * D + c];
    mean[(int64_t)prob * D + c] = s / rows;
}

// grid (chunks, problems), 256 threads: wave w takes rows 16 w .. 16 w + 15 of the chunk in ascending order
__global__ __launch_bounds__(KM_THREADS) void km_seed_dist_kernel(PcaRows r, int D, const float* __restrict__ rn, const float* __restrict__ target,
                                                                  int64_t target_stride, int first, float* __restrict__ mind,
                                                                  float* __restrict__ bestv, int32_t* __restrict__ besti) {
    __shared__ float sv[4];
    __shared__ int si[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, prob = blockIdx.y;
    const int64_t nch = gridDim.x, m0 = (int64_t)blockIdx.x * KMEANS_CHUNK + wave * 16;
    const float* const t = target + prob * target_stride;
    float bv = -1.f;
    int bi = 0x7fffffff;
    for (int i = 0; i < 16; ++i) {
        const int64_t m = m0 + i;
        if (m >= r.M) break;
        const float* const p = km_row(r, prob, m);
        const float scale = rn[(int64_t)prob * r.M + m];
        float acc = 0.f;
        for (int d = lane; d < D; d += 64) {
            const float diff = __fmul_rn(p[d], scale) - t[d];
            acc = fmaf(diff, diff, acc);
        }
        float v = wave_sum(acc);
        if (!first) v = fminf(mind[(int64_t)prob * r.M + m], v);
        if (lane == 0) mind[(int64_t)prob * r.M + m] = v;
        if (v > bv) { bv = v; bi = (int)m; }                     // ascending rows: the first of equal values is kept
    }
    if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (sv[w] > bv) { bv = sv[w]; bi = si[w]; }
        bestv[(int64_t)prob * nch + blockIdx.x] = bv;
        besti[(int64_t)prob * nch + blockIdx.x] = bi;
    }
}

// grid (problems), 256 threads
__global__ __launch_bounds__(KM_THREADS) void km_seed_pick_kernel(PcaRows r, int D, const float* __restrict__ rn, const float* __restrict__ bestv,
                                                                  const int32_t* __restrict__ besti, int64_t nch, int j, int k,
                                                                  float* __restrict__ cur, int32_t* __restrict__ init_index) {
    __shared__ float sv[4];
    __shared__ int si[4];
    const int tid = threadIdx.x, prob = blockIdx.x;
    float bv = -2.f;
    int bi = 0x7fffffff;
    for (int64_t c = tid; c < nch; c += KM_THREADS) {
        const float v = bestv[(int64_t)prob * nch + c];
        const int i = besti[(int64_t)prob * nch + c];
        if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { sv[tid >> 6] = bv; si[tid >> 6] = bi; }
    __syncthreads();
    bv = sv[0];
    bi = si[0];
    for (int w = 1; w < 4; ++w)
        if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
    if (bi < 0 || (int64_t)bi >= r.M) bi = 0;                    // rows of NaN only: no comparison held
    const float* const p = km_row(r, prob, bi);
    const float scale = rn[(int64_t)prob * r.M + bi];
    for (int d = tid; d < D; d += KM_THREADS) cur[((int64_t)prob * k + j) * D + d] = __fmul_rn(p[d], scale);
    if (tid == 0) init_index[(int64_t)prob * k + j] = bi;
}

// ---- the round -----------------------------------------------------------------------------------------------------------------
// grid (chunks, problems), 256 threads, LDS (k (D + 4) + KM_FIXED_LDS) floats.  NCT: 16-column tiles per wave compiled in
// (tile c of the D / 16 belongs to wave c % 4, its slot is c / 4); ACC: add the rows into the chunk's sums.
template <int NCT, bool ACC>
__global__ __launch_bounds__(KM_THREADS) void km_pass_kernel(PcaRows r, int D, int k, int normalize, const float* __restrict__ cent,
                                                             int64_t cent_stride, float* __restrict__ psum, int32_t* __restrict__ pcount,
                                                             float* __restrict__ pinertia, int32_t* __restrict__ labels,
                                                             float* __restrict__ dist2) {
    extern __shared__ __attribute__((aligned(16))) float km_lds[];
    const int cld = D + KM_CPAD;
    float* const sc = km_lds;                                    // [k][cld] the centroids
    float* const hn = sc + k * cld;                              // [16] |c_j|^2 / 2, +inf past k
    float* const ps = hn + 16;                                   // [4 waves][16 rows][16 centroids] partial dots
    double* const pss = reinterpret_cast<double*>(ps + 4 * 256); // [4 waves][16 rows] partial sums of squares
    float* const rw = reinterpret_cast<float*>(pss + 64);        // [16] the row's factor rn, 0 for a row past the end
    int* const lab = reinterpret_cast<int*>(rw + 16);            // [16] the row's cluster, -1 for a row past the end
    float* const d2s = reinterpret_cast<float*>(lab + 16);       // [16] the row's squared distance
    int* const cnt = reinterpret_cast<int*>(d2s + 16);           // [16] the chunk's counts
    float* const xt = reinterpret_cast<float*>(cnt + 16);        // [4 waves][16][KM_XT_LD]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fc = lane & 15, kr = lane >> 4;
    const int prob = blockIdx.y;
    const int64_t chunk = blockIdx.x, nch = gridDim.x;
    const int64_t m0 = chunk * KMEANS_CHUNK, m1 = m0 + KMEANS_CHUNK < r.M ? m0 + KMEANS_CHUNK : r.M;
    const int ntile = D >> 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    // the centroids, then half their squared norms: wave w those of j = w, w + 4, ...; lane l the fmaf chain over d = l, l + 64, ...
    const float* const cg = cent + prob * cent_stride;
    for (int idx = tid; idx < k * (D >> 2); idx += KM_THREADS) {
        const int j = idx / (D >> 2), q = idx - j * (D >> 2);
        *reinterpret_cast<f32x4*>(sc + j * cld + 4 * q) = *reinterpret_cast<const f32x4*>(cg + (int64_t)j * D + 4 * q);
    }
    if (tid < 16) {
        cnt[tid] = 0;
        if (tid >= k) hn[tid] = __builtin_inff();
    }
    __syncthreads();
    for (int j = wave; j < k; j += 4) {
        float a = 0.f;
        for (int d = lane; d < D; d += 64) a = fmaf(sc[j * cld + d], sc[j * cld + d], a);
        a = wave_sum(a);
        if (lane == 0) hn[j] = 0.5f * a;
    }
    __syncthreads();

    f32x4 sums[NCT];
#pragma unroll
    for (int i = 0; i < NCT; ++i) sums[i] = zero;
    float inertia = 0.f;
    const float* const cb = sc + (fc < k ? fc : 0) * cld + 4 * kr;         // lane (fc, kr): centroid fc, columns 16 c + 4 kr .. + 3
    float* const xw = xt + wave * (KM_TILE * KM_XT_LD);

    for (int64_t ms = m0; ms < m1; ms += KM_TILE) {
        // lane (fc, kr) holds row ms + fc, columns 16 c + 4 kr .. + 3 of each of its wave's tiles
        const int64_t m = ms + fc;
        const bool valid = m < m1;
        const float* const p = km_row(r, prob, valid ? m : m0) + 4 * kr;
        f32x4 xr[NCT];
        double ss = 0.0;
        f32x4 acc = zero;
#pragma unroll
        for (int i = 0; i < NCT; ++i) {
            const int c = wave + 4 * i;
            xr[i] = (valid && c < ntile) ? *reinterpret_cast<const f32x4*>(p + 16 * c) : zero;
        }
#pragma unroll
        for (int i = 0; i < NCT; ++i) {
            const int c = wave + 4 * i;
            if (c < ntile) {
                const f32x4 cv = *reinterpret_cast<const f32x4*>(cb + 16 * c);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ss = fma((double)xr[i][e], (double)xr[i][e], ss);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[i][e], cv[e], acc, 0, 0, 0);
                }
            }
        }
        // acc[e] = this wave's part of x . c for row 4 kr + e, centroid fc
#pragma unroll
        for (int e = 0; e < 4; ++e) ps[wave * 256 + (4 * kr + e) * 16 + fc] = acc[e];
        ss += __shfl_xor(ss, 16, 64);
        ss += __shfl_xor(ss, 32, 64);
        if (kr == 0) pss[wave * 16 + fc] = ss;
        __syncthreads();
        if (tid < KM_TILE) {
            const int64_t mr = ms + tid;
            const bool ok = mr < m1;
            const double s2 = ((pss[tid] + pss[16 + tid]) + pss[32 + tid]) + pss[48 + tid];
            const float scale = km_scale(s2, normalize);
            const float un2 = normalize ? (s2 > 0.0 ? 1.f : 0.f) : (float)s2;
            float best = -__builtin_inff();
            int bj = 0;
            for (int j = 0; j < k; ++j) {
                const float dot = ((ps[tid * 16 + j] + ps[256 + tid * 16 + j]) + ps[512 + tid * 16 + j]) + ps[768 + tid * 16 + j];
                const float s = fmaf(scale, dot, -hn[j]);
                if (s > best) { best = s; bj = j; }              // ascending j: the first of equal scores is kept
            }
            const float d2 = fmaxf(0.f, fmaf(-2.f, best, un2));
            lab[tid] = ok ? bj : -1;
            rw[tid] = ok ? scale : 0.f;
            d2s[tid] = ok ? d2 : 0.f;
            if (ok && labels) labels[(int64_t)prob * r.M + mr] = bj;
            if (ok && dist2) dist2[(int64_t)prob * r.M + mr] = d2;
        }
        __syncthreads();
        if (ACC) {
            if (tid == 0)
                for (int i = 0; i < KM_TILE; ++i)
                    if (lab[i] >= 0) {
                        inertia += d2s[i];
                        cnt[lab[i]] += 1;
                    }
            // sums[j][d] += w[row][j] x[row][d]: A = w (lane (fc, kr): centroid fc, row 4 s + kr), B = x (row 4 s + kr, column fc)
            float w[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) w[s] = lab[4 * s + kr] == fc ? rw[4 * s + kr] : 0.f;
#pragma unroll
            for (int i = 0; i < NCT; ++i) {
                const int c = wave + 4 * i;
                if (c < ntile) {
                    *reinterpret_cast<f32x4*>(xw + fc * KM_XT_LD + 4 * kr) = xr[i];
                    km_wave_lds_order();
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        sums[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s], xw[(4 * s + kr) * KM_XT_LD + fc], sums[i], 0, 0, 0);
                    km_wave_lds_order();
                }
            }
        }
    }
    if (!ACC) return;
    // sums[i][e]: centroid 4 kr + e, column 16 c + fc
    float* const out = psum + ((int64_t)prob * nch + chunk) * k * D;
#pragma unroll
    for (int i = 0; i < NCT; ++i) {
        const int c = wave + 4 * i;
        if (c < ntile)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * kr + e < k) out[(int64_t)(4 * kr + e) * D + 16 * c + fc] = sums[i][e];
    }
    __syncthreads();                                             // thread 0's last counts
    if (tid == 0) pinertia[(int64_t)prob * nch + chunk] = inertia;
    if (tid < 16) pcount[((int64_t)prob * nch + chunk) * 16 + tid] = cnt[tid];
}

// grid (ceil(D / 64), k, problems), 64 threads
__global__ void km_update_kernel(const float* __restrict__ psum, const int32_t* __restrict__ pcount, const float* __restrict__ pinertia,
                                 int64_t nch, int D, int k, float* __restrict__ cur, float* __restrict__ inertia_out, int inertia_ld) {
    const int c = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y, prob = blockIdx.z;
    if (blockIdx.x == 0 && j == 0 && threadIdx.x == 0) {
        float s = 0.f;
        for (int64_t ch = 0; ch < nch; ++ch) s += pinertia[(int64_t)prob * nch + ch];
        inertia_out[(int64_t)prob * inertia_ld] = s;
    }
    if (c >= D) return;
    int count = 0;
    for (int64_t ch = 0; ch < nch; ++ch) count += pcount[((int64_t)prob * nch + ch) * 16 + j];
    if (count == 0) return;                                      // an empty cluster keeps its centroid
    const float* const ps = psum + (int64_t)prob * nch * k * D + (int64_t)j * D + c;
    float s = ps[0];
#pragma unroll 8
    for (int64_t ch = 1; ch < nch; ++ch) s += ps[ch * k * D];
    cur[((int64_t)prob * k + j) * D + c] = s / (float)count;
}

// grid (problems), 256 threads
__global__ __launch_bounds__(KM_THREADS) void km_finish_kernel(const int32_t* __restrict__ pcount, const float* __restrict__ pinertia, int64_t nch,
                                                               int D, int k, const float* __restrict__ cur, float* __restrict__ inertia_out,
                                                               int inertia_ld, float* __restrict__ centroids, int32_t* __restrict__ counts,
                                                               int32_t* __restrict__ order) {
    __shared__ int cn[16], ord[16];
    const int tid = threadIdx.x, prob = blockIdx.x;
    if (tid < k) {
        int count = 0;
        for (int64_t ch = 0; ch < nch; ++ch) count += pcount[((int64_t)prob * nch + ch) * 16 + tid];
        cn[tid] = count;
    }
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int64_t ch = 0; ch < nch; ++ch) s += pinertia[(int64_t)prob * nch + ch];
        inertia_out[(int64_t)prob * inertia_ld] = s;
        for (int j = 0; j < k; ++j) ord[j] = j;                  // insertion sort: descending count, equal counts keep their order
        for (int j = 1; j < k; ++j) {
            const int oj = ord[j];
            int i = j - 1;
            while (i >= 0 && cn[ord[i]] < cn[oj]) { ord[i + 1] = ord[i]; --i; }
            ord[i + 1] = oj;
        }
        for (int j = 0; j < 16; ++j) order[(int64_t)prob * 16 + j] = j < k ? ord[j] : -1;
        for (int j = 0; j < k; ++j) counts[(int64_t)prob * k + j] = cn[ord[j]];
    }
    __syncthreads();
    for (int idx = tid; idx < k * D; idx += KM_THREADS) {
        const int j = idx / D, d = idx - j * D;
        centroids[(int64_t)prob * k * D + idx] = cur[((int64_t)prob * k + ord[j]) * D + d];
    }
}

bool km_shape_ok(const PcaRows& r, int nprob, int D, int k) {
    return r.x && (uintptr_t)r.x % 16 == 0 && r.ld >= D && r.ld % 4 == 0 && D > 0 && D % 32 == 0 && D <= PCA_MAX_D && r.P >= 1 &&
           r.n_prefix >= 0 && r.T == r.n_prefix + r.P && r.frames_per_problem >= 1 && nprob >= 1 && nprob <= 65535 && k >= 2 &&
           k <= KMEANS_MAX_K && r.M >= 1 && r.M <= 0x7fffffff && r.M == (int64_t)r.P * r.frames_per_problem;
}

template <int NCT, bool ACC>
int km_pass_launch(const PcaRows& r, int nprob, int D, int k, int normalize, const float* cent, int64_t cent_stride, float* psum,
                   int32_t* pcount, float* pinertia, int32_t* labels, float* dist2, hipStream_t st) {
    const size_t lds = (size_t)(k * (D + KM_CPAD) + KM_FIXED_LDS) * sizeof(float);
    if (lds > 160 * 1024) return -1;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&km_pass_kernel<NCT, ACC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024) != hipSuccess)
            return -2;
        attr_set = true;
    }
    hipLaunchKernelGGL((km_pass_kernel<NCT, ACC>), dim3((unsigned)kmeans_chunks(r.M), (unsigned)nprob), dim3(KM_THREADS), lds, st, r, D, k,
                       normalize, cent, cent_stride, psum, pcount, pinertia, labels, dist2);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

int launch_kmeans_seed(const PcaRows& r, int nprob, int D, int k, int normalize, float* cur, int32_t* init_index, float* rn, float* mind,
                       float* tmp, float* mean, float* bestv, int32_t* besti, hipStream_t st) {
    if (!km_shape_ok(r, nprob, D, k) || !cur || !init_index || !rn || !mind || !tmp || !mean || !bestv || !besti) return -1;
    const int64_t nch = kmeans_chunks(r.M);
    const dim3 chunks((unsigned)nch, (unsigned)nprob), wg(KM_THREADS);
    hipLaunchKernelGGL(km_rownorm_kernel, dim3((unsigned)((r.M + 3) / 4), (unsigned)nprob), wg, 0, st, r, D, normalize, rn);
    hipLaunchKernelGGL(km_mean_stage1_kernel, dim3((D + 63) / 64, (unsigned)nch, (unsigned)nprob), dim3(64), 0, st, r, D, nch, rn, tmp);
    hipLaunchKernelGGL(km_mean_stage2_kernel, dim3((D + 63) / 64, (unsigned)nprob), dim3(64), 0, st, tmp, D, nch, (float)r.M, mean);
    for (int j = 0; j < k; ++j) {
        if (j == 0) hipLaunchKernelGGL(km_seed_dist_kernel, chunks, wg, 0, st, r, D, rn, mean, (int64_t)D, 1, mind, bestv, besti);
        // j = 1 starts the running minimum over the seeds: what step 0 left in mind is the distance to the mean
        else hipLaunchKernelGGL(km_seed_dist_kernel, chunks, wg, 0, st, r, D, rn, cur + (int64_t)(j - 1) * D, (int64_t)k * D, j == 1 ? 1 : 0, mind, bestv, besti);
        hipLaunchKernelGGL(km_seed_pick_kernel, dim3((unsigned)nprob), wg, 0, st, r, D, rn, bestv, besti, nch, j, k, cur, init_index);
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_kmeans_pass(const PcaRows& r, int nprob, int D, int k, int normalize, const float* cent, int64_t cent_stride, float* psum,
                       int32_t* pcount, float* pinertia, int32_t* labels, float* dist2, hipStream_t st) {
    const bool acc = psum != nullptr;
    if (!km_shape_ok(r, nprob, D, k) || !cent || (uintptr_t)cent % 16 || cent_stride % 4 || (acc && (!pcount || !pinertia)) ||
        (!acc && (pcount || pinertia)) || kmeans_chunks(r.M) > 0x7fffffff)
        return -1;
#define KM_PASS(NCT)                                                                                                              \
    return acc ? km_pass_launch<NCT, true>(r, nprob, D, k, normalize, cent, cent_stride, psum, pcount, pinertia, labels, dist2, st) \
               : km_pass_launch<NCT, false>(r, nprob, D, k, normalize, cent, cent_stride, psum, pcount, pinertia, labels, dist2, st)
    if (D <= 64) { KM_PASS(1); }
    if (D <= 128) { KM_PASS(2); }
    if (D <= 384) { KM_PASS(6); }
    if (D <= 768) { KM_PASS(12); }
    if (D <= 1024) { KM_PASS(16); }
    KM_PASS(24);
#undef KM_PASS
}

int launch_kmeans_update(const float* psum, const int32_t* pcount, const float* pinertia, int64_t nch, int nprob, int D, int k, float* cur,
                         float* inertia_out, int inertia_ld, hipStream_t st) {
    if (!psum || !pcount || !pinertia || !cur || !inertia_out || nch < 1 || nprob < 1 || nprob > 65535 || D <= 0 || D > PCA_MAX_D || k < 2 ||
        k > KMEANS_MAX_K || inertia_ld < 1)
        return -1;
    hipLaunchKernelGGL(km_update_kernel, dim3((D + 63) / 64, k, (unsigned)nprob), dim3(64), 0, st, psum, pcount, pinertia, nch, D, k, cur,
                       inertia_out, inertia_ld);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_kmeans_finish(const int32_t* pcount, const float* pinertia, int64_t nch, int nprob, int D, int k, const float* cur,
                         float* inertia_out, int inertia_ld, float* centroids, int32_t* counts, int32_t* order, hipStream_t st) {
    if (!pcount || !pinertia || !cur || !inertia_out || !centroids || !counts || !order || nch < 1 || nprob < 1 || D <= 0 || D > PCA_MAX_D ||
        k < 2 || k > KMEANS_MAX_K || inertia_ld < 1)
        return -1;
    hipLaunchKernelGGL(km_finish_kernel, dim3((unsigned)nprob), dim3(KM_THREADS), 0, st, pcount, pinertia, nch, D, k, cur, inertia_out, inertia_ld,
                       centroids, counts, order);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
