// PCA over resident CLS rows: cbas_rows_pca_workspace_bytes / cbas_rows_pca_fit / cbas_rows_pca_project of
// include/cbas_mi355x.h, kernels and entry points in one file.  rows (N, D) fp16 with row stride ld.  The working row of a row x is
// u = x widened to fp32 (normalize = 0) or u = fl(x * rn) (normalize = 1), rn the reciprocal norm of rows_rn.h; no normalised copy is
// written, rn is applied where the row is used.  The eigenvectors are patch_pca.hip's launch_pca_eig, unchanged, on the C built here.
//
//   rows_rn_kernel     (rows_rn.h) rn of every row, for the mean and the covariance (normalize = 1 only)
//   fp_mean_*          mu = (1 / N) sum_m u_m: thread per column pair, one fp32 sum per column over the FP_CHUNK rows of a chunk in
//                      ascending order, then the chunks in ascending order, one division
//   fp_cov_kernel      pca_cov_kernel's tile (128 x 128 of the upper triangle per workgroup, 64 x 64 per wave, 32-row slabs staged
//                      centred into LDS with row stride 144 floats, v_mfma_f32_16x16x4_f32) fed from the fp16 rows, and with the row
//                      dimension cut into PARTS: a workgroup owns one tile pair of one part, runs one fmaf chain per element and
//                      chunk (the chain restarts at every chunk of FP_CHUNK rows) and adds the chunks' results in ascending order
//   fp_cov_reduce      C[i][j] = C[j][i] = (part 0 + part 1 + ...) / (N - 1) for i <= j, written over part 0: exactly symmetric
//   fp_project_kernel  one streaming pass: a wave owns two 16-row tiles; lane (fc, kr) holds, of every 32-column block, the 8 columns
//                      8 kr .. 8 kr + 7 of row fc (A operand) and of component fc (B operand, zero past k); the centred value
//                      fl(u - mu) is formed in registers.  normalize = 1 reads the wave's rows twice: once for rn, once for the scores
// Every sum has a fixed order, a function of (n_rows, dim) alone, and there are no atomics: two calls give the same bits.
#include "kernels.h"
#include "rows_api.h"
#include "rows_rn.h"

namespace {

constexpr int FP_THREADS = 256;
constexpr int FP_CHUNK = CBAS_ROWS_PCA_CHUNK;        // rows per fmaf chain and per partial column sum
constexpr int FP_MAX_PARTS = CBAS_ROWS_PCA_MAX_PARTS;
constexpr int FP_LDS_LD = 144;                       // floats per staged row: 128 + 16 (patch_pca.hip: bank spread of the four k rows)
constexpr int FP_SLAB = 32;                          // rows staged per step
constexpr int FP_TILE = 128;                         // rows a workgroup of the projection owns: 32 a wave
constexpr int FP_RT = 2;                             // 16-row tiles per wave
constexpr int64_t FP_MAX_N = 16777216;               // (float)n_rows and (float)(n_rows - 1) are exact

static_assert(FP_CHUNK % FP_SLAB == 0, "a chunk is a whole number of slabs");

// ---- mean ----------------------------------------------------------------------------------------------------------------------
// grid (ceil(D / 128), chunks), 64 threads: thread -> columns 2 t, 2 t + 1 of the block's 128
__global__ __launch_bounds__(64) void fp_mean_stage1_kernel(const uint16_t* __restrict__ rows, int64_t N, int D, int64_t ld,
                                                            const float* __restrict__ rn, float* __restrict__ tmp) {
    const int c = (blockIdx.x * 64 + threadIdx.x) * 2, ch = blockIdx.y;
    if (c >= D) return;
    const int64_t m0 = (int64_t)ch * FP_CHUNK, m1 = m0 + FP_CHUNK < N ? m0 + FP_CHUNK : N;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll 8
    for (int64_t m = m0; m < m1; ++m) {
        const f16x2 h = __builtin_bit_cast(f16x2, *reinterpret_cast<const uint32_t*>(rows + m * ld + c));
        float a = (float)h[0], b = (float)h[1];
        if (rn) {
            const float r = rn[m];
            a = __fmul_rn(a, r);
            b = __fmul_rn(b, r);
        }
        s0 = __fadd_rn(s0, a);
        s1 = __fadd_rn(s1, b);
    }
    tmp[(int64_t)ch * D + c] = s0;
    tmp[(int64_t)ch * D + c + 1] = s1;
}
// grid (ceil(D / 64)), 64 threads
__global__ __launch_bounds__(64) void fp_mean_stage2_kernel(const float* __restrict__ tmp, int D, int64_t nchunks, float n, float* __restrict__ mean) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= D) return;
    float s = 0.f;
    for (int64_t ch = 0; ch < nchunks; ++ch) s = __fadd_rn(s, tmp[ch * D + c]);
    mean[c] = __fdiv_rn(s, n);
}

// ---- covariance ------------------------------------------------------------------------------------------------------------------
// four halves of a row -> the working values
__device__ __forceinline__ f32x4 fp_widen(const uint16_t* p, float r, bool norm) {
    const f16x4 h = __builtin_bit_cast(f16x4, *reinterpret_cast<const uint2*>(p));
    f32x4 v = {(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    if (norm) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __fmul_rn(v[e], r);
    }
    return v;
}

// grid (tile pairs ti <= tj of the ceil(D / 128)^2 tiles, parts), 256 threads.  cpp: chunks per part
__global__ __launch_bounds__(FP_THREADS) void fp_cov_kernel(const uint16_t* __restrict__ rows, int64_t N, int D, int64_t ld,
                                                            const float* __restrict__ rn, const float* __restrict__ mean, int64_t cpp,
                                                            float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sa[FP_SLAB][FP_LDS_LD];
    __shared__ __attribute__((aligned(16))) float sb[FP_SLAB][FP_LDS_LD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int nt = (D + 127) / 128;
    int ti = 0, left = blockIdx.x;                   // pair index -> (ti, tj), ti <= tj, row by row of the upper triangle
    while (left >= nt - ti) { left -= nt - ti; ++ti; }
    const int tj = ti + left;
    const bool diag = ti == tj;
    const int64_t pm0 = (int64_t)blockIdx.y * cpp * FP_CHUNK, pm1 = pm0 + cpp * FP_CHUNK < N ? pm0 + cpp * FP_CHUNK : N;
    const int i0 = ti * 128, j0 = tj * 128;
    const bool norm = rn != nullptr;

    // staging: thread -> row (tid >> 5) + 8 q of the slab, columns 4 (tid & 31) .. + 3 of the tile (D % 4 == 0: all in or all out)
    const int sr = tid >> 5, c4 = (tid & 31) * 4;
    const bool a_in = i0 + c4 < D, b_in = !diag && j0 + c4 < D;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 mu_a = a_in ? *reinterpret_cast<const f32x4*>(mean + i0 + c4) : zero;
    const f32x4 mu_b = b_in ? *reinterpret_cast<const f32x4*>(mean + j0 + c4) : zero;
    f32x4 ra[4], rb[4];
    auto fetch = [&](int64_t ms) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t m = ms + sr + 8 * q;
            ra[q] = zero;
            rb[q] = zero;
            if (m < pm1) {                                       // rows past the part are staged as 0
                const uint16_t* const p = rows + m * ld;
                const float r = norm ? rn[m] : 1.f;
                if (a_in) ra[q] = fp_widen(p + i0 + c4, r, norm) - mu_a;
                if (b_in) rb[q] = fp_widen(p + j0 + c4, r, norm) - mu_b;
            }
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            *reinterpret_cast<f32x4*>(&sa[sr + 8 * q][c4]) = ra[q];
            if (!diag) *reinterpret_cast<f32x4*>(&sb[sr + 8 * q][c4]) = rb[q];
        }
    };

    // a wave whose 64 x 64 part lies past D, or below the diagonal of a diagonal tile, has nothing the reduction reads
    const bool live = i0 + wr * 64 < D && j0 + wc * 64 < D && !(diag && wr > wc);
    f32x4 acc[4][4], tot[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = tot[i][j] = zero;

    const float (*const B)[FP_LDS_LD] = diag ? sa : sb;
    const int kr = lane >> 4, fc = lane & 15;
    fetch(pm0);
    put();
    __syncthreads();
    for (int64_t ms = pm0; ms < pm1; ms += FP_SLAB) {
        const bool more = ms + FP_SLAB < pm1;
        if (more) fetch(ms + FP_SLAB);
        if (live) {
            if (ms > pm0 && ((ms - pm0) & (FP_CHUNK - 1)) == 0) {    // a new chunk: the chain restarts, the finished one is added
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) tot[i][j][e] = __fadd_rn(tot[i][j][e], acc[i][j][e]);
                        acc[i][j] = zero;
                    }
            }
#pragma unroll
            for (int kk = 0; kk < FP_SLAB / 4; ++kk) {           // rows ms + 4 kk + (0 .. 3): ascending, one fmaf chain per element
                float a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = sa[kk * 4 + kr][wr * 64 + i * 16 + fc];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = B[kk * 4 + kr][wc * 64 + j * 16 + fc];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();                                         // every wave is done with the slab
        if (more) {
            put();
            __syncthreads();
        }
    }
    if (!live) return;
    float* const out = part + (int64_t)blockIdx.y * D * D;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int gi = i0 + wr * 64 + i * 16 + kr * 4 + e;   // C/D map: row 4 (lane >> 4) + e, column lane & 15
            if (gi >= D) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gj = j0 + wc * 64 + j * 16 + fc;
                if (gj < D) out[(int64_t)gi * D + gj] = __fadd_rn(tot[i][j][e], acc[i][j][e]);      // the last chunk's result
            }
        }
}

// grid (ceil(D / 256), D), 256 threads: element (i = blockIdx.y, j) with i <= j
__global__ __launch_bounds__(256) void fp_cov_reduce_kernel(float* __restrict__ part, int D, int nparts, float dof) {
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= D || j < i) return;
    float s = part[(int64_t)i * D + j];
    for (int p = 1; p < nparts; ++p) s = __fadd_rn(s, part[((int64_t)p * D + i) * D + j]);
    s = __fdiv_rn(s, dof);
    part[(int64_t)i * D + j] = s;
    part[(int64_t)j * D + i] = s;
}

// ---- projection ------------------------------------------------------------------------------------------------------------------
// grid (ceil(N / FP_TILE)), 256 threads, no LDS: the mean and the k components (at most 56 KB) stay in the caches
template <bool NORM>
__global__ __launch_bounds__(FP_THREADS) void fp_project_kernel(const uint16_t* __restrict__ rows, int64_t N, int D, int64_t ld, int k,
                                                                const float* __restrict__ mean, const float* __restrict__ comp,
                                                                const float* __restrict__ scale, float* __restrict__ scores,
                                                                float* __restrict__ resid) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fc = lane & 15, kr = lane >> 4;
    const int nb = D >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * FP_TILE + 32 * wave;
    if (m0 >= N) return;                                         // the whole wave; the kernel has no barrier
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const uint4 zero16 = {0u, 0u, 0u, 0u};

    const uint16_t* p[FP_RT];
    bool valid[FP_RT];
    float rn[FP_RT];
#pragma unroll
    for (int t = 0; t < FP_RT; ++t) {
        const int64_t m = m0 + 16 * t + fc;
        valid[t] = m < N;                                        // a row past the end is read as zeros and never written
        p[t] = rows + (valid[t] ? m : 0) * ld + 8 * kr;
        rn[t] = 1.f;
    }
    if constexpr (NORM) {
#pragma unroll
        for (int t = 0; t < FP_RT; ++t) {
            float ss = 0.f;
            if (valid[t])
                for (int c = 0; c < nb; ++c) ss = rows_ss8(__builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(p[t] + 32 * c)), ss);
            ss += __shfl_xor(ss, 16, 64);                        // (l0 + l1) and (l2 + l3), then their sum: the same bits in all four
            ss += __shfl_xor(ss, 32, 64);
            rn[t] = rows_rn(ss);
        }
    }
    const float* const qrow = comp + (int64_t)(fc < k ? fc : 0) * D + 8 * kr;
    const float* const mrow = mean + 8 * kr;

    f32x4 acc[FP_RT][2];
    float nn[FP_RT];
#pragma unroll
    for (int t = 0; t < FP_RT; ++t) {
        acc[t][0] = acc[t][1] = zero;
        nn[t] = 0.f;
    }
    for (int c2 = 0; c2 < nb; c2 += 2) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = c2 + i;                                // block c: c % 2 = i
            if (c < nb) {
                const f32x4 mu0 = *reinterpret_cast<const f32x4*>(mrow + 32 * c), mu1 = *reinterpret_cast<const f32x4*>(mrow + 32 * c + 4);
                const f32x4 q0 = fc < k ? *reinterpret_cast<const f32x4*>(qrow + 32 * c) : zero;
                const f32x4 q1 = fc < k ? *reinterpret_cast<const f32x4*>(qrow + 32 * c + 4) : zero;
#pragma unroll
                for (int t = 0; t < FP_RT; ++t) {
                    const f16x8 h = __builtin_bit_cast(f16x8, valid[t] ? *reinterpret_cast<const uint4*>(p[t] + 32 * c) : zero16);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float u = (float)h[e];
                        if constexpr (NORM) u = __fmul_rn(u, rn[t]);
                        const float cv = __fsub_rn(u, e < 4 ? mu0[e] : mu1[e - 4]);
                        nn[t] = fmaf(cv, cv, nn[t]);
                        acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(cv, e < 4 ? q0[e] : q1[e - 4], acc[t][i], 0, 0, 0);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < FP_RT; ++t) {
        float n2 = nn[t];
        n2 += __shfl_xor(n2, 16, 64);                            // |u - mu|^2 of row fc = (n0 + n1) + (n2 + n3), in all four lanes
        n2 += __shfl_xor(n2, 32, 64);
        // acc[t][.][e]: row 4 kr + e of the tile against component fc; that row's |u - mu|^2 sits in lane 4 kr + e
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float s = __fadd_rn(acc[t][0][e], acc[t][1][e]);
            const int64_t m = m0 + 16 * t + 4 * kr + e;
            const bool live = m < N;
            if (resid) {
                float q2 = 0.f;
#pragma unroll
                for (int j = 0; j < PCA_MAX_K; ++j) {
                    const float v = __shfl(s, 16 * kr + j, 64);
                    if (j < k) q2 = fmaf(v, v, q2);
                }
                const float nrow = __shfl(n2, 4 * kr + e, 64);
                if (live && fc == 0) resid[m] = fmaxf(0.f, __fsub_rn(nrow, q2));
            }
            if (live && fc < k) scores[m * k + fc] = scale ? __fmul_rn(s, scale[fc]) : s;
        }
    }
}

// byte offsets into the workspace, each a multiple of 16; the covariance comes first
struct FpLayout {
    int64_t nchunks, cpp, nparts;
    int64_t cov, z, tmp, rn, total;
};

int fp_shape(const char* what, int32_t dim, int64_t ld, int32_t k, int32_t normalize) {
    if (rows_width_ok(what, "dim", dim, PCA_MAX_D) != CBAS_OK) return CBAS_EINVAL;
    if (k < 1 || k > PCA_MAX_K || k > dim) return cbas_fail(CBAS_EINVAL, "%s: k = %d (1 .. %d components, at most dim)", what, k, PCA_MAX_K);
    if (rows_ld_ok(what, "ld", ld, "dim", dim) != CBAS_OK) return CBAS_EINVAL;
    if (normalize != 0 && normalize != 1) return cbas_fail(CBAS_EINVAL, "%s: normalize = %d (0 or 1)", what, normalize);
    return CBAS_OK;
}

int fp_layout(const char* what, int64_t N, int32_t dim, int32_t k, FpLayout* L) {
    if (N < 2 || N > FP_MAX_N) return cbas_fail(CBAS_EINVAL, "%s: n_rows = %lld (2 .. %lld)", what, (long long)N, (long long)FP_MAX_N);
    L->nchunks = (N + FP_CHUNK - 1) / FP_CHUNK;
    L->cpp = (L->nchunks + FP_MAX_PARTS - 1) / FP_MAX_PARTS;
    L->nparts = (L->nchunks + L->cpp - 1) / L->cpp;
    RowsTake take;
    L->cov = take(L->nparts * dim * dim * 4);
    L->z = take((int64_t)k * dim * 4);
    L->tmp = take(L->nchunks * dim * 4);
    L->rn = take(N * 4);
    L->total = take.at;
    return CBAS_OK;
}

}  // namespace

extern "C" int64_t cbas_rows_pca_workspace_bytes(int64_t n_rows, int32_t dim, int32_t k) {
    const char* const what = "cbas_rows_pca_workspace_bytes";
    FpLayout L;
    if (fp_shape(what, dim, dim, k, 0) != CBAS_OK || fp_layout(what, n_rows, dim, k, &L) != CBAS_OK) return CBAS_EINVAL;
    return L.total;
}

extern "C" int cbas_rows_pca_fit(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, int32_t k, int32_t iters,
                                 int32_t normalize, float* mean_dev, float* components_dev, float* eigenvalues_dev,
                                 float* total_variance_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    const char* const what = "cbas_rows_pca_fit";
    FpLayout L;
    if (fp_shape(what, dim, ld, k, normalize) != CBAS_OK || fp_layout(what, n_rows, dim, k, &L) != CBAS_OK) return CBAS_EINVAL;
    if (iters < 1) return cbas_fail(CBAS_EINVAL, "%s: iters = %d (at least 1)", what, iters);
    if (!rows_f16_dev || !mean_dev || !components_dev || !eigenvalues_dev || !total_variance_dev || !workspace_dev)
        return cbas_fail(CBAS_EINVAL, "%s: a NULL pointer", what);
    if (((uintptr_t)rows_f16_dev | (uintptr_t)mean_dev | (uintptr_t)components_dev | (uintptr_t)workspace_dev) % 16)
        return cbas_fail(CBAS_EINVAL, "%s: rows, mean, components and workspace must be 16-byte aligned", what);
    if (((uintptr_t)eigenvalues_dev | (uintptr_t)total_variance_dev) % 4)
        return cbas_fail(CBAS_EINVAL, "%s: eigenvalues and total_variance must be 4-byte aligned", what);
    if (workspace_bytes < L.total)
        return cbas_fail(CBAS_EINVAL, "%s: workspace of %lld bytes, %lld needed (cbas_rows_pca_workspace_bytes)", what,
                         (long long)workspace_bytes, (long long)L.total);
    if (cbas_use_device_of(rows_f16_dev) != CBAS_OK) return CBAS_EHIP;
    hipStream_t st = (hipStream_t)stream;
    const uint16_t* const rows = (const uint16_t*)rows_f16_dev;
    const int D = dim;
    char* const ws = (char*)workspace_dev;
    float* const cov = (float*)(ws + L.cov);
    float* const z = (float*)(ws + L.z);
    float* const tmp = (float*)(ws + L.tmp);
    float* const rn = normalize ? (float*)(ws + L.rn) : nullptr;

    if (normalize)
        hipLaunchKernelGGL(rows_rn_kernel, dim3((unsigned)((n_rows * 4 + 255) / 256)), dim3(256), 0, st, rows, n_rows, D, ld, rn);
    hipLaunchKernelGGL(fp_mean_stage1_kernel, dim3((D + 127) / 128, (unsigned)L.nchunks), dim3(64), 0, st, rows, n_rows, D, ld, (const float*)rn, tmp);
    hipLaunchKernelGGL(fp_mean_stage2_kernel, dim3((D + 63) / 64), dim3(64), 0, st, (const float*)tmp, D, L.nchunks, (float)n_rows, mean_dev);
    const int nt = (D + 127) / 128;
    hipLaunchKernelGGL(fp_cov_kernel, dim3(nt * (nt + 1) / 2, (unsigned)L.nparts), dim3(FP_THREADS), 0, st, rows, n_rows, D, ld, (const float*)rn,
                       (const float*)mean_dev, L.cpp, cov);
    hipLaunchKernelGGL(fp_cov_reduce_kernel, dim3((D + 255) / 256, D), dim3(256), 0, st, cov, D, (int)L.nparts, (float)(n_rows - 1));
    HIP_TRY(hipGetLastError());
    LAUNCH_TRY(launch_pca_eig(cov, (int64_t)D * D, 1, D, k, iters, z, components_dev, eigenvalues_dev, total_variance_dev, st));
    return CBAS_OK;
}

extern "C" int cbas_rows_pca_project(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, int32_t k, int32_t normalize,
                                     const float* mean_dev, const float* components_dev, const float* scale_dev, float* scores_dev,
                                     float* residual_dev, void* stream) {
    const char* const what = "cbas_rows_pca_project";
    if (n_rows < 0 || (n_rows + FP_TILE - 1) / FP_TILE > 0x7fffffff)
        return cbas_fail(CBAS_EINVAL, "%s: n_rows = %lld (0 .. %lld)", what, (long long)n_rows, (long long)0x7fffffff * FP_TILE);
    if (fp_shape(what, dim, ld, k, normalize) != CBAS_OK) return CBAS_EINVAL;
    if (n_rows == 0) return CBAS_OK;
    if (!rows_f16_dev || !mean_dev || !components_dev || !scores_dev)
        return cbas_fail(CBAS_EINVAL, "%s: a NULL pointer (only scale and residual may be NULL)", what);
    if (((uintptr_t)rows_f16_dev | (uintptr_t)mean_dev | (uintptr_t)components_dev) % 16)
        return cbas_fail(CBAS_EINVAL, "%s: rows, mean and components must be 16-byte aligned", what);
    if (((uintptr_t)scale_dev | (uintptr_t)scores_dev | (uintptr_t)residual_dev) % 4)
        return cbas_fail(CBAS_EINVAL, "%s: scale, scores and residual must be 4-byte aligned", what);
    if (cbas_use_device_of(rows_f16_dev) != CBAS_OK) return CBAS_EHIP;
    const dim3 grid((unsigned)((n_rows + FP_TILE - 1) / FP_TILE)), wg(FP_THREADS);
    const uint16_t* const rows = (const uint16_t*)rows_f16_dev;
    if (normalize)
        hipLaunchKernelGGL(fp_project_kernel<true>, grid, wg, 0, (hipStream_t)stream, rows, n_rows, dim, ld, k, mean_dev, components_dev, scale_dev,
                           scores_dev, residual_dev);
    else
        hipLaunchKernelGGL(fp_project_kernel<false>, grid, wg, 0, (hipStream_t)stream, rows, n_rows, dim, ld, k, mean_dev, components_dev, scale_dev,
                           scores_dev, residual_dev);
    HIP_TRY(hipGetLastError());
    return CBAS_OK;
}
