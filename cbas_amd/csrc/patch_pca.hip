// PCA of patch features on the device: column mean, centred covariance, a few leading eigenvectors, projection
// (DESIGN.md section 16).  The rows are what cbas_enc_forward_*_tokens writes: n frames of T fp32 rows of D floats (row stride
// ld), the first n_prefix rows of a frame skipped, P = T - n_prefix patch rows taking part.  A PROBLEM is one covariance:
//   FRAME scope   n problems, problem b = the M = P patch rows of frame b
//   BATCH scope   one problem, the M = n P patch rows of all frames
// both through one code path: row m of problem b is patch row m % P of frame b * frames_per_problem + m / P, and the problem is
// a grid dimension of every kernel.  Nothing here depends on how many problems a launch carries, so a frame's FRAME-scope
// result has the bits it has when fitted alone.
//
//   pca_mean_*       mu = (1 / M) sum_m x_m: thread per column, PCA_MEAN_CHUNK rows each in ascending order, then the chunks in
//                    ascending order (the two-stage shape of head_train_kernels.hip's colsum with a fixed chunk LENGTH)
//   pca_cov_kernel   partial[c] = sum over the rows of chunk c (PCA_CHUNK rows) of (x - mu)(x - mu)^T on v_mfma_f32_16x16x4_f32:
//                    a 128 x 128 tile of the upper triangle per workgroup, 64 x 64 per wave, the rows centred as they are
//                    staged into LDS (32 rows x 128 columns per operand, row stride 144 floats: the four k rows a ds_read_b32
//                    touches lie on different banks); rows past the chunk and columns past D are staged as 0
//   pca_cov_reduce   C[i][j] = C[j][i] = (partial[0][i][j] + partial[1][i][j] + ...) / (M - 1) for i <= j, written over chunk 0
//                    (no other thread reads what a thread writes): exactly symmetric, chunk order fixed
//   pca_cq_kernel    Z = C Q, one wave per row of C, k fmaf chains over the lane's columns, then the xor tree
//   pca_orth_kernel  Q = modified Gram-Schmidt, applied twice, of Z: one workgroup per problem
//   pca_ritz_kernel  B = Q^T (C Q), cyclic Jacobi on B, eigenvalues descending, Q rotated, sign rule, trace of C
//   pca_project      scores[m][j] = (x_m - mu) . q_j, one wave per row
// Every sum has a fixed order and there are no atomics: two calls give the same bits.
#include "kernels.h"

namespace {

constexpr int COV_LDS_LD = 144;                     // floats per staged row: 128 + 16 (bank spread of the four k rows)
constexpr int COV_SLAB = 32;                        // rows staged per step
constexpr int PCA_THREADS = 256, PCA_WAVES = PCA_THREADS / 64;
constexpr int PCA_PER_THREAD = PCA_MAX_D / PCA_THREADS;       // 6 column slots per thread in the one-workgroup kernels
constexpr int JACOBI_SWEEPS = 12;                   // k <= 8: converged to fp32 rounding in 5 - 6; the rest are no-ops

__device__ __forceinline__ const float* pca_row(const PcaRows& r, int prob, int64_t m) {
    const int64_t f = (int64_t)prob * r.frames_per_problem + m / r.P;
    return r.x + (f * r.T + r.n_prefix + (m % r.P)) * r.ld;
}

// ---- mean ----------------------------------------------------------------------------------------------------------------------
// grid (ceil(D / 64), mean chunks, problems), 64 threads
__global__ void pca_mean_stage1_kernel(PcaRows r, int D, int nmc, float* __restrict__ tmp) {
    const int c = blockIdx.x * 64 + threadIdx.x, ch = blockIdx.y, prob = blockIdx.z;
    if (c >= D) return;
    const int64_t m0 = (int64_t)ch * PCA_MEAN_CHUNK, m1 = m0 + PCA_MEAN_CHUNK < r.M ? m0 + PCA_MEAN_CHUNK : r.M;
    float s = 0.f;
    for (int64_t m = m0; m < m1; ++m) s += pca_row(r, prob, m)[c];
    tmp[((int64_t)prob * nmc + ch) * D + c] = s;
}
// grid (ceil(D / 64), problems), 64 threads
__global__ void pca_mean_stage2_kernel(const float* __restrict__ tmp, int D, int nmc, float rows, float* __restrict__ mean) {
    const int c = blockIdx.x * 64 + threadIdx.x, prob = blockIdx.y;
    if (c >= D) return;
    float s = 0.f;
    for (int ch = 0; ch < nmc; ++ch) s += tmp[((int64_t)prob * nmc + ch) * D + c];
    mean[(int64_t)prob * D + c] = s / rows;
}

// ---- covariance ------------------------------------------------------------------------------------------------------------------
// grid (tile pairs ti <= tj of the ceil(D / 128)^2 tiles, row chunks, problems), 256 threads
__global__ __launch_bounds__(PCA_THREADS) void pca_cov_kernel(PcaRows r, const float* __restrict__ mean, int D, int nchunks,
                                                              float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sa[COV_SLAB][COV_LDS_LD];
    __shared__ __attribute__((aligned(16))) float sb[COV_SLAB][COV_LDS_LD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int nt = (D + 127) / 128;
    int ti = 0, left = blockIdx.x;                   // pair index -> (ti, tj), ti <= tj, row by row of the upper triangle
    while (left >= nt - ti) { left -= nt - ti; ++ti; }
    const int tj = ti + left;
    const bool diag = ti == tj;
    const int chunk = blockIdx.y, prob = blockIdx.z;
    const int64_t m0 = (int64_t)chunk * PCA_CHUNK, m1 = m0 + PCA_CHUNK < r.M ? m0 + PCA_CHUNK : r.M;
    const int i0 = ti * 128, j0 = tj * 128;

    // staging: thread -> row (tid >> 5) + 8 q of the slab, columns 4 (tid & 31) .. + 3 of the tile (D % 4 == 0: all in or all out)
    const int sr = tid >> 5, c4 = (tid & 31) * 4;
    const bool a_in = i0 + c4 < D, b_in = !diag && j0 + c4 < D;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const float* const mu = mean + (int64_t)prob * D;
    const f32x4 mu_a = a_in ? *reinterpret_cast<const f32x4*>(mu + i0 + c4) : zero;
    const f32x4 mu_b = b_in ? *reinterpret_cast<const f32x4*>(mu + j0 + c4) : zero;
    f32x4 ra[4], rb[4];
    auto fetch = [&](int64_t ms) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t m = ms + sr + 8 * q;
            ra[q] = zero;
            rb[q] = zero;
            if (m < m1) {
                const float* const p = pca_row(r, prob, m);
                if (a_in) ra[q] = *reinterpret_cast<const f32x4*>(p + i0 + c4) - mu_a;
                if (b_in) rb[q] = *reinterpret_cast<const f32x4*>(p + j0 + c4) - mu_b;
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
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = zero;

    const float (*const B)[COV_LDS_LD] = diag ? sa : sb;
    const int kr = lane >> 4, fc = lane & 15;
    fetch(m0);
    put();
    __syncthreads();
    for (int64_t ms = m0; ms < m1; ms += COV_SLAB) {
        const bool more = ms + COV_SLAB < m1;
        if (more) fetch(ms + COV_SLAB);
        if (live) {
#pragma unroll
            for (int kk = 0; kk < COV_SLAB / 4; ++kk) {          // rows ms + 4 kk + (0 .. 3): ascending, one fmaf chain per element
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
    float* const out = part + ((int64_t)prob * nchunks + chunk) * D * D;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int gi = i0 + wr * 64 + i * 16 + kr * 4 + e;   // C/D map: row 4 (lane >> 4) + e, column lane & 15
            if (gi >= D) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gj = j0 + wc * 64 + j * 16 + fc;
                if (gj < D) out[(int64_t)gi * D + gj] = acc[i][j][e];
            }
        }
}

// grid (ceil(D / 256), D, problems), 256 threads: element (i = blockIdx.y, j) with i <= j
__global__ void pca_cov_reduce_kernel(float* __restrict__ part, int D, int nchunks, float dof) {
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= D || j < i) return;
    float* const C = part + (int64_t)blockIdx.z * nchunks * D * D;
    float s = C[(int64_t)i * D + j];
    for (int c = 1; c < nchunks; ++c) s += C[((int64_t)c * D + i) * D + j];
    s = s / dof;
    C[(int64_t)i * D + j] = s;
    C[(int64_t)j * D + i] = s;
}

// ---- subspace iteration --------------------------------------------------------------------------------------------------------
// the fixed start pattern: a 32-bit integer hash of (d, j) mapped to [-1, 1) - no RNG state, nothing read from the data
__device__ __forceinline__ float pca_start(int d, int j) {
    unsigned u = (unsigned)(d + 1) * 2654435761u ^ (unsigned)(j + 1) * 2246822519u;
    u ^= u >> 15;
    u *= 2246822519u;
    u ^= u >> 13;
    return (float)(u >> 8) * (1.0f / 8388608.0f) - 1.0f;          // 24 bits x 2^-23: exact
}
// grid (ceil(k D / 256), problems)
__global__ void pca_start_kernel(float* __restrict__ Z, int D, int k) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= k * D) return;
    Z[(int64_t)blockIdx.y * k * D + idx] = pca_start(idx % D, idx / D);
}

// Z[j][d] = sum_e C[d][e] Q[j][e].  grid (D / 4, problems), 256 threads: one wave per row d
__global__ __launch_bounds__(PCA_THREADS) void pca_cq_kernel(const float* __restrict__ C, int64_t c_stride, const float* __restrict__ Q,
                                                             float* __restrict__ Z, int D, int k) {
    const int lane = threadIdx.x & 63, prob = blockIdx.y;
    const int d = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (d >= D) return;
    const float* const crow = C + prob * c_stride + (int64_t)d * D;
    const float* const q = Q + (int64_t)prob * k * D;
    float acc[PCA_MAX_K];
#pragma unroll
    for (int j = 0; j < PCA_MAX_K; ++j) acc[j] = 0.f;
    for (int idx = lane; idx < (D >> 2); idx += 64) {
        const f32x4 c = reinterpret_cast<const f32x4*>(crow)[idx];
#pragma unroll
        for (int j = 0; j < PCA_MAX_K; ++j)
            if (j < k) {
                const f32x4 v = reinterpret_cast<const f32x4*>(q + (int64_t)j * D)[idx];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j] = fmaf(c[e], v[e], acc[j]);
            }
    }
#pragma unroll
    for (int j = 0; j < PCA_MAX_K; ++j)
        if (j < k) {
            const float s = wave_sum(acc[j]);
            if (lane == 0) Z[((int64_t)prob * k + j) * D + d] = s;
        }
}

// sum over the workgroup, every thread gets it: the wave's xor tree, then the four wave results in ascending order
__device__ __forceinline__ float pca_block_sum(float v, float* red, int tid) {
    v = wave_sum(v);
    __syncthreads();                                   // the previous use of red is over
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// a column of D floats held by the workgroup: thread t owns d = t, t + 256, ... (slot s: d = t + 256 s)
struct PcaCol {
    float v[PCA_PER_THREAD];
};
__device__ __forceinline__ float pca_dot(const PcaCol& a, const PcaCol& b, int D, float* red, int tid) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < PCA_PER_THREAD; ++t)
        if (tid + PCA_THREADS * t < D) s = fmaf(a.v[t], b.v[t], s);
    return pca_block_sum(s, red, tid);
}
template <int K>
__device__ __forceinline__ void pca_load(PcaCol (&q)[K], const float* __restrict__ src, int D, int k, int tid) {
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int t = 0; t < PCA_PER_THREAD; ++t) {
            const int d = tid + PCA_THREADS * t;
            q[j].v[t] = (j < k && d < D) ? src[(int64_t)j * D + d] : 0.f;
        }
}

// Q = MGS(MGS(Z)).  grid (problems), 256 threads.  K: the compiled column count (k <= K), so the columns stay in registers
template <int K>
__global__ __launch_bounds__(PCA_THREADS) void pca_orth_kernel(const float* __restrict__ Z, float* __restrict__ Q, int D, int k) {
    __shared__ float red[PCA_WAVES];
    const int tid = threadIdx.x, prob = blockIdx.x;
    PcaCol q[K];
    pca_load<K>(q, Z + (int64_t)prob * k * D, D, k, tid);
    for (int rep = 0; rep < 2; ++rep) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (j >= k) break;
#pragma unroll
            for (int i = 0; i < j; ++i) {
                const float p = pca_dot(q[i], q[j], D, red, tid);
#pragma unroll
                for (int t = 0; t < PCA_PER_THREAD; ++t) q[j].v[t] = fmaf(-p, q[i].v[t], q[j].v[t]);
            }
            const float nrm = sqrtf(pca_dot(q[j], q[j], D, red, tid));
#pragma unroll
            for (int t = 0; t < PCA_PER_THREAD; ++t) q[j].v[t] = nrm > 0.f ? q[j].v[t] / nrm : 0.f;      // a null column stays null
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int t = 0; t < PCA_PER_THREAD; ++t) {
            const int d = tid + PCA_THREADS * t;
            if (j < k && d < D) Q[((int64_t)prob * k + j) * D + d] = q[j].v[t];
        }
}

// Rayleigh-Ritz.  Q (orthonormal, in `comp`) and Z = C Q in; components, eigenvalues and the trace of C out.
// grid (problems), 256 threads
template <int K>
__global__ __launch_bounds__(PCA_THREADS) void pca_ritz_kernel(const float* __restrict__ C, int64_t c_stride, const float* __restrict__ Z,
                                                               float* __restrict__ comp, float* __restrict__ eig,
                                                               float* __restrict__ total_var, int D, int k) {
    __shared__ float red[PCA_WAVES];
    __shared__ float Bm[PCA_MAX_K][PCA_MAX_K], Vm[PCA_MAX_K][PCA_MAX_K];
    __shared__ int perm[PCA_MAX_K];
    __shared__ float best_v[PCA_WAVES];
    __shared__ int best_d[PCA_WAVES];
    __shared__ float sign;
    const int tid = threadIdx.x, prob = blockIdx.x;
    PcaCol q[K], z[K];
    pca_load<K>(q, comp + (int64_t)prob * k * D, D, k, tid);
    pca_load<K>(z, Z + (int64_t)prob * k * D, D, k, tid);

    // trace of C: thread t adds its diagonal entries in ascending order
    float tr = 0.f;
    for (int d = tid; d < D; d += PCA_THREADS) tr += C[prob * c_stride + (int64_t)d * D + d];
    tr = pca_block_sum(tr, red, tid);

    // B = Q^T Z: the upper triangle, mirrored
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = i; j < K; ++j) {
            if (j >= k) break;
            const float b = pca_dot(q[i], z[j], D, red, tid);
            if (tid == 0) Bm[i][j] = Bm[j][i] = b;
        }
    __syncthreads();
    if (tid == 0) {
        // cyclic Jacobi: V^T B V -> diagonal.  k <= 8: one lane's work
        for (int i = 0; i < k; ++i)
            for (int j = 0; j < k; ++j) Vm[i][j] = i == j ? 1.f : 0.f;
        for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep)
            for (int p = 0; p < k - 1; ++p)
                for (int s = p + 1; s < k; ++s) {
                    const float apq = Bm[p][s];
                    if (apq == 0.f) continue;
                    const float theta = (Bm[s][s] - Bm[p][p]) / (2.f * apq);
                    const float t = (theta >= 0.f ? 1.f : -1.f) / (fabsf(theta) + sqrtf(fmaf(theta, theta, 1.f)));
                    const float c = 1.f / sqrtf(fmaf(t, t, 1.f)), sn = t * c;
                    for (int i = 0; i < k; ++i) {             // columns p, s
                        const float bp = Bm[i][p], bs = Bm[i][s];
                        Bm[i][p] = c * bp - sn * bs;
                        Bm[i][s] = sn * bp + c * bs;
                    }
                    for (int i = 0; i < k; ++i) {             // rows p, s
                        const float bp = Bm[p][i], bs = Bm[s][i];
                        Bm[p][i] = c * bp - sn * bs;
                        Bm[s][i] = sn * bp + c * bs;
                    }
                    Bm[p][s] = Bm[s][p] = 0.f;
                    for (int i = 0; i < k; ++i) {
                        const float vp = Vm[i][p], vs = Vm[i][s];
                        Vm[i][p] = c * vp - sn * vs;
                        Vm[i][s] = sn * vp + c * vs;
                    }
                }
        // descending eigenvalues; equal ones keep their order
        for (int j = 0; j < k; ++j) perm[j] = j;
        for (int j = 1; j < k; ++j) {
            const int pj = perm[j];
            int i = j - 1;
            while (i >= 0 && Bm[perm[i]][perm[i]] < Bm[pj][pj]) { perm[i + 1] = perm[i]; --i; }
            perm[i + 1] = pj;
        }
        for (int j = 0; j < k; ++j) eig[(int64_t)prob * k + j] = Bm[perm[j]][perm[j]];
        total_var[prob] = tr;
    }
    __syncthreads();

    // component j = sum_i Q_i V[i][perm j] (i ascending), then the sign rule: its entry of largest magnitude is positive, ties to
    // the lowest index
    for (int j = 0; j < k; ++j) {
        const int pj = perm[j];
        float out[PCA_PER_THREAD];
        float bv = -1.f;
        int bd = 0x7fffffff;
#pragma unroll
        for (int t = 0; t < PCA_PER_THREAD; ++t) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < K; ++i)
                if (i < k) s = fmaf(q[i].v[t], Vm[i][pj], s);
            out[t] = s;
            const int d = tid + PCA_THREADS * t;
            if (d < D && fabsf(s) > bv) { bv = fabsf(s); bd = d; }          // ascending d: the first of equal magnitudes is kept
        }
        // argmax over the wave, then over the four waves: larger magnitude wins, equal magnitudes go to the lower index
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int od = __shfl_xor(bd, o, 64);
            if (ov > bv || (ov == bv && od < bd)) { bv = ov; bd = od; }
        }
        __syncthreads();
        if ((tid & 63) == 0) { best_v[tid >> 6] = bv; best_d[tid >> 6] = bd; }
        __syncthreads();
        bv = best_v[0];
        bd = best_d[0];
        for (int w = 1; w < PCA_WAVES; ++w)
            if (best_v[w] > bv || (best_v[w] == bv && best_d[w] < bd)) { bv = best_v[w]; bd = best_d[w]; }
        // the owner of entry bd publishes its sign
        __syncthreads();
        if (bd < D && (bd & (PCA_THREADS - 1)) == tid) {
            float val = 0.f;
#pragma unroll
            for (int t = 0; t < PCA_PER_THREAD; ++t)
                if (tid + PCA_THREADS * t == bd) val = out[t];
            sign = val < 0.f ? -1.f : 1.f;
        }
        __syncthreads();
        const float sg = sign;
#pragma unroll
        for (int t = 0; t < PCA_PER_THREAD; ++t) {
            const int d = tid + PCA_THREADS * t;
            if (d < D) comp[((int64_t)prob * k + j) * D + d] = sg * out[t];
        }
    }
}

// ---- projection ------------------------------------------------------------------------------------------------------------------
// grid (ceil(P / 4), n), 256 threads: one wave per patch row; basis b of frame f is f * basis_step (0: one basis for all)
__global__ __launch_bounds__(PCA_THREADS) void pca_project_kernel(const float* __restrict__ x, int64_t ld, int T, int n_prefix, int D, int k,
                                                                  int basis_step, const float* __restrict__ mean,
                                                                  const float* __restrict__ comp, float* __restrict__ scores) {
    const int lane = threadIdx.x & 63, f = blockIdx.y, P = T - n_prefix;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    const int64_t b = (int64_t)f * basis_step;
    const float* const row = x + ((int64_t)f * T + n_prefix + p) * ld;
    const float* const mu = mean + b * D;
    const float* const q = comp + b * k * D;
    float acc[PCA_MAX_K];
#pragma unroll
    for (int j = 0; j < PCA_MAX_K; ++j) acc[j] = 0.f;
    for (int idx = lane; idx < (D >> 2); idx += 64) {
        const f32x4 c = reinterpret_cast<const f32x4*>(row)[idx] - reinterpret_cast<const f32x4*>(mu)[idx];
#pragma unroll
        for (int j = 0; j < PCA_MAX_K; ++j)
            if (j < k) {
                const f32x4 v = reinterpret_cast<const f32x4*>(q + (int64_t)j * D)[idx];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j] = fmaf(c[e], v[e], acc[j]);
            }
    }
#pragma unroll
    for (int j = 0; j < PCA_MAX_K; ++j)
        if (j < k) {
            const float s = wave_sum(acc[j]);
            if (lane == 0) scores[((int64_t)f * P + p) * k + j] = s;
        }
}

bool pca_shape_ok(const PcaRows& r, int nprob, int D) {
    return r.x && (uintptr_t)r.x % 16 == 0 && r.ld >= D && r.ld % 4 == 0 && D > 0 && D % 32 == 0 && D <= PCA_MAX_D && r.P >= 1 &&
           r.n_prefix >= 0 && r.T == r.n_prefix + r.P && r.M >= 2 && r.frames_per_problem >= 1 && nprob >= 1 && nprob <= 65535;
}

}  // namespace

int64_t pca_cov_chunks(int64_t M) { return (M + PCA_CHUNK - 1) / PCA_CHUNK; }
int64_t pca_mean_chunks(int64_t M) { return (M + PCA_MEAN_CHUNK - 1) / PCA_MEAN_CHUNK; }

int launch_pca_mean(const PcaRows& r, int nprob, int D, float* tmp, float* mean, hipStream_t st) {
    const int64_t nmc = pca_mean_chunks(r.M);
    if (!pca_shape_ok(r, nprob, D) || !tmp || !mean || nmc > 65535) return -1;
    hipLaunchKernelGGL(pca_mean_stage1_kernel, dim3((D + 63) / 64, (unsigned)nmc, (unsigned)nprob), dim3(64), 0, st, r, D, (int)nmc, tmp);
    hipLaunchKernelGGL(pca_mean_stage2_kernel, dim3((D + 63) / 64, (unsigned)nprob), dim3(64), 0, st, tmp, D, (int)nmc, (float)r.M, mean);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_pca_cov(const PcaRows& r, int nprob, int D, const float* mean, float* part, hipStream_t st) {
    const int64_t nch = pca_cov_chunks(r.M);
    if (!pca_shape_ok(r, nprob, D) || !mean || !part || (uintptr_t)mean % 16 || (uintptr_t)part % 16 || nch > 65535) return -1;
    const int nt = (D + 127) / 128;
    hipLaunchKernelGGL(pca_cov_kernel, dim3(nt * (nt + 1) / 2, (unsigned)nch, (unsigned)nprob), dim3(PCA_THREADS), 0, st, r, mean, D,
                       (int)nch, part);
    hipLaunchKernelGGL(pca_cov_reduce_kernel, dim3((D + 255) / 256, D, (unsigned)nprob), dim3(256), 0, st, part, D, (int)nch,
                       (float)(r.M - 1));
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

#define PCA_K_SWITCH(k, KERNEL, ...)                                                   \
    if ((k) <= 2) hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__);                          \
    else if ((k) <= 4) hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__);                     \
    else hipLaunchKernelGGL(KERNEL<8>, __VA_ARGS__);

int launch_pca_eig(const float* C, int64_t c_stride, int nprob, int D, int k, int iters, float* Z, float* comp, float* eig,
                   float* total_var, hipStream_t st) {
    if (!C || !Z || !comp || !eig || !total_var || ((uintptr_t)C | (uintptr_t)Z | (uintptr_t)comp) % 16 || c_stride % 4 || nprob < 1 ||
        nprob > 65535 || D <= 0 || D % 32 || D > PCA_MAX_D || k < 1 || k > PCA_MAX_K || k > D || iters < 1)
        return -1;
    const dim3 cq_grid(D / 4, (unsigned)nprob), one(nprob), wg(PCA_THREADS);
    hipLaunchKernelGGL(pca_start_kernel, dim3((k * D + 255) / 256, (unsigned)nprob), dim3(256), 0, st, Z, D, k);
    PCA_K_SWITCH(k, pca_orth_kernel, one, wg, 0, st, Z, comp, D, k);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(pca_cq_kernel, cq_grid, wg, 0, st, C, c_stride, comp, Z, D, k);
        PCA_K_SWITCH(k, pca_orth_kernel, one, wg, 0, st, Z, comp, D, k);
    }
    hipLaunchKernelGGL(pca_cq_kernel, cq_grid, wg, 0, st, C, c_stride, comp, Z, D, k);
    PCA_K_SWITCH(k, pca_ritz_kernel, one, wg, 0, st, C, c_stride, Z, comp, eig, total_var, D, k);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_pca_project(const float* x, int64_t ld, int n, int T, int n_prefix, int D, int k, int basis_step, const float* mean,
                       const float* comp, float* scores, hipStream_t st) {
    if (!x || !mean || !comp || !scores || ((uintptr_t)x | (uintptr_t)mean | (uintptr_t)comp) % 16 || ld < D || ld % 4 || n < 1 ||
        n > 65535 || n_prefix < 0 || T <= n_prefix || D <= 0 || D % 32 || D > PCA_MAX_D || k < 1 || k > PCA_MAX_K ||
        (basis_step != 0 && basis_step != 1))
        return -1;
    hipLaunchKernelGGL(pca_project_kernel, dim3((unsigned)((T - n_prefix + 3) / 4), (unsigned)n), dim3(PCA_THREADS), 0, st, x, ld, T,
                       n_prefix, D, k, basis_step, mean, comp, scores);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
