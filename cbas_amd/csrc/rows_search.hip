// Cosine search over resident CLS rows: cbas_rows_search_workspace_bytes / cbas_rows_search of
// include/cbas_mi355x.h, kernels and entry points in one file.  rows (N, D) fp16 with row stride ld, queries (Q, D) fp32.
//
//   rs_qnorm_kernel      rq of every query: one wave per query, lane l the fp64 fma chain over d = l, l + 64, ..., then the xor tree
//                        32, 16, .., 1; rq = fp32(1 / sqrt(s)), 0 for a zero query
//   rs_score_kernel      THE PASS.  The (at most 16) queries of a group resident in LDS, zero rows past the last; one wave per tile of
//                        16 rows, the whole width: lane (fc, kr) reads the 8 halves d = 32 c + 8 kr .. + 7 of row fc of the tile for
//                        c = 0 .. D / 32 - 1 (16 bytes a load, RS_DEPTH loads in flight) and widens them (exact);
//                        v_mfma_f32_16x16x4_f32 number (c, e) multiplies the columns 32 c + 8 kr + e, kr = 0 .. 3, of the 16 rows
//                        with those of the 16 queries (exact products) and adds them in ascending kr.
//                        THE ORDER OF THE SUMS, a function of D alone:
//                          dot(x, q) = chain0 + chain1; chain p = the fp32 fmaf chain, from 0, over the columns d with (d / 32) % 2 = p,
//                                      ordered by (d / 32, d % 8, (d % 32) / 8) ascending
//                          s = (l0 + l1) + (l2 + l3); l_kr = the fp32 fmaf chain, from 0, of x_d^2 over the columns d with
//                                      (d % 32) / 8 = kr, ascending in d
//                        rn = fp32(1 / sqrt((double)s)), 0 when s = 0; trace[q][m] = fl(fl(dot * rn) * rq).  A tile belongs to one wave
//                        from its first column to its last, so neither the grid, nor N, nor the query's slot enters any sum.
//   rs_clip_fill_kernel  the clip of every row (-1 outside every clip) from the clip table; an entry outside the rows is flagged and
//   rs_clip_check_kernel skipped, and a row that two entries claim holds one of them, which the other finds: overlap flagged
//   rs_peaks_kernel      one workgroup per chunk of RS_CHUNK rows and query: the peaks among the candidates (in a clip, not masked,
//                        over the threshold), compacted in ascending row order, and the chunk's k best of them
//   rs_merge_kernel      RS_FAN lists into one, until one is left: the result
// The k best of a workgroup's entries are placed by RANK: an entry's position is the number of entries that beat it (a larger
// score, or an equal score and a lower row); rows are distinct, so the ranks are too.  No atomics anywhere.
#include "kernels.h"
#include "rows_api.h"
#include "rows_rn.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_QPAD = 4;                           // LDS query rows are D + 4 floats apart
constexpr int RS_DEPTH = 4;                          // 32-column blocks a lane has in flight beside the ones it multiplies (even)
constexpr int RS_CHUNK = 1024;                       // rows per first-stage list: fixed, whatever N and the device
constexpr int RS_FAN = 16;                           // lists per merge: RS_FAN * 64 entries fill the workgroup's 1024 slots
constexpr int RS_MAX_Q = 64, RS_MAX_K = 64, RS_MAX_GAP = 65535, RS_MAX_D = 1536;
constexpr unsigned RS_FLAG_TABLE = 1u, RS_FLAG_OVERLAP = 2u;

// grid (ceil(Q / 4)), 256 threads: one wave per query
__global__ __launch_bounds__(RS_THREADS) void rs_qnorm_kernel(const float* __restrict__ queries, int D, int Q, float* __restrict__ rq) {
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    const float* const p = queries + (int64_t)q * D;
    double ss = 0.0;
    for (int d = lane; d < D; d += 64) ss = fma((double)p[d], (double)p[d], ss);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if (lane == 0) rq[q] = ss > 0.0 ? (float)(1.0 / sqrt(ss)) : 0.f;
}

// grid (workgroups, query groups), 256 threads, LDS 16 (D + 4) floats; wave g of the grid's takes the tiles g, g + waves, ...
__global__ __launch_bounds__(RS_THREADS) void rs_score_kernel(const uint16_t* __restrict__ rows, int64_t N, int D, int64_t ld,
                                                              const float* __restrict__ queries, int Q, const float* __restrict__ rq,
                                                              float* __restrict__ trace) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const int qld = D + RS_QPAD;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fc = lane & 15, kr = lane >> 4;
    const int q0 = blockIdx.y * 16, nq = Q - q0 < 16 ? Q - q0 : 16;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const uint4 zero16 = {0u, 0u, 0u, 0u};

    for (int idx = tid; idx < 16 * (D >> 2); idx += RS_THREADS) {
        const int j = idx / (D >> 2), c = idx - j * (D >> 2);
        *reinterpret_cast<f32x4*>(rs_lds + j * qld + 4 * c) =
            j < nq ? *reinterpret_cast<const f32x4*>(queries + (int64_t)(q0 + j) * D + 4 * c) : zero;
    }
    __syncthreads();
    const float my_rq = fc < nq ? rq[q0 + fc] : 0.f;
    const float* const qb = rs_lds + fc * qld + 8 * kr;          // lane (fc, kr): query fc, columns 32 c + 8 kr .. + 7
    const int nb = D >> 5;
    const int64_t ntiles = (N + 15) >> 4, nwaves = (int64_t)gridDim.x * 4;

    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < ntiles; t += nwaves) {
        const int64_t m = t * 16 + fc;
        const bool valid = m < N;                                // a row past the end is read as zeros and never written
        const uint16_t* const p = rows + (valid ? m : 0) * ld + 8 * kr;
        uint4 buf[RS_DEPTH], nx[RS_DEPTH];
#pragma unroll
        for (int i = 0; i < RS_DEPTH; ++i) buf[i] = (valid && i < nb) ? *reinterpret_cast<const uint4*>(p + 32 * i) : zero16;
        f32x4 acc0 = zero, acc1 = zero;
        float ss = 0.f;
        for (int c0 = 0; c0 < nb; c0 += RS_DEPTH) {
#pragma unroll
            for (int i = 0; i < RS_DEPTH; ++i) {
                const int c = c0 + RS_DEPTH + i;
                nx[i] = (valid && c < nb) ? *reinterpret_cast<const uint4*>(p + 32 * c) : zero16;
            }
#pragma unroll
            for (int i = 0; i < RS_DEPTH; ++i) {
                const int c = c0 + i;
                if (c < nb) {
                    const f32x4 qa = *reinterpret_cast<const f32x4*>(qb + 32 * c);
                    const f32x4 qv = *reinterpret_cast<const f32x4*>(qb + 32 * c + 4);
                    const f16x8 h = __builtin_bit_cast(f16x8, buf[i]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float x = (float)h[e];
                        const float qe = e < 4 ? qa[e] : qv[e - 4];
                        ss = fmaf(x, x, ss);
                        if (i & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x, qe, acc1, 0, 0, 0);       // c0 is even: c % 2 = i % 2
                        else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x, qe, acc0, 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < RS_DEPTH; ++i) buf[i] = nx[i];
        }
        ss += __shfl_xor(ss, 16, 64);                            // (l0 + l1) and (l2 + l3), then their sum: the same bits in all four
        ss += __shfl_xor(ss, 32, 64);
        const float rn = rows_rn(ss);
        // acc[e]: row 4 kr + e of the tile against query fc; that row's rn sits in lane 4 kr + e
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float rn_row = __shfl(rn, 4 * kr + e, 64);
            const float dot = acc0[e] + acc1[e];
            const int64_t mr = t * 16 + 4 * kr + e;
            if (mr < N && fc < nq) trace[(int64_t)(q0 + fc) * N + mr] = __fmul_rn(__fmul_rn(dot, rn_row), my_rq);
        }
    }
}

__device__ __forceinline__ bool rs_entry_ok(int64_t first, int64_t rows, int64_t N) {
    return first >= 0 && rows >= 0 && first <= N && rows <= N - first;
}
// grid (n_clips, slices), 256 threads; clip_id is -1 everywhere before the fill
__global__ __launch_bounds__(RS_THREADS) void rs_clip_fill_kernel(const int64_t* __restrict__ table, int64_t N, int32_t* __restrict__ clip_id,
                                                                  unsigned* __restrict__ flags) {
    const int c = blockIdx.x;
    const int64_t first = table[2 * (int64_t)c], rows = table[2 * (int64_t)c + 1];
    if (!rs_entry_ok(first, rows, N)) {
        if (threadIdx.x == 0 && blockIdx.y == 0) flags[0] = RS_FLAG_TABLE;
        return;
    }
    for (int64_t i = (int64_t)blockIdx.y * RS_THREADS + threadIdx.x; i < rows; i += (int64_t)gridDim.y * RS_THREADS) clip_id[first + i] = c;
}
__global__ __launch_bounds__(RS_THREADS) void rs_clip_check_kernel(const int64_t* __restrict__ table, int64_t N,
                                                                   const int32_t* __restrict__ clip_id, unsigned* __restrict__ flags) {
    const int c = blockIdx.x;
    const int64_t first = table[2 * (int64_t)c], rows = table[2 * (int64_t)c + 1];
    if (!rs_entry_ok(first, rows, N)) return;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.y * RS_THREADS + threadIdx.x; i < rows; i += (int64_t)gridDim.y * RS_THREADS) bad |= clip_id[first + i] != c;
    if (bad) flags[1] = RS_FLAG_OVERLAP;
}

// The workgroup's entries (thread t holds those numbered j * 256 + t, j = 0 .. 3) in ascending number at the front of cs / ci;
// returns how many.  wc: 16 ints of LDS.
__device__ __forceinline__ int rs_compact(const bool (&keep)[4], const float (&s)[4], const int64_t (&x)[4], float* cs, int64_t* ci, int* wc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int before[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned long long b = __ballot(keep[j]);
        before[j] = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wc[j * 4 + wave] = __popcll(b);
    }
    __syncthreads();
    int total = 0, at[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if ((i & 3) == wave) at[i >> 2] = total;                 // the entries of (j, wave) follow those of every (j', wave') before it
        total += wc[i];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (keep[j]) {
            cs[at[j] + before[j]] = s[j];
            ci[at[j] + before[j]] = x[j];
        }
    __syncthreads();
    return total;
}

// out[r] = the entry of rank r < k among the C of cs / ci; (-inf, -1) past the last
__device__ __forceinline__ void rs_place(const float* cs, const int64_t* ci, int C, int k, float* __restrict__ out_s, int64_t* __restrict__ out_i) {
    for (int i = threadIdx.x; i < C; i += RS_THREADS) {
        const float s = cs[i];
        const int64_t x = ci[i];
        int rank = 0;
        for (int j = 0; j < C; ++j) {
            const float sj = cs[j];
            rank += (sj > s || (sj == s && ci[j] < x)) ? 1 : 0;
        }
        if (rank < k) {
            out_s[rank] = s;
            out_i[rank] = x;
        }
    }
    for (int i = (C < k ? C : k) + threadIdx.x; i < k; i += RS_THREADS) {
        out_s[i] = -__builtin_inff();
        out_i[i] = -1;
    }
}

struct RsSelect {
    const float* trace;
    int64_t N;
    const int64_t* table;
    const int32_t* clip_id;
    const uint8_t* mask;
    int gap, use_threshold;
    float threshold;
    int k;
};

// grid (chunks, Q), 256 threads: list (q, chunk) = k entries at (q * chunks + chunk) * k
__global__ __launch_bounds__(RS_THREADS) void rs_peaks_kernel(RsSelect p, float* __restrict__ list_s, int64_t* __restrict__ list_i) {
    __shared__ float cs[RS_CHUNK];
    __shared__ int64_t ci[RS_CHUNK];
    __shared__ int wc[16];
    const int q = blockIdx.y;
    const int64_t chunk = blockIdx.x, m0 = chunk * RS_CHUNK;
    const float* const tr = p.trace + (int64_t)q * p.N;
    bool keep[4];
    float s[4];
    int64_t x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t m = m0 + j * RS_THREADS + threadIdx.x;
        keep[j] = false;
        s[j] = 0.f;
        x[j] = m;
        if (m >= p.N) continue;
        const int c = p.clip_id[m];
        if (c < 0 || (p.mask && p.mask[m] == 0)) continue;
        const float v = tr[m];
        if (p.use_threshold && !(v >= p.threshold)) continue;
        const int64_t lo = p.table[2 * (int64_t)c], hi = lo + p.table[2 * (int64_t)c + 1] - 1;     // checked before this launch
        const int64_t a = m - p.gap > lo ? m - p.gap : lo, b = m + p.gap < hi ? m + p.gap : hi;
        bool peak = true;
        for (int64_t d = 1; peak && (m - d >= a || m + d <= b); ++d) {                            // the nearest first: most rows lose early
            if (m - d >= a && !(tr[m - d] < v)) peak = false;                                     // an equal score at a lower row wins
            if (m + d <= b && tr[m + d] > v) peak = false;
        }
        keep[j] = peak;
        s[j] = v;
    }
    const int C = rs_compact(keep, s, x, cs, ci, wc);
    const int64_t at = ((int64_t)q * gridDim.x + chunk) * p.k;
    rs_place(cs, ci, C, p.k, list_s + at, list_i + at);
}

// grid (ceil(n_in / RS_FAN), Q), 256 threads: lists g RS_FAN .. of the n_in of a query into list g of the output
__global__ __launch_bounds__(RS_THREADS) void rs_merge_kernel(const float* __restrict__ in_s, const int64_t* __restrict__ in_i, int64_t n_in, int k,
                                                              float* __restrict__ out_s, int64_t* __restrict__ out_i) {
    __shared__ float cs[RS_FAN * RS_MAX_K];
    __shared__ int64_t ci[RS_FAN * RS_MAX_K];
    __shared__ int wc[16];
    const int q = blockIdx.y;
    const int64_t g = blockIdx.x, l0 = g * RS_FAN;
    const int nl = (int)(n_in - l0 < RS_FAN ? n_in - l0 : RS_FAN);
    const int64_t base = ((int64_t)q * n_in + l0) * k;
    bool keep[4];
    float s[4];
    int64_t x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = j * RS_THREADS + threadIdx.x;
        keep[j] = false;
        s[j] = 0.f;
        x[j] = -1;
        if (e < nl * k) {
            s[j] = in_s[base + e];
            x[j] = in_i[base + e];
            keep[j] = x[j] >= 0;
        }
    }
    const int C = rs_compact(keep, s, x, cs, ci, wc);
    const int64_t at = ((int64_t)q * gridDim.x + g) * k;
    rs_place(cs, ci, C, k, out_s + at, out_i + at);
}

// byte offsets into the workspace, each a multiple of 16
struct RsLayout {
    int64_t nch, nch2;
    int64_t rq, flags, clip_id, a_s, a_i, b_s, b_i, total;
};

// 0, or CBAS_EINVAL with the message set
int rs_layout(const char* what, int64_t n_rows, int32_t n_queries, int32_t k, RsLayout* L) {
    if (n_rows < 1) return cbas_fail(CBAS_EINVAL, "%s: n_rows = %lld (at least 1)", what, (long long)n_rows);
    if (n_queries < 1 || n_queries > RS_MAX_Q) return cbas_fail(CBAS_EINVAL, "%s: n_queries = %d (1 .. %d)", what, n_queries, RS_MAX_Q);
    if (k < 1 || k > RS_MAX_K) return cbas_fail(CBAS_EINVAL, "%s: k = %d (1 .. %d)", what, k, RS_MAX_K);
    L->nch = (n_rows + RS_CHUNK - 1) / RS_CHUNK;
    if (L->nch > 0x7fffffff) return cbas_fail(CBAS_EINVAL, "%s: n_rows = %lld is more than one call takes", what, (long long)n_rows);
    L->nch2 = (L->nch + RS_FAN - 1) / RS_FAN;
    RowsTake take;
    L->rq = take(RS_MAX_Q * 4);
    L->flags = take(16);
    L->clip_id = take(n_rows * 4);
    L->a_s = take(L->nch * n_queries * k * 4);
    L->a_i = take(L->nch * n_queries * k * 8);
    L->b_s = take(L->nch2 * n_queries * k * 4);
    L->b_i = take(L->nch2 * n_queries * k * 8);
    L->total = take.at;
    return CBAS_OK;
}

}  // namespace

extern "C" int64_t cbas_rows_search_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t k) {
    RsLayout L;
    if (rs_layout("cbas_rows_search_workspace_bytes", n_rows, n_queries, k, &L) != CBAS_OK) return CBAS_EINVAL;
    return L.total;
}

extern "C" int cbas_rows_search(const uint16_t* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, const float* queries_dev,
                                int32_t n_queries, const int64_t* clip_table_dev, int32_t n_clips, const uint8_t* mask_dev, int32_t min_gap,
                                int32_t use_threshold, float threshold, int32_t k, float* trace_dev, int64_t* index_dev, float* score_dev,
                                void* workspace_dev, int64_t workspace_bytes, void* stream) {
    const char* const what = "cbas_rows_search";
    RsLayout L;
    if (rs_layout(what, n_rows, n_queries, k, &L) != CBAS_OK) return CBAS_EINVAL;
    if (rows_width_ok(what, "dim", dim, RS_MAX_D) != CBAS_OK || rows_ld_ok(what, "ld", ld, "dim", dim) != CBAS_OK) return CBAS_EINVAL;
    if (min_gap < 0 || min_gap > RS_MAX_GAP) return cbas_fail(CBAS_EINVAL, "%s: min_gap = %d (0 .. %d)", what, min_gap, RS_MAX_GAP);
    if (n_clips < 1) return cbas_fail(CBAS_EINVAL, "%s: n_clips = %d (at least 1)", what, n_clips);
    if (!rows_f16_dev || !queries_dev || !clip_table_dev || !trace_dev || !index_dev || !score_dev || !workspace_dev)
        return cbas_fail(CBAS_EINVAL, "%s: a NULL pointer (only mask_dev may be NULL)", what);
    if (((uintptr_t)rows_f16_dev | (uintptr_t)queries_dev | (uintptr_t)trace_dev | (uintptr_t)workspace_dev) % 16)
        return cbas_fail(CBAS_EINVAL, "%s: rows, queries, trace and workspace must be 16-byte aligned", what);
    if (((uintptr_t)clip_table_dev | (uintptr_t)index_dev) % 8 || (uintptr_t)score_dev % 4)
        return cbas_fail(CBAS_EINVAL, "%s: clip_table and index must be 8-byte aligned, score 4-byte aligned", what);
    if (workspace_bytes < L.total)
        return cbas_fail(CBAS_EINVAL, "%s: workspace of %lld bytes, %lld needed (cbas_rows_search_workspace_bytes)", what,
                         (long long)workspace_bytes, (long long)L.total);
    int device = 0, n_cu = 0;
    if (cbas_use_device_of(rows_f16_dev, &device) != CBAS_OK) return CBAS_EHIP;
    HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    hipStream_t st = (hipStream_t)stream;
    char* const ws = (char*)workspace_dev;
    float* const rq = (float*)(ws + L.rq);
    unsigned* const flags = (unsigned*)(ws + L.flags);
    int32_t* const clip_id = (int32_t*)(ws + L.clip_id);

    // the clip table, before anything is indexed with it
    HIP_TRY(hipMemsetAsync(flags, 0, 16, st));
    HIP_TRY(hipMemsetAsync(clip_id, 0xff, (size_t)n_rows * 4, st));
    int64_t slices = L.nch / n_clips + 1;
    if (slices > 64) slices = 64;
    const dim3 clip_grid((unsigned)n_clips, (unsigned)slices), wg(RS_THREADS);
    hipLaunchKernelGGL(rs_clip_fill_kernel, clip_grid, wg, 0, st, clip_table_dev, n_rows, clip_id, flags);
    hipLaunchKernelGGL(rs_clip_check_kernel, clip_grid, wg, 0, st, clip_table_dev, n_rows, (const int32_t*)clip_id, flags);
    HIP_TRY(hipGetLastError());
    unsigned bad[2] = {0u, 0u};
    HIP_TRY(hipMemcpyAsync(bad, flags, sizeof(bad), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad[0] & RS_FLAG_TABLE) return cbas_fail(CBAS_EINVAL, "%s: a clip table entry reaches outside the %lld rows", what, (long long)n_rows);
    if (bad[1] & RS_FLAG_OVERLAP) return cbas_fail(CBAS_EINVAL, "%s: two clip table entries overlap", what);

    // the scores
    const size_t lds = (size_t)16 * (dim + RS_QPAD) * sizeof(float);
    if (rows_lds_opt_in(&rs_score_kernel, lds) != CBAS_OK) return CBAS_EHIP;
    hipLaunchKernelGGL(rs_qnorm_kernel, dim3((n_queries + 3) / 4), wg, 0, st, queries_dev, dim, n_queries, rq);
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 4) per_cu = 4;
    if (per_cu < 1) per_cu = 1;
    const int64_t tile_groups = ((n_rows + 15) / 16 + 3) / 4;
    int64_t blocks = (int64_t)(n_cu > 0 ? n_cu : 256) * per_cu;
    if (blocks > tile_groups) blocks = tile_groups;
    hipLaunchKernelGGL(rs_score_kernel, dim3((unsigned)blocks, (unsigned)((n_queries + 15) / 16)), wg, lds, st, rows_f16_dev, n_rows, dim, ld,
                       queries_dev, n_queries, (const float*)rq, trace_dev);
    HIP_TRY(hipGetLastError());

    // the peaks of every chunk, then RS_FAN lists into one until the result is left
    const RsSelect sel{trace_dev, n_rows, clip_table_dev, clip_id, mask_dev, min_gap, use_threshold ? 1 : 0, threshold, k};
    float* buf_s[2] = {(float*)(ws + L.a_s), (float*)(ws + L.b_s)};
    int64_t* buf_i[2] = {(int64_t*)(ws + L.a_i), (int64_t*)(ws + L.b_i)};
    int64_t n = L.nch;
    int src = 0;
    hipLaunchKernelGGL(rs_peaks_kernel, dim3((unsigned)n, (unsigned)n_queries), wg, 0, st, sel, n == 1 ? score_dev : buf_s[0],
                       n == 1 ? index_dev : buf_i[0]);
    while (n > 1) {
        const int64_t n_out = (n + RS_FAN - 1) / RS_FAN;
        hipLaunchKernelGGL(rs_merge_kernel, dim3((unsigned)n_out, (unsigned)n_queries), wg, 0, st, (const float*)buf_s[src],
                           (const int64_t*)buf_i[src], n, k, n_out == 1 ? score_dev : buf_s[src ^ 1], n_out == 1 ? index_dev : buf_i[src ^ 1]);
        n = n_out;
        src ^= 1;
    }
    HIP_TRY(hipGetLastError());
    return CBAS_OK;
}
