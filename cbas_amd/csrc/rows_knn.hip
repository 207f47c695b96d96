// Weighted k-nearest-neighbour labels for resident CLS rows: cbas_rows_knn_workspace_bytes / cbas_rows_knn of
// include/cbas_mi355x.h, kernels and entry points in one file.  rows (N, D) fp16 with row stride ld, the labelled bank (M, D) fp16
// with row stride bank_ld.  The (N, M) matrix of cosines exists only a (RK_TILE, RK_BLOCK) block at a time, in LDS.
//
// THE DEFINITION
//   cos[m][j]   = fl(fl(dot * rn_row[m]) * rn_bank[j]).  dot: the fp32-accumulated sum of the exact products of the two fp16 rows on
//                 the fp16 matrix pipe, one v_mfma_f32_16x16x32_f16 per 32 columns in ascending order of the columns, all into one
//                 accumulator that starts at 0 (the hardware's order inside an instruction; a width that is no multiple of 64 ends
//                 with one instruction of zeros, which changes nothing but the sign of a zero).
//                 rn = fp32(1 / sqrt((double)s)), 0 when s = 0; s = (l0 + l1) + (l2 + l3) in fp32, l_j the fmaf chain, from 0, of
//                 x_d^2 over the columns d with (d % 32) / 8 = j, ascending (the s of rows_search.hip).  A zero row has rn = 0, so
//                 every cosine with it is exactly 0.  sims, when given, receives cos for every pair, excluded ones included.
//   excluded    bank entry j for row m when both group arrays are given and bank_group[j] == row_group[m] >= 0
//   neighbours  of row m: the k best entries that are not excluded; a beats b when cos[a] > cos[b], or cos[a] == cos[b] and a < b
//                 (rs_place's rule).  Written in that order; (-1, -inf) past the last.  A function of the cosine bits and the bank
//                 indices alone: not of the blocking of the bank, the tile a row falls into, N or the grid.
//   vote        s_0 = the best neighbour's score; w_r = fl(expf(__fdiv_rn(fl(s_r - s_0), T)) * cw[label_r]); Z = the fp32 sum of
//                 w_r in ascending rank; num_c = the fp32 sum of w_r over the neighbours with label c in ascending rank;
//                 probs[m][c] = num_c / Z.  A row without a neighbour gets zeros.
//
//   rows_rn_kernel    (rows_rn.h) rn of every store row and of every bank row: 4 lanes a row, lane j the chain l_j
//   rk_label_kernel   a label outside [0, C) sets a flag, read back before the pass is queued
//   rk_knn_kernel     THE PASS.  A workgroup owns RK_TILE = 128 store rows and walks the bank in blocks of RK_BLOCK = 64 entries;
//                     both operands come through LDS in chunks of RK_KC = 64 columns, two buffers, the next chunk's global loads in
//                     flight under the current chunk's MFMAs.  Wave w multiplies rows 32 w .. 32 w + 31 with the 64 entries: 8
//                     accumulators, 6 LDS reads for 8 MFMAs a 32-column step.  A finished block is scaled, masked (-inf for an
//                     excluded entry or one past M) and laid into LDS; thread t < 128 then takes row t's values that beat its list's
//                     worst entry (the lowest score, among equal scores the highest index) in its place and finds the worst again.
//                     The k best of a stream under a total order do not depend on the order of arrival.  After the last block the
//                     lists are put in order by rank placement and the same thread votes.  No atomics.
#include "kernels.h"
#include "rows_api.h"
#include "rows_rn.h"

namespace {

constexpr int RK_THREADS = 256;
constexpr int RK_TILE = 128;                         // store rows a workgroup owns (tests/rows_knn_ref.py: TILE)
constexpr int RK_BLOCK = 64;                         // bank entries per block (tests/rows_knn_ref.py: BLOCK)
constexpr int RK_KC = 64;                            // columns per staged chunk
constexpr int RK_LDA = RK_KC + 8;                    // halves between staged rows: 144 bytes, the 16 rows of an operand read hit 64 banks
constexpr int RK_LDS = RK_BLOCK + 1;                 // floats between the rows of the block of cosines
constexpr int RK_STAGE = (RK_TILE + RK_BLOCK) * RK_LDA;      // halves per staging buffer
constexpr int RK_MAX_M = 65536, RK_MAX_K = 64, RK_MAX_C = 64, RK_MAX_D = 1536;

__global__ __launch_bounds__(RK_THREADS) void rk_label_kernel(const int32_t* __restrict__ label, int M, int C, unsigned* __restrict__ flags) {
    const int j = blockIdx.x * RK_THREADS + threadIdx.x;
    if (j < M && (unsigned)label[j] >= (unsigned)C) flags[0] = 1u;
}

struct RkArgs {
    const uint16_t* rows;
    int64_t N;
    int D;
    int64_t ld;
    const uint16_t* bank;
    int M;
    int64_t bank_ld;
    const int32_t* bank_label;
    const int32_t* bank_group;
    const int32_t* row_group;
    int C;
    const float* class_weight;
    int k;
    float temperature;
    const float* rn_rows;
    const float* rn_bank;
    float* probs;
    int32_t* nn_index;
    float* nn_score;
    float* sims;
};

// the 16-byte pieces of chunk `it` that this thread stages: 4 of the tile, 2 of the bank block; zeros past N, M and D
__device__ __forceinline__ void rk_fetch(const RkArgs& a, int64_t m0, int it, int nkc, uint4 (&pa)[4], uint4 (&pb)[2]) {
    const int b = it / nkc, k0 = (it - b * nkc) * RK_KC;
    const int c8 = threadIdx.x & 7, r = threadIdx.x >> 3;
    const bool kin = k0 + 8 * c8 < a.D;
    const uint4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + r + 32 * i;
        pa[i] = (kin && m < a.N) ? *reinterpret_cast<const uint4*>(a.rows + m * a.ld + k0 + 8 * c8) : zero;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int j = b * RK_BLOCK + r + 32 * i;
        pb[i] = (kin && j < a.M) ? *reinterpret_cast<const uint4*>(a.bank + (int64_t)j * a.bank_ld + k0 + 8 * c8) : zero;
    }
}

__device__ __forceinline__ void rk_stage(uint16_t* buf, const uint4 (&pa)[4], const uint4 (&pb)[2]) {
    const int c8 = threadIdx.x & 7, r = threadIdx.x >> 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(buf + (r + 32 * i) * RK_LDA + 8 * c8) = pa[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<uint4*>(buf + (RK_TILE + r + 32 * i) * RK_LDA + 8 * c8) = pb[i];
}

// grid (ceil(N / RK_TILE)), 256 threads, LDS 2 RK_STAGE halves + RK_TILE RK_LDS floats + 2 k RK_TILE words
__global__ __launch_bounds__(RK_THREADS) void rk_knn_kernel(RkArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rk_lds[];
    uint16_t* const stage = reinterpret_cast<uint16_t*>(rk_lds);
    float* const S = reinterpret_cast<float*>(rk_lds + 2 * RK_STAGE * 2);
    float* const ls = S + RK_TILE * RK_LDS;                      // list entry r of row t at [r * RK_TILE + t]
    int* const li = reinterpret_cast<int*>(ls + a.k * RK_TILE);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fc = lane & 15, kr = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.x * RK_TILE;
    const int k = a.k;
    const float ninf = -__builtin_inff();
    const bool groups = a.bank_group && a.row_group;

    for (int i = tid; i < k * RK_TILE; i += RK_THREADS) {
        ls[i] = ninf;
        li[i] = -1;
    }
    // this lane's 8 rows of the accumulators: row 32 wave + 16 ri + 4 kr + e
    float rnr[2][4];
    int rgr[2][4];
#pragma unroll
    for (int ri = 0; ri < 2; ++ri)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t m = m0 + 32 * wave + 16 * ri + 4 * kr + e;
            rnr[ri][e] = m < a.N ? a.rn_rows[m] : 0.f;
            rgr[ri][e] = (groups && m < a.N) ? a.row_group[m] : -1;
        }

    const int nkc = (a.D + RK_KC - 1) / RK_KC, nblk = (a.M + RK_BLOCK - 1) / RK_BLOCK;
    const int total = nkc * nblk;
    uint4 pa[4], pb[2];
    rk_fetch(a, m0, 0, nkc, pa, pb);
    rk_stage(stage, pa, pb);
    __syncthreads();

    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[2][4];
    float rnb[4];
    int bg[4];
    int kc = 0, blk = 0;
    float ws = ninf;                                             // row tid's worst list entry: its score, bank index and slot
    int wi = -1, wslot = 0;
    for (int it = 0; it < total; ++it) {
        if (kc == 0) {
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) {
                const int j = blk * RK_BLOCK + 16 * ci + fc;
                rnb[ci] = j < a.M ? a.rn_bank[j] : 0.f;
                bg[ci] = (groups && j < a.M) ? a.bank_group[j] : -2;
#pragma unroll
                for (int ri = 0; ri < 2; ++ri) acc[ri][ci] = zero;
            }
        }
        const bool more = it + 1 < total;
        if (more) rk_fetch(a, m0, it + 1, nkc, pa, pb);
        const uint16_t* const A = stage + (it & 1) * RK_STAGE + (32 * wave + fc) * RK_LDA + 8 * kr;
        const uint16_t* const B = stage + (it & 1) * RK_STAGE + (RK_TILE + fc) * RK_LDA + 8 * kr;
#pragma unroll
        for (int ks = 0; ks < RK_KC / 32; ++ks) {
            f16x8 fa[2], fb[4];
#pragma unroll
            for (int ri = 0; ri < 2; ++ri) fa[ri] = *reinterpret_cast<const f16x8*>(A + 16 * ri * RK_LDA + 32 * ks);
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) fb[ci] = *reinterpret_cast<const f16x8*>(B + 16 * ci * RK_LDA + 32 * ks);
#pragma unroll
            for (int ri = 0; ri < 2; ++ri)
#pragma unroll
                for (int ci = 0; ci < 4; ++ci) acc[ri][ci] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[ri], fb[ci], acc[ri][ci], 0, 0, 0);
        }
        if (more) rk_stage(stage + ((it & 1) ^ 1) * RK_STAGE, pa, pb);
        __syncthreads();
        if (++kc < nkc) continue;
        kc = 0;

        // the block's cosines: acc[ri][ci][e] = row 32 wave + 16 ri + 4 kr + e against entry 16 ci + fc
        const int j0 = blk * RK_BLOCK;
#pragma unroll
        for (int ri = 0; ri < 2; ++ri)
#pragma unroll
            for (int ci = 0; ci < 4; ++ci)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = 32 * wave + 16 * ri + 4 * kr + e, j = j0 + 16 * ci + fc;
                    const float c = __fmul_rn(__fmul_rn(acc[ri][ci][e], rnr[ri][e]), rnb[ci]);
                    if (a.sims && m0 + row < a.N && j < a.M) a.sims[(m0 + row) * a.M + j] = c;
                    const bool out = j >= a.M || (rgr[ri][e] >= 0 && rgr[ri][e] == bg[ci]);
                    S[row * RK_LDS + 16 * ci + fc] = out ? ninf : c;
                }
        __syncthreads();
        if (tid < RK_TILE) {
            // The list is a SET between blocks: a candidate that beats the list's worst entry replaces it, and the worst is found
            // again (k independent LDS reads, no chain of shifts).  Candidates are the values at or over the worst score, as a mask,
            // taken from the block's last column down: a bank whose similarity rises along its index - labelled frames in the order
            // of time, scored against a later frame - then brings at most k of a block's 64 values into the list, not all of them.
            unsigned long long cand = 0ull;
#pragma unroll 16
            for (int c = 0; c < RK_BLOCK; ++c) cand |= (unsigned long long)(S[tid * RK_LDS + c] >= ws ? 1 : 0) << c;
            while (cand) {
                const int c = 63 - __clzll((long long)cand);
                cand &= ~(1ull << c);
                const float s = S[tid * RK_LDS + c];
                const int j = j0 + c;
                if (s > ws || (s == ws && j < wi)) {
                    ls[wslot * RK_TILE + tid] = s;
                    li[wslot * RK_TILE + tid] = j;
                    ws = ls[tid];
                    wi = li[tid];
                    wslot = 0;
                    for (int r = 1; r < k; ++r) {                // the worst: the lowest score, among equal scores the highest index
                        const float v = ls[r * RK_TILE + tid];
                        const int x = li[r * RK_TILE + tid];
                        if (v < ws || (v == ws && x > wi)) {
                            ws = v;
                            wi = x;
                            wslot = r;
                        }
                    }
                }
            }
        }
        __syncthreads();
        ++blk;
    }

    // the lists in order, by rank placement (rs_place's idiom), into the LDS the staging buffers and the block of cosines had: an
    // entry's position is the number of entries that beat it; the empty slots follow the last valid one
    float* const ss = reinterpret_cast<float*>(rk_lds);
    int* const si = reinterpret_cast<int*>(ss + k * RK_TILE);
    for (int i = tid; i < k * RK_TILE; i += RK_THREADS) {
        const int row = i & (RK_TILE - 1), r = i / RK_TILE;
        const float v = ls[r * RK_TILE + row];
        const int x = li[r * RK_TILE + row];
        int valid = 0, beat = 0, empty_before = 0;
        for (int q = 0; q < k; ++q) {
            const float vq = ls[q * RK_TILE + row];
            const int xq = li[q * RK_TILE + row];
            if (xq >= 0) {
                ++valid;
                beat += (vq > v || (vq == v && xq < x)) ? 1 : 0;
            } else {
                empty_before += q < r ? 1 : 0;
            }
        }
        const int rank = x >= 0 ? beat : valid + empty_before;
        ss[rank * RK_TILE + row] = x >= 0 ? v : ninf;
        si[rank * RK_TILE + row] = x >= 0 ? x : -1;
    }
    __syncthreads();
    if (a.nn_index || a.nn_score)
        for (int i = tid; i < k * RK_TILE; i += RK_THREADS) {
            const int row = i / k, r = i - row * k;
            if (m0 + row >= a.N) continue;
            if (a.nn_index) a.nn_index[(m0 + row) * k + r] = si[r * RK_TILE + row];
            if (a.nn_score) a.nn_score[(m0 + row) * k + r] = ss[r * RK_TILE + row];
        }
    __syncthreads();
    // the vote: w_r and label_r take the places of the row's scores and indices, then every class sums its own in ascending rank
    if (tid < RK_TILE && m0 + tid < a.N) {
        const float s0 = ss[tid];
        float Z = 0.f;
        int n = 0;
        for (; n < k; ++n) {
            const int idx = si[n * RK_TILE + tid];
            if (idx < 0) break;
            const int lab = a.bank_label[idx];
            const bool ok = (unsigned)lab < (unsigned)a.C;       // flagged before the pass: never an index
            const float e = expf(__fdiv_rn(__fsub_rn(ss[n * RK_TILE + tid], s0), a.temperature));
            const float w = !ok ? 0.f : a.class_weight ? __fmul_rn(e, a.class_weight[lab]) : e;
            Z = __fadd_rn(Z, w);
            ss[n * RK_TILE + tid] = w;
            si[n * RK_TILE + tid] = ok ? lab : -1;
        }
        float* const out = a.probs + (m0 + tid) * a.C;
        for (int c = 0; c < a.C; ++c) {
            float num = 0.f;
            for (int r = 0; r < n; ++r)
                if (si[r * RK_TILE + tid] == c) num = __fadd_rn(num, ss[r * RK_TILE + tid]);
            out[c] = n > 0 ? __fdiv_rn(num, Z) : 0.f;
        }
    }
}

// byte offsets into the workspace, each a multiple of 16
struct RkLayout {
    int64_t flags, rn_bank, rn_rows, total;
};

// 0, or CBAS_EINVAL with the message set
int rk_layout(const char* what, int64_t N, int32_t M, int32_t k, RkLayout* L) {
    if (N < 0 || (N + RK_TILE - 1) / RK_TILE > 0x7fffffff)
        return cbas_fail(CBAS_EINVAL, "%s: N = %lld (0 .. %lld)", what, (long long)N, (long long)0x7fffffff * RK_TILE);
    if (M < 1 || M > RK_MAX_M) return cbas_fail(CBAS_EINVAL, "%s: M = %d (1 .. %d)", what, M, RK_MAX_M);
    if (k < 1 || k > RK_MAX_K) return cbas_fail(CBAS_EINVAL, "%s: k = %d (1 .. %d)", what, k, RK_MAX_K);
    RowsTake take;
    L->flags = take(16);
    L->rn_bank = take((int64_t)M * 4);
    L->rn_rows = take(N * 4);
    L->total = take.at;
    return CBAS_OK;
}

}  // namespace

extern "C" int64_t cbas_rows_knn_workspace_bytes(int64_t N, int32_t M, int32_t k) {
    RkLayout L;
    if (rk_layout("cbas_rows_knn_workspace_bytes", N, M, k, &L) != CBAS_OK) return CBAS_EINVAL;
    return L.total;
}

extern "C" int cbas_rows_knn(const void* rows_f16_dev, int64_t N, int32_t D, int64_t ld, const void* bank_f16_dev, int32_t M, int64_t bank_ld,
                             const int32_t* bank_label_dev, const int32_t* bank_group_dev, const int32_t* row_group_dev, int32_t C,
                             const float* class_weight_dev, int32_t k, float temperature, float* probs_dev, int32_t* nn_index_dev,
                             float* nn_score_dev, float* sims_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    const char* const what = "cbas_rows_knn";
    RkLayout L;
    if (rk_layout(what, N, M, k, &L) != CBAS_OK) return CBAS_EINVAL;
    if (rows_width_ok(what, "D", D, RK_MAX_D) != CBAS_OK || rows_ld_ok(what, "ld", ld, "D", D) != CBAS_OK ||
        rows_ld_ok(what, "bank_ld", bank_ld, "D", D) != CBAS_OK)
        return CBAS_EINVAL;
    if (C < 1 || C > RK_MAX_C) return cbas_fail(CBAS_EINVAL, "%s: C = %d (1 .. %d)", what, C, RK_MAX_C);
    if (!(temperature > 0.f) || !(temperature <= 3.402823466e38f))
        return cbas_fail(CBAS_EINVAL, "%s: temperature = %g (finite and greater than 0)", what, (double)temperature);
    if (N == 0) return CBAS_OK;
    if (!rows_f16_dev || !bank_f16_dev || !bank_label_dev || !probs_dev || !workspace_dev)
        return cbas_fail(CBAS_EINVAL, "%s: a NULL pointer (only the groups, class_weight, nn_index, nn_score and sims may be NULL)", what);
    if (((uintptr_t)rows_f16_dev | (uintptr_t)bank_f16_dev | (uintptr_t)workspace_dev) % 16)
        return cbas_fail(CBAS_EINVAL, "%s: rows, bank and workspace must be 16-byte aligned", what);
    if (((uintptr_t)bank_label_dev | (uintptr_t)bank_group_dev | (uintptr_t)row_group_dev | (uintptr_t)class_weight_dev | (uintptr_t)probs_dev |
         (uintptr_t)nn_index_dev | (uintptr_t)nn_score_dev | (uintptr_t)sims_dev) % 4)
        return cbas_fail(CBAS_EINVAL, "%s: the int32 and float arrays must be 4-byte aligned", what);
    if (workspace_bytes < L.total)
        return cbas_fail(CBAS_EINVAL, "%s: workspace of %lld bytes, %lld needed (cbas_rows_knn_workspace_bytes)", what, (long long)workspace_bytes,
                         (long long)L.total);
    if (cbas_use_device_of(rows_f16_dev) != CBAS_OK) return CBAS_EHIP;
    hipStream_t st = (hipStream_t)stream;
    char* const ws = (char*)workspace_dev;
    unsigned* const flags = (unsigned*)(ws + L.flags);
    float* const rn_bank = (float*)(ws + L.rn_bank);
    float* const rn_rows = (float*)(ws + L.rn_rows);
    const dim3 wg(RK_THREADS);

    // the labels, before anything is indexed with one; the reciprocal norms meanwhile
    HIP_TRY(hipMemsetAsync(flags, 0, 16, st));
    hipLaunchKernelGGL(rk_label_kernel, dim3((M + RK_THREADS - 1) / RK_THREADS), wg, 0, st, bank_label_dev, M, C, flags);
    hipLaunchKernelGGL(rows_rn_kernel, dim3((unsigned)(((int64_t)M * 4 + RK_THREADS - 1) / RK_THREADS)), wg, 0, st, (const uint16_t*)bank_f16_dev,
                       (int64_t)M, D, bank_ld, rn_bank);
    hipLaunchKernelGGL(rows_rn_kernel, dim3((unsigned)((N * 4 + RK_THREADS - 1) / RK_THREADS)), wg, 0, st, (const uint16_t*)rows_f16_dev, N, D, ld,
                       rn_rows);
    HIP_TRY(hipGetLastError());
    unsigned bad = 0u;
    HIP_TRY(hipMemcpyAsync(&bad, flags, sizeof(bad), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad) return cbas_fail(CBAS_EINVAL, "%s: a bank label lies outside [0, C = %d)", what, C);

    const size_t lds = (size_t)2 * RK_STAGE * 2 + (size_t)RK_TILE * RK_LDS * 4 + (size_t)2 * k * RK_TILE * 4;
    if (rows_lds_opt_in(&rk_knn_kernel, lds) != CBAS_OK) return CBAS_EHIP;
    const RkArgs args{(const uint16_t*)rows_f16_dev, N, D, ld, (const uint16_t*)bank_f16_dev, M, bank_ld, bank_label_dev, bank_group_dev,
                      row_group_dev, C, class_weight_dev, k, temperature, rn_rows, rn_bank, probs_dev, nn_index_dev, nn_score_dev, sims_dev};
    hipLaunchKernelGGL(rk_knn_kernel, dim3((unsigned)((N + RK_TILE - 1) / RK_TILE)), wg, lds, st, args);
    HIP_TRY(hipGetLastError());
    return CBAS_OK;
}
