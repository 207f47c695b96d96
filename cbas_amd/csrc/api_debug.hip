// Bring-up, test and measurement harnesses of the DEBUG build (include/cbas_mi355x_debug.h): stand-alone GEMM timing and
// bit-exactness entry points, the lane-overlap probe, the MX-fp8 GEMM in isolation, the MFMA neighbour.  Compiled only with
// -DCBAS_BUILD_DEBUG=1 (python -m cbas_amd.build --debug); the product library does not contain this file.
#include <math.h>
#include <string.h>
#include <new>
#include <vector>
#include <algorithm>
#include <chrono>

#include "api_common.h"
#include "kernels.h"
#include "vit32_epilogue.h"

#if !CBAS_BUILD_DEBUG
#error "api_debug.hip belongs to the debug build only (-DCBAS_BUILD_DEBUG=1)"
#endif

extern "C" int cbas_debug_build(void) { return 1; }

static int pos_interp_mode_ok(int mode) { return mode == CBAS_POS_INTERP_BICUBIC_AA || mode == CBAS_POS_INTERP_BICUBIC; }

extern "C" int cbas_debug_pos_interp_matrix(int mode, int in_size, int out_size, float* W) {
    if (!pos_interp_mode_ok(mode) || in_size < 1 || out_size < 1 || !W) return cbas_fail(CBAS_EINVAL, "cbas_debug_pos_interp_matrix: bad argument");
    cbas_pos_interp_matrix(mode, in_size, out_size, W);
    return CBAS_OK;
}

extern "C" int cbas_debug_pos_table(int mode, const float* src, int G, int D, int nh, int nw, float* out) {
    if (!pos_interp_mode_ok(mode) || G < 1 || D < 1 || nh < 1 || nw < 1 || !src || !out) return cbas_fail(CBAS_EINVAL, "cbas_debug_pos_table: bad argument");
    cbas_build_pos_table(mode, src, G, D, nh, nw, out);
    return CBAS_OK;
}

// ---- bring-up: stand-alone GEMM timing / bit-exactness harness ---------------------------------
namespace {
__global__ void fill_random_f16(f16* p, int64_t n, uint32_t seed, float scale) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t x = (uint32_t)i * 2654435761u ^ seed;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    p[i] = (f16)(((float)(x & 0xFFFF) / 32768.0f - 1.0f) * scale);
}
__global__ void mask_bytes_kernel(uint32_t* p, int64_t n) {       // clear bit 3 of every byte: no e4m3 NaN codes
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] &= 0x77777777u;
}
__global__ void checksum_u16(const uint16_t* p, int64_t n, unsigned long long* out) {
    unsigned long long s = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        s += (unsigned long long)p[i] * (unsigned long long)((i % 1021) + 1);
    atomicAdd(out, s);
}
}  // namespace

// bring-up / tests: a register-only v_mfma_f32_32x32x16_f16 loop on every SIMD (two waves each), queued on `stream` - the
// neighbour beside which round 4's head kernels returned wrong values in lanes 48-63 (common.h); tests run the head beside it
namespace {
__global__ __launch_bounds__(512) void mfma_neighbor_kernel(int iters, float* sink) {
    typedef float f16v __attribute__((ext_vector_type(16)));
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    f16x8 a[4], b[4];
    for (int i = 0; i < 4; ++i)
        for (int e = 0; e < 8; ++e) {
            unsigned x = (t * 64 + i * 8 + e) * 2654435761u; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
            a[i][e] = (f16)(((int)(x & 0xffff) - 32768) * (1.0f / 32768.0f));
            b[i][e] = (f16)(((int)(x >> 16) - 32768) * (1.0f / 32768.0f));
        }
    f16v c[4];
    for (int i = 0; i < 4; ++i)
        for (int e = 0; e < 16; ++e) c[i][e] = 0.f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[(i + r) & 3], b[(i * 2 + r) & 3], c[i], 0, 0, 0);
    }
    float s = 0.f;
    for (int i = 0; i < 4; ++i)
        for (int e = 0; e < 16; ++e) s += c[i][e];
    if (s == 123.456f) sink[t] = s;
}
}  // namespace

extern "C" int cbas_debug_mfma_neighbor(int iters, void* stream) {
    static float* sink = nullptr;
    int dev = 0, cus = 256;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (!sink) HIP_TRY(hipMalloc(&sink, (size_t)cus * 512 * sizeof(float)));
    if (iters <= 0) return cbas_fail(CBAS_EINVAL, "iters=%d", iters);
    hipLaunchKernelGGL(mfma_neighbor_kernel, dim3((unsigned)cus), dim3(512), 0, (hipStream_t)stream, iters, sink);
    return hipGetLastError() == hipSuccess ? CBAS_OK : cbas_fail(CBAS_EHIP, "mfma_neighbor launch failed");
}

// precision-4 GEMM (split operands) alone: epi = 1 q|k|v (RoPE), 2 residual, 3 GELU; tile = 0 (planner) / 128 / 160 / 192 / 256
// rows of the ping-pong form, -1 = the 128 x 128 8-wave kernel; prints the block timeline.  Timing only (random operands).
extern "C" int cbas_debug_gemm_split_bench(int M, int N, int K, int epi, int tile, int iters, float* ms_out) {
    if (M <= 256 || N % 256 || K % 64 || iters <= 0 || epi < 1 || epi > 3) return cbas_fail(CBAS_EINVAL, "bad split GEMM bench shape");
    if (epi == 1 && (N % 3 || (N / 3) % 64)) return cbas_fail(CBAS_EINVAL, "q|k|v bench needs N = 3 D, D a multiple of 64");
    float *A = nullptr, *Wt = nullptr, *out = nullptr, *bias = nullptr, *rope = nullptr;
    HIP_TRY(hipMalloc(&A, (int64_t)M * K * 4));
    HIP_TRY(hipMalloc(&Wt, (int64_t)N * K * 4));
    HIP_TRY(hipMalloc(&out, (int64_t)M * N * 4));
    HIP_TRY(hipMalloc(&bias, (int64_t)N * 4));
    HIP_TRY(hipMalloc(&rope, 2 * 196 * 64 * 4));
    HIP_TRY(hipMemset(bias, 0, (int64_t)N * 4));
    HIP_TRY(hipMemset(out, 0, (int64_t)M * N * 4));
    HIP_TRY(hipMemset(rope, 0, 2 * 196 * 64 * 4));
    hipLaunchKernelGGL(fill_random_f16, dim3((unsigned)(((int64_t)M * K * 2 + 255) / 256)), dim3(256), 0, 0, (f16*)A, (int64_t)M * K * 2, 1u, 1.0f);
    hipLaunchKernelGGL(fill_random_f16, dim3((unsigned)(((int64_t)N * K * 2 + 255) / 256)), dim3(256), 0, 0, (f16*)Wt, (int64_t)N * K * 2, 2u, 0.05f);
    Gemm32VitParams p{};
    p.A = A; p.lda = K; p.W = Wt; p.M = M; p.N = N; p.K = K; p.bias = bias; p.lambda = bias; p.out = out; p.ldo = N;
    p.tokens_per_frame = 201; p.n_prefix = 5; p.patches_per_frame = 196; p.rope_cos = rope; p.rope_sin = rope + 196 * 64; p.D = N / 3;
    p.rope_fac = rope; p.rope_nh = 14; p.rope_nw = 14; p.rope_magic = (unsigned)((1ull << 32) / 14u) + 1u;   // zeros: timing only
    p.split = 1; p.a_scale = 1.f; p.w_scale = 1.f; p.out_scale = 1.f;
    const GemmEpilogue e = (GemmEpilogue)epi;
    auto run = [&]() { return tile < 0 ? launch_gemm_f32_vit(e, p, 0) : launch_gemm_split_pp(e, p, 0); };
    vit32_split_set_forms(tile < 0 ? 2 : -1);
    gemm_split_pp_set_tile(tile > 0 ? tile : 0, nullptr);
    int rc = run();
    if (rc) return cbas_fail(CBAS_EINVAL, "split GEMM launch failed (rc=%d)", rc);
    HIP_TRY(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, 0));
    for (int i = 0; i < iters; ++i) run();
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (ms_out) *ms_out = ms / iters;
    if (tile >= 0) {
        const int nblk = GEMM_STAMP_BLOCKS;
        unsigned long long* st = nullptr;
        HIP_TRY(hipMalloc(&st, (size_t)nblk * 72));
        HIP_TRY(hipMemset(st, 0, (size_t)nblk * 72));
        gemm_split_pp_set_tile(tile > 0 ? tile : 0, st);
        run();
        HIP_TRY(hipDeviceSynchronize());
        gemm_split_pp_set_tile(0, nullptr);
        std::vector<unsigned long long> hs((size_t)nblk * 9);
        HIP_TRY(hipMemcpy(hs.data(), st, (size_t)nblk * 72, hipMemcpyDeviceToHost));
        double pro = 0, loop = 0, epi_c = 0, real = 0; int n = 0;
        for (int b = 0; b < nblk; ++b) {
            if (!hs[4 * b + 3]) continue;
            pro += (double)(hs[4 * b + 1] - hs[4 * b]); loop += (double)(hs[4 * b + 2] - hs[4 * b + 1]);
            epi_c += (double)(hs[4 * b + 3] - hs[4 * b + 2]); real += (double)hs[(size_t)nblk * 4 + b]; ++n;
        }
        if (n) printf("  stamps (first tile of each workgroup): %d workgroups; avg prologue %.0f, K loop %.0f (%.0f per K-tile), epilogue %.0f cycles; "
                      "in-kernel clock %.2f GHz\n", n, pro / n, loop / n, loop / n / (K / 32), epi_c / n, real > 0 ? loop / real * 0.1 : 0.0);
        double lp = 0, ll = 0, le = 0; int ln = 0;
        for (int b = 0; b < nblk; ++b) {
            const unsigned long long* o = &hs[(size_t)nblk * 5 + 4 * (size_t)b];
            if (!o[3]) continue;
            lp += (double)(o[1] - o[0]); ll += (double)(o[2] - o[1]); le += (double)(o[3] - o[2]); ++ln;
        }
        if (ln) printf("  last tile of the %d workgroups that ran more than one: prologue %.0f, K loop %.0f, epilogue %.0f cycles\n",
                       ln, lp / ln, ll / ln, le / ln);
        fflush(stdout);
        hipFree(st);
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(A); hipFree(Wt); hipFree(out); hipFree(bias); hipFree(rope);
    return CBAS_OK;
}

// precision-4 GEMM forms against each other on the same random split operands: the ping-pong form at `tile` rows (0 = planner)
// and the 128 x 128 kernels; n_diff = output 32-bit words that differ (the forms promise 0).  epi as above; the residual
// form starts both runs from the same x.
namespace {
__global__ void count_diff_u32(const uint32_t* a, const uint32_t* b, int64_t n, unsigned long long* out) {
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) c += a[i] != b[i];
    if (c) atomicAdd(out, c);
}
}  // namespace
extern "C" int cbas_debug_gemm_split_compare(int M, int N, int K, int epi, int tile, int64_t* n_diff) {
    if (M <= 0 || N % 256 || K % 64 || epi < 1 || epi > 3 || !n_diff) return cbas_fail(CBAS_EINVAL, "bad split GEMM compare shape");
    if (epi == 1 && (N % 3 || (N / 3) % 64)) return cbas_fail(CBAS_EINVAL, "q|k|v compare needs N = 3 D, D a multiple of 64");
    float *A = nullptr, *Wt = nullptr, *o1 = nullptr, *o2 = nullptr, *x0 = nullptr, *bias = nullptr, *rope = nullptr;
    unsigned long long* cnt = nullptr;
    const int64_t no = (int64_t)M * N;
    HIP_TRY(hipMalloc(&A, (int64_t)M * K * 4));
    HIP_TRY(hipMalloc(&Wt, (int64_t)N * K * 4));
    HIP_TRY(hipMalloc(&o1, no * 4)); HIP_TRY(hipMalloc(&o2, no * 4)); HIP_TRY(hipMalloc(&x0, no * 4));
    HIP_TRY(hipMalloc(&bias, (int64_t)N * 4 * 2));
    HIP_TRY(hipMalloc(&rope, 2 * 196 * 64 * 4));
    HIP_TRY(hipMalloc(&cnt, 8));
    HIP_TRY(hipMemset(cnt, 0, 8));
    auto fill = [&](float* p, int64_t n_f16, unsigned seed, float sc) {
        hipLaunchKernelGGL(fill_random_f16, dim3((unsigned)((n_f16 + 255) / 256)), dim3(256), 0, 0, (f16*)p, n_f16, seed, sc);
    };
    fill(A, (int64_t)M * K * 2, 1u, 1.0f);
    fill(Wt, (int64_t)N * K * 2, 2u, 0.05f);
    // fp32 side data: bias / lambda, x, cos / sin - any finite numbers do (random halves widened by the conversion kernel)
    f16* tmp = nullptr;
    HIP_TRY(hipMalloc(&tmp, (no > 2 * 196 * 64 ? no : 2 * 196 * 64) * 2));
    auto fill32 = [&](float* p, int64_t n, unsigned seed, float sc) {
        hipLaunchKernelGGL(fill_random_f16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, tmp, n, seed, sc);
        return launch_f16_to_f32(tmp, p, n, 0);
    };
    if (fill32(bias, (int64_t)N * 2, 3u, 0.5f) || fill32(x0, no, 4u, 2.0f) || fill32(rope, 2 * 196 * 64, 5u, 1.0f)) return cbas_fail(CBAS_EHIP, "fill failed");
    // the tables are angles.tile(2) ([tf]:190): columns d and d + 32 of a row hold the same number - the tile epilogue relies on it
    HIP_TRY(hipMemcpy2D(rope + 32, 64 * 4, rope, 64 * 4, 32 * 4, 2 * 196, hipMemcpyDeviceToDevice));
    Gemm32VitParams p{};
    p.A = A; p.lda = K; p.W = Wt; p.M = M; p.N = N; p.K = K; p.bias = bias; p.lambda = bias + N; p.ldo = N;
    p.tokens_per_frame = 201; p.n_prefix = 5; p.patches_per_frame = 196; p.rope_cos = rope; p.rope_sin = rope + 196 * 64; p.D = N / 3;
    p.split = 1; p.a_scale = 2.f; p.w_scale = 4.f; p.out_scale = 4.f;
    const GemmEpilogue e = (GemmEpilogue)epi;
    int rc = 0;
    for (int form = 0; form < 2 && !rc; ++form) {
        float* o = form ? o2 : o1;
        HIP_TRY(hipMemcpy(o, x0, no * 4, hipMemcpyDeviceToDevice));
        p.out = o;
        if (form == 0) { gemm_split_pp_set_tile(tile > 0 ? tile : 0, nullptr); vit32_split_set_forms(3); }
        else vit32_split_set_forms(0);
        rc = launch_gemm_f32_vit(e, p, 0);
        HIP_TRY(hipDeviceSynchronize());
    }
    gemm_split_pp_set_tile(0, nullptr);
    vit32_split_set_forms(-1);
    if (rc) return cbas_fail(CBAS_EINVAL, "split GEMM launch failed (rc=%d)", rc);
    hipLaunchKernelGGL(count_diff_u32, dim3(1024), dim3(256), 0, 0, (const uint32_t*)o1, (const uint32_t*)o2, no, cnt);
    unsigned long long hc = 0;
    HIP_TRY(hipMemcpy(&hc, cnt, 8, hipMemcpyDeviceToHost));
    *n_diff = (int64_t)hc;
    hipFree(A); hipFree(Wt); hipFree(o1); hipFree(o2); hipFree(x0); hipFree(bias); hipFree(rope); hipFree(cnt); hipFree(tmp);
    return CBAS_OK;
}

extern "C" int cbas_debug_gemm_bench(int M, int N, int K, int tile, int iters, float* ms_out,
                                     unsigned long long* checksum_out) {
    // tile >= 100: residual epilogue (o_proj/down_proj style, fp32 in/out) with tile id = tile - 100;
    // tile >= 200: q|k|v epilogue (RoPE tables of 196 patches, 201 tokens per frame, D = N / 3) with tile id = tile - 200
    // + 500: MX-fp8 operands (random e4m3 bytes, unit scales; the GELU form then writes fp8 + scales): timing only
    // 3000 + tile id: the gated MLP's gate | up epilogue (EPI_SWIGLU: N = 2 F interleaved columns, F columns stored): timing only
    const bool swiglu = tile >= 3000;
    if (swiglu) tile -= 3000;
    const bool ln = tile >= 2000;            // 2000 + ...: the LayerNorm-fold form of the epilogue (timing only: zero statistics)
    if (ln) tile -= 2000;
    const bool want_stamps = tile >= 1000;   // 1000 + tile: also print the block timeline statistics
    tile %= 1000;
    const bool f8 = tile >= 500;
    if (f8) tile -= 500;
    const bool qkv = tile >= 200;
    const bool resid = !qkv && tile >= 100;
    if (qkv) tile -= 200;
    if (resid) tile -= 100;
    if (qkv && (N % 3 || (N / 3) % 64)) return cbas_fail(CBAS_EINVAL, "q|k|v bench needs N = 3 D, D a multiple of 64");
    if (M <= 0 || N % 128 || K % 64 || iters <= 0) return cbas_fail(CBAS_EINVAL, "bad GEMM bench shape");
    if (swiglu && (tile >= 100 || ln)) return cbas_fail(CBAS_EINVAL, "the gated bench form is an fp16 up-projection form of its own");
    const int64_t M_pad = round_up(M, 256);
    f16 *A = nullptr, *Wt = nullptr, *out = nullptr;
    float* bias = nullptr;
    unsigned long long* cs = nullptr;
    HIP_TRY(hipMalloc(&A, M_pad * (int64_t)K * 2));
    HIP_TRY(hipMalloc(&Wt, (int64_t)N * K * 2));
    HIP_TRY(hipMalloc(&out, M_pad * (int64_t)N * 2));
    HIP_TRY(hipMalloc(&bias, (int64_t)N * 4));
    HIP_TRY(hipMalloc(&cs, 8));
    HIP_TRY(hipMemset(bias, 0, (int64_t)N * 4));
    HIP_TRY(hipMemset(out, 0, M_pad * (int64_t)N * 2));
    HIP_TRY(hipMemset(cs, 0, 8));
    hipLaunchKernelGGL(fill_random_f16, dim3((unsigned)((M_pad * K + 255) / 256)), dim3(256), 0, 0, A, M_pad * K, 1u, 1.0f);
    hipLaunchKernelGGL(fill_random_f16, dim3((unsigned)(((int64_t)N * K + 255) / 256)), dim3(256), 0, 0, Wt, (int64_t)N * K, 2u, 0.05f);
    GemmParams p{};
    p.tile = tile; p.A = A; p.W = Wt; p.M = M; p.M_pad = (int)M_pad; p.N = N; p.K = K; p.bias = bias; p.out_f16 = out; p.ldo = N;
    uint32_t* sc8 = nullptr;
    if (f8) {                                    // the fp16 buffers reinterpreted as bytes (first half used); NaN codes masked out
        if (K % 256 || N % 256) return cbas_fail(CBAS_EINVAL, "fp8 GEMM bench needs N, K multiples of 256");
        hipLaunchKernelGGL(mask_bytes_kernel, dim3(4096), dim3(256), 0, 0, (uint32_t*)A, M_pad * (int64_t)K / 4);
        hipLaunchKernelGGL(mask_bytes_kernel, dim3(4096), dim3(256), 0, 0, (uint32_t*)Wt, (int64_t)N * K / 4);
        const int64_t sc_ld = M_pad > N ? M_pad : N;
        HIP_TRY(hipMalloc(&sc8, (size_t)(K / 128 + N / 128) * sc_ld * 4));
        HIP_TRY(hipMemset(sc8, 0x7a, (size_t)(K / 128 + N / 128) * sc_ld * 4));     // E8M0 2^-5 per block: products stay finite
        p.A8 = (const uint8_t*)A; p.W8 = (const uint8_t*)Wt; p.A_sc = sc8; p.W_sc = sc8; p.sc_lda = (int)sc_ld; p.sc_ldw = (int)sc_ld;
        p.out_f8 = (uint8_t*)out; p.out_sc = sc8 + (size_t)(K / 128) * sc_ld; p.sc_ldo = (int)sc_ld;
    }
    float* x32 = nullptr;
    if (resid) {
        HIP_TRY(hipMalloc(&x32, M_pad * (int64_t)N * 4));
        HIP_TRY(hipMemset(x32, 0, M_pad * (int64_t)N * 4));
        p.out_f32 = x32; p.lambda = bias;      // lambda = 0: x stays 0, timing only
    }
    float* rope = nullptr;
    if (qkv) {
        HIP_TRY(hipMalloc(&rope, 2 * 196 * 64 * 4));
        HIP_TRY(hipMemset(rope, 0, 2 * 196 * 64 * 4));
        p.rope_cos = rope; p.rope_sin = rope + 196 * 64; p.D = N / 3; p.tokens_per_frame = 201; p.n_prefix = 5;
        p.rope_fac = rope; p.rope_nh = 14; p.rope_nw = 14; p.rope_magic = (unsigned)((1ull << 32) / 14u) + 1u;   // zeros: timing only
    }
    float2* lnst = nullptr;
    f16* x16 = nullptr;
    float* colsum = nullptr;
    if (ln) {
        if (f8) return cbas_fail(CBAS_EINVAL, "the LayerNorm fold is an fp16 form");
        HIP_TRY(hipMalloc(&lnst, 4 * M_pad * sizeof(float2)));
        HIP_TRY(hipMemset(lnst, 0, 4 * M_pad * sizeof(float2)));
        HIP_TRY(hipMalloc(&colsum, (int64_t)N * 4));
        HIP_TRY(hipMemset(colsum, 0, (int64_t)N * 4));
        if (resid) { HIP_TRY(hipMalloc(&x16, M_pad * (int64_t)N * 2)); p.x16_out = x16; p.ln_out = lnst; }
        else { p.ln_in = lnst; p.ln_colsum = colsum; p.ln_parts = K / 256; p.ln_eps = 1.0f; }
        p.ln_ld = (int)M_pad;
        if (!p.tile) p.tile = GEMM_TILE_PP_AUTO;
    }
    if (swiglu) p.ldo = N / 2;
    const GemmEpilogue epi = swiglu ? EPI_SWIGLU : qkv ? (ln ? EPI_QKV_LN : EPI_QKV) : resid ? (ln ? EPI_RESID_LN : EPI_RESID) : f8 ? EPI_GELU_F8 : (ln ? EPI_GELU_LN : EPI_GELU);
    int rc = launch_gemm(epi, p, 0);
    if (rc) return cbas_fail(CBAS_EINVAL, "launch_gemm failed for tile %d (rc=%d)", tile, rc);
    HIP_TRY(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, 0));
    for (int i = 0; i < iters; ++i) launch_gemm(epi, p, 0);
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (ms_out) *ms_out = ms / iters;
    if (want_stamps) {
        const int nblk = GEMM_STAMP_BLOCKS;
        unsigned long long* st = nullptr;
        HIP_TRY(hipMalloc(&st, (size_t)nblk * 72));
        HIP_TRY(hipMemset(st, 0, (size_t)nblk * 72));
        p.stamps = st;
        launch_gemm(epi, p, 0);                  // straight after the timed launches: the clock is the loaded one
        HIP_TRY(hipDeviceSynchronize());
        std::vector<unsigned long long> hs((size_t)nblk * 9);
        HIP_TRY(hipMemcpy(hs.data(), st, (size_t)nblk * 72, hipMemcpyDeviceToHost));
        double pro = 0, loop = 0, epi_c = 0, real = 0; int n = 0;
        for (int b = 0; b < nblk; ++b) {
            if (!hs[4 * b + 3]) continue;
            pro += (double)(hs[4 * b + 1] - hs[4 * b]); loop += (double)(hs[4 * b + 2] - hs[4 * b + 1]);
            epi_c += (double)(hs[4 * b + 3] - hs[4 * b + 2]); real += (double)hs[(size_t)nblk * 4 + b]; ++n;
        }
        // s_memtime ticks are shader cycles; the K loop's span in s_memrealtime (100 MHz) ticks gives the in-kernel clock
        printf("  stamps (first tile of each workgroup): %d workgroups; avg prologue %.0f, K loop %.0f, epilogue %.0f cycles; "
               "in-kernel clock %.2f GHz\n", n, pro / n, loop / n, epi_c / n, real > 0 ? loop / real * 0.1 : 0.0);
        double lp = 0, ll = 0, le = 0; int ln = 0;
        for (int b = 0; b < nblk; ++b) {
            const unsigned long long* o = &hs[(size_t)nblk * 5 + 4 * (size_t)b];
            if (!o[3]) continue;
            lp += (double)(o[1] - o[0]); ll += (double)(o[2] - o[1]); le += (double)(o[3] - o[2]); ++ln;
        }
        if (ln) printf("  last tile of the %d workgroups that ran more than one: prologue %.0f, K loop %.0f, epilogue %.0f cycles\n",
                       ln, lp / ln, ll / ln, le / ln);
        fflush(stdout);
        p.stamps = nullptr;
        hipFree(st);
    }
    hipLaunchKernelGGL(checksum_u16, dim3(1024), dim3(256), 0, 0, (const uint16_t*)out, (int64_t)M * N, cs);
    if (checksum_out) HIP_TRY(hipMemcpy(checksum_out, cs, 8, hipMemcpyDeviceToHost));
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(A); hipFree(Wt); hipFree(out); hipFree(bias); hipFree(cs); if (x32) hipFree(x32); if (rope) hipFree(rope); if (sc8) hipFree(sc8);
    if (lnst) hipFree(lnst); if (x16) hipFree(x16); if (colsum) hipFree(colsum);
    return CBAS_OK;
}

// Bring-up: how kernels of two compute lanes share the chip.  Runs, each on its own stream and concurrently, `iters`
// launches of: bit 0 the up projection (12 864 x 3072 x 768, GELU epilogue), bit 1 LayerNorm (12 864 x 768), bit 2 the
// resident attention kernel (64 frames x 201 tokens, 12 heads), bit 3 the down projection (residual epilogue);
// ms_out[b] = average time per launch of component b as seen on its stream, ms_out[4] = wall time of the whole run.
extern "C" int cbas_debug_overlap(int mode, int iters, float* ms_out) {
    if (iters <= 0 || !ms_out) return cbas_fail(CBAS_EINVAL, "bad arguments");
    const char* te = getenv("CBAS_OVL_T");                   // tokens per frame of the attention component (default 201)
    const int Ta = te ? atoi(te) : 201;
    const int n = 64, T = 201, D = 768, F = 3072, M = n * T;
    const int64_t M_pad = round_up(M, 256);
    f16 *h16 = nullptr, *u16 = nullptr, *qkv = nullptr, *ctx = nullptr, *Wu = nullptr, *Wd = nullptr, *ln_out = nullptr;
    float *x = nullptr, *x2 = nullptr, *vec = nullptr;
    HIP_TRY(hipMalloc(&h16, M_pad * D * 2)); HIP_TRY(hipMalloc(&u16, M_pad * (int64_t)F * 2));
    HIP_TRY(hipMalloc(&qkv, M_pad * 3 * D * 2)); HIP_TRY(hipMalloc(&ctx, M_pad * D * 2)); HIP_TRY(hipMalloc(&ln_out, M_pad * D * 2));
    HIP_TRY(hipMalloc(&Wu, (int64_t)F * D * 2)); HIP_TRY(hipMalloc(&Wd, (int64_t)F * D * 2));
    HIP_TRY(hipMalloc(&x, M_pad * D * 4)); HIP_TRY(hipMalloc(&x2, M_pad * D * 4)); HIP_TRY(hipMalloc(&vec, F * 4));
    HIP_TRY(hipMemset(vec, 0, F * 4)); HIP_TRY(hipMemset(x, 0, M_pad * D * 4)); HIP_TRY(hipMemset(x2, 0, M_pad * D * 4));
    auto fill = [&](f16* p, int64_t cnt, unsigned seed, float sc) {
        hipLaunchKernelGGL(fill_random_f16, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, 0, p, cnt, seed, sc);
    };
    fill(h16, M_pad * D, 1u, 1.0f); fill(u16, M_pad * (int64_t)F, 2u, 1.0f); fill(qkv, M_pad * 3 * D, 3u, 1.0f);
    fill(Wu, (int64_t)F * D, 4u, 0.05f); fill(Wd, (int64_t)F * D, 5u, 0.02f);
    HIP_TRY(hipDeviceSynchronize());
    GemmParams up{}; up.A = h16; up.W = Wu; up.M = M; up.M_pad = (int)M_pad; up.N = F; up.K = D; up.bias = vec; up.out_f16 = u16; up.ldo = F;
    GemmParams dn{}; dn.A = u16; dn.W = Wd; dn.M = M; dn.M_pad = (int)M_pad; dn.N = D; dn.K = F; dn.bias = vec; dn.lambda = vec; dn.out_f32 = x2; dn.ldo = D;
    hipStream_t st[4]; hipEvent_t e0[4], e1[4];
    for (int b = 0; b < 4; ++b) { HIP_TRY(hipStreamCreateWithFlags(&st[b], hipStreamNonBlocking)); HIP_TRY(hipEventCreate(&e0[b])); HIP_TRY(hipEventCreate(&e1[b])); }
    auto launch = [&](int b) -> int {
        switch (b) {
            case 0: return launch_gemm(EPI_GELU, up, st[0]);
            case 1: return launch_layernorm_f16(x, D, vec, vec, ln_out, M, D, 1e-5f, st[1]);
            case 2: return launch_attention(qkv, nullptr, ctx, nullptr, 0, n * T / Ta, Ta, D, 12, st[2]);
            default: return launch_gemm(EPI_RESID, dn, st[3]);
        }
    };
    for (int b = 0; b < 4; ++b) if (mode & (1 << b)) for (int i = 0; i < 3; ++i) if (launch(b)) return cbas_fail(CBAS_EINVAL, "launch %d failed", b);
    HIP_TRY(hipDeviceSynchronize());
    const auto w0 = std::chrono::steady_clock::now();
    for (int b = 0; b < 4; ++b) if (mode & (1 << b)) HIP_TRY(hipEventRecord(e0[b], st[b]));
    for (int i = 0; i < iters; ++i)                       // interleaved submission, like two lanes queueing their kernels
        for (int b = 0; b < 4; ++b) if (mode & (1 << b)) launch(b);
    for (int b = 0; b < 4; ++b) if (mode & (1 << b)) HIP_TRY(hipEventRecord(e1[b], st[b]));
    HIP_TRY(hipDeviceSynchronize());
    ms_out[4] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
    for (int b = 0; b < 4; ++b) {
        ms_out[b] = 0.f;
        if (mode & (1 << b)) { float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, e0[b], e1[b])); ms_out[b] = ms / iters; }
        hipStreamDestroy(st[b]); hipEventDestroy(e0[b]); hipEventDestroy(e1[b]);
    }
    hipFree(h16); hipFree(u16); hipFree(qkv); hipFree(ctx); hipFree(ln_out); hipFree(Wu); hipFree(Wd); hipFree(x); hipFree(x2); hipFree(vec);
    return CBAS_OK;
}

// Bring-up / test harness of the MX-fp8 GEMM: quantise A [M][K] and W [N][K] (fp32, host) with the library's own
// block quantiser, run out = A_q * W_q^T through the fp8 ping-pong kernel (residual epilogue on a zero stream with
// bias 0 and lambda 1), and hand back the product together with the quantised operands, so a test can recompute it
// from exactly those bytes and scales.  A_sc / W_sc: [K/128][M_pad resp. N] dwords (GemmParams layout), M_pad = M up to 256.
extern "C" int cbas_debug_gemm_f8(int M, int N, int K, int tile, const float* A_host, const float* W_host, float* out_host,
                                  uint8_t* A8_host, uint32_t* Asc_host, uint8_t* W8_host, uint32_t* Wsc_host) {
    if (M <= 0 || N % 256 || K % 256 || !A_host || !W_host || !out_host) return cbas_fail(CBAS_EINVAL, "bad fp8 GEMM test shape");
    const int64_t M_pad = round_up(M, 256);
    float *A = nullptr, *W = nullptr, *x = nullptr, *bias = nullptr, *lam = nullptr;
    uint8_t *A8 = nullptr, *W8 = nullptr;
    uint32_t *Asc = nullptr, *Wsc = nullptr;
    HIP_TRY(hipMalloc(&A, M_pad * (int64_t)K * 4));
    HIP_TRY(hipMalloc(&W, (int64_t)N * K * 4));
    HIP_TRY(hipMalloc(&x, M_pad * (int64_t)N * 4));
    HIP_TRY(hipMalloc(&bias, (int64_t)N * 4));
    HIP_TRY(hipMalloc(&lam, (int64_t)N * 4));
    HIP_TRY(hipMalloc(&A8, M_pad * (int64_t)K));
    HIP_TRY(hipMalloc(&W8, (int64_t)N * K));
    HIP_TRY(hipMalloc(&Asc, M_pad * (int64_t)K / 32));
    HIP_TRY(hipMalloc(&Wsc, (int64_t)N * K / 32));
    HIP_TRY(hipMemset(A, 0, M_pad * (int64_t)K * 4));
    HIP_TRY(hipMemset(x, 0, M_pad * (int64_t)N * 4));
    HIP_TRY(hipMemset(bias, 0, (int64_t)N * 4));
    HIP_TRY(hipMemcpy(A, A_host, (int64_t)M * K * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(W, W_host, (int64_t)N * K * 4, hipMemcpyHostToDevice));
    std::vector<float> ones((size_t)N, 1.0f);
    HIP_TRY(hipMemcpy(lam, ones.data(), (int64_t)N * 4, hipMemcpyHostToDevice));
    LAUNCH_TRY(launch_pack_fp8_weight(A, A8, Asc, (int)M_pad, K, (int)M_pad, 0, 0));
    LAUNCH_TRY(launch_pack_fp8_weight(W, W8, Wsc, N, K, N, 0, 0));
    GemmParams p{};
    p.tile = tile; p.A8 = A8; p.W8 = W8; p.A_sc = Asc; p.W_sc = Wsc; p.sc_lda = (int)M_pad;
    p.M = M; p.M_pad = (int)M_pad; p.N = N; p.K = K; p.lda = K; p.bias = bias; p.lambda = lam; p.out_f32 = x; p.ldo = N;
    int rc = tile ? launch_gemm_8ph(EPI_RESID, p, tile, 0) : launch_gemm(EPI_RESID, p, 0);
    if (rc) return cbas_fail(CBAS_EINVAL, "fp8 GEMM launch failed (rc=%d)", rc);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_host, x, (int64_t)M * N * 4, hipMemcpyDeviceToHost));
    if (A8_host) HIP_TRY(hipMemcpy(A8_host, A8, (int64_t)M * K, hipMemcpyDeviceToHost));
    if (Asc_host) HIP_TRY(hipMemcpy(Asc_host, Asc, M_pad * (int64_t)K / 32, hipMemcpyDeviceToHost));
    if (W8_host) HIP_TRY(hipMemcpy(W8_host, W8, (int64_t)N * K, hipMemcpyDeviceToHost));
    if (Wsc_host) HIP_TRY(hipMemcpy(Wsc_host, Wsc, (int64_t)N * K / 32, hipMemcpyDeviceToHost));
    hipFree(A); hipFree(W); hipFree(x); hipFree(bias); hipFree(lam); hipFree(A8); hipFree(W8); hipFree(Asc); hipFree(Wsc);
    return CBAS_OK;
}

// ---- tests: one GEMM / attention launch on host operands (include/cbas_mi355x_debug.h) -----------------------------------
namespace {
// q | k | v rows [rows][3D] fp32 (q already x 1/8) -> the head-split operands of precision 4, as the q|k|v epilogue writes
// them (store_head_split4 with the ATT_* scales; q's 1/8 is already in the value); q_rows: a [rows][D] q image (sec0 = 0 only)
__global__ void pack_head_split_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t rows, int width, int D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // one thread = 4 consecutive columns
    const int per_row = width / 4;
    if (i >= rows * per_row) return;
    const int64_t r = i / per_row;
    const int c = (int)(i - r * per_row) * 4;
    const int sec = c / D, hc = c - sec * D;
    const float sc = sec == 0 ? ATT_QS : (sec == 1 ? ATT_KS : ATT_VS);
    store_head_split4(dst + r * width + sec * D + (hc & ~63), hc & 63, *reinterpret_cast<const f32x4*>(src + r * width + c), sc);
}

struct DevBufs {                       // frees what it holds on every return path
    std::vector<void*> p;
    template <typename T> hipError_t alloc(T** out, size_t bytes) {
        *out = nullptr;
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(out), bytes ? bytes : 4);
        if (e == hipSuccess) p.push_back(*out);
        return e;
    }
    ~DevBufs() { for (void* q : p) (void)hipFree(q); }
};
}  // namespace

// The up projection in the four forms the fp8 plans use: {fp16, MX-fp8} operands x {fp16, MX-fp8} result (see the header).
extern "C" int cbas_debug_gemm_gelu_forms(int M, int N, int K, int tile, int a_fp8, int out_fp8, const float* A_host,
                                          const float* W_host, const float* bias_host, uint16_t* out16_host, uint8_t* out8_host,
                                          uint32_t* outsc_host, uint8_t* A8_host, uint32_t* Asc_host, uint8_t* W8_host,
                                          uint32_t* Wsc_host) {
    if (M <= 0 || N <= 0 || K <= 0 || N % 256 || K % 256 || !A_host || !W_host || !bias_host || (out_fp8 ? !out8_host || !outsc_host : !out16_host))
        return cbas_fail(CBAS_EINVAL, "bad GELU GEMM test shape / pointers");
    const int64_t M_pad = round_up(M, 256);
    DevBufs bufs;
    float *A = nullptr, *W = nullptr, *bias = nullptr;
    HIP_TRY(bufs.alloc(&A, M_pad * (int64_t)K * 4));
    HIP_TRY(bufs.alloc(&W, (int64_t)N * K * 4));
    HIP_TRY(bufs.alloc(&bias, (int64_t)N * 4));
    HIP_TRY(hipMemset(A, 0, M_pad * (int64_t)K * 4));
    HIP_TRY(hipMemcpy(A, A_host, (int64_t)M * K * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(W, W_host, (int64_t)N * K * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(bias, bias_host, (int64_t)N * 4, hipMemcpyHostToDevice));
    GemmParams p{};
    p.tile = tile; p.M = M; p.M_pad = (int)M_pad; p.N = N; p.K = K; p.lda = K; p.bias = bias; p.ldo = N;
    uint8_t *A8 = nullptr, *W8 = nullptr;
    uint32_t *Asc = nullptr, *Wsc = nullptr;
    if (a_fp8) {
        HIP_TRY(bufs.alloc(&A8, M_pad * (int64_t)K));
        HIP_TRY(bufs.alloc(&W8, (int64_t)N * K));
        HIP_TRY(bufs.alloc(&Asc, M_pad * (int64_t)K / 32));
        HIP_TRY(bufs.alloc(&Wsc, (int64_t)N * K / 32));
        LAUNCH_TRY(launch_pack_fp8_weight(A, A8, Asc, (int)M_pad, K, (int)M_pad, 0, 0));
        LAUNCH_TRY(launch_pack_fp8_weight(W, W8, Wsc, N, K, N, 0, 0));
        p.A8 = A8; p.W8 = W8; p.A_sc = Asc; p.W_sc = Wsc; p.sc_lda = (int)M_pad;
    } else {
        f16 *A16 = nullptr, *W16 = nullptr;
        HIP_TRY(bufs.alloc(&A16, M_pad * (int64_t)K * 2));
        HIP_TRY(bufs.alloc(&W16, (int64_t)N * K * 2));
        LAUNCH_TRY(launch_convert_f16(A, A16, nullptr, M_pad * (int64_t)K, 0));
        LAUNCH_TRY(launch_convert_f16(W, W16, nullptr, (int64_t)N * K, 0));
        p.A = A16; p.W = W16;
    }
    f16* o16 = nullptr;
    uint8_t* o8 = nullptr;
    uint32_t* osc = nullptr;
    if (out_fp8) {
        HIP_TRY(bufs.alloc(&o8, (int64_t)M * N));
        HIP_TRY(bufs.alloc(&osc, (int64_t)(N / 128) * M_pad * 4));
        HIP_TRY(hipMemset(osc, 0, (int64_t)(N / 128) * M_pad * 4));
        p.out_f8 = o8; p.out_sc = osc; p.sc_ldo = (int)M_pad;
    } else {
        HIP_TRY(bufs.alloc(&o16, (int64_t)M * N * 2));
        p.out_f16 = o16;
    }
    const GemmEpilogue epi = out_fp8 ? EPI_GELU_F8 : EPI_GELU;
    const int rc = tile ? launch_gemm_8ph(epi, p, tile, 0) : launch_gemm(epi, p, 0);
    if (rc) return cbas_fail(CBAS_EINVAL, "GELU GEMM launch failed (a_fp8=%d out_fp8=%d tile=%d rc=%d)", a_fp8, out_fp8, tile, rc);
    HIP_TRY(hipDeviceSynchronize());
    if (out_fp8) {
        HIP_TRY(hipMemcpy(out8_host, o8, (int64_t)M * N, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(outsc_host, osc, (int64_t)(N / 128) * M_pad * 4, hipMemcpyDeviceToHost));
    } else {
        HIP_TRY(hipMemcpy(out16_host, o16, (int64_t)M * N * 2, hipMemcpyDeviceToHost));
    }
    if (a_fp8) {
        if (A8_host) HIP_TRY(hipMemcpy(A8_host, A8, (int64_t)M * K, hipMemcpyDeviceToHost));
        if (Asc_host) HIP_TRY(hipMemcpy(Asc_host, Asc, M_pad * (int64_t)K / 32, hipMemcpyDeviceToHost));
        if (W8_host) HIP_TRY(hipMemcpy(W8_host, W8, (int64_t)N * K, hipMemcpyDeviceToHost));
        if (Wsc_host) HIP_TRY(hipMemcpy(Wsc_host, Wsc, (int64_t)N * K / 32, hipMemcpyDeviceToHost));
    }
    return CBAS_OK;
}

// ONE gate | up GEMM of a gated MLP (EPI_SWIGLU) on host operands: the harness interleaves W_g / W_u and their biases with the
// library's own routine (launch_interleave_gate_up), converts / splits them as cbas_enc_create_mlp does, and returns what the
// launch stored (see the header).
extern "C" int cbas_debug_gemm_swiglu(int arith, int tile, int forms, int M, int M_alloc, int F, int K, int lda, const float* A_host,
                                      const float* Wg_host, const float* Wu_host, const float* bg_host, const float* bu_host,
                                      float a_scale, float w_scale, float out_scale, void* out_host) {
    if (arith != 0 && arith != 3 && arith != 4) return cbas_fail(CBAS_EINVAL, "arith %d: 0, 3 or 4", arith);
    if (M <= 0 || M_alloc < M || F <= 0 || F % 64 || K <= 0 || K % 64 || lda < K || lda % 32 || !A_host || !Wg_host || !Wu_host || !bg_host ||
        !bu_host || !out_host)
        return cbas_fail(CBAS_EINVAL, "bad gated GEMM test shape / pointers (F %% 64, K %% 64, lda %% 32 must be 0)");
    if (arith == 4 && !(a_scale > 0.f && w_scale > 0.f && out_scale > 0.f)) return cbas_fail(CBAS_EINVAL, "split operands need positive scales");
    const size_t na = (size_t)M_alloc * lda, nw = (size_t)F * K, osz = (size_t)M * F * (arith == 0 ? 2 : 4);
    DevBufs B;
    float *A32, *Wg, *Wu, *bg, *bu, *Wgu, *bgu;
    void* out;
    HIP_TRY(B.alloc(&A32, na * 4));
    HIP_TRY(B.alloc(&Wg, nw * 4));
    HIP_TRY(B.alloc(&Wu, nw * 4));
    HIP_TRY(B.alloc(&bg, (size_t)F * 4));
    HIP_TRY(B.alloc(&bu, (size_t)F * 4));
    HIP_TRY(B.alloc(&Wgu, 2 * nw * 4));
    HIP_TRY(B.alloc(&bgu, 2 * (size_t)F * 4));
    HIP_TRY(B.alloc(&out, osz));
    HIP_TRY(hipMemcpy(A32, A_host, na * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(Wg, Wg_host, nw * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(Wu, Wu_host, nw * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(bg, bg_host, (size_t)F * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(bu, bu_host, (size_t)F * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(out, out_host, osz, hipMemcpyHostToDevice));          // the caller's canaries: rows >= M of a tile must not be stored
    LAUNCH_TRY(launch_interleave_gate_up(Wg, Wu, Wgu, F, K, 0));
    LAUNCH_TRY(launch_interleave_gate_up(bg, bu, bgu, F, 1, 0));
    int rcode = 0;
    if (arith == 0) {
        f16 *A16, *W16;
        HIP_TRY(B.alloc(&A16, na * 2));
        HIP_TRY(B.alloc(&W16, 2 * nw * 2));
        LAUNCH_TRY(launch_convert_f16(A32, A16, nullptr, (int64_t)na, 0));
        LAUNCH_TRY(launch_convert_f16(Wgu, W16, nullptr, (int64_t)(2 * nw), 0));
        GemmParams p{};
        p.tile = tile; p.A = A16; p.lda = lda; p.W = W16; p.M = M; p.M_pad = M_alloc; p.N = 2 * F; p.K = K; p.bias = bgu;
        p.out_f16 = (f16*)out; p.ldo = F;
        rcode = launch_gemm(EPI_SWIGLU, p, 0);
    } else {
        const bool split = arith == 4;
        const float *Ag = A32, *Wq = Wgu;
        if (split) {
            float *As, *Ws;
            HIP_TRY(B.alloc(&As, na * 4));
            HIP_TRY(B.alloc(&Ws, 2 * nw * 4));
            LAUNCH_TRY(launch_pack_split_weight(A32, As, M_alloc, lda, a_scale, 0));
            LAUNCH_TRY(launch_pack_split_weight(Wgu, Ws, 2 * (int64_t)F, K, w_scale, 0));
            Ag = As; Wq = Ws;
        }
        Gemm32VitParams p{};
        p.A = Ag; p.lda = lda; p.W = Wq; p.M = M; p.N = 2 * F; p.K = K; p.bias = bgu; p.out = (float*)out; p.ldo = F;
        p.split = split; p.a_scale = split ? a_scale : 1.f; p.w_scale = split ? w_scale : 1.f; p.out_scale = out_scale;
        if (split) {
            vit32_split_set_forms(forms);
            gemm_split_pp_set_tile(tile > 0 ? tile : 0, nullptr);
        }
        rcode = launch_gemm_f32_vit(EPI_SWIGLU, p, 0);
        if (split) { gemm_split_pp_set_tile(0, nullptr); vit32_split_set_forms(-1); }
    }
    if (rcode) return cbas_fail(CBAS_EINVAL, "gated GEMM launch failed (arith %d, tile %d, forms %d: rc=%d)", arith, tile, forms, rcode);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_host, out, osz, hipMemcpyDeviceToHost));
    return CBAS_OK;
}

extern "C" int cbas_debug_gemm_run(const cbas_debug_gemm_args* a) {
    if (!a || a->struct_bytes != (int64_t)sizeof(cbas_debug_gemm_args))
        return cbas_fail(CBAS_EINVAL, "cbas_debug_gemm_args: struct_bytes %lld, library expects %lld", a ? (long long)a->struct_bytes : -1ll,
                         (long long)sizeof(cbas_debug_gemm_args));
    const int arith = a->arith, epi = a->epi;
    if (arith != 0 && arith != 1 && arith != 3 && arith != 4) return cbas_fail(CBAS_EINVAL, "arith %d", arith);
    if (epi < EPI_PATCH || epi > EPI_GELU) return cbas_fail(CBAS_EINVAL, "epi %d", epi);
    if (a->M <= 0 || a->M_alloc < a->M || a->K <= 0 || a->lda < a->K || a->ldo < a->N || a->N <= 0 || !a->A || !a->W || !a->bias || !a->out)
        return cbas_fail(CBAS_EINVAL, "bad GEMM test shape / pointers");
    if ((epi == EPI_RESID && !a->lambda) || (arith == 4 && a->lda % 32))
        return cbas_fail(CBAS_EINVAL, "EPI_RESID needs lambda; split operands need lda %% 32 == 0");
    const bool patch = epi == EPI_PATCH, rope = epi == EPI_QKV && a->rope_cos && a->rope_sin;
    if (patch && (a->P <= 0 || a->M % a->P || (int64_t)(a->M / a->P) * a->T > a->out_rows || a->T < a->n_prefix + a->P))
        return cbas_fail(CBAS_EINVAL, "EPI_PATCH: M must be frames x P and out_rows >= frames x T");
    if (!patch && a->out_rows < a->M) return cbas_fail(CBAS_EINVAL, "out_rows < M");
    if (epi == EPI_QKV && (a->T <= 0 || a->n_prefix < 0)) return cbas_fail(CBAS_EINVAL, "EPI_QKV needs T and n_prefix");
    if (rope && (a->rope_nh <= 0 || a->rope_nw <= 0 || a->P != a->rope_nh * a->rope_nw || a->T > a->n_prefix + a->P))
        return cbas_fail(CBAS_EINVAL, "RoPE: P = nh x nw and T <= n_prefix + P");
    const bool out16 = (arith == 0 || arith == 1) && (epi == EPI_QKV || epi == EPI_GELU);
    const size_t osz = (size_t)a->out_rows * a->ldo * (out16 ? 2 : 4);
    const size_t na = (size_t)a->M_alloc * a->lda, nw = (size_t)a->N * a->K;
    DevBufs B;
    float *A32, *W32, *bias, *lam = nullptr, *pos = nullptr, *rc = nullptr, *rs = nullptr, *fac = nullptr;
    void* out;
    HIP_TRY(B.alloc(&A32, na * 4));
    HIP_TRY(B.alloc(&W32, nw * 4));
    HIP_TRY(B.alloc(&bias, (size_t)a->N * 4));
    HIP_TRY(B.alloc(&out, osz));
    HIP_TRY(hipMemcpy(A32, a->A, na * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(W32, a->W, nw * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(bias, a->bias, (size_t)a->N * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(out, a->out, osz, hipMemcpyHostToDevice));
    if (a->lambda) { HIP_TRY(B.alloc(&lam, (size_t)a->N * 4)); HIP_TRY(hipMemcpy(lam, a->lambda, (size_t)a->N * 4, hipMemcpyHostToDevice)); }
    if (patch && a->pos) {
        HIP_TRY(B.alloc(&pos, (size_t)a->P * a->N * 4));
        HIP_TRY(hipMemcpy(pos, a->pos, (size_t)a->P * a->N * 4, hipMemcpyHostToDevice));
    }
    const int nh = a->rope_nh, nwd = a->rope_nw;
    if (rope) {
        const size_t nt = (size_t)a->P * 64;
        HIP_TRY(B.alloc(&rc, nt * 4));
        HIP_TRY(B.alloc(&rs, nt * 4));
        HIP_TRY(hipMemcpy(rc, a->rope_cos, nt * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(rs, a->rope_sin, nt * 4, hipMemcpyHostToDevice));
        if (a->rope_lds) {             // the by-axis copy, built from the tables as ensure_rope builds it (api_enc.hip)
            std::vector<float> f((size_t)(nh + nwd) * 32);
            for (int iy = 0; iy < nh; ++iy)
                for (int d = 0; d < 16; ++d) {
                    f[(size_t)iy * 32 + d] = a->rope_cos[(size_t)(iy * nwd) * 64 + d];
                    f[(size_t)iy * 32 + 16 + d] = a->rope_sin[(size_t)(iy * nwd) * 64 + d];
                }
            for (int ix = 0; ix < nwd; ++ix)
                for (int d = 0; d < 16; ++d) {
                    f[(size_t)(nh + ix) * 32 + d] = a->rope_cos[(size_t)ix * 64 + 16 + d];
                    f[(size_t)(nh + ix) * 32 + 16 + d] = a->rope_sin[(size_t)ix * 64 + 16 + d];
                }
            HIP_TRY(B.alloc(&fac, f.size() * 4));
            HIP_TRY(hipMemcpy(fac, f.data(), f.size() * 4, hipMemcpyHostToDevice));
        }
    }
    const unsigned magic = rope ? (unsigned)((1ull << 32) / (unsigned)nwd) + 1u : 0u;
    int rcode = 0;
    if (arith == 0 || arith == 1) {
        f16 *A16, *Wh, *Wl = nullptr;
        HIP_TRY(B.alloc(&A16, na * 2));
        HIP_TRY(B.alloc(&Wh, nw * 2));
        if (arith == 1) HIP_TRY(B.alloc(&Wl, nw * 2));
        LAUNCH_TRY(launch_convert_f16(A32, A16, nullptr, (int64_t)na, 0));
        LAUNCH_TRY(launch_convert_f16(W32, Wh, Wl, (int64_t)nw, 0));
        GemmParams p{};
        p.tile = a->tile; p.group_m = a->group_m; p.A = A16; p.lda = a->lda; p.W = Wh; p.W_lo = Wl;
        p.M = a->M; p.M_pad = a->M_alloc; p.N = a->N; p.K = a->K; p.bias = bias; p.lambda = lam; p.ldo = a->ldo;
        if (out16) p.out_f16 = (f16*)out; else p.out_f32 = (float*)out;
        p.patches_per_frame = a->P; p.tokens_per_frame = a->T; p.n_prefix = a->n_prefix; p.in_scale = a->in_scale; p.pos = pos;
        p.rope_cos = rc; p.rope_sin = rs; p.rope_fac = fac; p.rope_nh = nh; p.rope_nw = nwd; p.rope_magic = magic;
        p.D = a->D; p.sec0 = a->sec0;
        rcode = launch_gemm((GemmEpilogue)epi, p, 0);
    } else {
        const bool split = arith == 4;
        const float *Ag = A32, *Wg = W32;
        if (split) {
            float *As, *Ws;
            HIP_TRY(B.alloc(&As, na * 4));
            HIP_TRY(B.alloc(&Ws, nw * 4));
            LAUNCH_TRY(launch_pack_split_weight(A32, As, a->M_alloc, a->lda, a->a_scale, 0));
            LAUNCH_TRY(launch_pack_split_weight(W32, Ws, a->N, a->K, a->w_scale, 0));
            Ag = As; Wg = Ws;
        }
        Gemm32VitParams p{};
        p.A = Ag; p.lda = a->lda; p.W = Wg; p.M = a->M; p.N = a->N; p.K = a->K; p.bias = bias; p.lambda = lam;
        p.out = (float*)out; p.ldo = a->ldo;
        p.patches_per_frame = a->P; p.tokens_per_frame = a->T; p.n_prefix = a->n_prefix; p.pos = pos;
        p.rope_cos = rc; p.rope_sin = rs; p.rope_fac = fac; p.rope_nh = nh; p.rope_nw = nwd; p.rope_magic = magic;
        p.D = a->D; p.sec0 = a->sec0;
        p.split = split; p.a_scale = split ? a->a_scale : 1.f; p.w_scale = split ? a->w_scale : 1.f; p.out_scale = a->out_scale;
        if (split) {
            vit32_split_set_forms(a->tile < 0 ? 0 : a->forms);
            gemm_split_pp_set_tile(a->tile > 0 ? a->tile : 0, nullptr);
        }
        rcode = launch_gemm_f32_vit((GemmEpilogue)epi, p, 0);
        if (split) { gemm_split_pp_set_tile(0, nullptr); vit32_split_set_forms(-1); }
    }
    if (rcode) return cbas_fail(CBAS_EINVAL, "GEMM launch failed (arith %d, epi %d, tile %d: rc=%d)", arith, epi, a->tile, rcode);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(a->out, out, osz, hipMemcpyDeviceToHost));
    return CBAS_OK;
}

// ONE MX-fp8 launch as vit_qkv / vit_tail issue it (see the header): M_pad, sc_lda and the W window (n0, n_total) are the
// caller's, the operand and scale arrays are allocated at exactly the sizes the launch is told about.
extern "C" int cbas_debug_gemm_f8_run(const cbas_debug_gemm_f8_args* a) {
    if (!a || a->struct_bytes != (int64_t)sizeof(cbas_debug_gemm_f8_args))
        return cbas_fail(CBAS_EINVAL, "cbas_debug_gemm_f8_args: struct_bytes %lld, library expects %lld", a ? (long long)a->struct_bytes : -1ll,
                         (long long)sizeof(cbas_debug_gemm_f8_args));
    const int epi = a->epi;
    if (epi != EPI_QKV && epi != EPI_RESID && epi != EPI_GELU) return cbas_fail(CBAS_EINVAL, "epi %d: EPI_QKV, EPI_RESID or EPI_GELU", epi);
    if (a->tile != 0 && (a->tile < GEMM_TILE_PP_256x256 || a->tile > GEMM_TILE_PP_AUTO)) return cbas_fail(CBAS_EINVAL, "tile %d: 0 or 13..17", a->tile);
    if (a->M <= 0 || a->M_alloc < a->M || a->N <= 0 || a->N % 256 || a->K <= 0 || a->K % 256 || a->sc_lda < a->M_alloc || a->n0 < 0 ||
        (int64_t)a->n0 + a->N > a->n_total || a->ldo < a->N || a->out_rows < a->M || a->group_m < 0)
        return cbas_fail(CBAS_EINVAL, "bad fp8 GEMM test shape (N %% 256, K %% 256, M <= M_alloc <= sc_lda, n0 + N <= n_total, N <= ldo, M <= out_rows)");
    if ((int64_t)a->M_alloc * a->K >= (1ll << 31) || (int64_t)a->n_total * a->K >= (1ll << 31))
        return cbas_fail(CBAS_EINVAL, "operands beyond the kernel's 32-bit byte offsets");
    if (!a->A8 || !a->A_sc || !a->W8 || !a->W_sc || !a->bias || !a->out || (a->quantise && (!a->A || !a->W)) || (epi == EPI_RESID && !a->lambda))
        return cbas_fail(CBAS_EINVAL, "fp8 GEMM test: missing pointer (quantise needs A and W, EPI_RESID lambda)");
    const bool rope = epi == EPI_QKV && a->rope_cos && a->rope_sin;
    if (epi == EPI_QKV && (a->T <= 0 || a->n_prefix < 0 || a->D <= 0 || a->D % 64 || a->N % a->D || a->sec0 < 0 || a->N / a->D + a->sec0 > 3))
        return cbas_fail(CBAS_EINVAL, "EPI_QKV needs T, n_prefix, D %% 64 == 0, N a multiple of D and sec0 + N / D <= 3");
    if (rope && (a->rope_nh <= 0 || a->rope_nw <= 0 || a->P != a->rope_nh * a->rope_nw || a->T > a->n_prefix + a->P))
        return cbas_fail(CBAS_EINVAL, "RoPE: P = nh x nw and T <= n_prefix + P");
    const int M_alloc = a->M_alloc, N = a->N, K = a->K, n_total = a->n_total;
    const bool out16 = epi != EPI_RESID;
    const size_t osz = (size_t)a->out_rows * a->ldo * (out16 ? 2 : 4);
    const size_t na = (size_t)M_alloc * K, nw = (size_t)n_total * K;
    const size_t nsa = (size_t)(K / 128) * a->sc_lda, nsw = (size_t)(K / 128) * n_total;       // dwords
    DevBufs B;
    uint8_t *A8, *W8;
    uint32_t *Asc, *Wsc;
    float *bias, *lam = nullptr, *rc = nullptr, *rs = nullptr, *fac = nullptr;
    void* out;
    HIP_TRY(B.alloc(&A8, na));
    HIP_TRY(B.alloc(&W8, nw));
    HIP_TRY(B.alloc(&Asc, nsa * 4));
    HIP_TRY(B.alloc(&Wsc, nsw * 4));
    HIP_TRY(B.alloc(&bias, (size_t)N * 4));
    HIP_TRY(B.alloc(&out, osz));
    HIP_TRY(hipMemcpy(A8, a->A8, na, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(W8, a->W8, nw, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(Asc, a->A_sc, nsa * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(Wsc, a->W_sc, nsw * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(bias, a->bias, (size_t)N * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(out, a->out, osz, hipMemcpyHostToDevice));
    if (a->lambda) { HIP_TRY(B.alloc(&lam, (size_t)N * 4)); HIP_TRY(hipMemcpy(lam, a->lambda, (size_t)N * 4, hipMemcpyHostToDevice)); }
    if (a->quantise) {
        float *A32, *W32;
        HIP_TRY(B.alloc(&A32, na * 4));
        HIP_TRY(B.alloc(&W32, nw * 4));
        HIP_TRY(hipMemcpy(A32, a->A, na * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(W32, a->W, nw * 4, hipMemcpyHostToDevice));
        LAUNCH_TRY(launch_pack_fp8_weight(A32, A8, Asc, M_alloc, K, a->sc_lda, 0, 0));
        LAUNCH_TRY(launch_pack_fp8_weight(W32, W8, Wsc, n_total, K, n_total, 0, 0));
    }
    const int nh = a->rope_nh, nwd = a->rope_nw;
    if (rope) {
        const size_t nt = (size_t)a->P * 64;
        HIP_TRY(B.alloc(&rc, nt * 4));
        HIP_TRY(B.alloc(&rs, nt * 4));
        HIP_TRY(hipMemcpy(rc, a->rope_cos, nt * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(rs, a->rope_sin, nt * 4, hipMemcpyHostToDevice));
        if (a->rope_lds) {             // the by-axis copy, built from the tables as cbas_debug_gemm_run builds it
            std::vector<float> f((size_t)(nh + nwd) * 32);
            for (int iy = 0; iy < nh; ++iy)
                for (int d = 0; d < 16; ++d) {
                    f[(size_t)iy * 32 + d] = a->rope_cos[(size_t)(iy * nwd) * 64 + d];
                    f[(size_t)iy * 32 + 16 + d] = a->rope_sin[(size_t)(iy * nwd) * 64 + d];
                }
            for (int ix = 0; ix < nwd; ++ix)
                for (int d = 0; d < 16; ++d) {
                    f[(size_t)(nh + ix) * 32 + d] = a->rope_cos[(size_t)ix * 64 + 16 + d];
                    f[(size_t)(nh + ix) * 32 + 16 + d] = a->rope_sin[(size_t)ix * 64 + 16 + d];
                }
            HIP_TRY(B.alloc(&fac, f.size() * 4));
            HIP_TRY(hipMemcpy(fac, f.data(), f.size() * 4, hipMemcpyHostToDevice));
        }
    }
    GemmParams p{};
    p.tile = a->tile; p.group_m = a->group_m;
    p.A8 = A8; p.A_sc = Asc; p.sc_lda = a->sc_lda; p.lda = K;
    p.W8 = W8 + (size_t)a->n0 * K; p.W_sc = Wsc + a->n0;
    if (n_total != N) p.sc_ldw = n_total;
    p.M = a->M; p.M_pad = M_alloc; p.N = N; p.K = K; p.bias = bias; p.lambda = lam; p.ldo = a->ldo;
    if (out16) p.out_f16 = (f16*)out; else p.out_f32 = (float*)out;
    p.tokens_per_frame = a->T; p.n_prefix = a->n_prefix; p.D = a->D; p.sec0 = a->sec0;
    p.rope_cos = rc; p.rope_sin = rs; p.rope_fac = fac; p.rope_nh = nh; p.rope_nw = nwd;
    p.rope_magic = rope ? (unsigned)((1ull << 32) / (unsigned)nwd) + 1u : 0u;
    const int rcode = launch_gemm((GemmEpilogue)epi, p, 0);
    if (rcode) return cbas_fail(CBAS_EINVAL, "fp8 GEMM launch failed (epi %d, tile %d: rc=%d)", epi, a->tile, rcode);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(a->out, out, osz, hipMemcpyDeviceToHost));
    if (a->quantise) {
        HIP_TRY(hipMemcpy(a->A8, A8, na, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(a->W8, W8, nw, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(a->A_sc, Asc, nsa * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(a->W_sc, Wsc, nsw * 4, hipMemcpyDeviceToHost));
    }
    return CBAS_OK;
}

extern "C" int cbas_debug_attention_run(const cbas_debug_attention_args* a) {
    if (!a || a->struct_bytes != (int64_t)sizeof(cbas_debug_attention_args))
        return cbas_fail(CBAS_EINVAL, "cbas_debug_attention_args: struct_bytes %lld, library expects %lld", a ? (long long)a->struct_bytes : -1ll,
                         (long long)sizeof(cbas_debug_attention_args));
    const int arith = a->arith, n = a->n, T = a->T, D = a->D;
    if (arith != 0 && arith != 3 && arith != 4) return cbas_fail(CBAS_EINVAL, "arith %d", arith);
    const int64_t rows = (int64_t)n * T, orows_min = a->q_cls ? n : rows;
    if (n <= 0 || T <= 0 || D != a->n_heads * 64 || a->rows_alloc < rows || a->out_rows < orows_min || !a->qkv || !a->out)
        return cbas_fail(CBAS_EINVAL, "bad attention test shape / pointers");
    // the device image is padded past the caller's rows (zeros): whatever a kernel may stage beyond the last frame lies inside it
    const int64_t dev_rows = round_up(a->rows_alloc, 256) + 256;
    const size_t nq = (size_t)a->rows_alloc * 3 * D, ndev = (size_t)dev_rows * 3 * D, ncls = (size_t)n * D;
    const size_t osz = (size_t)a->out_rows * D * (arith == 0 ? 2 : 4);
    DevBufs B;
    float *q32, *c32 = nullptr;
    void* out;
    HIP_TRY(B.alloc(&q32, ndev * 4));
    HIP_TRY(hipMemset(q32, 0, ndev * 4));
    HIP_TRY(hipMemcpy(q32, a->qkv, nq * 4, hipMemcpyHostToDevice));
    if (a->q_cls) {
        HIP_TRY(B.alloc(&c32, (size_t)round_up(n, 256) * D * 4));
        HIP_TRY(hipMemset(c32, 0, (size_t)round_up(n, 256) * D * 4));
        HIP_TRY(hipMemcpy(c32, a->q_cls, ncls * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(B.alloc(&out, osz));
    HIP_TRY(hipMemcpy(out, a->out, osz, hipMemcpyHostToDevice));
    int rc = 0;
    if (arith == 0) {
        f16 *q16, *c16 = nullptr;
        HIP_TRY(B.alloc(&q16, ndev * 2));
        LAUNCH_TRY(launch_convert_f16(q32, q16, nullptr, (int64_t)ndev, 0));
        if (c32) {
            HIP_TRY(B.alloc(&c16, (size_t)round_up(n, 256) * D * 2));
            LAUNCH_TRY(launch_convert_f16(c32, c16, nullptr, (int64_t)round_up(n, 256) * D, 0));
        }
        rc = launch_attention(q16, c16, out, nullptr, 0, n, T, D, a->n_heads, 0);
    } else if (arith == 3) {
        rc = launch_attention_f32(q32, c32, (float*)out, n, T, D, a->n_heads, 0.f, 0);
    } else {
        float *qs, *cs = nullptr;
        HIP_TRY(B.alloc(&qs, ndev * 4));
        const int64_t t4 = dev_rows * (3 * D / 4);
        hipLaunchKernelGGL(pack_head_split_kernel, dim3((unsigned)((t4 + 255) / 256)), dim3(256), 0, 0, q32, qs, dev_rows, 3 * D, D);
        if (c32) {
            const int64_t crow = round_up(n, 256);
            HIP_TRY(B.alloc(&cs, (size_t)crow * D * 4));
            const int64_t c4 = crow * (D / 4);
            hipLaunchKernelGGL(pack_head_split_kernel, dim3((unsigned)((c4 + 255) / 256)), dim3(256), 0, 0, c32, cs, crow, D, D);
        }
        HIP_TRY(hipGetLastError());
        rc = launch_attention_f32(qs, cs, (float*)out, n, T, D, a->n_heads, 16.f, 0);    // the encoder's context scale (api_enc.hip)
    }
    if (rc) return cbas_fail(CBAS_EINVAL, "attention launch failed (arith %d, T %d: rc=%d)", arith, T, rc);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(a->out, out, osz, hipMemcpyDeviceToHost));
    return CBAS_OK;
}

// ---- tests: one launch of the CLS attention map kernel on host arrays ----
namespace {
// the first ncols columns (whole heads of 64) of rows of stride ld -> the head-split image at the same place, values x scale
__global__ void pack_heads_split_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t rows, int64_t ld, int ncols, float scale) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // one thread = 4 consecutive columns
    const int per_row = ncols / 4;
    if (i >= rows * per_row) return;
    const int64_t r = i / per_row;
    const int c = (int)(i - r * per_row) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + r * ld + c);
    f16x4v hi, lo;                                     // store_head_split4's values, each product and difference kept scalar (common.h)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float x = keep_scalar(v[e] * scale);
        const f16 h = (f16)x;
        hi[e] = h;
        lo[e] = (f16)keep_scalar(x - (float)h);
    }
    char* const head = reinterpret_cast<char*>(dst + r * ld + (c & ~63));
    *reinterpret_cast<f16x4v*>(head + (c & 63) * 2) = hi;
    *reinterpret_cast<f16x4v*>(head + 128 + (c & 63) * 2) = lo;
}
}  // namespace

extern "C" int cbas_debug_cls_attention(int arith, const float* q_host, const float* K_host, int n, int T, int NH, int n_prefix,
                                        int64_t ldq, int64_t ldk, float* heads_host, float* map_host) {
    if (arith != 0 && arith != 3 && arith != 4) return cbas_fail(CBAS_EINVAL, "arith %d", arith);
    if (!q_host || !K_host || (!heads_host && !map_host) || n <= 0 || T <= 0 || NH <= 0 || n_prefix <= 0 || n_prefix > T ||
        ldq < 64 * (int64_t)NH || ldk < 64 * (int64_t)NH || ldq % 8 || ldk % 8 || (int64_t)n * T * ldk > ((int64_t)1 << 30) ||
        (int64_t)n * ldq > ((int64_t)1 << 30))
        return cbas_fail(CBAS_EINVAL, "bad CLS attention test shape / pointers");
    const size_t nq = (size_t)n * ldq, nk = (size_t)n * T * ldk, nh = (size_t)n * NH * T, nm = (size_t)n * (T - n_prefix);
    DevBufs B;
    float *q32, *K32, *heads = nullptr, *map = nullptr;
    HIP_TRY(B.alloc(&q32, nq * 4));
    HIP_TRY(B.alloc(&K32, nk * 4));
    HIP_TRY(hipMemcpy(q32, q_host, nq * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(K32, K_host, nk * 4, hipMemcpyHostToDevice));
    if (heads_host) HIP_TRY(B.alloc(&heads, nh * 4));
    if (map_host) HIP_TRY(B.alloc(&map, nm * 4));
    int rc = 0;
    if (arith == 0) {
        f16 *q16, *K16;
        HIP_TRY(B.alloc(&q16, nq * 2));
        HIP_TRY(B.alloc(&K16, nk * 2));
        LAUNCH_TRY(launch_convert_f16(q32, q16, nullptr, (int64_t)nq, 0));
        LAUNCH_TRY(launch_convert_f16(K32, K16, nullptr, (int64_t)nk, 0));
        rc = launch_cls_attention<f16>(q16, ldq, K16, ldk, n, T, NH, n_prefix, 0, heads, map, 0);
    } else if (arith == 3) {
        rc = launch_cls_attention<float>(q32, ldq, K32, ldk, n, T, NH, n_prefix, 0, heads, map, 0);
    } else {
        float *qs, *Ks;
        HIP_TRY(B.alloc(&qs, nq * 4));
        HIP_TRY(B.alloc(&Ks, nk * 4));
        HIP_TRY(hipMemset(qs, 0, nq * 4));
        HIP_TRY(hipMemset(Ks, 0, nk * 4));
        const int64_t tq = (int64_t)n * NH * 16, tk = (int64_t)n * T * NH * 16;
        hipLaunchKernelGGL(pack_heads_split_kernel, dim3((unsigned)((tq + 255) / 256)), dim3(256), 0, 0, q32, qs, (int64_t)n, ldq, NH * 64, ATT_QS);
        hipLaunchKernelGGL(pack_heads_split_kernel, dim3((unsigned)((tk + 255) / 256)), dim3(256), 0, 0, K32, Ks, (int64_t)n * T, ldk, NH * 64, ATT_KS);
        HIP_TRY(hipGetLastError());
        rc = launch_cls_attention<float>(qs, ldq, Ks, ldk, n, T, NH, n_prefix, 1, heads, map, 0);
    }
    if (rc) return cbas_fail(CBAS_EINVAL, "CLS attention launch failed (arith %d, T %d: rc=%d)", arith, T, rc);
    HIP_TRY(hipDeviceSynchronize());
    if (heads_host) HIP_TRY(hipMemcpy(heads_host, heads, nh * 4, hipMemcpyDeviceToHost));
    if (map_host && nm) HIP_TRY(hipMemcpy(map_host, map, nm * 4, hipMemcpyDeviceToHost));
    return CBAS_OK;
}

// ---- tests: one launch of the head-mean attention kernel / of the rollout chain step (attention_rollout.hip) on host arrays ----
extern "C" int cbas_debug_attention_mean(int arith, const float* q_host, const float* K_host, int n, int T, int NH, int64_t ldq, int64_t ldk,
                                         int blend, float* out_host) {
    if (arith != 0 && arith != 3 && arith != 4) return cbas_fail(CBAS_EINVAL, "arith %d", arith);
    if (!q_host || !K_host || !out_host || n <= 0 || T <= 0 || NH <= 0 || ldq < 64 * (int64_t)NH || ldk < 64 * (int64_t)NH || ldq % 8 || ldk % 8 ||
        (int64_t)n * T * ldk > ((int64_t)1 << 30) || (int64_t)n * T * ldq > ((int64_t)1 << 30) || (int64_t)n * T * T > ((int64_t)1 << 30))
        return cbas_fail(CBAS_EINVAL, "bad attention-mean test shape / pointers");
    if (!attention_mean_rows_per_block(T))
        return cbas_fail(CBAS_EINVAL, "T = %d: one query row's scores and sums (64 + 2 T floats) do not fit 64 KiB of LDS", T);
    const size_t nq = (size_t)n * T * ldq, nk = (size_t)n * T * ldk, no = (size_t)n * T * T;
    DevBufs B;
    float *q32, *K32, *out;
    HIP_TRY(B.alloc(&q32, nq * 4));
    HIP_TRY(B.alloc(&K32, nk * 4));
    HIP_TRY(B.alloc(&out, no * 4));
    HIP_TRY(hipMemcpy(q32, q_host, nq * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(K32, K_host, nk * 4, hipMemcpyHostToDevice));
    int rc = 0;
    if (arith == 0) {
        f16 *q16, *K16;
        HIP_TRY(B.alloc(&q16, nq * 2));
        HIP_TRY(B.alloc(&K16, nk * 2));
        LAUNCH_TRY(launch_convert_f16(q32, q16, nullptr, (int64_t)nq, 0));
        LAUNCH_TRY(launch_convert_f16(K32, K16, nullptr, (int64_t)nk, 0));
        rc = launch_attention_mean<f16>(q16, ldq, K16, ldk, n, T, NH, 0, blend, out, 0);
    } else if (arith == 3) {
        rc = launch_attention_mean<float>(q32, ldq, K32, ldk, n, T, NH, 0, blend, out, 0);
    } else {
        float *qs, *Ks;
        HIP_TRY(B.alloc(&qs, nq * 4));
        HIP_TRY(B.alloc(&Ks, nk * 4));
        HIP_TRY(hipMemset(qs, 0, nq * 4));
        HIP_TRY(hipMemset(Ks, 0, nk * 4));
        const int64_t tq = (int64_t)n * T * NH * 16;
        hipLaunchKernelGGL(pack_heads_split_kernel, dim3((unsigned)((tq + 255) / 256)), dim3(256), 0, 0, q32, qs, (int64_t)n * T, ldq, NH * 64, ATT_QS);
        hipLaunchKernelGGL(pack_heads_split_kernel, dim3((unsigned)((tq + 255) / 256)), dim3(256), 0, 0, K32, Ks, (int64_t)n * T, ldk, NH * 64, ATT_KS);
        HIP_TRY(hipGetLastError());
        rc = launch_attention_mean<float>(qs, ldq, Ks, ldk, n, T, NH, 1, blend, out, 0);
    }
    if (rc) return cbas_fail(CBAS_EINVAL, "attention-mean launch failed (arith %d, T %d: rc=%d)", arith, T, rc);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_host, out, no * 4, hipMemcpyDeviceToHost));
    return CBAS_OK;
}

extern "C" int cbas_debug_rollout_step(const float* A_host, const float* R_host, int n, int T, float* out_host) {
    if (!A_host || !R_host || !out_host || n <= 0 || T <= 0 || (int64_t)n * T * T > ((int64_t)1 << 28))
        return cbas_fail(CBAS_EINVAL, "bad rollout-step test shape / pointers");
    const size_t no = (size_t)n * T * T;
    DevBufs B;
    float *A, *R, *out;
    HIP_TRY(B.alloc(&A, no * 4));
    HIP_TRY(B.alloc(&R, no * 4));
    HIP_TRY(B.alloc(&out, no * 4));
    HIP_TRY(hipMemcpy(A, A_host, no * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(R, R_host, no * 4, hipMemcpyHostToDevice));
    const int rc = launch_rollout_step(A, R, out, n, T, 0);
    if (rc) return cbas_fail(CBAS_EINVAL, "rollout-step launch failed (T %d: rc=%d)", T, rc);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_host, out, no * 4, hipMemcpyDeviceToHost));
    return CBAS_OK;
}

// ---- tests: one launch of a row-wise kernel (LayerNorm forms, the MX-fp8 row, the ConvNeXt producers) on host operands ----
extern "C" int cbas_debug_rows_run(const cbas_debug_rows_args* a) {
    if (!a || a->struct_bytes != (int64_t)sizeof(cbas_debug_rows_args))
        return cbas_fail(CBAS_EINVAL, "cbas_debug_rows_args: struct_bytes %lld, library expects %lld", a ? (long long)a->struct_bytes : -1ll,
                         (long long)sizeof(cbas_debug_rows_args));
    const int op = a->op, D = a->D, M = a->M, n = a->n, h = a->h, w = a->w;
    const int64_t ld = a->ld;
    const bool vit_ln = op >= CBAS_DEBUG_ROWS_LN_F16 && op <= CBAS_DEBUG_ROWS_LN_F8;
    const bool cls = op == CBAS_DEBUG_ROWS_FINAL_CLS || op == CBAS_DEBUG_ROWS_CNX_POOL_LN;
    const bool stem = op == CBAS_DEBUG_ROWS_CNX_STEM_U8 || op == CBAS_DEBUG_ROWS_CNX_STEM_F32;
    const bool cnx = op >= CBAS_DEBUG_ROWS_CNX_LN_ROWS && op <= CBAS_DEBUG_ROWS_CNX_POOL_LN;
    const bool tok_rows = op == CBAS_DEBUG_ROWS_TOKEN_ROWS, tok_cnx = tok_rows && (h || w), tok_sim = op == CBAS_DEBUG_ROWS_TOKEN_SIM;
    if (op < CBAS_DEBUG_ROWS_LN_F16 || op > CBAS_DEBUG_ROWS_TOKEN_SIM) return cbas_fail(CBAS_EINVAL, "op %d", op);
    // what the launch reads (x_need) and writes (out_need, out2_need), in bytes: the images must hold it
    int64_t x_need = 0, out_need = 0, out2_need = 0;
    if (!stem) {
        if (D <= 0 || D % 4 || (!tok_sim && (!a->gamma || !a->beta))) return cbas_fail(CBAS_EINVAL, "D = %d: a positive multiple of 4; gamma / beta", D);
        if ((vit_ln || op == CBAS_DEBUG_ROWS_FINAL_CLS || (tok_rows && !tok_cnx)) && D > 1280) return cbas_fail(CBAS_EINVAL, "D = %d: the ViT LayerNorms stop at 1280", D);
        if (op == CBAS_DEBUG_ROWS_LN_SPLIT && D % 32) return cbas_fail(CBAS_EINVAL, "LN_SPLIT: D %% 32");
        if (op == CBAS_DEBUG_ROWS_LN_F8 && (D % 128 || D < 256 || D > 1024)) return cbas_fail(CBAS_EINVAL, "LN_F8: D = 256 .. 1024 in steps of 128");
        if ((cnx || tok_cnx) && (D % 32 || D > 1536)) return cbas_fail(CBAS_EINVAL, "ConvNeXt width %d: a multiple of 32 up to 1536", D);
    }
    if (tok_rows || tok_sim) {
        // TOKEN_ROWS: sc_ld = the output images' row stride; TOKEN_SIM: M = the prefix rows P0, wt = int32 query indices or NULL
        const int64_t rows = tok_sim ? (int64_t)n * a->T : tok_cnx ? (int64_t)n * ((int64_t)h * w + 1) : M;
        const int64_t rows_in = tok_cnx ? (int64_t)n * h * w : rows;
        if (ld < D || ld % 4) return cbas_fail(CBAS_EINVAL, "ld = %lld: at least D and a multiple of 4", (long long)ld);
        if (tok_sim ? (n <= 0 || a->T <= 0 || M < 0 || M >= a->T) : tok_cnx ? (n <= 0 || h <= 0 || w <= 0) : M <= 0)
            return cbas_fail(CBAS_EINVAL, "token op %d: n = %d, M = %d, T = %d, grid %d x %d", op, n, M, a->T, h, w);
        x_need = ((rows_in - 1) * ld + D) * 4;
        if (tok_sim) {
            out_need = (int64_t)n * (a->T - M) * 4;
        } else {
            if (a->sc_ld < D || a->sc_ld % 4) return cbas_fail(CBAS_EINVAL, "sc_ld (output row stride) = %d: at least D and a multiple of 4", a->sc_ld);
            if (!a->out && !a->out2) return cbas_fail(CBAS_EINVAL, "out (fp32) and out2 (fp16) both NULL");
            out_need = a->out ? ((rows - 1) * a->sc_ld + D) * 4 : 0;
            out2_need = a->out2 ? ((rows - 1) * a->sc_ld + D) * 2 : 0;
        }
    } else if (vit_ln || op == CBAS_DEBUG_ROWS_CNX_LN_ROWS) {
        if (M <= 0 || ld < D) return cbas_fail(CBAS_EINVAL, "M = %d, ld = %lld: M > 0 and ld >= D", M, (long long)ld);
        const int64_t span = ((int64_t)(M - 1) * ld + D) * 4;
        if (vit_ln) x_need = span; else out_need = span;
        if (op == CBAS_DEBUG_ROWS_LN_F16) out_need = (int64_t)M * D * 2;
        if (op == CBAS_DEBUG_ROWS_LN_F32 || op == CBAS_DEBUG_ROWS_LN_SPLIT) out_need = (int64_t)M * D * 4;
        if (op == CBAS_DEBUG_ROWS_LN_F8) {
            if (a->sc_ld < M) return cbas_fail(CBAS_EINVAL, "sc_ld %d < M %d", a->sc_ld, M);
            out_need = (int64_t)M * D;
            out2_need = (int64_t)(D / 128) * a->sc_ld * 4;
        }
    } else {
        if (n <= 0) return cbas_fail(CBAS_EINVAL, "n = %d", n);
        if (op == CBAS_DEBUG_ROWS_FINAL_CLS) {
            if (a->T <= 0) return cbas_fail(CBAS_EINVAL, "T = %d", a->T);
            x_need = ((int64_t)(n - 1) * a->T * D + D) * 4;
        } else if (stem) {
            if (h < 4 || w < 4) return cbas_fail(CBAS_EINVAL, "stem: a %d x %d frame is smaller than one 4 x 4 patch", h, w);
            const int ho = h / 4, wo = w / 4;
            if (op == CBAS_DEBUG_ROWS_CNX_STEM_U8) {
                if (a->frame_stride <= 0 || a->row_stride <= 0 || a->pixel_stride <= 0) return cbas_fail(CBAS_EINVAL, "stem: strides must be positive");
                x_need = (int64_t)(n - 1) * a->frame_stride + (int64_t)(4 * ho - 1) * a->row_stride + (int64_t)(4 * wo - 1) * a->pixel_stride + 1;
            } else {
                x_need = (int64_t)n * h * w * 4;
            }
            out_need = (int64_t)n * ho * wo * 32 * 4;
        } else {
            if (h <= 0 || w <= 0 || ld < D) return cbas_fail(CBAS_EINVAL, "grid %d x %d, ld = %lld: positive, ld >= C", h, w, (long long)ld);
            x_need = (((int64_t)n * h * w - 1) * ld + D) * 4;
            if (op == CBAS_DEBUG_ROWS_CNX_DOWNSAMPLE) {
                if (h < 2 || w < 2) return cbas_fail(CBAS_EINVAL, "downsample: a %d x %d grid has no 2 x 2 window", h, w);
                out_need = (int64_t)n * (h / 2) * (w / 2) * 4 * D * 4;
            } else if (op == CBAS_DEBUG_ROWS_CNX_DWCONV_LN) {
                if (!a->wt || !a->bias) return cbas_fail(CBAS_EINVAL, "dwconv: wt / bias");
                out_need = (int64_t)n * h * w * D * 4;
            }
        }
        if (cls) {
            if (!a->out && !a->out2) return cbas_fail(CBAS_EINVAL, "cls_f32 and cls_f16 both NULL");
            out_need = a->out ? (int64_t)n * D * 4 : 0;
            out2_need = a->out2 ? (int64_t)n * D * 2 : 0;
        }
    }
    if ((x_need && (!a->x || a->x_bytes < x_need)) || (out_need && (!a->out || a->out_bytes < out_need)) ||
        (out2_need && (!a->out2 || a->out2_bytes < out2_need)))
        return cbas_fail(CBAS_EINVAL, "op %d: an image is missing or too small (x %lld of %lld, out %lld of %lld, out2 %lld of %lld bytes)", op,
                         (long long)a->x_bytes, (long long)x_need, (long long)a->out_bytes, (long long)out_need, (long long)a->out2_bytes,
                         (long long)out2_need);
    DevBufs B;
    char *x = nullptr, *out = nullptr, *out2 = nullptr;
    float *gamma = nullptr, *beta = nullptr, *wt = nullptr, *bias = nullptr;
    unsigned* counter = nullptr;
    const auto upload = [&B](auto** dev, const void* host, size_t bytes) -> hipError_t {
        const hipError_t e = B.alloc(dev, bytes);
        return e != hipSuccess ? e : hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice);
    };
    if (x_need) HIP_TRY(upload(&x, a->x, (size_t)a->x_bytes));
    if (out_need) HIP_TRY(upload(&out, a->out, (size_t)a->out_bytes));
    if (out2_need) HIP_TRY(upload(&out2, a->out2, (size_t)a->out2_bytes));
    if (!stem && !tok_sim) {
        HIP_TRY(upload(&gamma, a->gamma, (size_t)D * 4));
        HIP_TRY(upload(&beta, a->beta, (size_t)D * 4));
    }
    int* query = nullptr;
    f16* x16 = nullptr;
    if (tok_sim && a->wt) HIP_TRY(upload(&query, a->wt, (size_t)n * 4));
    if (tok_sim && a->split) {                                       // the fp16 form reads the same image converted (RNE)
        HIP_TRY(B.alloc(&x16, (size_t)a->x_bytes / 2));
        LAUNCH_TRY(launch_convert_f16(reinterpret_cast<const float*>(x), x16, nullptr, a->x_bytes / 4, 0));
    }
    if (op == CBAS_DEBUG_ROWS_CNX_DWCONV_LN) {
        HIP_TRY(upload(&wt, a->wt, (size_t)49 * D * 4));
        HIP_TRY(upload(&bias, a->bias, (size_t)D * 4));
    }
    if ((cls || tok_rows) && a->counter) HIP_TRY(upload(&counter, a->counter, 4));
    const float* xf = reinterpret_cast<const float*>(x);
    float* of = reinterpret_cast<float*>(out);
    const float eps = a->eps;
    const int split = a->split ? 1 : 0;
    int rc = -1;
    switch (op) {
        case CBAS_DEBUG_ROWS_LN_F16: rc = launch_layernorm_f16(xf, ld, gamma, beta, (f16*)out, M, D, eps, 0); break;
        case CBAS_DEBUG_ROWS_LN_F32: rc = launch_layernorm_f32(xf, ld, gamma, beta, of, M, D, eps, 0, 0); break;
        case CBAS_DEBUG_ROWS_LN_SPLIT: rc = launch_layernorm_f32(xf, ld, gamma, beta, of, M, D, eps, 1, 0); break;
        case CBAS_DEBUG_ROWS_LN_F8: rc = launch_layernorm_f8(xf, ld, gamma, beta, (uint8_t*)out, (uint32_t*)out2, a->sc_ld, M, D, eps, 0); break;
        case CBAS_DEBUG_ROWS_FINAL_CLS: rc = launch_final_norm_cls(xf, gamma, beta, of, (f16*)out2, n, a->T, D, eps, 0, counter); break;
        case CBAS_DEBUG_ROWS_CNX_STEM_U8:
            rc = launch_cnx_stem_im2col_u8((const uint8_t*)x, n, h, w, a->frame_stride, a->row_stride, a->pixel_stride, of, split, 0);
            break;
        case CBAS_DEBUG_ROWS_CNX_STEM_F32: rc = launch_cnx_stem_im2col_f32(xf, n, h, w, of, split, 0); break;
        case CBAS_DEBUG_ROWS_CNX_LN_ROWS: rc = launch_cnx_ln_rows(of, ld, gamma, beta, M, D, eps, 0); break;
        case CBAS_DEBUG_ROWS_CNX_DOWNSAMPLE: rc = launch_cnx_downsample(xf, ld, n, h, w, gamma, beta, D, eps, of, split, 0); break;
        case CBAS_DEBUG_ROWS_CNX_DWCONV_LN: rc = launch_cnx_dwconv_ln(xf, ld, n, h, w, wt, bias, gamma, beta, D, eps, of, split, 0); break;
        case CBAS_DEBUG_ROWS_CNX_POOL_LN: rc = launch_cnx_pool_ln(xf, ld, n, h * w, gamma, beta, D, eps, of, (f16*)out2, counter, 0); break;
        case CBAS_DEBUG_ROWS_TOKEN_ROWS:
            rc = tok_cnx ? launch_cnx_token_rows(xf, ld, n, h * w, gamma, beta, D, eps, of, (f16*)out2, a->sc_ld, counter, 0)
                         : launch_final_norm_rows(xf, ld, gamma, beta, of, (f16*)out2, a->sc_ld, M, D, eps, counter, 0);
            break;
        case CBAS_DEBUG_ROWS_TOKEN_SIM:
            rc = x16 ? launch_token_similarity<f16>(x16, ld, n, a->T, D, M, query, of, 0)
                     : launch_token_similarity<float>(xf, ld, n, a->T, D, M, query, of, 0);
            break;
    }
    if (rc) return cbas_fail(CBAS_EINVAL, "row kernel launch failed (op %d, D %d: rc=%d)", op, D, rc);
    HIP_TRY(hipDeviceSynchronize());
    if (out_need) HIP_TRY(hipMemcpy(a->out, out, (size_t)a->out_bytes, hipMemcpyDeviceToHost));
    if (out2_need) HIP_TRY(hipMemcpy(a->out2, out2, (size_t)a->out2_bytes, hipMemcpyDeviceToHost));
    if (counter) HIP_TRY(hipMemcpy(a->counter, counter, 4, hipMemcpyDeviceToHost));
    return CBAS_OK;
}

// ---- tests: one launch of a ViT ingest kernel or a create-time weight packer on host operands ----
extern "C" int cbas_debug_pack_run(const cbas_debug_pack_args* a) {
    if (!a || a->struct_bytes != (int64_t)sizeof(cbas_debug_pack_args))
        return cbas_fail(CBAS_EINVAL, "cbas_debug_pack_args: struct_bytes %lld, library expects %lld", a ? (long long)a->struct_bytes : -1ll,
                         (long long)sizeof(cbas_debug_pack_args));
    const int op = a->op, n = a->n, h = a->h, w = a->w, ps = a->ps, D = a->D, K = a->K, NP = a->n_prefix;
    const int64_t N = a->N, F = a->F;
    if (op < CBAS_DEBUG_PACK_IM2COL_U8 || op > CBAS_DEBUG_PACK_FP8_W) return cbas_fail(CBAS_EINVAL, "op %d", op);
    const bool im2col = op <= CBAS_DEBUG_PACK_IM2COL_F32_F32;
    const bool u8 = op == CBAS_DEBUG_PACK_IM2COL_U8 || op == CBAS_DEBUG_PACK_IM2COL_U8_F32;
    const bool patch_w = op == CBAS_DEBUG_PACK_PATCH_W || op == CBAS_DEBUG_PACK_PATCH_W_F32;
    // what the launch reads (in_need) and writes (out_need), in bytes: the images must hold it.  A product that leaves int64
    // is a size no image holds.
    bool ovf = false;
    const auto mul = [&ovf](int64_t x, int64_t y) { int64_t r = 0; if (__builtin_mul_overflow(x, y, &r)) ovf = true; return r; };
    const auto add = [&ovf](int64_t x, int64_t y) { int64_t r = 0; if (__builtin_add_overflow(x, y, &r)) ovf = true; return r; };
    int64_t in_need[2] = {0, 0}, out_need[4] = {0, 0, 0, 0};
    bool out_opt[4] = {false, false, false, false};
    if (im2col || patch_w) {
        if (ps != 14 && ps != 16) return cbas_fail(CBAS_EINVAL, "ps = %d: 14 or 16", ps);
        if (D <= 0) return cbas_fail(CBAS_EINVAL, "D = %d", D);
    }
    if (im2col) {
        if (n <= 0 || h < ps || w < ps) return cbas_fail(CBAS_EINVAL, "%d frames of %d x %d: n > 0 and at least one %d x %d patch", n, h, w, ps, ps);
        if (NP < 1 || D % 4) return cbas_fail(CBAS_EINVAL, "n_prefix = %d, D = %d: n_prefix >= 1, D a multiple of 4", NP, D);
        const int nh = h / ps, nw = w / ps;
        const int64_t P = (int64_t)nh * nw, T = P + NP;
        if (mul(n, T) > 0x7fffffff) return cbas_fail(CBAS_EINVAL, "%d frames of %lld rows: beyond 2^31 - 1 rows", n, (long long)T);
        if (u8) {
            if (a->frame_stride <= 0 || a->row_stride <= 0 || a->pixel_stride <= 0) return cbas_fail(CBAS_EINVAL, "strides must be positive");
            in_need[0] = add(add(mul(n - 1, a->frame_stride), mul(nh * ps - 1, a->row_stride)), add(mul(nw * ps - 1, a->pixel_stride), 1));
        } else {
            in_need[0] = mul(mul(n, h), mul(w, 4));
        }
        in_need[1] = mul(mul(NP, D), 4);
        out_need[0] = mul(mul(n, P), op == CBAS_DEBUG_PACK_IM2COL_U8 ? 256 * 2 : 256 * 4);      // 256 fp16; 512 fp16 = 256 f32 slots
        out_need[1] = mul(mul(n, T), mul(D, 4));
    } else if (patch_w) {
        if (D > (1 << 22)) return cbas_fail(CBAS_EINVAL, "D = %d: the packer indexes D * 512 elements in 32 bits", D);
        in_need[0] = (int64_t)D * 3 * ps * ps * 4;
        if (op == CBAS_DEBUG_PACK_PATCH_W) {
            if ((a->out[1] == nullptr) != (a->out[3] == nullptr)) return cbas_fail(CBAS_EINVAL, "PATCH_W: lo and lo2 are NULL together or not at all");
            out_need[0] = out_need[1] = (int64_t)D * 256 * 2;
            out_need[2] = out_need[3] = (int64_t)D * 512 * 2;
            out_opt[1] = out_opt[3] = true;
        } else {
            out_need[0] = (int64_t)D * 256 * 4;
        }
    } else if (op == CBAS_DEBUG_PACK_SPLIT_W) {
        if (N <= 0 || K <= 0 || K % 32) return cbas_fail(CBAS_EINVAL, "SPLIT_W: N = %lld, K = %d: N > 0, K a positive multiple of 32", (long long)N, K);
        in_need[0] = out_need[0] = mul(mul(N, K), 4);
    } else if (op == CBAS_DEBUG_PACK_CONVERT_F16) {
        if (N <= 0) return cbas_fail(CBAS_EINVAL, "CONVERT_F16: N = %lld", (long long)N);
        in_need[0] = mul(N, 4);
        out_need[0] = out_need[1] = mul(N, 2);
        out_opt[1] = true;
    } else if (op == CBAS_DEBUG_PACK_INTERLEAVE) {
        if (F <= 0 || F % 32 || K <= 0) return cbas_fail(CBAS_EINVAL, "INTERLEAVE: F = %lld, K = %d: F a positive multiple of 32, K > 0", (long long)F, K);
        in_need[0] = in_need[1] = mul(mul(F, K), 4);
        out_need[0] = mul(in_need[0], 2);
    } else {
        if (N <= 0 || N > 0x7fffffff || K <= 0 || K % 128) return cbas_fail(CBAS_EINVAL, "FP8_W: N = %lld, K = %d: N > 0, K a positive multiple of 128", (long long)N, K);
        if (a->n0 < 0 || a->n0 + N > a->n_total) return cbas_fail(CBAS_EINVAL, "FP8_W: columns %d .. %lld of %d", a->n0, (long long)(a->n0 + N), a->n_total);
        in_need[0] = mul(mul(N, K), 4);
        out_need[0] = mul(N, K);
        out_need[1] = mul(mul(K / 128, a->n_total), 4);
    }
    if (ovf) return cbas_fail(CBAS_EINVAL, "op %d: a size or stride leaves 64 bits", op);
    for (int i = 0; i < 2; ++i)
        if (in_need[i] && (!a->in[i] || a->in_bytes[i] < in_need[i]))
            return cbas_fail(CBAS_EINVAL, "op %d: in[%d] is missing or too small (%lld of %lld bytes)", op, i, (long long)a->in_bytes[i], (long long)in_need[i]);
    for (int i = 0; i < 4; ++i) {
        if (!out_need[i]) continue;
        if (!a->out[i] ? !out_opt[i] : a->out_bytes[i] < out_need[i])
            return cbas_fail(CBAS_EINVAL, "op %d: out[%d] is missing or too small (%lld of %lld bytes)", op, i, (long long)a->out_bytes[i], (long long)out_need[i]);
    }
    DevBufs B;
    char *in[2] = {nullptr, nullptr}, *out[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 2; ++i)
        if (in_need[i]) {
            HIP_TRY(B.alloc(&in[i], (size_t)a->in_bytes[i]));
            HIP_TRY(hipMemcpy(in[i], a->in[i], (size_t)a->in_bytes[i], hipMemcpyHostToDevice));
        }
    for (int i = 0; i < 4; ++i)
        if (out_need[i] && a->out[i]) {
            HIP_TRY(B.alloc(&out[i], (size_t)a->out_bytes[i]));
            HIP_TRY(hipMemcpy(out[i], a->out[i], (size_t)a->out_bytes[i], hipMemcpyHostToDevice));
        }
    const float* in0 = reinterpret_cast<const float*>(in[0]);
    const float* in1 = reinterpret_cast<const float*>(in[1]);
    float* x = reinterpret_cast<float*>(out[1]);
    const int T = im2col ? (h / ps) * (w / ps) + NP : 0;
    const int split = a->split ? 1 : 0;
    int rc = -1;
    switch (op) {
        case CBAS_DEBUG_PACK_IM2COL_U8:
            rc = launch_im2col_u8((const uint8_t*)in[0], n, h, w, a->frame_stride, a->row_stride, a->pixel_stride, (f16*)out[0], x, in1, NP, D, T, ps, 0);
            break;
        case CBAS_DEBUG_PACK_IM2COL_F32: rc = launch_im2col_f32(in0, n, h, w, (f16*)out[0], x, in1, NP, D, T, ps, 0); break;
        case CBAS_DEBUG_PACK_IM2COL_U8_F32:
            rc = launch_im2col_u8_f32((const uint8_t*)in[0], n, h, w, a->frame_stride, a->row_stride, a->pixel_stride, (float*)out[0], x, in1, NP, D, T,
                                      ps, split, 0);
            break;
        case CBAS_DEBUG_PACK_IM2COL_F32_F32: rc = launch_im2col_f32_f32(in0, n, h, w, (float*)out[0], x, in1, NP, D, T, ps, split, 0); break;
        case CBAS_DEBUG_PACK_PATCH_W: rc = launch_pack_patch_weight(in0, (f16*)out[0], (f16*)out[1], (f16*)out[2], (f16*)out[3], D, ps, 0); break;
        case CBAS_DEBUG_PACK_PATCH_W_F32: rc = launch_pack_patch_weight_f32(in0, (float*)out[0], D, ps, 0); break;
        case CBAS_DEBUG_PACK_SPLIT_W: rc = launch_pack_split_weight(in0, (float*)out[0], N, K, a->scale, 0); break;
        case CBAS_DEBUG_PACK_CONVERT_F16: rc = launch_convert_f16(in0, (f16*)out[0], (f16*)out[1], N, 0); break;
        case CBAS_DEBUG_PACK_INTERLEAVE: rc = launch_interleave_gate_up(in0, in1, (float*)out[0], F, K, 0); break;
        case CBAS_DEBUG_PACK_FP8_W: rc = launch_pack_fp8_weight(in0, (uint8_t*)out[0], (uint32_t*)out[1], (int)N, K, a->n_total, a->n0, 0); break;
    }
    if (rc) return cbas_fail(rc == -1 ? CBAS_EINVAL : CBAS_EHIP, "pack launch failed (op %d: rc=%d)", op, rc);
    HIP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < 4; ++i)
        if (out[i]) HIP_TRY(hipMemcpy(a->out[i], out[i], (size_t)a->out_bytes[i], hipMemcpyDeviceToHost));
    return CBAS_OK;
}

// ---- tests: one launch of a classifier-head kernel (the exact-fp32 GEMM, the small training kernels) on host operands ----
namespace {
struct HeadNeed { int64_t in[4] = {0, 0, 0, 0}, out[3] = {0, 0, 0}; bool in_opt[4] = {false, false, false, false}; };

// bytes entry e's launch reads (in) and writes (out); returns a message for a shape the launcher would mis-handle
const char* head_entry_need(int op, bool multi, const cbas_debug_head_entry& e, HeadNeed* nd) {
    const int64_t n = e.n;
    if (n < (multi ? 0 : 1)) return "n below 1 (a trial-batched entry: below 0)";
    if (n > 0x7fffffff) return "n beyond 2^31 - 1";
    switch (op) {
        case CBAS_DEBUG_HEAD_TRANSPOSE_PAD:
            if (e.cols < 1 || e.ld < e.cols || e.rows_pad < n) return "transpose_pad: cols >= 1, ld >= cols, rows_pad >= rows";
            nd->in[0] = ((n - 1) * e.ld + e.cols) * 4;
            nd->out[0] = (int64_t)e.cols * e.rows_pad * 4;
            break;
        case CBAS_DEBUG_HEAD_GELU_DROPOUT_FWD:
        case CBAS_DEBUG_HEAD_GELU_DROPOUT_BWD:
            if (e.thr > (1u << 24)) return "thr beyond 2^24";
            nd->in[0] = n * 4; nd->out[0] = n * 4;
            break;
        case CBAS_DEBUG_HEAD_CE_TERMS:
        case CBAS_DEBUG_HEAD_CE_GRAD:
            if (e.C < 1 || e.C > 64) return "C outside 1 .. 64";
            nd->in[0] = n * e.C * 4; nd->in[1] = n * 4; nd->in[2] = (int64_t)e.C * 4; nd->in_opt[2] = true;
            if (op == CBAS_DEBUG_HEAD_CE_GRAD) { nd->in[3] = 8; nd->out[0] = n * e.C * 4; }
            else nd->out[0] = n * 8;
            break;
        case CBAS_DEBUG_HEAD_COV_OFFDIAG:
            if (n > 4096) return "cov_offdiag: n beyond 4096";
            nd->in[0] = n * n * 4; nd->out[0] = n * n * 4; nd->out[1] = n * 4;
            break;
        case CBAS_DEBUG_HEAD_SUB_COLMEAN:
            if (e.cols < 1) return "sub_colmean: cols >= 1";
            nd->in[0] = n * e.cols * 4; nd->in[1] = (int64_t)e.cols * 4; nd->out[0] = n * e.cols * 4;
            break;
        case CBAS_DEBUG_HEAD_COLSUM:
            if (e.cols < (multi ? 0 : 1) || e.ld < e.cols) return "colsum: cols >= 1 (trial-batched: >= 0), ld >= cols";
            if (multi && e.scale != 1.0f) return "the trial-batched column sum has no scale";
            if (multi && e.cols > 0 && n < 1) return "colsum: rows >= 1";
            nd->in[0] = n > 0 && e.cols > 0 ? ((n - 1) * e.ld + e.cols) * 4 : 0;
            nd->out[0] = (int64_t)COLSUM_CHUNKS * e.cols * 4; nd->out[1] = (int64_t)e.cols * 4;
            break;
        case CBAS_DEBUG_HEAD_ADD_VEC:
            nd->in[0] = n * 4; nd->in[1] = n * 4; nd->in_opt[1] = true; nd->out[0] = n * 4;
            break;
        case CBAS_DEBUG_HEAD_ADAM:
            if (e.step < 1) return "adam: step >= 1";
            nd->in[0] = n * 4; nd->out[0] = nd->out[1] = nd->out[2] = n * 4;
            break;
        default: return "op";
    }
    return nullptr;
}
}  // namespace

extern "C" int cbas_debug_head_run(const cbas_debug_head_args* a) {
    if (!a || a->struct_bytes != (int64_t)sizeof(cbas_debug_head_args) || a->entry_bytes != (int64_t)sizeof(cbas_debug_head_entry))
        return cbas_fail(CBAS_EINVAL, "cbas_debug_head_args: struct_bytes %lld / entry_bytes %lld, library expects %lld / %lld",
                         a ? (long long)a->struct_bytes : -1ll, a ? (long long)a->entry_bytes : -1ll, (long long)sizeof(cbas_debug_head_args),
                         (long long)sizeof(cbas_debug_head_entry));
    const int op = a->op, k = a->k;
    const bool multi = a->multi != 0;
    if (op < CBAS_DEBUG_HEAD_GEMM || op > CBAS_DEBUG_HEAD_ADAM) return cbas_fail(CBAS_EINVAL, "op %d", op);
    if (k < 1 || k > TRAIN_MULTI_MAX || !a->entries) return cbas_fail(CBAS_EINVAL, "k = %d: 1 .. %d entries", k, TRAIN_MULTI_MAX);
    if (multi && (op == CBAS_DEBUG_HEAD_GEMM || op == CBAS_DEBUG_HEAD_TRANSPOSE_PAD || op == CBAS_DEBUG_HEAD_SUB_COLMEAN))
        return cbas_fail(CBAS_EINVAL, "op %d has no trial-batched launcher", op);
    const int ne = multi ? k : 1;
    const cbas_debug_head_entry* E = a->entries;
    HeadNeed need[TRAIN_MULTI_MAX];
    Gemm32Params g{};
    const bool gemm = op == CBAS_DEBUG_HEAD_GEMM;
    const int splits = a->splits > 1 ? a->splits : 1;
    if (gemm) {
        const int64_t ldw = a->ldw ? a->ldw : a->K, Kt = (int64_t)a->K * splits;
        g.lda = a->lda; g.ldo = a->ldo; g.M = a->M; g.N = a->N; g.N_alloc = a->N_alloc; g.K = a->K; g.ldw = a->ldw;
        g.splits = a->splits; g.split_stride = a->split_stride;
        // launch_gemm_f32's own refusals, before anything is allocated, and what it does not check
        if (a->M <= 0 || a->M > (1 << 24) || a->N <= 0 || a->N % 4 || a->K < 32 || a->K % 32 || a->N_alloc < a->N || a->lda % 4 || a->ldo % 4 || a->ldw % 4 ||
            a->splits < 0 || a->splits > 64 || (a->gelu != 0 && a->gelu != 1))
            return cbas_fail(CBAS_EINVAL, "GEMM: M > 0, N %% 4, K a positive multiple of 32, N_alloc >= N, lda / ldo / ldw %% 4, splits 0 .. 64, gelu 0 / 1");
        if (a->lda < Kt || ldw < Kt || a->ldo < a->N) return cbas_fail(CBAS_EINVAL, "GEMM: lda / ldw below the k range read, or ldo < N");
        if (splits > 1 && (E[0].in[2] || a->gelu || a->split_stride % 4 || a->ldo != a->N || a->split_stride < a->M * a->N))
            return cbas_fail(CBAS_EINVAL, "split-K: no bias, no GELU, ldo = N, split_stride %% 4 == 0 and >= M N");
        need[0].in[0] = ((a->M - 1) * a->lda + Kt) * 4;
        need[0].in[1] = ((int64_t)(a->N_alloc - 1) * ldw + Kt) * 4;
        need[0].in[2] = (int64_t)a->N * 4; need[0].in_opt[2] = true;
        need[0].out[0] = ((a->M - 1) * a->ldo + a->N) * 4;
        if (splits > 1) need[0].out[1] = ((splits - 1) * a->split_stride + a->M * a->N) * 4;
    } else {
        for (int j = 0; j < ne; ++j) {
            const char* msg = head_entry_need(op, multi, E[j], &need[j]);
            if (msg) return cbas_fail(CBAS_EINVAL, "op %d entry %d: %s", op, j, msg);
            if (op == CBAS_DEBUG_HEAD_ADAM && E[j].wd_special != E[0].wd_special) return cbas_fail(CBAS_EINVAL, "adam: one wd_special per launch");
        }
    }
    for (int j = 0; j < ne; ++j) {
        for (int i = 0; i < 4; ++i) {
            const bool absent = !E[j].in[i];
            if (need[j].in[i] && !(absent && need[j].in_opt[i]) && (absent || E[j].in_bytes[i] < need[j].in[i]))
                return cbas_fail(CBAS_EINVAL, "op %d entry %d: in[%d] is missing or too small (%lld of %lld bytes)", op, j, i,
                                 (long long)E[j].in_bytes[i], (long long)need[j].in[i]);
        }
        for (int i = 0; i < 3; ++i)
            if (need[j].out[i] && (!E[j].out[i] || E[j].out_bytes[i] < need[j].out[i]))
                return cbas_fail(CBAS_EINVAL, "op %d entry %d: out[%d] is missing or too small (%lld of %lld bytes)", op, j, i,
                                 (long long)E[j].out_bytes[i], (long long)need[j].out[i]);
    }
    // labels are indices into cw: checked on the host images before anything is launched
    if (op == CBAS_DEBUG_HEAD_CE_TERMS || op == CBAS_DEBUG_HEAD_CE_GRAD)
        for (int j = 0; j < ne; ++j) {
            const int* lab = static_cast<const int*>(E[j].in[1]);
            for (int64_t w = 0; w < E[j].n; ++w)
                if (lab[w] < 0 || lab[w] >= E[j].C) return cbas_fail(CBAS_EINVAL, "ce entry %d: label %d of window %lld outside [0, %d)", j, lab[w], (long long)w, E[j].C);
        }
    DevBufs B;
    char* din[TRAIN_MULTI_MAX][4] = {};
    char* dout[TRAIN_MULTI_MAX][3] = {};
    for (int j = 0; j < ne; ++j) {
        for (int i = 0; i < 4; ++i)
            if (E[j].in[i] && (need[j].in[i] || need[j].in_opt[i])) {
                HIP_TRY(B.alloc(&din[j][i], (size_t)E[j].in_bytes[i]));
                if (E[j].in_bytes[i] > 0) HIP_TRY(hipMemcpy(din[j][i], E[j].in[i], (size_t)E[j].in_bytes[i], hipMemcpyHostToDevice));
            }
        for (int i = 0; i < 3; ++i)
            if (E[j].out[i] && E[j].out_bytes[i] > 0) {
                HIP_TRY(B.alloc(&dout[j][i], (size_t)E[j].out_bytes[i]));
                HIP_TRY(hipMemcpy(dout[j][i], E[j].out[i], (size_t)E[j].out_bytes[i], hipMemcpyHostToDevice));
            }
    }
    const auto fin = [&](int j, int i) { return reinterpret_cast<const float*>(din[j][i]); };
    const auto fout = [&](int j, int i) { return reinterpret_cast<float*>(dout[j][i]); };
    const cbas_debug_head_entry& e0 = E[0];
    int rc = -1;
    if (gemm) {
        g.A = fin(0, 0); g.W = fin(0, 1); g.bias = fin(0, 2);
        g.out = splits > 1 ? fout(0, 1) : fout(0, 0);
        rc = launch_gemm_f32(g, a->gelu, 0);
        if (!rc && splits > 1) rc = launch_splitk_reduce(fout(0, 1), splits, a->split_stride, a->M * a->N, fout(0, 0), 0);
    } else if (!multi) {
        switch (op) {
            case CBAS_DEBUG_HEAD_TRANSPOSE_PAD: rc = launch_transpose_pad(fin(0, 0), e0.n, e0.cols, e0.ld, fout(0, 0), e0.rows_pad, 0); break;
            case CBAS_DEBUG_HEAD_GELU_DROPOUT_FWD: rc = launch_gelu_dropout(fin(0, 0), fout(0, 0), e0.n, e0.key, e0.thr, e0.scale, 0, 0); break;
            case CBAS_DEBUG_HEAD_GELU_DROPOUT_BWD: rc = launch_gelu_dropout(fin(0, 0), fout(0, 0), e0.n, e0.key, e0.thr, e0.scale, 1, 0); break;
            case CBAS_DEBUG_HEAD_CE_TERMS:
                rc = launch_ce_terms(fin(0, 0), reinterpret_cast<const int*>(din[0][1]), fin(0, 2), e0.n, e0.C, e0.eps, fout(0, 0), 0);
                break;
            case CBAS_DEBUG_HEAD_CE_GRAD:
                rc = launch_ce_grad(fin(0, 0), reinterpret_cast<const int*>(din[0][1]), fin(0, 2), fin(0, 3), e0.n, e0.C, e0.eps, fout(0, 0), 0);
                break;
            case CBAS_DEBUG_HEAD_COV_OFFDIAG: rc = launch_cov_offdiag(fin(0, 0), (int)e0.n, e0.cscale, e0.gscale, fout(0, 0), fout(0, 1), 0); break;
            case CBAS_DEBUG_HEAD_SUB_COLMEAN: rc = launch_sub_colmean(fin(0, 0), fin(0, 1), e0.n, e0.cols, fout(0, 0), 0); break;
            case CBAS_DEBUG_HEAD_COLSUM: rc = launch_colsum(fin(0, 0), e0.n, e0.cols, e0.ld, e0.scale, fout(0, 0), fout(0, 1), 0); break;
            case CBAS_DEBUG_HEAD_ADD_VEC: rc = launch_add_vec(fin(0, 0), fin(0, 1), fout(0, 0), (int)e0.n, 0); break;
            case CBAS_DEBUG_HEAD_ADAM:
                rc = launch_adam_step(fout(0, 0), fin(0, 0), fout(0, 1), fout(0, 2), e0.n, e0.lr, e0.wd, e0.wd_lo, e0.wd_hi, e0.wd_special, e0.step, 0);
                break;
        }
    } else {
        switch (op) {
            case CBAS_DEBUG_HEAD_GELU_DROPOUT_FWD:
            case CBAS_DEBUG_HEAD_GELU_DROPOUT_BWD: {
                GeluBatch b{};
                for (int j = 0; j < k; ++j) { b.Z[j] = fin(j, 0); b.io[j] = fout(j, 0); b.n[j] = E[j].n; b.key[j] = E[j].key; b.thr[j] = E[j].thr; b.scale[j] = E[j].scale; }
                rc = launch_gelu_dropout_multi(b, k, op == CBAS_DEBUG_HEAD_GELU_DROPOUT_BWD, 0);
                break;
            }
            case CBAS_DEBUG_HEAD_CE_TERMS:
            case CBAS_DEBUG_HEAD_CE_GRAD: {
                CeBatch b{};
                for (int j = 0; j < k; ++j) {
                    b.logits[j] = fin(j, 0); b.labels[j] = reinterpret_cast<const int*>(din[j][1]); b.cw[j] = fin(j, 2); b.sums[j] = fin(j, 3);
                    b.out[j] = fout(j, 0); b.n[j] = E[j].n; b.C[j] = E[j].C; b.eps[j] = E[j].eps;
                }
                rc = launch_ce_multi(b, k, op == CBAS_DEBUG_HEAD_CE_GRAD, 0);
                break;
            }
            case CBAS_DEBUG_HEAD_COV_OFFDIAG: {
                CovBatch b{};
                for (int j = 0; j < k; ++j) { b.cov[j] = fin(j, 0); b.G[j] = fout(j, 0); b.sq[j] = fout(j, 1); b.n[j] = (int)E[j].n; b.cscale[j] = E[j].cscale; b.gscale[j] = E[j].gscale; }
                rc = launch_cov_offdiag_multi(b, k, 0);
                break;
            }
            case CBAS_DEBUG_HEAD_COLSUM: {
                ColsumBatch b{};
                for (int j = 0; j < k; ++j) { b.src[j] = fin(j, 0); b.tmp[j] = fout(j, 0); b.dst[j] = fout(j, 1); b.rows[j] = E[j].n; b.ld[j] = E[j].ld; b.cols[j] = E[j].cols; }
                rc = launch_colsum_multi(b, k, 0);
                break;
            }
            case CBAS_DEBUG_HEAD_ADD_VEC: {
                VecBatch b{};
                for (int j = 0; j < k; ++j) { b.a[j] = fin(j, 0); b.b[j] = fin(j, 1); b.out[j] = fout(j, 0); b.n[j] = (int)E[j].n; }
                rc = launch_add_vec_multi(b, k, 0);
                break;
            }
            case CBAS_DEBUG_HEAD_ADAM: {
                AdamBatch b{};
                for (int j = 0; j < k; ++j) {
                    b.p[j] = fout(j, 0); b.g[j] = fin(j, 0); b.m[j] = fout(j, 1); b.v[j] = fout(j, 2); b.n[j] = E[j].n; b.wd_lo[j] = E[j].wd_lo; b.wd_hi[j] = E[j].wd_hi;
                    adam_bias_corrections(E[j].lr, E[j].step, &b.lr_c1[j], &b.inv_sqrt_c2[j]);
                    b.wd[j] = E[j].wd;
                }
                b.wd_special = e0.wd_special;
                rc = launch_adam_step_multi(b, k, 0);
                break;
            }
        }
    }
    if (rc) return cbas_fail(CBAS_EINVAL, "head kernel launch failed (op %d, multi %d: rc=%d)", op, (int)multi, rc);
    HIP_TRY(hipDeviceSynchronize());
    for (int j = 0; j < ne; ++j)
        for (int i = 0; i < 3; ++i)
            if (E[j].out[i] && E[j].out_bytes[i] > 0 && dout[j][i]) HIP_TRY(hipMemcpy(E[j].out[i], dout[j][i], (size_t)E[j].out_bytes[i], hipMemcpyDeviceToHost));
    return CBAS_OK;
}

// ---- tests: one launch of a sequential classifier-head kernel (LSTM, BPTT, attention pooling, centre) on host operands ----
extern "C" int cbas_debug_head_seq_run(const cbas_debug_head_seq_args* a) {
    if (!a || a->struct_bytes != (int64_t)sizeof(cbas_debug_head_seq_args))
        return cbas_fail(CBAS_EINVAL, "cbas_debug_head_seq_args: struct_bytes %lld, library expects %lld", a ? (long long)a->struct_bytes : -1ll,
                         (long long)sizeof(cbas_debug_head_seq_args));
    constexpr int NI = 10, NO = 5;
    const int op = a->op, h = a->h, H2 = a->H2, T = a->T, lo = a->lo, hi = a->hi, Cn = a->C, L0 = a->L0;
    const int64_t nw = a->n_windows;
    if (op < CBAS_DEBUG_SEQ_LSTM_INFER || op > CBAS_DEBUG_SEQ_CENTRE) return cbas_fail(CBAS_EINVAL, "op %d", op);
    const bool lstm = op <= CBAS_DEBUG_SEQ_LSTM_TRAIN_BWD, centre = op == CBAS_DEBUG_SEQ_CENTRE, pool = !lstm && !centre;
    const bool pool_train = op == CBAS_DEBUG_SEQ_POOL_TRAIN_FWD || op == CBAS_DEBUG_SEQ_POOL_TRAIN_BWD;
    // everything the launchers do not check, before anything is allocated: a refusal must not become a launch
    if (nw < 1 || nw > (1 << 24) || T < 1 || T > (1 << 16)) return cbas_fail(CBAS_EINVAL, "n_windows = %lld, T = %d: both at least 1", (long long)nw, T);
    if (lstm && (h < 16 || h > 128 || h % 16)) return cbas_fail(CBAS_EINVAL, "h = %d: the LSTM kernels exist for h = 16, 32, .. 128", h);
    if ((op == CBAS_DEBUG_SEQ_LSTM_INFER || pool) && !(0 <= lo && lo < hi && hi <= T))
        return cbas_fail(CBAS_EINVAL, "centre range [lo, hi) = [%d, %d) of T = %d: 0 <= lo < hi <= T", lo, hi, T);
    if (pool) {
        if (Cn < 1 || Cn > 64) return cbas_fail(CBAS_EINVAL, "C = %d: the pooling kernels hold 1 .. 64 classes", Cn);
        if (H2 < 1 || H2 > 256) return cbas_fail(CBAS_EINVAL, "H2 = %d: the pooling kernels hold 2h <= 256 columns", H2);
        if (!pool_train && H2 % 2) return cbas_fail(CBAS_EINVAL, "POOL_INFER: H2 = %d is not 2 h", H2);
        if (pool_train && H2 % 32) return cbas_fail(CBAS_EINVAL, "H2 = %d: training pooling needs H2 %% 32 == 0", H2);
        if (pool_train && hi - lo > 128) return cbas_fail(CBAS_EINVAL, "hi - lo = %d: training pooling holds at most 128 scores", hi - lo);
    }
    if (centre && (L0 < 1 || L0 > (1 << 20))) return cbas_fail(CBAS_EINVAL, "L0 = %d: at least 1", L0);
    // bytes the launch reads (in) and writes (out); opt: the image may be NULL
    int64_t in_need[NI] = {}, out_need[NO] = {};
    bool in_opt[NI] = {}, out_opt[NO] = {};
    const int64_t nc = hi - lo;
    const int64_t g8 = nw * T * 8 * h * 4, s2 = nw * T * 2 * h * 4, whh = (int64_t)2 * 4 * h * h * 4;
    switch (op) {
        case CBAS_DEBUG_SEQ_LSTM_INFER: in_need[0] = g8; in_need[1] = whh; out_need[0] = nw * nc * 2 * h * 4; break;
        case CBAS_DEBUG_SEQ_LSTM_TRAIN_FWD: in_need[0] = g8; in_need[1] = whh; out_need[0] = g8; out_need[1] = out_need[2] = s2; break;
        case CBAS_DEBUG_SEQ_LSTM_TRAIN_BWD:
            in_need[0] = s2; in_need[1] = g8; in_need[2] = in_need[3] = s2; in_need[4] = whh; out_need[0] = g8; out_need[1] = s2;
            break;
        case CBAS_DEBUG_SEQ_POOL_INFER:
        case CBAS_DEBUG_SEQ_POOL_TRAIN_FWD:
        case CBAS_DEBUG_SEQ_POOL_TRAIN_BWD:
            in_need[0] = nw * (pool_train ? T : nc) * H2 * 4; in_need[1] = nw * Cn * 4; in_need[2] = (int64_t)H2 * 4;
            in_need[3] = (int64_t)Cn * H2 * 4; in_need[4] = (int64_t)Cn * 4;
            if (op == CBAS_DEBUG_SEQ_POOL_INFER) {
                out_need[0] = out_need[1] = nw * Cn * 4; out_need[2] = nw * H2 * 4;
                out_opt[0] = out_opt[1] = out_opt[2] = true;
                if (!a->out[0] && !a->out[1] && !a->out[2]) return cbas_fail(CBAS_EINVAL, "POOL_INFER: probs, logits and latent are all NULL");
            } else if (op == CBAS_DEBUG_SEQ_POOL_TRAIN_FWD) {
                out_need[0] = out_need[1] = nw * nc * 4; out_need[2] = nw * H2 * 4; out_need[3] = out_need[4] = nw * Cn * 4;
            } else {
                in_need[5] = in_need[6] = nw * nc * 4; in_need[7] = in_need[8] = nw * Cn * 4; in_need[9] = nw * H2 * 4; in_opt[9] = true;
                out_need[0] = nw * T * H2 * 4; out_need[1] = out_need[2] = nw * Cn * 4; out_need[3] = nw * (H2 + 12) * 4;
            }
            break;
        case CBAS_DEBUG_SEQ_CENTRE: out_need[0] = nw * T * L0 * 4; break;
    }
    for (int i = 0; i < NI; ++i)
        if (in_need[i] && !(in_opt[i] && !a->in[i]) && (!a->in[i] || a->in_bytes[i] < in_need[i]))
            return cbas_fail(CBAS_EINVAL, "op %d: in[%d] is missing (NULL) or too small (%lld of %lld bytes)", op, i, (long long)a->in_bytes[i],
                             (long long)in_need[i]);
    for (int i = 0; i < NO; ++i)
        if (out_need[i] && !(out_opt[i] && !a->out[i]) && (!a->out[i] || a->out_bytes[i] < out_need[i]))
            return cbas_fail(CBAS_EINVAL, "op %d: out[%d] is missing (NULL) or too small (%lld of %lld bytes)", op, i, (long long)a->out_bytes[i],
                             (long long)out_need[i]);
    DevBufs B;
    char* din[NI] = {};
    char* dout[NO] = {};
    for (int i = 0; i < NI; ++i)
        if (in_need[i] && a->in[i]) {
            HIP_TRY(B.alloc(&din[i], (size_t)a->in_bytes[i]));
            HIP_TRY(hipMemcpy(din[i], a->in[i], (size_t)a->in_bytes[i], hipMemcpyHostToDevice));
        }
    for (int i = 0; i < NO; ++i)
        if (out_need[i] && a->out[i]) {
            HIP_TRY(B.alloc(&dout[i], (size_t)a->out_bytes[i]));
            HIP_TRY(hipMemcpy(dout[i], a->out[i], (size_t)a->out_bytes[i], hipMemcpyHostToDevice));
        }
    float* scal = nullptr;                                            // training pooling reads its three scalars from memory
    if (pool_train) {
        const float hs[3] = {a->b_att, a->att_temp, a->gate};
        HIP_TRY(B.alloc(&scal, sizeof(hs)));
        HIP_TRY(hipMemcpy(scal, hs, sizeof(hs), hipMemcpyHostToDevice));
    }
    const auto fin = [&](int i) { return reinterpret_cast<const float*>(din[i]); };
    const auto fout = [&](int i) { return reinterpret_cast<float*>(dout[i]); };
    HeadDims d{};
    d.C = Cn; d.T = T; d.L0 = L0; d.h = lstm ? h : H2 / 2; d.lo = lo; d.hi = hi;
    TrainPoolParams pp{};
    pp.hout = fin(0); pp.lin_logits = fin(1); pp.w_att = fin(2); pp.w_lin2 = fin(3); pp.b_lin2 = fin(4);
    pp.b_att = scal; pp.att_temp = scal ? scal + 1 : nullptr; pp.gate = scal ? scal + 2 : nullptr;
    pp.T = T; pp.H2 = H2; pp.C = Cn; pp.lo = lo; pp.hi = hi;
    int rc = -1;
    switch (op) {
        case CBAS_DEBUG_SEQ_LSTM_INFER: rc = launch_head_lstm(fin(0), fin(1), d, lo, hi, nw, fout(0), 0); break;
        case CBAS_DEBUG_SEQ_LSTM_TRAIN_FWD: rc = launch_lstm_train_fwd(fin(0), fin(1), h, T, nw, fout(0), fout(1), fout(2), 0); break;
        case CBAS_DEBUG_SEQ_LSTM_TRAIN_BWD: rc = launch_lstm_train_bwd(fin(0), fin(1), fin(2), fin(3), fin(4), h, T, nw, fout(0), fout(1), 0); break;
        case CBAS_DEBUG_SEQ_POOL_INFER:
            rc = launch_head_pool(fin(0), fin(1), d, fin(2), a->b_att, a->att_temp, fin(3), fin(4), a->gate, a->temperature, nw, fout(0), fout(1),
                                  fout(2), 0);
            break;
        case CBAS_DEBUG_SEQ_POOL_TRAIN_FWD: rc = launch_pool_train_fwd(pp, nw, fout(0), fout(1), fout(2), fout(3), fout(4), 0); break;
        case CBAS_DEBUG_SEQ_POOL_TRAIN_BWD:
            rc = launch_pool_train_bwd(pp, nw, fin(5), fin(6), fin(7), fin(8), fin(9), fout(0), fout(1), fout(2), fout(3), 0);
            break;
        case CBAS_DEBUG_SEQ_CENTRE: rc = launch_head_centre(fout(0), nw, T, L0, 0); break;
    }
    if (rc) return cbas_fail(CBAS_EINVAL, "head sequence kernel launch failed (op %d: rc=%d)", op, rc);
    HIP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < NO; ++i)
        if (dout[i]) HIP_TRY(hipMemcpy(a->out[i], dout[i], (size_t)a->out_bytes[i], hipMemcpyDeviceToHost));
    return CBAS_OK;
}

// ---- tests: one launch of a classifier-head expand kernel (inference, training forward, training backward) on host operands ----
extern "C" int cbas_debug_build_temporal(int T, float alpha, int lo, int hi, float* tmat, float* lin_vec) {
    if (T < 3 || T > 101 || !(0 <= lo && lo < hi && hi <= T) || !tmat || !lin_vec)
        return cbas_fail(CBAS_EINVAL, "cbas_debug_build_temporal: T = %d (3 .. 101), [lo, hi) = [%d, %d), or a NULL image", T, lo, hi);
    head_build_temporal(T, (double)alpha, lo, hi, tmat, lin_vec);      // the widening api_head_train.hip's trainer_init applies
    return CBAS_OK;
}

extern "C" int cbas_debug_head_expand_run(const cbas_debug_head_expand_args* a) {
    if (!a || a->struct_bytes != (int64_t)sizeof(cbas_debug_head_expand_args))
        return cbas_fail(CBAS_EINVAL, "cbas_debug_head_expand_args: struct_bytes %lld, library expects %lld", a ? (long long)a->struct_bytes : -1ll,
                         (long long)sizeof(cbas_debug_head_expand_args));
    constexpr int NI = 9, NO = 3;
    constexpr int64_t BIG = (int64_t)1 << 40;
    const int op = a->op, T = a->T, Bn = a->Bn, NS = a->NS, Cn = a->C, NP = a->NPROJ, lo = a->lo, hi = a->hi;
    const int64_t nw = a->n_windows;
    if (op < CBAS_DEBUG_EXPAND_INFER || op > CBAS_DEBUG_EXPAND_TRAIN_BWD) return cbas_fail(CBAS_EINVAL, "op %d", op);
    const bool infer = op == CBAS_DEBUG_EXPAND_INFER, bwd = op == CBAS_DEBUG_EXPAND_TRAIN_BWD;
    const bool sliding = infer && a->sliding != 0;
    // everything the launchers do not check, before anything is allocated: a refusal must not become a launch
    if (nw < 1 || nw > (1 << 16)) return cbas_fail(CBAS_EINVAL, "n_windows = %lld: 1 .. 65536", (long long)nw);
    if (T < 3 || T > 101) return cbas_fail(CBAS_EINVAL, "T = %d: the expand kernels serve windows of 3 .. 101 positions", T);
    if (Bn < 64 || Bn > 256 || Bn % 64) return cbas_fail(CBAS_EINVAL, "Bn = %d: a multiple of 64 in 64 .. 256", Bn);
    if (NS != 2 && NS != 3) return cbas_fail(CBAS_EINVAL, "NS = %d: 2 or 3 bottleneck streams", NS);
    const int F = NS * Bn;
    if (Cn < 1 || Cn > 64 || Cn > F) return cbas_fail(CBAS_EINVAL, "C = %d: 1 .. 64 classes, at most NS Bn", Cn);
    if (NP < F + Cn || NP % 4 || NP > (1 << 16))
        return cbas_fail(CBAS_EINVAL, "NPROJ = %d: a multiple of 4, at least NS Bn + C = %d", NP, F + Cn);
    if (bwd && NP - F > F) return cbas_fail(CBAS_EINVAL, "NPROJ = %d: the backward's block of %d threads writes at most that many columns past NS Bn", NP, F);
    if (infer && !(0 <= lo && lo < hi && hi <= T))
        return cbas_fail(CBAS_EINVAL, "centre range [lo, hi) = [%d, %d) of T = %d: 0 <= lo < hi <= T", lo, hi, T);
    if (infer ? (size_t)T * F * sizeof(float) > 160 * 1024 : train_expand_lds_bytes(T, Bn, NP) > 160 * 1024)
        return cbas_fail(CBAS_EINVAL, "LDS: T = %d, Bn = %d, NS = %d, NPROJ = %d needs more than 160 KiB", T, Bn, NS, NP);
    if (!infer && a->thr >= (1u << 24)) return cbas_fail(CBAS_EINVAL, "thr = %u: a 24-bit threshold (below 2^24)", a->thr);
    // bytes the launch reads (in) and writes (out)
    int64_t in_need[NI] = {}, out_need[NO] = {};
    const int64_t rows = nw * T;
    if (infer) {
        int64_t proj_rows = rows;
        if (sliding) {
            const int64_t nf = a->n_frames, w0 = a->w0, r0 = a->r0;
            if (nf < 1 || nf > BIG) return cbas_fail(CBAS_EINVAL, "sliding: n_frames = %lld: at least 1", (long long)nf);
            if (w0 < -BIG || w0 > BIG || r0 < -BIG || r0 > BIG) return cbas_fail(CBAS_EINVAL, "sliding: w0 = %lld or r0 = %lld out of range", (long long)w0, (long long)r0);
            // row_of(w, t) = clamp(w0 + w + t - T / 2, 0, n_frames - 1) - r0 is monotone in w + t: its extremes sit at the corners
            const auto clampf = [&](int64_t f) { return f < 0 ? 0 : (f > nf - 1 ? nf - 1 : f); };
            const int64_t rmin = clampf(w0 - T / 2) - r0, rmax = clampf(w0 + (nw - 1) + (T - 1) - T / 2) - r0;
            const int64_t have = a->in[0] ? a->in_bytes[0] / ((int64_t)NP * 4) : 0;
            if (rmin < 0 || rmax >= have)
                return cbas_fail(CBAS_EINVAL, "sliding: the windows read proj rows %lld .. %lld, the image holds rows 0 .. %lld (in[0] NULL or too small)",
                                 (long long)rmin, (long long)rmax, (long long)have - 1);
            proj_rows = rmax + 1;
        }
        in_need[0] = proj_rows * NP * 4; in_need[1] = in_need[2] = in_need[3] = (int64_t)F * 4; in_need[4] = (int64_t)Cn * 4;
        out_need[0] = rows * F * 4; out_need[1] = nw * Cn * 4;
    } else if (!bwd) {
        in_need[0] = rows * NP * 4; in_need[1] = in_need[2] = in_need[3] = (int64_t)F * 4; in_need[4] = (int64_t)Cn * 4;
        in_need[5] = (int64_t)3 * T * T * 4; in_need[6] = (int64_t)T * 4;
        out_need[0] = out_need[1] = rows * F * 4; out_need[2] = nw * Cn * 4;
    } else {
        in_need[0] = rows * F * 4; in_need[2] = (int64_t)F * 4; in_need[5] = (int64_t)3 * T * T * 4; in_need[6] = (int64_t)T * 4;
        in_need[7] = rows * F * 4; in_need[8] = nw * Cn * 4;
        out_need[0] = rows * NP * 4; out_need[1] = nw * 3 * F * 4;
    }
    for (int i = 0; i < NI; ++i)
        if (in_need[i] && (!a->in[i] || a->in_bytes[i] < in_need[i]))
            return cbas_fail(CBAS_EINVAL, "op %d: in[%d] is missing (NULL) or too small (%lld of %lld bytes)", op, i, (long long)a->in_bytes[i],
                             (long long)in_need[i]);
    for (int i = 0; i < NO; ++i)
        if (out_need[i] && (!a->out[i] || a->out_bytes[i] < out_need[i]))
            return cbas_fail(CBAS_EINVAL, "op %d: out[%d] is missing (NULL) or too small (%lld of %lld bytes)", op, i, (long long)a->out_bytes[i],
                             (long long)out_need[i]);
    DevBufs B;
    char* din[NI] = {};
    char* dout[NO] = {};
    for (int i = 0; i < NI; ++i)
        if (in_need[i]) {
            HIP_TRY(B.alloc(&din[i], (size_t)a->in_bytes[i]));
            HIP_TRY(hipMemcpy(din[i], a->in[i], (size_t)a->in_bytes[i], hipMemcpyHostToDevice));
        }
    for (int i = 0; i < NO; ++i)
        if (out_need[i]) {
            HIP_TRY(B.alloc(&dout[i], (size_t)a->out_bytes[i]));
            HIP_TRY(hipMemcpy(dout[i], a->out[i], (size_t)a->out_bytes[i], hipMemcpyHostToDevice));
        }
    const auto fin = [&](int i) { return reinterpret_cast<const float*>(din[i]); };
    const auto fout = [&](int i) { return reinterpret_cast<float*>(dout[i]); };
    int rc = -1;
    if (infer) {
        HeadDims d{};
        d.C = Cn; d.T = T; d.Bn = Bn; d.NS = NS; d.lo = lo; d.hi = hi; d.NPROJ = NP; d.alpha = a->alpha;
        rc = launch_head_expand(fin(0), d, fin(1), fin(2), fin(3), fin(4), nw, sliding ? 1 : 0, a->w0, a->r0, a->n_frames, fout(0), fout(1), 0);
    } else {
        TrainExpandParams p{};
        p.proj = bwd ? nullptr : fin(0); p.tmat = fin(5); p.lin_vec = fin(6); p.b_bott = fin(1); p.ln_w = fin(2); p.ln_b = fin(3); p.b_lin1 = fin(4);
        p.T = T; p.Bn = Bn; p.NPROJ = NP; p.C = Cn; p.NS = NS;
        for (int k = 0; k < 3; ++k) p.key[k] = a->key[k];
        p.thr = a->thr; p.scale = a->scale;
        rc = bwd ? launch_train_expand_bwd(p, nw, fin(0), fin(7), fin(8), fout(0), fout(1), 0)
                 : launch_train_expand_fwd(p, nw, fout(0), fout(1), fout(2), 0);
    }
    if (rc) return cbas_fail(CBAS_EINVAL, "head expand kernel launch failed (op %d: rc=%d)", op, rc);
    HIP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < NO; ++i)
        if (dout[i]) HIP_TRY(hipMemcpy(a->out[i], dout[i], (size_t)a->out_bytes[i], hipMemcpyDeviceToHost));
    return CBAS_OK;
}
