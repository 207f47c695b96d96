// Host-callable launchers of the HIP kernels (internal to libcbas_mi355x; not part of the C ABI).
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------
// fp16 x fp16 -> fp32 MFMA GEMM:  C[M,N] = A[M,K] * W[N,K]^T  with fused epilogues.
// A and W are row-major with K contiguous (the HF Linear weight layout, no transpose needed).
// ---------------------------------------------------------------------------------------------
enum GemmEpilogue {
    EPI_PATCH = 0,   // x[b*T + n_prefix + p][n] = acc*in_scale + bias[n]           (fp32 out)
    EPI_QKV   = 1,   // + bias, RoPE on patch rows of q and k, q *= 1/8              (fp16 out)
    EPI_RESID = 2,   // x[m][n] += (acc + bias[n]) * lambda[n]                        (fp32 in/out)
    EPI_GELU  = 3,   // u[m][n] = gelu_erf(acc + bias[n])                             (fp16 out)
    EPI_GELU_F8 = 4, // the same, stored as MX-fp8: e4m3 bytes + one E8M0 scale per 32 columns (precision 2)
    // LayerNorm folded into the GEMMs around it (gemm_f16_8ph.hip only; GemmParams "LayerNorm fold" fields):
    EPI_QKV_LN = 5,   // EPI_QKV on raw fp16 x with W = fp16(gamma o W): rstd * (acc - mean * colsum) + bias', then as EPI_QKV
    EPI_GELU_LN = 6,  // EPI_GELU likewise
    EPI_RESID_LN = 7, // EPI_RESID that also writes fp16 x and the per-row statistics the next EPI_*_LN needs
    // fp8 plans (gemm_f16_8ph.hip only): what EPI_GELU_F8 becomes on fp16 operands - the GELU value is rounded to fp16 first, so
    // the bytes and scales are the quantisation of exactly what EPI_GELU would have stored (callers pass EPI_GELU_F8)
    EPI_GELU_F8_H = 8,
    // gated MLP (DINOv3 S+ / H+, [tf]:360-373): W = gate | up interleaved in blocks of 32 rows (launch_interleave_gate_up), N = 2F;
    // a 64-column group holds 32 gate columns, then the up columns of the same 32 outputs, and writes 32 output columns:
    //   h[m][n / 2 + c] = silu(acc[n + c] + bias[n + c]) * (acc[n + 32 + c] + bias[n + 32 + c]),  n % 64 == 0, c < 32
    // in the format EPI_GELU writes (fp16; fp32; the split image with out_scale), leading dimension ldo >= N / 2
    EPI_SWIGLU = 9,
};
constexpr int epi_base(int epi) {
    return epi == EPI_QKV_LN ? EPI_QKV : epi == EPI_GELU_LN ? EPI_GELU : epi == EPI_RESID_LN ? EPI_RESID : epi == EPI_GELU_F8_H ? EPI_GELU_F8 : epi;
}

enum GemmTile { GEMM_TILE_AUTO = 0, GEMM_TILE_128x128 = 1, GEMM_TILE_256x128 = 2, GEMM_TILE_128x256 = 3,
                GEMM_TILE_256x256 = 4,
                GEMM_TILE_192x256 = 7, GEMM_TILE_64x128 = 8, GEMM_TILE_SKINNY = 9,
                GEMM_TILE_PP_256x256 = 13,      // gemm_f16_8ph.hip: 8 waves, ping-pong phases, counted vmcnt
                GEMM_TILE_PP_192x256 = 14, GEMM_TILE_PP_160x256 = 15, GEMM_TILE_PP_128x256 = 16,
                GEMM_TILE_PP_AUTO = 17 };       // planner: uniform tile height, or 256-row tiles + 128-row tail

constexpr int GEMM_STAMP_BLOCKS = 16384;     // GemmParams::stamps: [GEMM_STAMP_BLOCKS][4] s_memtime stamps of a workgroup's first tile + [GEMM_STAMP_BLOCKS] loop spans in s_memrealtime ticks + [GEMM_STAMP_BLOCKS][4] stamps of its last tile
constexpr int ROPE_LDS_ROWS = 192;            // (nh + nw) rows of 128 bytes the q|k|v kernel holds in LDS (24 KiB)
struct GemmParams {
    int tile;            // GemmTile (0 = pick by shape)
    int group_m;         // raster: row-panels per group (0/1 = N-fastest order)
    unsigned long long* stamps;   // bring-up only: per-block s_memtime stamps [grid][4], or nullptr
    const f16* A;        // [M_pad][lda]
    int lda;             // row stride of A in elements (0: K).  lda = T*D reads one row per frame (the CLS rows)
    const f16* W;        // [N][K]  (hi part when split)
    const f16* W_lo;     // [N][K]  residual W - fp16(W) as fp16, or nullptr
    // MX-fp8 operands (precision 2; gemm_f16_8ph.hip only): e4m3 bytes, K contiguous, plus E8M0 block scales, one
    // byte per 32 k-elements, stored K-tile-major as dwords: sc[(k / 128) * ld + row] byte (k % 128) / 32.
    // A8 != nullptr selects the fp8 kernel (A / W above are then unused).  The output format follows the epilogue, not the
    // operands (fp8 plans): EPI_GELU on fp8 operands writes fp16, EPI_GELU_F8 on fp16 operands writes out_f8 / out_sc.
    const uint8_t* A8;   // [M_pad][lda]
    const uint8_t* W8;   // [N][K]
    const uint32_t* A_sc;   // [K/128][sc_lda]
    const uint32_t* W_sc;   // [K/128][sc_ldw]
    int sc_lda;
    int sc_ldw;          // 0: N (W_sc may point into a wider array, e.g. the k|v columns of the fused q|k|v scales)
    uint8_t* out_f8;     // EPI_GELU_F8: [M][ldo] bytes
    uint32_t* out_sc;    // EPI_GELU_F8: [N/128][sc_ldo] (A_sc layout of the consumer)
    int sc_ldo;
    int M;               // valid rows (stores are skipped for rows >= M)
    int M_pad;           // rows allocated in A (loads of rows >= M_pad are clamped)
    int N;               // multiple of 128
    int K;               // multiple of 64
    const float* bias;   // [N]
    const float* lambda; // [N]   (EPI_RESID)
    float* out_f32;      // EPI_PATCH / EPI_RESID: residual stream x, leading dim ldo
    f16* out_f16;        // EPI_QKV / EPI_GELU / EPI_SWIGLU
    int ldo;
    // EPI_PATCH
    int patches_per_frame;   // P
    int tokens_per_frame;    // T
    int n_prefix;            // 1 + R
    float in_scale;          // 1/255 for uint8 input, 1 for float input
    const float* pos;        // [P][N] additive position embedding for the frame's patch grid, or nullptr (DINOv3)
    // EPI_QKV
    const float* rope_cos;   // [P][64], or nullptr: no RoPE (DINOv2)
    const float* rope_sin;   // [P][64]
    // the same numbers factorised by axis (columns 0-15 of a table row depend on the patch row only, 16-31 on the patch
    // column only): [nh + nw][32] floats, row r < nh = {cos(16) | sin(16)} of patch row r, row nh + c = those of patch
    // column c.  The ping-pong kernel keeps this copy in LDS (nullptr, or more than ROPE_LDS_ROWS rows: global table).
    const float* rope_fac;
    int rope_nh, rope_nw;
    unsigned rope_magic;     // floor(2^32 / rope_nw) + 1: patch row = umulhi(patch, rope_magic)
    int D;                   // hidden size (q | k | v sections of width D)
    int sec0;                // section of output column 0 (0: the full q|k|v GEMM; 1: W holds only k|v)
    // ---- LayerNorm folded into the GEMMs around it (gemm_f16_8ph.hip only; see "LayerNorm fold" in api_enc.hip) ----
    // producer side, EPI_RESID_LN: besides the fp32 residual stream the epilogue writes its fp16 copy (the NEXT GEMM's A
    // operand, un-normalised) and, per row and 256-column block (= one N tile), the statistics LayerNorm needs of it:
    //   ln_out[(col / 256) * ln_ld + m] = { sum of the block's 256 values, sum of squares about the BLOCK mean }
    f16* x16_out;            // [M][N]
    float2* ln_out;          // [N / 256][ln_ld]
    // consumer side, EPI_QKV_LN / EPI_GELU_LN: A holds raw fp16 x, W = fp16(gamma o W), bias = beta W^T + b; the epilogue
    // forms rstd * (acc - mean * ln_colsum[n]) + bias[n] with mean / rstd pooled from the row's ln_parts blocks
    // (exact pooled-variance formula: as robust as the two-pass form of layernorm_f16_kernel)
    const float2* ln_in;     // [ln_parts][ln_ld]
    const float* ln_colsum;  // [N]: sum over k of the fp16 folded weights
    int ln_parts;            // K / 256 (<= 4)
    int ln_ld;               // row stride of ln_in / ln_out (>= M)
    float ln_eps;
};

int launch_gemm(GemmEpilogue epi, const GemmParams& p, hipStream_t stream);

int launch_gemm_8ph(GemmEpilogue epi, const GemmParams& p, int tile, hipStream_t stream);
int launch_gemm_skinny(GemmEpilogue epi, const GemmParams& p, hipStream_t stream);     // M <= 64 (gemm_f16_skinny.hip)

// ---------------------------------------------------------------------------------------------
// ViT element-wise / attention kernels
// ---------------------------------------------------------------------------------------------
// The four ingest launchers (two here, two under precision 3): P = (height / ps) (width / ps) patches per frame in the 16 x 16
// slot layout A[b P + py (width / ps) + px][16 i + j] = pixel (py ps + i, px ps + j), i, j < ps (ps = 14 or 16); slots with
// j >= ps in rows i < ps are written as zeros, slot rows i >= ps are never written (the buffer is zeroed at allocation).  Pixel
// rows and columns past the last whole patch are never read.  Rows b T + r, r < n_prefix, of x [n T][D] receive
// prefix_tokens[r] bit for bit; nothing else of x is written.  -1: a null pointer, n <= 0, ps not 14 or 16, a frame smaller than
// one patch, n_prefix < 1, D <= 0 or D % 4, T < P + n_prefix, a negative frame or row stride, a pixel stride below 1.
bool im2col_args_ok(const void* frames, const void* A, const float* x, const float* prefix_tokens, int n, int height, int width,
                    int n_prefix, int D, int T, int ps);
// uint8 pixels -> im2col matrix A[n*P][256] fp16 holding the INTEGER pixel values (exact in fp16);
// also writes the CLS/register prefix rows of the residual stream x.
int launch_im2col_u8(const uint8_t* frames, int n, int height, int width, int64_t frame_stride,
                     int64_t row_stride, int64_t pixel_stride, f16* A, float* x, const float* prefix_tokens,
                     int n_prefix, int D, int T, int ps, hipStream_t stream);
// float32 (n,H,W) in [0,1] -> A[n*P][512] fp16 as hi|lo halves along K (x = hi + lo to ~2^-22)
int launch_im2col_f32(const float* frames, int n, int height, int width, f16* A, float* x,
                      const float* prefix_tokens, int n_prefix, int D, int T, int ps, hipStream_t stream);

// LayerNorm over the last dim (fp32 in, fp16 out), rows = M
// ldx = row stride of x in elements (D for the whole residual stream, T*D for the CLS rows only)
int launch_layernorm_f16(const float* x, int64_t ldx, const float* gamma, const float* beta, f16* out, int M, int D,
                         float eps, hipStream_t stream);
// the same with an MX-fp8 result: out8 [M][D] e4m3 bytes, out_sc [D/128][sc_ld] block scales (GemmParams::A_sc layout)
int launch_layernorm_f8(const float* x, int64_t ldx, const float* gamma, const float* beta, uint8_t* out8,
                        uint32_t* out_sc, int sc_ld, int M, int D, float eps, hipStream_t stream);
// LayerNorm fold, first layer: fp32 x [M][D] -> fp16 copy x16 [M][D] + per 64-column block statistics
// ln_out[(col / 256) * ln_ld + m] = {sum, sum of squares about the block mean} (what EPI_RESID_LN writes for later layers)
int launch_ln_stats_x16(const float* x, f16* x16, float2* ln_out, int ln_ld, int M, int D, hipStream_t stream);
// LayerNorm fold, create time: W [N][K] fp32, gamma / beta [K], b [N] ->
//   Wf [N][K] = fp16(gamma_k W_nk),  colsum[n] = sum_k float(Wf_nk),  biasf[n] = b[n] + sum_k beta_k W_nk
int launch_fold_ln_weight(const float* W, const float* gamma, const float* beta, const float* b, f16* Wf, float* colsum,
                          float* biasf, int N, int K, hipStream_t stream);
// Final LayerNorm on the CLS row of every frame: x[b*T] -> cls_f32[b][D] / cls_f16[b][D]
// `nonfinite` (may be NULL): incremented once per frame whose CLS row holds a NaN / infinity or a finite value whose square
// overflows the variance (rstd = 0: the row would come out as beta)
int launch_final_norm_cls(const float* x, const float* gamma, const float* beta, float* cls_f32,
                          f16* cls_f16, int n, int T, int D, float eps, hipStream_t stream, unsigned* nonfinite = nullptr);

// Multi-head attention over frames: qkv16 [n*T][3D] (q pre-scaled by 1/8, RoPE applied) -> o16 [n*T][D]
// q_cls != nullptr: only the CLS query of every frame (the last layer: [tf]:540-541 + cbas.py:677 consume row 0
// alone): q_cls [n][D] holds the projected CLS queries, out is then [n][D]; K and V still come from qkv.
// out_sc != nullptr: the context is stored as MX-fp8 (out = e4m3 bytes [n*T][D], out_sc [D/128][sc_ld] scales)
int launch_attention(const f16* qkv, const f16* q_cls, void* out, uint32_t* out_sc, int sc_ld, int n, int T, int D,
                     int n_heads, hipStream_t stream);

// cls_attention.hip: the CLS query's softmax row over every token, per head and head-averaged over the patch tokens
// (compare_encoders.py:36-49).  E = f16 (precisions 0, 1, 2) or float (3; 4 with split != 0: q and K in the head-split hi | lo
// form of store_head_split4, scales ATT_QS / ATT_KS).  q [n] rows of stride ldq (bias added, x 1/8), K [n*T] rows of stride ldk,
// both pointing at head 0's first column; NP prefix tokens.  heads_out (n, NH, T) and map_out (n, T - NP), fp32; either may be
// nullptr, not both.  One workgroup per frame, fixed summation order, no scratch.  -1: bad argument, or T beyond the 64 KiB of LDS
// (2 T - NP floats: about 8 000 tokens).
constexpr int64_t CLS_ATTENTION_LDS_BYTES = 64 * 1024 - 256;      // dynamic LDS of a launch: (2 T - NP) floats must fit
template <typename E>
int launch_cls_attention(const E* q, int64_t ldq, const E* K, int64_t ldk, int n, int T, int NH, int NP, int split,
                         float* heads_out, float* map_out, hipStream_t stream);

// attention_rollout.hip: the head-mean softmax rows of EVERY query of a layer, and the rollout chain over the layers.
//   launch_attention_mean: out (n, T, T) fp32, out[b][i][t] = (1 / NH) sum_h softmax_t(q[b T + i, h] . K[b T + t, h]); q and K
//   are [n*T] rows of stride ldq / ldk in the storage forms of launch_cls_attention (E, split), pointing at head 0's first column
//   (q bias added and x 1/8).  blend != 0 writes 0.5 out + 0.5 I instead.  LDS: QB (64 + 2 T) floats for QB query rows per
//   workgroup (attention_mean_rows_per_block: 16 down to 1, 0 = T does not fit, about 8 100 tokens).  -1: bad argument or such a T.
//   launch_rollout_step: out = A R per frame, (n, T, T) each, out distinct from both.  launch_rollout_row: out (n, T - NP) =
//   columns NP.. of row query_idx[b] (clamped to [0, T); NULL: row 0) of R.  All fp32, fixed summation order, no atomics.
constexpr int64_t ATTENTION_MEAN_LDS_BYTES = 64 * 1024 - 256;
int attention_mean_rows_per_block(int64_t T);
template <typename E>
int launch_attention_mean(const E* q, int64_t ldq, const E* K, int64_t ldk, int n, int T, int NH, int split, int blend, float* out,
                          hipStream_t stream);
int launch_rollout_step(const float* A, const float* R, float* out, int n, int T, hipStream_t stream);
int launch_rollout_row(const float* R, int n, int T, int NP, const int* query_idx, float* out, hipStream_t stream);

// tokens_out.hip: every token's final hidden state (transformers' last_hidden_state) instead of the CLS row alone, and patch
// similarity maps.  out_f32 / out_f16: rows of stride ld_out elements (>= the width, a multiple of 4); either may be nullptr, not
// both.  Rows are normalised by the code of the CLS kernels (row_norm.h): row 0 of a frame has launch_final_norm_cls's /
// launch_cnx_pool_ln's bits.  `nonfinite` (may be NULL) rises by one per ROW that comes out non-finite.  -1: bad argument.
//   ViT: out[r] = LayerNorm(x[r]), r < M (= n T); x rows of stride ldx; D % 4 == 0, D <= 1280
int launch_final_norm_rows(const float* x, int64_t ldx, const float* gamma, const float* beta, float* out_f32, f16* out_f16,
                           int64_t ld_out, int64_t M, int D, float eps, unsigned* nonfinite, hipStream_t stream);
//   the raw rows (transformers' hidden_states[l]): out[r] = x[r], r < M, as fp32 and / or fp16 (round to nearest even); D % 4 == 0
int launch_copy_rows(const float* x, int64_t ldx, float* out_f32, f16* out_f16, int64_t ld_out, int64_t M, int D, unsigned* nonfinite,
                     hipStream_t stream);
//   ConvNeXt: out[b (hw + 1)] = LayerNorm(mean over the hw pixels of frame b), out[b (hw + 1) + 1 + p] = LayerNorm(x[b hw + p]);
//   x rows of stride ld holding C values (C % 32 == 0, C <= 1536)
int launch_cnx_token_rows(const float* x, int64_t ld, int n, int hw, const float* gamma, const float* beta, int C, float eps,
                          float* out_f32, f16* out_f16, int64_t ld_out, unsigned* nonfinite, hipStream_t stream);
//   map[b][p] = cos(tokens[b][q_b], tokens[b][P0 + p]), p < T - P0: E = float or f16 rows (n, T) of stride ld, sums in fp32 in a
//   fixed order; q_b = query_idx[b] clamped to [0, T) (NULL: row 0, the CLS / pooled row); a zero-norm row gives 0
template <typename E>
int launch_token_similarity(const E* tokens, int64_t ld, int n, int T, int D, int P0, const int* query_idx, float* map,
                            hipStream_t stream);

// gated MLP, create time: out [2F][K] = rows of gate [F][K] and up [F][K] interleaved in blocks of 32 - out rows [64 b, 64 b + 32)
// are gate rows [32 b, 32 b + 32), out rows [64 b + 32, 64 b + 64) the up rows of the same outputs (K = 1: the biases); F % 32 == 0
int launch_interleave_gate_up(const float* gate, const float* up, float* out, int64_t F, int K, hipStream_t stream);
// fp32 -> fp16 weight conversion, n elements: hi[i] = fp16(src[i]) (round to nearest even; beyond 65504 infinity), and, unless lo is
// NULL, lo[i] = fp16(src[i] - hi[i]).  -1: src or hi NULL, n <= 0
int launch_convert_f16(const float* src, f16* hi, f16* lo, int64_t n, hipStream_t stream);
// patch weight (D,3,ps,ps) fp32 -> W' = (c0 + c1) + c2 over the 3 identical input channels, in fp32, in the 16 x 16 slot layout
// (zero where i >= ps or j >= ps) -> hi = fp16(W'), lo = fp16(W' - hi), each (D,256), and hi2 / lo2 (D,512) = [W' | W'] along K for
// the float-input path.  lo and lo2 may be NULL together.  -1: another null pointer, D <= 0, ps not 14 or 16
// (launch_pack_patch_weight, declared below)
// fp32 weight [N][K] -> MX-fp8: e4m3 bytes [N][K] + block scales [K/128][N] (GemmParams::W_sc layout); K % 128 == 0
// sc row n of this call is column n0 + n of a scale array with n_total columns (q, k, v packed into one [3D][D] weight)
int launch_pack_fp8_weight(const float* src, uint8_t* w8, uint32_t* sc, int N, int K, int n_total, int n0, hipStream_t stream);
int launch_pack_patch_weight(const float* w, f16* hi, f16* lo, f16* hi2, f16* lo2, int D, int ps, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// precision 3: the reference's fp32 CPU arithmetic (backend/cbas.py:433-434 autocast off on CPU; [tf]:523-548) on
// v_mfma_f32_16x16x4_f32 - exact fp32 products and sums, k-ordered (vit_f32.hip).  Every buffer is fp32.
// ---------------------------------------------------------------------------------------------
struct Gemm32VitParams {
    const float* A; int64_t lda;   // [M][lda], first K columns used (lda = T*D reads one row per frame: the CLS rows)
    const float* W;                // [N][K], the HF Linear weight as stored
    int M, N, K;                   // N % 128 == 0, K % 32 == 0
    const float* bias;             // [N]
    const float* lambda;           // [N]   (EPI_RESID)
    float* out; int64_t ldo;       // EPI_PATCH / EPI_RESID: the residual stream x; EPI_QKV / EPI_GELU / EPI_SWIGLU: qkv / u
    // EPI_PATCH
    int patches_per_frame, tokens_per_frame, n_prefix;
    const float* pos;              // DINOv2 position embedding [P][N], or nullptr
    // EPI_QKV
    const float* rope_cos;         // [P][64], or nullptr: no RoPE
    const float* rope_sin;
    // the same numbers by axis (GemmParams::rope_fac): the ping-pong kernel's split form keeps them in LDS (or nullptr)
    const float* rope_fac; int rope_nh, rope_nw; unsigned rope_magic;
    int D;                         // hidden size (q | k | v sections of width D)
    int sec0;                      // section of output column 0
    // precision 4: the same fp32 operands, products on the fp16 matrix pipe as a three-term split (vit_f32.hip).
    // a_scale / w_scale: powers of two the operands are multiplied by before the split (keeps the low halves out of
    // fp16's subnormal range); the accumulators are multiplied by 1 / (a_scale * w_scale) - all exact.
    int split;                     // A and W are in the split format (vit_f32.hip); EPI_GELU / EPI_SWIGLU then write their output split too
    float a_scale, w_scale;        // the scales A and W were split with
    float out_scale;               // EPI_GELU / EPI_SWIGLU with split: scale of the split output (the down projection's a_scale)
};
int launch_gemm_f32_vit(GemmEpilogue epi, const Gemm32VitParams& p, hipStream_t stream);
// precision 4, M > 256, N % 256 == 0: the ping-pong kernel's split-operand form (gemm_f16_8ph.hip); -1 = not its shape
int launch_gemm_split_pp(GemmEpilogue epi, const Gemm32VitParams& p, hipStream_t stream);
void vit32_split_set_forms(int forms);   // bring-up: which precision-4 GEMM forms run (bit 0 ping-pong, bit 1 skinny; -1 = environment)
void gemm_split_pp_set_tile(int tile, unsigned long long* stamps);   // bring-up: forced tile height (0 = planner), block timeline stamps
// uint8 pixels -> A[n*P][256] fp32 = float(double(pixel) / 255.0), the reference's cbas.py:431 value bit for bit
// (+ prefix rows of x, as launch_im2col_u8)
// split != 0 (precision 4): A in the split hi | lo format of vit_f32.hip
int launch_im2col_u8_f32(const uint8_t* frames, int n, int height, int width, int64_t frame_stride, int64_t row_stride,
                         int64_t pixel_stride, float* A, float* x, const float* prefix_tokens, int n_prefix, int D, int T,
                         int ps, int split, hipStream_t stream);
// float32 (n,H,W) -> A[n*P][256] fp32, values as they are
int launch_im2col_f32_f32(const float* frames, int n, int height, int width, float* A, float* x,
                          const float* prefix_tokens, int n_prefix, int D, int T, int ps, int split, hipStream_t stream);
// precision 4: fp32 weight [N][K] -> split format at the same byte size, values multiplied by `scale` first: hi = fp16(w scale),
// lo = fp16(w scale - hi), bit for bit - except that the low half of a ZERO weight is a zero of either sign (measured: -0.0 for
// w = -0.0, where the subtraction alone gives +0.0; the compiler fuses scale, rounding and subtraction into mixed-precision FMAs).
// hi + lo is the same -0.0 either way.  -1: N <= 0, K % 32
int launch_pack_split_weight(const float* w, float* out, int64_t N, int K, float scale, hipStream_t stream);
// patch weight (D,3,ps,ps) fp32 -> (D,256) fp32 in the 16x16 slot layout, summed over the 3 identical input channels in
// double and rounded once
int launch_pack_patch_weight_f32(const float* w, float* out, int D, int ps, hipStream_t stream);
int launch_layernorm_f32(const float* x, int64_t ldx, const float* gamma, const float* beta, float* out, int M, int D,
                         float eps, int split, hipStream_t stream);
// qkv [n*T][3D] fp32 (q pre-scaled by 1/8, RoPE applied) -> out [n*T][D] fp32; q_cls as launch_attention
// split_scale > 0 (precision 4): the context is written in the split format, multiplied by split_scale
int launch_attention_f32(const float* qkv, const float* q_cls, float* out, int n, int T, int D, int n_heads,
                         float split_scale, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// DINOv3 ConvNeXt (precision 3 / 4, convnext_f32.hip): channels-last fp32 rows (frame, y, x), row stride ld >= C, C % 32 == 0.
// split != 0 (precision 4): the GEMM operand A is written in the split hi | lo format of vit32_epilogue.h, scale 1.
// ---------------------------------------------------------------------------------------------
// stem: the 4 x 4 / stride-4 patch of output pixel m at A[m][4 i + j] (k < 16), A[m][16..31] = 0
int launch_cnx_stem_im2col_u8(const uint8_t* frames, int n, int height, int width, int64_t frame_stride, int64_t row_stride,
                              int64_t pixel_stride, float* A, int split, hipStream_t stream);
int launch_cnx_stem_im2col_f32(const float* frames, int n, int height, int width, float* A, int split, hipStream_t stream);
// LayerNorm over the first C columns of M rows, in place
int launch_cnx_ln_rows(float* x, int64_t ld, const float* gamma, const float* beta, int64_t M, int C, float eps, hipStream_t stream);
// 2 x 2 / stride-2 downsample operand: A[m][(2 kh + kw) C + c] = LayerNorm(x[pixel (2 oy + kh, 2 ox + kw)])[c]
int launch_cnx_downsample(const float* x, int64_t ldx, int n, int hi, int wi, const float* gamma, const float* beta, int C, float eps,
                          float* A, int split, hipStream_t stream);
// A[m][c] = LayerNorm(depthwise 7 x 7 (x) + bias)[c]; wt = the taps tap-major [49][C]
int launch_cnx_dwconv_ln(const float* x, int64_t ld, int n, int hh, int ww, const float* wt, const float* bias, const float* gamma,
                         const float* beta, int C, float eps, float* A, int split, hipStream_t stream);
// row 0 of DINOv3ConvNextModel: LayerNorm(mean over the hw pixels of each frame) -> cls_f32 / cls_f16 [n][C]; `nonfinite` as
// launch_final_norm_cls
int launch_cnx_pool_ln(const float* x, int64_t ld, int n, int hw, const float* gamma, const float* beta, int C, float eps,
                       float* cls_f32, f16* cls_f16, unsigned* nonfinite, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// classifier head (all fp32)
// ---------------------------------------------------------------------------------------------
struct Gemm32Params {
    const float* A; int64_t lda;   // [M][lda], first K columns used
    const float* W;                // [N_alloc][K]
    const float* bias;             // [N] or nullptr
    float* out; int64_t ldo;       // [M][ldo]
    int64_t M; int N; int N_alloc; int K;   // N % 4 == 0, K % 32 == 0
    // split-K (head training's weight gradients: K = windows x seq_len, only a handful of output tiles):
    // grid.z = splits, block z accumulates k in [z*K, (z+1)*K) of operands whose row strides are lda / ldw and
    // writes its partial tile to out + z*split_stride (no bias); launch_splitk_reduce adds the partials in order.
    int64_t ldw;          // row stride of W (0: K)
    int splits;           // 0/1: plain GEMM
    int64_t split_stride; // floats between partial outputs
};
int launch_gemm_f32(const Gemm32Params& p, int gelu, hipStream_t stream);
// dst[i] = sum_z partial[z*stride + i], z ascending (deterministic), i < n
int launch_splitk_reduce(const float* partial, int splits, int64_t stride, int64_t n, float* dst, hipStream_t stream);

struct HeadDims {
    int I, C, T, Bn, L0, h;   // in_features, classes, seq_len, bottleneck dim, lin0 dim, lstm hidden
    int NS;                   // bottleneck streams: 3 (cls, delta, acc) or 2 when use_acceleration = False
    int lo, hi;               // centre window [lo, hi) in window time
    int NPROJ;                // projection width: NS*Bn + C rounded up to a multiple of 4
    float alpha;
};

// fp16 rows -> fp32 rows (exact), n elements
int launch_f16_to_f32(const f16* src, float* dst, int64_t n, hipStream_t stream);

// Per-window EMA / delta / acceleration on the PROJECTED rows, + bias, GELU, LayerNorm -> aug[w][t][3Bn];
// also the linear branch lin_logits[w][C] = mean_{t in centre}(EMA(proj_lin1)_t) + b_lin1.
// sliding: proj row of (w,t) = clamp(w0 + w + t - T/2, 0, n_frames-1) - r0 ; else (w*T + t).
int launch_head_expand(const float* proj, const HeadDims& d, const float* b_bott, const float* ln_w,
                       const float* ln_b, const float* b_lin1, int64_t n_windows, int sliding, int64_t w0,
                       int64_t r0, int64_t n_frames, float* aug, float* lin_logits, hipStream_t stream);
// xl[w][t][:] -= mean_t xl[w][t][:]
int launch_head_centre(float* xl, int64_t n_windows, int T, int L0, hipStream_t stream);
// Recurrent half of one BiLSTM layer: gin[w][t][dir*4h + gate*h + unit] holds W_ih x + b; runs fwd steps
// 0..ohi-1 and bwd steps T-1..olo, writes hout[w][t-olo][dir*h + unit] for t in [olo,ohi).  The last
// layer uses the centre window (olo,ohi) = (lo,hi); inner layers of a stacked LSTM use (0,T).
int launch_head_lstm(const float* gin, const float* w_hh, const HeadDims& d, int olo, int ohi, int64_t n_windows,
                     float* hout, hipStream_t stream);
// attention pooling + lin2 + gate lerp + softmax(logits / max(1e-3, T))
int launch_head_pool(const float* hout, const float* lin_logits, const HeadDims& d, const float* w_att,
                     float b_att, float att_temp, const float* w_lin2, const float* b_lin2, float gate_sigmoid,
                     float temperature, int64_t n_windows, float* probs, float* logits, float* latent,
                     hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// classifier-head training (head_train_kernels.hip; orchestration in api_head_train.hip)
// ---------------------------------------------------------------------------------------------
constexpr int COLSUM_CHUNKS = 64;

struct TrainExpandParams {
    const float* proj;       // [w][T][NPROJ] per-position projections (cls | delta | acc | lin1 | pad)
    const float* tmat;       // [3][T][T] temporal operators (EMA, delta o EMA, accel o EMA)
    const float* lin_vec;    // [T] mean over the centre window of the EMA rows
    const float *b_bott, *ln_w, *ln_b, *b_lin1;
    int T, Bn, NPROJ, C;
    int NS;                      // bottleneck streams (3, or 2 without the acceleration stream)
    unsigned long long key[3];   // dropout stream keys of the three bottlenecks for this step
    unsigned thr;                // keep <=> hash24 >= thr
    float scale;                 // 1 / (1 - p)
};
struct TrainPoolParams {
    const float *hout, *lin_logits, *w_att, *b_att, *att_temp, *w_lin2, *b_lin2, *gate;
    int T, H2, C, lo, hi;
};

// dst [cols][rows_pad] = src^T, columns rows..rows_pad zero-filled
int launch_transpose_pad(const float* src, int64_t rows, int cols, int64_t ld, float* dst, int64_t rows_pad, hipStream_t st);
size_t train_expand_lds_bytes(int T, int Bn, int NPROJ);     // dynamic LDS the expand kernels need (<= 160 KiB)
// host (api_head_train.hip): the temporal operators a trainer uploads, tmat [3][T][T] and lin_vec [T]; T >= 3, 0 <= lo < hi <= T
void head_build_temporal(int T, double alpha, int lo, int hi, float* tmat, float* lin_vec);
int launch_train_expand_fwd(const TrainExpandParams& p, int64_t n_windows, float* Y, float* aug, float* lin_logits, hipStream_t st);
int launch_train_expand_bwd(const TrainExpandParams& p, int64_t n_windows, const float* Y, const float* daug, const float* dlin,
                            float* dproj, float* part, hipStream_t st);
int launch_gelu_dropout(const float* Z, float* io, int64_t n, unsigned long long key, unsigned thr, float scale, int backward,
                        hipStream_t st);
int launch_lstm_train_fwd(const float* gin, const float* w_hh, int h, int T, int64_t n_windows, float* act, float* cst,
                          float* hout, hipStream_t st);
int launch_lstm_train_bwd(const float* dhout, const float* act, const float* cst, const float* hout, const float* w_hh, int h,
                          int T, int64_t n_windows, float* dgin, float* hprev, hipStream_t st);
int launch_pool_train_fwd(const TrainPoolParams& p, int64_t n_windows, float* attw, float* scores, float* latent,
                          float* lstm_logits, float* final_logits, hipStream_t st);
int launch_pool_train_bwd(const TrainPoolParams& p, int64_t n_windows, const float* attw, const float* scores,
                          const float* lstm_logits, const float* dfinal, const float* dlat_cov, float* dhout,
                          float* dlstm_logits, float* dlin_logits, float* part, hipStream_t st);
int launch_ce_terms(const float* logits, const int* labels, const float* cw, int64_t n, int C, float eps, float* terms,
                    hipStream_t st);
int launch_ce_grad(const float* logits, const int* labels, const float* cw, const float* sums, int64_t n, int C, float eps,
                   float* dlogits, hipStream_t st);
int launch_cov_offdiag(const float* cov, int n, float cscale, float gscale, float* G, float* sq, hipStream_t st);
int launch_sub_colmean(const float* src, const float* colsum, int64_t rows, int cols, float* dst, hipStream_t st);
// deterministic column sums of src [rows][cols] (row stride ld): dst[c] = scale * sum_r src[r][c]; tmp: COLSUM_CHUNKS * cols floats
int launch_colsum(const float* src, int64_t rows, int cols, int64_t ld, float scale, float* tmp, float* dst, hipStream_t st);
int launch_add_vec(const float* a, const float* b, float* out, int n, hipStream_t st);      // b == nullptr: copy
int launch_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float wd, int64_t wd_lo, int64_t wd_hi,
                     float wd_special, int step, hipStream_t st);
void adam_bias_corrections(float lr, int step, float* lr_c1, float* inv_sqrt_c2);      // what launch_adam_step hands its kernel

// Trial-batched forms of the small kernels above, for the k <= TRAIN_MULTI_MAX trainers of one
// cbas_head_train_step_rows_multi call: entry j of each table is trainer j's operands of the single-trial launcher, and the
// result is bit for bit what that launcher writes (same per-element expressions, same COLSUM_CHUNKS split of the rows).
// An entry whose count (n / cols) is 0 takes no part.  The tables travel as kernel arguments.
constexpr int TRAIN_MULTI_MAX = 8;
struct GeluBatch {
    const float* Z[TRAIN_MULTI_MAX]; float* io[TRAIN_MULTI_MAX]; int64_t n[TRAIN_MULTI_MAX]; unsigned long long key[TRAIN_MULTI_MAX];
    unsigned thr[TRAIN_MULTI_MAX]; float scale[TRAIN_MULTI_MAX];
};
struct CeBatch {      // out: terms (launch_ce_terms) or dlogits (launch_ce_grad, which also reads sums)
    const float* logits[TRAIN_MULTI_MAX]; const int* labels[TRAIN_MULTI_MAX]; const float* cw[TRAIN_MULTI_MAX];
    const float* sums[TRAIN_MULTI_MAX]; float* out[TRAIN_MULTI_MAX]; int64_t n[TRAIN_MULTI_MAX]; int C[TRAIN_MULTI_MAX];
    float eps[TRAIN_MULTI_MAX];
};
struct CovBatch {
    const float* cov[TRAIN_MULTI_MAX]; float* G[TRAIN_MULTI_MAX]; float* sq[TRAIN_MULTI_MAX]; int n[TRAIN_MULTI_MAX];
    float cscale[TRAIN_MULTI_MAX], gscale[TRAIN_MULTI_MAX];
};
struct ColsumBatch {  // scale 1
    const float* src[TRAIN_MULTI_MAX]; float* tmp[TRAIN_MULTI_MAX]; float* dst[TRAIN_MULTI_MAX]; int64_t rows[TRAIN_MULTI_MAX];
    int64_t ld[TRAIN_MULTI_MAX]; int cols[TRAIN_MULTI_MAX];
};
struct VecBatch {     // b[j] == nullptr: copy
    const float* a[TRAIN_MULTI_MAX]; const float* b[TRAIN_MULTI_MAX]; float* out[TRAIN_MULTI_MAX]; int n[TRAIN_MULTI_MAX];
};
struct AdamBatch {    // lr_c1 / inv_sqrt_c2 from adam_bias_corrections
    float* p[TRAIN_MULTI_MAX]; const float* g[TRAIN_MULTI_MAX]; float* m[TRAIN_MULTI_MAX]; float* v[TRAIN_MULTI_MAX];
    int64_t n[TRAIN_MULTI_MAX], wd_lo[TRAIN_MULTI_MAX], wd_hi[TRAIN_MULTI_MAX];
    float lr_c1[TRAIN_MULTI_MAX], inv_sqrt_c2[TRAIN_MULTI_MAX], wd[TRAIN_MULTI_MAX]; float wd_special;
};
int launch_gelu_dropout_multi(const GeluBatch& b, int k, int backward, hipStream_t st);
int launch_ce_multi(const CeBatch& b, int k, int grad, hipStream_t st);
int launch_cov_offdiag_multi(const CovBatch& b, int k, hipStream_t st);
int launch_colsum_multi(const ColsumBatch& b, int k, hipStream_t st);
int launch_add_vec_multi(const VecBatch& v, int k, hipStream_t st);
int launch_adam_step_multi(const AdamBatch& a, int k, hipStream_t st);

// rows_gather.hip: x_out[w][t][:] = float(rows_f16[first_row[w] + t][:]); rows outside [0, n_rows) read as zeros.
// Returns -1 for a null pointer, a non-positive size or a window beyond the limits below.
constexpr int ROWS_GATHER_MAX_SEQ = 1 << 16;
constexpr int64_t ROWS_GATHER_MAX_WINDOW = (int64_t)1 << 23;      // seq_len * dim elements (grid.y stays under 65 536 blocks)
int launch_rows_gather(const uint16_t* rows_f16, int64_t n_rows, int dim, const int64_t* first_row, int n_windows, int seq_len,
                       float* x_out, hipStream_t st);

// head_score_kernels.hip: the per-batch host work of the reference's scoring and calibration loops, on the device.
// launch_head_score: pred[w] = first index of the row maximum of logits (n, C) (-1 for a row with a NaN), confusion[y][pred] += 1
// (64-bit integer atomics; labels / confusion may both be null, pred may be null); *flags |= the bits below.
constexpr int HEAD_SCORE_MAX_CLASSES = 64;
constexpr unsigned HEAD_SCORE_FLAG_NAN = 1u;        // a logit row holds a NaN
constexpr unsigned HEAD_SCORE_FLAG_LABEL = 2u;      // a label outside [0, C)
int launch_head_score(const float* logits, const int* labels, int64_t n, int C, int* pred, unsigned long long* confusion,
                      unsigned* flags, hipStream_t st);
// launch_logits_nll: out2 = {mean cross-entropy of logits / temp, its derivative with respect to temp}, summed in a fixed
// order.  partials: LOGITS_NLL_MAX_BLOCKS 8-byte words; ticket: the first word of a 16-byte block that the launcher zeroes.
constexpr int LOGITS_NLL_MAX_BLOCKS = 128;
int launch_logits_nll(const float* logits, const int* labels, int64_t n, int C, float temp, unsigned long long* partials,
                      unsigned* ticket, float* out2, hipStream_t st);

// head_report_kernels.hip: the disagreement report of a training job (backend/workthreads.py:760-803) on device probabilities.
// launch_probs_top1: pred[r] = first index of the row maximum of probs (n, C) and conf[r] = that maximum; a row with a NaN gets
// pred -1, conf NaN and *flags |= HEAD_SCORE_FLAG_NAN.
int launch_probs_top1(const float* probs, int64_t n, int C, int* pred, float* conf, unsigned* flags, hipStream_t st);
// The run scan.  All pointers are device pointers; clip_table is (n_clips, 2) = (first frame in pred / conf, frames).
struct RunsParams {
    const int* pred;
    const float* conf;
    int64_t n_frames_total;
    const int64_t* clip_table;
    int n_clips;
    const int *inst_clip, *inst_start, *inst_end, *inst_label;
    int n_instances;
    const int* name_rank;
    int n_classes;
};
struct RunRecord {          // = cbas_disagreement_run of include/cbas_mi355x.h
    int instance, start_frame, end_frame, model_prediction;
    double model_confidence;
};
constexpr unsigned RUNS_FLAG_CLIP = 1u;     // an instance names a clip outside the table
constexpr unsigned RUNS_FLAG_LABEL = 2u;    // a label outside [-1, C)
constexpr unsigned RUNS_FLAG_RANGE = 4u;    // start < 0 or end < start
constexpr unsigned RUNS_FLAG_TABLE = 8u;    // a table entry outside the n_frames_total frames
constexpr unsigned RUNS_FLAG_PRED = 16u;    // a prediction outside [-1, C)
// launch_runs_count: counts[i] = runs of instance i, offsets[0 .. n_instances] = their exclusive scan and the total; *flags |= the
// bits above (a refused instance counts 0 runs).  launch_runs_emit: the n_records = offsets[n_instances] records, ordered by
// (instance, run start); the caller has checked the flags and the room in `records`.
int launch_runs_count(const RunsParams& p, int* counts, long long* offsets, unsigned* flags, hipStream_t st);
int launch_runs_emit(const RunsParams& p, const long long* offsets, RunRecord* records, long long n_records, unsigned* flags,
                     hipStream_t st);
// launch_runs_scan: offsets[i] = counts[0] + ... + counts[i - 1] for i in [0, n], by one workgroup (the scan both record
// writers share).
int launch_runs_scan(const int* counts, int n, long long* offsets, hipStream_t st);

// head_post_kernels.hip: what CBAS does with a clip's probabilities after inference (backend/cbas.py:903-1000), on the device.
// All clips lie back to back in the per-frame arrays; clip_table is (n_clips, 2) = (first frame, frames), as above.
constexpr unsigned POST_FLAG_TABLE = 1u;    // a table entry outside the n_frames_total frames
constexpr unsigned POST_FLAG_VALUE = 2u;    // a label outside [-1, C)
// launch_labels_median: out = scipy.signal.medfilt(pred, kernel_size) per clip (zero padding at both ends of every clip).
int launch_labels_median(const int* pred, int64_t n_frames_total, const int64_t* clip_table, int n_clips, int C, int kernel_size,
                         int* out, unsigned* flags, hipStream_t st);
struct LabelRunsParams {
    const int* key;
    const float* conf;
    int64_t n_frames_total;
    const int64_t* clip_table;
    int n_clips, n_classes, use_threshold;
    double threshold;
};
struct LabelRunRecord {     // = cbas_label_run of include/cbas_mi355x.h
    int clip, start_frame, end_frame, label;
    double confidence;
};
// launch_label_runs_count: counts[c] = runs of clip c, offsets = their exclusive scan and the total; *flags |= POST_FLAG_*.
// launch_label_runs_emit: the first min(offsets[n_clips], capacity) records ordered by (clip, start); reads the total on the device.
int launch_label_runs_count(const LabelRunsParams& p, int* counts, long long* offsets, unsigned* flags, hipStream_t st);
int launch_label_runs_emit(const LabelRunsParams& p, const long long* offsets, LabelRunRecord* records, long long capacity,
                           unsigned* flags, hipStream_t st);
// launch_activity_bins: bins[j] += frames f of bin j with (double)p[f][b] * is_max(f) >= threshold; the caller zeroes bins.
int launch_activity_bins(const float* probs, int64_t n, int C, int behavior, double threshold, int64_t bin_frames,
                         unsigned long long* bins, int64_t n_bins, hipStream_t st);

// patch_pca.hip: PCA of patch features.  Rows as cbas_enc_forward_*_tokens lays them out; a problem is one
// covariance: row m of problem b is patch row m % P of frame b * frames_per_problem + m / P (FRAME scope: frames_per_problem = 1,
// M = P; BATCH scope: one problem, frames_per_problem = n, M = n P).
constexpr int PCA_CHUNK = 1024;          // rows per partial covariance: fixed, whatever n and the device
constexpr int PCA_MEAN_CHUNK = 64;       // rows per partial column sum
constexpr int PCA_MAX_K = 8, PCA_MAX_D = 1536;
struct PcaRows {
    const float* x;
    int64_t ld;
    int T, n_prefix, P;
    int64_t M;
    int frames_per_problem;
};
int64_t pca_cov_chunks(int64_t M);       // partial covariances per problem
int64_t pca_mean_chunks(int64_t M);      // partial column sums per problem
// mean [nprob][D]; tmp: nprob * pca_mean_chunks(M) * D floats
int launch_pca_mean(const PcaRows& r, int nprob, int D, float* tmp, float* mean, hipStream_t st);
// part: nprob * pca_cov_chunks(M) * D * D floats; on return problem b's D x D covariance (exactly symmetric) starts at
// part + b * pca_cov_chunks(M) * D * D
int launch_pca_cov(const PcaRows& r, int nprob, int D, const float* mean, float* part, hipStream_t st);
// the k leading eigenpairs of nprob symmetric D x D matrices (problem b at C + b * c_stride) by `iters` rounds of subspace
// iteration and a Rayleigh-Ritz step: comp [nprob][k][D], eig [nprob][k] descending, total_var [nprob] = trace; Z: nprob * k * D floats
int launch_pca_eig(const float* C, int64_t c_stride, int nprob, int D, int k, int iters, float* Z, float* comp, float* eig,
                   float* total_var, hipStream_t st);
// scores [n][P][k] = (x - mean_b) . comp_b[j]; basis b of frame f is f * basis_step (0: one basis for every frame, 1: one per frame)
int launch_pca_project(const float* x, int64_t ld, int n, int T, int n_prefix, int D, int k, int basis_step, const float* mean,
                       const float* comp, float* scores, hipStream_t st);

// patch_kmeans.hip: k-means of patch features.  Rows and problems as above (PcaRows); every per-cluster sum
// and the inertia are formed per chunk of KMEANS_CHUNK rows in ascending row order, the chunks then added in ascending order.
constexpr int KMEANS_CHUNK = 64;         // rows per partial sum: fixed, whatever n and the device
constexpr int KMEANS_MAX_K = 16;
inline int64_t kmeans_chunks(int64_t M) { return (M + KMEANS_CHUNK - 1) / KMEANS_CHUNK; }
// the seeds of every problem: cur [nprob][k][D] (seeding order), init_index [nprob][k]; scratch: rn, mind [nprob][M], tmp [nprob]
// [chunks][D], mean [nprob][D], bestv / besti [nprob][chunks]
int launch_kmeans_seed(const PcaRows& r, int nprob, int D, int k, int normalize, float* cur, int32_t* init_index, float* rn, float* mind,
                       float* tmp, float* mean, float* bestv, int32_t* besti, hipStream_t st);
// one pass over the rows: problem b's rows against the k centroids at cent + b * cent_stride (0: one set for every problem).
// psum [nprob][chunks][k][D], pcount [nprob][chunks][16], pinertia [nprob][chunks]: all three, or all NULL (assignment only);
// labels / dist2 [nprob][M]: each may be NULL
int launch_kmeans_pass(const PcaRows& r, int nprob, int D, int k, int normalize, const float* cent, int64_t cent_stride, float* psum,
                       int32_t* pcount, float* pinertia, int32_t* labels, float* dist2, hipStream_t st);
// cur[j] = (sum of the chunks' psum[j]) / count_j where count_j > 0; inertia_out[b * inertia_ld] = the chunks' inertia
int launch_kmeans_update(const float* psum, const int32_t* pcount, const float* pinertia, int64_t nch, int nprob, int D, int k, float* cur,
                         float* inertia_out, int inertia_ld, hipStream_t st);
// the final counts and inertia from a pass, the clusters ordered by descending count (ties: seeding order): centroids [nprob][k][D],
// counts [nprob][k], order [nprob][16] (output position -> seeding position)
int launch_kmeans_finish(const int32_t* pcount, const float* pinertia, int64_t nch, int nprob, int D, int k, const float* cur,
                         float* inertia_out, int inertia_ld, float* centroids, int32_t* counts, int32_t* order, hipStream_t st);
