/*
 * cbas_mi355x_debug.h - bring-up, test and measurement-harness entry points of the DEBUG build of the library
 * (libcbas_mi355x_debug.so: `python -m cbas_amd.build --debug`, every source compiled with -DCBAS_BUILD_DEBUG=1).
 *
 * None of this is part of the drop-in boundary: the product library (libcbas_mi355x.so, include/cbas_mi355x.h) exports no
 * symbol declared here (tests/test_host_logic.py checks `nm -D`).  The GPU test suite and scripts/ load the debug build
 * (CBAS_BUILD_DEBUG=1 in the environment, read by cbas_amd/_lib.py); bench.py, __graft_entry__.smoke() and a CBAS
 * installation load the product build.  The debug build is a superset: same kernels, same product entry points.
 */
#ifndef CBAS_MI355X_DEBUG_H
#define CBAS_MI355X_DEBUG_H

#include "cbas_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 in the debug build (the product build does not export the symbol at all). */
int cbas_debug_build(void);

/* Bring-up/debug: run the forward pass only up to (layer, stage) and copy an internal buffer to
 * the host.  stage: 0 embeddings (x), then per layer 1 LN1(h16) 2 QKV(qkv16) 3 attention(h16)
 * 4 o_proj residual (x) 5 LN2 (h16) 6 up_proj+GELU (u16) 7 down_proj residual (x).
 * which: 0 x f32 (rows,D)  1 h16 (rows,D)  2 qkv16 (rows,3D)  3 u16 (rows,F); rows = n*T.
 * ConvNeXt handles (family 1): stop_layer 0 stops after the stem and its LayerNorm, stop_layer 1 + i after stage i (stop_stage
 * is ignored); which = 4 + stop_layer then reads that tensor as f32 (n*h*w, C) rows (frame, y, x), C = the stage's width. */
int cbas_enc_debug_forward_u8(cbas_enc* h, const uint8_t* frames_dev, int n, int height, int width,
                              int64_t frame_stride, int64_t row_stride, int64_t pixel_stride,
                              int stop_layer, int stop_stage);
int cbas_enc_debug_read(cbas_enc* h, int which, void* host_out, int64_t n_bytes);

/* Bring-up / tests: switch an implementation detail of the handle.  Options:
 *   "rope_lds"  1 (default): the q|k|v epilogue reads the RoPE angles, factorised by axis, from LDS; 0: from the [P][64]
 *               table in global memory ([tf]:96-121, 168-200 either way).  Bit-identical results.
 *   "ln_fold"   1: LayerNorm ([tf]:404, 410) is folded into the GEMMs around it - o_proj / down_proj write a fp16 copy of
 *               the residual stream and per-row statistics, q|k|v / up_proj run on it with gamma folded into their weights and
 *               apply mean / rstd in their epilogues; 0: separate LayerNorm kernels.  The two settings agree to fp16 rounding
 *               (both within the 1e-3 CLS bar, both batch-invariant); fp16 path with hidden_size a multiple of 256 only.
 *               Default 0: with two batches in flight the separate kernels already hide under the other lane's GEMMs
 *               (measured +0 ... +1 % for the fold; -5 % of kernel time with a single batch in flight).
 *   "split_kernels"  precision 4, PROCESS-WIDE: which GEMM forms run - bit 0 the ping-pong kernel's split-operand form
 *               (M > 256, N a multiple of 256), bit 1 the 8-slot-ring skinny form (M <= 256); cleared bits fall to the
 *               128 x 128 kernels.  -1 (default): both on, or as CBAS_SPLIT_PP=0 / CBAS_SPLIT_SKINNY=0 say.  Every
 *               setting forms the same products in the same order per output element: bit-identical rows. */
int cbas_enc_debug_option(cbas_enc* h, const char* name, int value);

/* Bring-up / tests (round 4).
 *   cbas_debug_gemm_split_bench: precision 4's GEMM alone on random split operands (epi 1 q|k|v, 2 residual, 3 GELU; tile 0 =
 *       planner, 128 / 160 / 192 / 256 rows of the ping-pong form, -1 = the 128 x 128 kernel), prints its block timeline.
 *   cbas_debug_mfma_neighbor: queue a register-only v_mfma_f32_32x32x16_f16 loop (every SIMD, two waves each, `iters` rounds
 *       of 8 MFMAs) on `stream`: the neighbour beside which the head is checked for bit-stability
 *       (scripts/head_beside_encoder.py).
 *   cbas_head_debug_read: copy the first n_floats of a head workspace buffer of the last pass to the host
 *       (0 rows32, 1 proj, 2 aug, 3 xl, 4 gin, 5 hout, 6 lin_logits); the device is synchronised first. */
int cbas_debug_gemm_split_bench(int M, int N, int K, int epi, int tile, int iters, float* ms_out);
/* the same GEMM through the ping-pong / skinny forms and through the 128 x 128 kernels on the same random operands:
 * n_diff = 32-bit output words that differ (0 by construction: same products in the same order) */
int cbas_debug_gemm_split_compare(int M, int N, int K, int epi, int tile, int64_t* n_diff);
int cbas_debug_mfma_neighbor(int iters, void* stream);
int cbas_head_debug_read(cbas_head* h, int which, float* host_out, int64_t n_floats);

/* Bring-up: time the fp16 GEMM kernel alone on random operands (GELU epilogue, M x N x K,
 * tile: 0 auto, 1 128x128, 2 256x128, 3 128x256, 4 256x256, 5+ experimental variants) and return a
 * position-weighted checksum of the fp16 output, so tile variants can be compared bit for bit.  3000 + tile: the gated MLP's
 * gate | up epilogue (EPI_SWIGLU) on the same N = 2 F columns, F columns stored (scripts/gated_rate.py). */
int cbas_debug_gemm_bench(int M, int N, int K, int tile, int iters, float* ms_out,
                          unsigned long long* checksum_out);

/* Bring-up: how kernels of two compute lanes share the chip.  Concurrently, each on its own stream, `iters` launches of
 * bit 0 the up projection (12 864 x 3072 x 768, GELU), bit 1 LayerNorm (12 864 x 768), bit 2 attention (64 x 201 tokens,
 * 12 heads), bit 3 the down projection (residual epilogue).  ms_out[0..3] = average milliseconds per launch of each
 * component on its stream, ms_out[4] = wall milliseconds of the whole run (scripts/overlap_kernels.py). */
int cbas_debug_overlap(int mode, int iters, float* ms_out);

/* Bring-up / tests: the MX-fp8 GEMM of precision 2 in isolation.  A (M x K) and W (N x K) fp32 host matrices are
 * quantised with the library's block quantiser (e4m3 elements, one E8M0 scale per 32 k-elements), multiplied by the
 * fp8 kernel (tile: 0 = the shape's default, 13..16 = a fixed ping-pong tile) and out = A_q W_q^T (M x N fp32) is
 * returned together with the quantised bytes and scales ([K/128][round_up(M,256)] resp. [K/128][N] dwords, byte b of
 * a dword = block b of that 128-wide K-tile).  N % 256 == 0, K % 256 == 0. */
int cbas_debug_gemm_f8(int M, int N, int K, int tile, const float* A_host, const float* W_host, float* out_host,
                       uint8_t* A8_host, uint32_t* Asc_host, uint8_t* W8_host, uint32_t* Wsc_host);

/* Tests: the up projection's GEMM (GELU epilogue, bias) in each of the four operand / result forms of the fp8 plans.
 * a_fp8: operands quantised as cbas_debug_gemm_f8 does (and returned the same way), else rounded to fp16.  out_fp8: the result
 * is MX-fp8 - out8_host [M][N] e4m3 bytes + outsc_host [N/128][round_up(M,256)] dwords, the layout the down projection reads
 * its A operand in - else out16_host [M][N] fp16 bits.  Pointers of the form not asked for may be NULL.  tile as above. */
int cbas_debug_gemm_gelu_forms(int M, int N, int K, int tile, int a_fp8, int out_fp8, const float* A_host, const float* W_host,
                               const float* bias_host, uint16_t* out16_host, uint8_t* out8_host, uint32_t* outsc_host,
                               uint8_t* A8_host, uint32_t* Asc_host, uint8_t* W8_host, uint32_t* Wsc_host);

/* Tests: ONE gate | up GEMM of a gated MLP (EPI_SWIGLU: h = silu(A W_g^T + b_g) * (A W_u^T + b_u), neither factor stored) on host
 * operands, in a chosen arithmetic and form (tests/test_gpu_gated_mlp.py compares it with a float64 reference).
 *   arith  0: fp16 operands, h stored as fp16 [M][F];  3: fp32, h stored as fp32 [M][F];
 *          4: split operands (A x a_scale, W x w_scale), h stored as the down projection's split image: per row and 32 columns 128
 *             bytes [hi 32 x fp16 | lo 32 x fp16] of h x out_scale, column 16 h + 4 g + e at position 8 g + 4 h + e of each half
 *   tile   arith 0: a GemmTile (0 the planner's choice - skinny for M <= 64; 1 / 2 / 3 / 4 / 7 the 16-wave 128x128 / 256x128 /
 *          128x256 / 256x256 / 192x256 tiles, 8 its 64x128 tile, 9 skinny, 13..17 the ping-pong tiles 256 / 192 / 160 / 128 rows /
 *          planner with tail, persistent once there are more tiles than CUs);  arith 4: the ping-pong form's tile height (0 planner)
 *   forms  arith 4: bit 0 the ping-pong form (M > 256), bit 1 the skinny form (M <= 256), 0 the 128 x 128 kernels, -1 the environment
 * A_host [M_alloc][lda] (lda >= K: lda = T * D reads one row per frame, the pruned last layer's CLS rows), W_g / W_u [F][K],
 * b_g / b_u [F]; F % 64 == 0, K % 64 == 0, lda % 32 == 0.  out_host [M][F] goes up first (canaries) and comes back. */
int cbas_debug_gemm_swiglu(int arith, int tile, int forms, int M, int M_alloc, int F, int K, int lda, const float* A_host,
                           const float* Wg_host, const float* Wu_host, const float* bg_host, const float* bu_host,
                           float a_scale, float w_scale, float out_scale, void* out_host);

/* Tests: ONE library GEMM launch on host operands (tests/test_gpu_kernel_reference.py compares it with a float64 reference).
 * The harness converts / splits the fp32 host operands on the device with the library's own routines (launch_convert_f16,
 * launch_pack_split_weight), uploads the initial output buffer (the residual stream for EPI_RESID / EPI_PATCH, canaries
 * elsewhere), launches, and copies the WHOLE output buffer back: rows >= M and columns >= N are the caller's canaries.
 *   arith  0: fp16 A and W (launch_gemm)   1: fp16 A, W as hi + lo (launch_gemm)   3: fp32 (launch_gemm_f32_vit)
 *          4: split operands (launch_gemm_f32_vit: ping-pong / skinny / 128 x 128 forms)
 *   epi    EPI_PATCH 0, EPI_QKV 1, EPI_RESID 2, EPI_GELU 3
 *   tile   arith 0 / 1: a GemmTile id (0 = the library's pick); arith 4: 0 = the planner, 128 / 160 / 192 / 256 = a ping-pong
 *          tile height, -1 = the 128 x 128 kernels (every form off)
 *   forms  arith 4, tile >= 0: vit32_split_set_forms bits (-1: the environment's); restored to -1 on return
 * out holds out_rows x ldo elements in the output's native width: fp32 (EPI_PATCH / EPI_RESID, every arith 3 epilogue),
 * fp16 (EPI_QKV / EPI_GELU of arith 0 / 1), or the raw split image at fp32 size (EPI_QKV / EPI_GELU of arith 4: the head-split
 * layout of the attention operands, resp. the GEMM operand layout scaled by out_scale); the test decodes it. */
typedef struct cbas_debug_gemm_args {
    int64_t struct_bytes;        /* sizeof(cbas_debug_gemm_args): a mismatch is rejected */
    int arith, epi, tile, forms, group_m;
    int M, M_alloc, N, K, lda, ldo, D, sec0;
    int T, n_prefix, P, rope_nh, rope_nw, rope_lds;   /* rope_lds: hand the kernels the by-axis table (LDS copy) too */
    int out_rows;                /* rows of the output buffer (>= M; EPI_PATCH: frames x T) */
    float in_scale, a_scale, w_scale, out_scale;
    const float* A;              /* [M_alloc][lda] */
    const float* W;              /* [N][K] */
    const float* bias;           /* [N] */
    const float* lambda;         /* [N] (EPI_RESID), or NULL */
    const float* pos;            /* [P][N] (EPI_PATCH), or NULL */
    const float* rope_cos;       /* [P][64] (EPI_QKV), or NULL: no RoPE */
    const float* rope_sin;
    void* out;                   /* in / out: [out_rows][ldo] */
} cbas_debug_gemm_args;
int cbas_debug_gemm_run(const cbas_debug_gemm_args* a);

/* Tests: ONE MX-fp8 GEMM launch (gemm_f16_8ph.hip, F8 = true) as api_enc.hip's vit_qkv / vit_tail issue it
 * (tests/test_gpu_fp8_gemm_reference.py compares it with the float64 product of exactly the bytes and scales it was given).
 *   epi      EPI_QKV 1 (fp16 out), EPI_RESID 2 (fp32 out: rows < M of `out` hold the residual), EPI_GELU 3 (fp16 out)
 *   tile     0 = launch_gemm's own choice (the 128-row tile, or the planner from 120 256-row tiles on), 13..17 = a ping-pong tile
 *   M_alloc  rows of A, passed as M_pad (>= M, any value: the kernel clamps its A rows and scale rows at M_alloc - 1)
 *   sc_lda   row stride of the A scale image in dwords (>= M_alloc)
 *   n_total, n0   W and its scale image have n_total rows; the launch multiplies by rows n0 .. n0 + N: W8 + n0 K, W_sc + n0 and,
 *            when n_total != N, sc_ldw = n_total (how vit_qkv hands the k | v weights of the fused q|k|v image to the launch)
 *   quantise 1: A [M_alloc][K] and W [n_total][K] are fp32 and are packed on the device with launch_pack_fp8_weight; the bytes and
 *               scale images come back in A8 / A_sc / W8 / W_sc
 *            0: A8 / A_sc / W8 / W_sc are the operands, used as given (A and W are not read)
 *   In both forms the four arrays are uploaded first, so what the packer does not write (scale dwords of rows M_alloc .. sc_lda)
 *   keeps the caller's fill.  A8 [M_alloc][K], A_sc [K/128][sc_lda], W8 [n_total][K], W_sc [K/128][n_total]: exactly these sizes
 *   are allocated on the device.  Byte b of a scale dword = block b of that 128-wide K-tile.
 *   The q|k|v fields, bias, lambda and out ([out_rows][ldo], uploaded first, copied back whole) are those of cbas_debug_gemm_args.
 * N % 256 == 0, K % 256 == 0. */
typedef struct cbas_debug_gemm_f8_args {
    int64_t struct_bytes;        /* sizeof(cbas_debug_gemm_f8_args): a mismatch is rejected */
    int epi, tile, group_m, quantise;
    int M, M_alloc, N, K, sc_lda, n_total, n0, ldo, out_rows;
    int D, sec0, T, n_prefix, P, rope_nh, rope_nw, rope_lds;
    const float* A;              /* quantise 1: [M_alloc][K] */
    const float* W;              /* quantise 1: [n_total][K] */
    uint8_t* A8;                 /* [M_alloc][K] e4m3 bytes: out (quantise 1) / in (0) */
    uint32_t* A_sc;              /* [K/128][sc_lda] */
    uint8_t* W8;                 /* [n_total][K] */
    uint32_t* W_sc;              /* [K/128][n_total] */
    const float* bias;           /* [N] */
    const float* lambda;         /* [N] (EPI_RESID), or NULL */
    const float* rope_cos;       /* [P][64] (EPI_QKV), or NULL: no RoPE */
    const float* rope_sin;
    void* out;                   /* in / out: [out_rows][ldo], fp16 (EPI_QKV / EPI_GELU) or fp32 (EPI_RESID) */
} cbas_debug_gemm_f8_args;
int cbas_debug_gemm_f8_run(const cbas_debug_gemm_f8_args* a);

/* Tests: ONE attention launch on a host q|k|v image [rows_alloc][3D] (q already x 1/8 and RoPE'd; rows_alloc >= n T, the
 * rows past n T are uploaded as given).  arith 0: fp16 operands (launch_attention); 3: fp32 (launch_attention_f32); 4: the
 * head-split operands of precision 4 (packed with store_head_split4 and the ATT_* scales), context in the split operand
 * layout x 16 as the encoder uses it.  q_cls [n][D] or NULL: the CLS-only form.  out: [out_rows][D] (fp16 / fp32 / split
 * image), uploaded first and copied back whole: rows >= n T (n) are the caller's canaries. */
typedef struct cbas_debug_attention_args {
    int64_t struct_bytes;
    int arith, n, T, D, n_heads, rows_alloc, out_rows;
    const float* qkv;
    const float* q_cls;
    void* out;
} cbas_debug_attention_args;
int cbas_debug_attention_run(const cbas_debug_attention_args* a);

/* Tests: ONE launch of the CLS attention map kernel (cls_attention.hip) on host arrays.  arith 0: fp16 operands (the values
 * are converted, so the caller supplies fp16-representable ones); 3: fp32; 4: the head-split hi | lo operands of precision 4
 * (q x 16, K x 4, packed as the q|k|v epilogue packs them).  q_host: n rows of stride ldq floats, K_host: n T rows of stride
 * ldk floats, the NH heads in columns 0 .. 64 NH - 1 of both (q already x 1/8); n_prefix = NP.  heads_host (n, NH, T) and
 * map_host (n, T - NP) fp32; either may be NULL, not both. */
int cbas_debug_cls_attention(int arith, const float* q_host, const float* K_host, int n, int T, int NH, int n_prefix,
                             int64_t ldq, int64_t ldk, float* heads_host, float* map_host);

/* Tests: ONE launch of the head-mean attention kernel (attention_rollout.hip) on host arrays, operands as
 * cbas_debug_cls_attention takes them except that q_host holds EVERY token's query: n T rows of stride ldq.  out_host (n, T, T)
 * fp32: out[b][i][t] = the mean over the heads of softmax_t(q[b T + i] . K[b T + t]); blend != 0: 0.5 out + 0.5 I.  A T whose row
 * does not fit the kernel's LDS is CBAS_EINVAL and nothing is launched. */
int cbas_debug_attention_mean(int arith, const float* q_host, const float* K_host, int n, int T, int NH, int64_t ldq, int64_t ldk,
                              int blend, float* out_host);
/* ... and of the rollout chain step: out = A R per frame, (n, T, T) fp32 each. */
int cbas_debug_rollout_step(const float* A_host, const float* R_host, int n, int T, float* out_host);

/* Tests: ONE launch of a row-wise encoder kernel on host operands (tests/test_gpu_rows_reference.py compares it with the float64
 * references of oracle/kernel_ref.py).  The harness uploads x (x_bytes) and the caller's pre-filled output images (out_bytes /
 * out2_bytes / *counter), runs exactly one launcher on the default stream and copies the whole output images back: whatever
 * the launch does not own is the caller's canary.  It refuses (CBAS_EINVAL, nothing launched) every shape a launcher would
 * mis-handle: M or n <= 0, D % 4 != 0 (LN_SPLIT and the ConvNeXt ops: D % 32) or beyond the launcher's switch (ViT 1280, LN_F8
 * 256 .. 1024 in steps of 128, ConvNeXt 1536), ld < D, sc_ld < M, null pointers, and any row / frame / pixel stride whose last
 * read or write would leave x_bytes / out_bytes / out2_bytes.
 *   op                launcher                              x                          out (out2)
 *   LN_F16            launch_layernorm_f16                  [M][ld] f32                [M][D] fp16
 *   LN_F32, LN_SPLIT  launch_layernorm_f32 (split 0 / 1)    [M][ld] f32                [M][D] f32 / split image
 *   LN_F8             launch_layernorm_f8                   [M][ld] f32                [M][D] e4m3 bytes (out2: [D/128][sc_ld] dwords)
 *   FINAL_CLS         launch_final_norm_cls                 [n][T][D] f32 (row 0 read) cls_f32 [n][D] (out2: cls_f16 [n][D]); either may be NULL
 *   CNX_STEM_U8       launch_cnx_stem_im2col_u8 (split)     bytes, the three strides   A [n (h/4) (w/4)][32]
 *   CNX_STEM_F32      launch_cnx_stem_im2col_f32 (split)    [n][h][w] f32              A [n (h/4) (w/4)][32]
 *   CNX_LN_ROWS       launch_cnx_ln_rows                    -                          in place: [M][ld] f32
 *   CNX_DOWNSAMPLE    launch_cnx_downsample (split)         [n][h][w][ld] f32          A [n (h/2) (w/2)][4 D]
 *   CNX_DWCONV_LN     launch_cnx_dwconv_ln (split)          [n][h][w][ld] f32          A [n h w][D]; wt [49][D], bias [D]
 *   CNX_POOL_LN       launch_cnx_pool_ln                    [n][h w][ld] f32           as FINAL_CLS
 *   TOKEN_ROWS        h = w = 0: launch_final_norm_rows     [M][ld] f32                f32 rows [M][sc_ld] (out2: fp16 rows [M][sc_ld])
 *                     else: launch_cnx_token_rows           [n][h w][ld] f32           rows [n (h w + 1)][sc_ld], both forms; either may be NULL
 *   TOKEN_SIM         launch_token_similarity               [n][T][ld] f32             map [n][T - M] f32
 * TOKEN_ROWS reads the output images' row stride from sc_ld (>= D, % 4; ld likewise).  TOKEN_SIM reads the prefix rows P0 from M
 * (0 <= M < T) and the per-frame query indices, n int32, from wt (NULL: row 0); split = 1 runs the fp16 form on the image
 * converted to fp16 (round to nearest even).
 * counter (FINAL_CLS / CNX_POOL_LN / TOKEN_ROWS): the non-finite counter, in / out; NULL hands the launcher nonfinite = NULL. */
enum {
    CBAS_DEBUG_ROWS_LN_F16 = 0, CBAS_DEBUG_ROWS_LN_F32 = 1, CBAS_DEBUG_ROWS_LN_SPLIT = 2, CBAS_DEBUG_ROWS_LN_F8 = 3,
    CBAS_DEBUG_ROWS_FINAL_CLS = 4, CBAS_DEBUG_ROWS_CNX_STEM_U8 = 5, CBAS_DEBUG_ROWS_CNX_STEM_F32 = 6,
    CBAS_DEBUG_ROWS_CNX_LN_ROWS = 7, CBAS_DEBUG_ROWS_CNX_DOWNSAMPLE = 8, CBAS_DEBUG_ROWS_CNX_DWCONV_LN = 9,
    CBAS_DEBUG_ROWS_CNX_POOL_LN = 10, CBAS_DEBUG_ROWS_TOKEN_ROWS = 11, CBAS_DEBUG_ROWS_TOKEN_SIM = 12
};
typedef struct cbas_debug_rows_args {
    int64_t struct_bytes;        /* sizeof(cbas_debug_rows_args): a mismatch is rejected */
    int op, split;               /* split: the split = 1 form of the CNX_STEM_* / CNX_DOWNSAMPLE / CNX_DWCONV_LN operand */
    int M;                       /* rows (LN_*, CNX_LN_ROWS) */
    int n;                       /* frames (every other op) */
    int D;                       /* D, resp. the ConvNeXt width C */
    int T;                       /* FINAL_CLS: tokens per frame */
    int h, w;                    /* frame height / width in pixels (stem), resp. the grid of the spatial ops */
    int sc_ld;                   /* LN_F8: rows of a K-tile's scale image */
    float eps;
    int64_t ld;                  /* row stride of x (CNX_LN_ROWS: of out) in elements */
    int64_t frame_stride, row_stride, pixel_stride;     /* CNX_STEM_U8, bytes */
    const void* x;
    int64_t x_bytes;
    const float* gamma;          /* [D] */
    const float* beta;           /* [D] */
    const float* wt;             /* CNX_DWCONV_LN: [49][D] */
    const float* bias;           /* CNX_DWCONV_LN: [D] */
    void* out;                   /* in / out */
    int64_t out_bytes;
    void* out2;                  /* in / out: LN_F8 scales, cls_f16 */
    int64_t out2_bytes;
    uint32_t* counter;           /* in / out, or NULL */
} cbas_debug_rows_args;
int cbas_debug_rows_run(const cbas_debug_rows_args* a);

/* Tests: ONE launch of a ViT ingest kernel or a create-time weight packer on host operands (tests/test_gpu_ingest_reference.py
 * compares it bit for bit with the references of oracle/kernel_ref.py), handled like cbas_debug_rows_run: the harness uploads
 * every in[] image and the caller's pre-filled out[] images whole, runs exactly one launcher on the default stream, synchronises
 * and copies every out[] image back whole - whatever the launch does not own is the caller's canary.
 *   op              launcher                               in[]                                    out[]
 *   IM2COL_U8       launch_im2col_u8                       0 bytes + the three strides,            0 A [n P][256] fp16, 1 x [n T][D] f32
 *                                                          1 prefix [n_prefix][D] f32
 *   IM2COL_F32      launch_im2col_f32                      0 [n][h][w] f32, 1 prefix               0 A [n P][512] fp16 (hi | lo), 1 x
 *   IM2COL_U8_F32   launch_im2col_u8_f32 (split 0 / 1)     as IM2COL_U8                            0 A [n P][256] f32 / split image, 1 x
 *   IM2COL_F32_F32  launch_im2col_f32_f32 (split 0 / 1)    as IM2COL_F32                           0 A [n P][256] f32 / split image, 1 x
 *   PATCH_W         launch_pack_patch_weight               0 w (D, 3, ps, ps) f32                  0 hi, 1 lo (D, 256) fp16; 2 hi2, 3 lo2 (D, 512)
 *   PATCH_W_F32     launch_pack_patch_weight_f32           0 w (D, 3, ps, ps) f32                  0 (D, 256) f32
 *   SPLIT_W         launch_pack_split_weight               0 [N][K] f32; scale                     0 split image [N][K] float slots
 *   CONVERT_F16     launch_convert_f16                     0 N floats                              0 hi, 1 lo [N] fp16
 *   INTERLEAVE      launch_interleave_gate_up              0 gate, 1 up [F][K] f32                 0 [2 F][K] f32
 *   FP8_W           launch_pack_fp8_weight                 0 [N][K] f32; n_total, n0               0 e4m3 bytes [N][K], 1 [K/128][n_total] dwords
 * The im2col ops: P = (h / ps) (w / ps) patches per frame, T = P + n_prefix rows of x per frame; x rows b T + r, r < n_prefix,
 * receive prefix row r and nothing else of x is written.  PATCH_W: out[1] and out[3] may be NULL together; CONVERT_F16: out[1] may
 * be NULL.  It refuses (CBAS_EINVAL, nothing allocated or launched): a NULL image other than those; n, D, N or F <= 0; ps
 * outside {14, 16}; h < ps or w < ps; n_prefix < 1; D % 4; K <= 0, K % 32 (SPLIT_W), K % 128 (FP8_W); F % 32; n0 < 0 or n0 + N >
 * n_total; a non-positive stride; and any stride or size whose last read or write would leave the stated byte counts. */
enum {
    CBAS_DEBUG_PACK_IM2COL_U8 = 0, CBAS_DEBUG_PACK_IM2COL_F32 = 1, CBAS_DEBUG_PACK_IM2COL_U8_F32 = 2,
    CBAS_DEBUG_PACK_IM2COL_F32_F32 = 3, CBAS_DEBUG_PACK_PATCH_W = 4, CBAS_DEBUG_PACK_PATCH_W_F32 = 5, CBAS_DEBUG_PACK_SPLIT_W = 6,
    CBAS_DEBUG_PACK_CONVERT_F16 = 7, CBAS_DEBUG_PACK_INTERLEAVE = 8, CBAS_DEBUG_PACK_FP8_W = 9
};
typedef struct cbas_debug_pack_args {
    int64_t struct_bytes;        /* sizeof(cbas_debug_pack_args): a mismatch is rejected */
    int op, split;               /* split: the split = 1 form of IM2COL_U8_F32 / IM2COL_F32_F32 */
    int n, h, w;                 /* im2col: frames, frame height / width in pixels */
    int ps;                      /* im2col, PATCH_W*: patch size, 14 or 16 */
    int n_prefix;                /* im2col: prefix rows per frame */
    int D;                       /* im2col: width of x and prefix; PATCH_W*: output rows */
    int K;                       /* SPLIT_W, INTERLEAVE, FP8_W: columns */
    int n_total, n0;             /* FP8_W: columns of the scale image, this call's first column */
    float scale;                 /* SPLIT_W */
    int64_t N;                   /* SPLIT_W, FP8_W: rows; CONVERT_F16: elements */
    int64_t F;                   /* INTERLEAVE: rows of gate and of up */
    int64_t frame_stride, row_stride, pixel_stride;     /* IM2COL_U8, IM2COL_U8_F32: bytes */
    const void* in[2];
    int64_t in_bytes[2];
    void* out[4];                /* in / out */
    int64_t out_bytes[4];
} cbas_debug_pack_args;
int cbas_debug_pack_run(const cbas_debug_pack_args* a);

/* Tests: ONE launch of a classifier-head kernel with an exact or tightly derivable reference on host operands
 * (tests/test_gpu_head_kernels_reference.py compares it with the references of oracle/kernel_ref.py): the exact-fp32 GEMM of
 * gemm_f32.hip (plain, fused GELU, split-K + its reduction) and the element-wise, reduction and optimiser kernels of
 * head_train_kernels.hip, single-trial or trial-batched (`_multi`).  The harness uploads every in[] image and the caller's
 * pre-filled out[] images (whole, out_bytes each: what the launch does not own is the caller's canary), runs exactly one
 * launcher on the default stream (GEMM with splits > 1: launch_gemm_f32 into the partial image, then launch_splitk_reduce),
 * synchronises and copies the out[] images back.  It refuses (CBAS_EINVAL, nothing launched): whatever launch_gemm_f32 rejects,
 * K < 32, lda / ldw below the k range read, ldo < N, split-K with ldo != N or split_stride < M N; k outside 1 ..
 * TRAIN_MULTI_MAX (8); multi = 1 for an op without a `_multi` launcher; a size below 1 (multi = 1: below 0); C outside 1 .. 64;
 * a label outside [0, C); rows_pad < rows; ld < cols; a trial-batched column sum with scale != 1; trial-batched Adam entries
 * whose wd_special differ; step < 1; and any image that is missing or smaller than what the launch reads or writes.
 *   op                launcher (multi = 1)                          in[0..3]                                   out[0..2]
 *   GEMM              launch_gemm_f32 (+ launch_splitk_reduce)      A [M][lda], W [N_alloc][ldw], bias [N] / -  result [M][ldo], partial (splits > 1)
 *   TRANSPOSE_PAD     launch_transpose_pad                          src [n][ld]                                dst [cols][rows_pad]
 *   GELU_DROPOUT_FWD  launch_gelu_dropout (.._multi) backward 0     Z [n]                                      io [n]
 *   GELU_DROPOUT_BWD  ... backward 1                                Z [n]                                      io [n] (d in, d out)
 *   CE_TERMS          launch_ce_terms (launch_ce_multi grad 0)      logits [n][C], labels [n] int32, cw [C] / - terms [n][2]
 *   CE_GRAD           launch_ce_grad (launch_ce_multi grad 1)       ..., in[3] sums [2]                        dlogits [n][C]
 *   COV_OFFDIAG       launch_cov_offdiag (.._multi)                 cov [n][n]                                 G [n][n], sq [n]
 *   SUB_COLMEAN       launch_sub_colmean                            src [n][cols], colsum [cols]               dst [n][cols]
 *   COLSUM            launch_colsum (.._multi: scale 1)             src [n][ld]                                tmp [64][cols], dst [cols]
 *   ADD_VEC           launch_add_vec (.._multi)                     a [n], b [n] / - (copy)                    out [n]
 *   ADAM              launch_adam_step (.._multi)                   g [n]                                      p [n], m [n], v [n]
 * n is the entry's element / window / row count.  multi = 0 runs the single-trial launcher on entry 0; multi = 1 runs the
 * `_multi` launcher on all k entries, which may differ in size (0 included: such an entry takes no part, its images may be
 * absent, and an absent image reaches the launcher's table as a null pointer - the kernels touch no entry past its count). */
enum {
    CBAS_DEBUG_HEAD_GEMM = 0, CBAS_DEBUG_HEAD_TRANSPOSE_PAD = 1, CBAS_DEBUG_HEAD_GELU_DROPOUT_FWD = 2,
    CBAS_DEBUG_HEAD_GELU_DROPOUT_BWD = 3, CBAS_DEBUG_HEAD_CE_TERMS = 4, CBAS_DEBUG_HEAD_CE_GRAD = 5,
    CBAS_DEBUG_HEAD_COV_OFFDIAG = 6, CBAS_DEBUG_HEAD_SUB_COLMEAN = 7, CBAS_DEBUG_HEAD_COLSUM = 8, CBAS_DEBUG_HEAD_ADD_VEC = 9,
    CBAS_DEBUG_HEAD_ADAM = 10
};
typedef struct cbas_debug_head_entry {
    int64_t n;                   /* elements / windows / rows (see the table) */
    int64_t rows_pad, ld;        /* TRANSPOSE_PAD; row stride of src (TRANSPOSE_PAD, COLSUM) */
    int64_t wd_lo, wd_hi;        /* ADAM: [wd_lo, wd_hi) decays with wd_special */
    uint64_t key;                /* GELU_DROPOUT_*: the dropout stream's key */
    int cols, C, step;
    uint32_t thr;                /* GELU_DROPOUT_*: keep <=> top 24 hash bits >= thr */
    float eps;                   /* CE_*: label smoothing */
    float scale;                 /* GELU_DROPOUT_*: 1 / (1 - p); COLSUM: the factor on the sums */
    float cscale, gscale;        /* COV_OFFDIAG */
    float lr, wd, wd_special;    /* ADAM */
    const void* in[4];
    int64_t in_bytes[4];
    void* out[3];                /* in / out */
    int64_t out_bytes[3];
} cbas_debug_head_entry;
typedef struct cbas_debug_head_args {
    int64_t struct_bytes;        /* sizeof(cbas_debug_head_args): a mismatch is rejected */
    int64_t entry_bytes;         /* sizeof(cbas_debug_head_entry): likewise */
    int op, multi, k;            /* k entries (GEMM, TRANSPOSE_PAD, SUB_COLMEAN: entry 0 holds the images) */
    int gelu, splits;            /* GEMM */
    int N, N_alloc, K;           /* GEMM (K: the k range of ONE split) */
    int64_t M, lda, ldw, ldo, split_stride;
    const cbas_debug_head_entry* entries;
} cbas_debug_head_args;
int cbas_debug_head_run(const cbas_debug_head_args* a);

/* Tests: ONE launch of a sequential classifier-head kernel on host operands (tests/test_gpu_head_seq_reference.py compares it with
 * the float64 references of oracle/kernel_ref.py): the recurrent LSTM of inference (head_kernels.hip) and of training with its
 * BPTT (head_train_kernels.hip), the attention pooling of both, and head_centre.  The harness uploads every in[] image and the
 * caller's pre-filled out[] images whole, runs exactly one launcher on the default stream, synchronises and copies every out[]
 * image back whole: what the launch does not own is the caller's canary.  It refuses (CBAS_EINVAL, nothing allocated or
 * launched): h not one of 16, 32, .. 128 (LSTM ops); n_windows < 1, T < 1; 0 <= lo < hi <= T violated; pooling with C outside
 * 1 .. 64 or H2 outside 1 .. 256, training pooling also with H2 % 32 != 0 or hi - lo > 128; CENTRE with L0 < 1; a NULL
 * non-optional image; an image smaller than what the launch reads or writes.
 *   op               launcher               in[]                                                     out[]
 *   LSTM_INFER       launch_head_lstm       gin [w][T][8h], w_hh [2][4h][h]                          hout [w][hi-lo][2h]
 *   LSTM_TRAIN_FWD   launch_lstm_train_fwd  gin, w_hh                                                act [w][T][8h], cst, hout [w][T][2h]
 *   LSTM_TRAIN_BWD   launch_lstm_train_bwd  dhout [w][T][2h], act, cst, hout, w_hh                   dgin [w][T][8h], hprev [w][T][2h]
 *   POOL_INFER       launch_head_pool       hout [w][hi-lo][H2], lin_logits [w][C], w_att [H2],      probs [w][C], logits [w][C], latent [w][H2]
 *                                           w_lin2 [C][H2], b_lin2 [C]                               (each may be NULL, not all)
 *   POOL_TRAIN_FWD   launch_pool_train_fwd  hout [w][T][H2], lin_logits, w_att, w_lin2, b_lin2       attw, scores [w][hi-lo], latent [w][H2],
 *                                                                                                    lstm_logits, final_logits [w][C]
 *   POOL_TRAIN_BWD   launch_pool_train_bwd  the five above, attw, scores, lstm_logits, dfinal        dhout [w][T][H2], dlstm_logits, dlin_logits
 *                                           [w][C], dlat_cov [w][H2] or NULL                         [w][C], part [w][H2 + 12]
 *   CENTRE           launch_head_centre     -                                                        xl [w][T][L0], in place
 * b_att, att_temp and gate are the scalars of the struct: POOL_INFER takes att_temp as the temperature already formed and gate
 * as sigmoid(gate); the training ops take the raw parameters (uploaded as one-element images) and form softplus / sigmoid. */
enum {
    CBAS_DEBUG_SEQ_LSTM_INFER = 0, CBAS_DEBUG_SEQ_LSTM_TRAIN_FWD = 1, CBAS_DEBUG_SEQ_LSTM_TRAIN_BWD = 2, CBAS_DEBUG_SEQ_POOL_INFER = 3,
    CBAS_DEBUG_SEQ_POOL_TRAIN_FWD = 4, CBAS_DEBUG_SEQ_POOL_TRAIN_BWD = 5, CBAS_DEBUG_SEQ_CENTRE = 6
};
typedef struct cbas_debug_head_seq_args {
    int64_t struct_bytes;        /* sizeof(cbas_debug_head_seq_args): a mismatch is rejected */
    int op;
    int h;                       /* LSTM ops: hidden units per direction */
    int H2;                      /* pooling ops: width of a hout row (2 h) */
    int T, lo, hi;               /* window length; the centre range (CENTRE ignores lo / hi; LSTM_TRAIN_*: unused) */
    int C, L0;
    int64_t n_windows;
    float b_att, att_temp, gate, temperature;
    const void* in[10];
    int64_t in_bytes[10];
    void* out[5];                /* in / out */
    int64_t out_bytes[5];
} cbas_debug_head_seq_args;
int cbas_debug_head_seq_run(const cbas_debug_head_seq_args* a);

/* Tests: ONE launch of a classifier-head expand kernel on host operands (tests/test_gpu_head_expand_reference.py compares it with
 * the float64 references of oracle/kernel_ref.py), handled like cbas_debug_head_seq_run: every in[] image and the caller's
 * pre-filled out[] images are uploaded whole, one launcher runs on the default stream, every out[] image is copied back whole.
 *   op          launcher                 in[]                                                          out[]
 *   INFER       launch_head_expand       0 proj [rows][NPROJ], 1 b_bott, 2 ln_w, 3 ln_b [NS Bn],        aug [w][T][NS Bn], lin_logits [w][C]
 *                                        4 b_lin1 [C]
 *   TRAIN_FWD   launch_train_expand_fwd  0 .. 4 as above (proj [w][T][NPROJ]), 5 tmat [3][T][T],        Y, aug [w][T][NS Bn], lin_logits [w][C]
 *                                        6 lin_vec [T]
 *   TRAIN_BWD   launch_train_expand_bwd  0 Y [w][T][NS Bn], 2 ln_w, 5 tmat, 6 lin_vec,                  dproj [w][T][NPROJ], part [w][3 NS Bn]
 *                                        7 daug [w][T][NS Bn], 8 dlin [w][C]
 * INFER without `sliding` reads proj row w T + t; with it, row clamp(w0 + w + t - T / 2, 0, n_frames - 1) - r0.
 * It refuses (CBAS_EINVAL, nothing allocated or launched): n_windows < 1; T outside 3 .. 101; Bn not 64, 128, 192 or 256; NS not
 * 2 or 3; C outside 1 .. 64; NPROJ below NS Bn + C or not a multiple of 4, TRAIN_BWD also NPROJ - NS Bn above the block's NS Bn
 * threads; INFER without 0 <= lo < hi <= T; a shape whose LDS need exceeds 160 KiB (INFER: T NS Bn floats; training:
 * train_expand_lds_bytes); training with thr >= 2^24; sliding with n_frames < 1 or with a clamped row outside the proj image;
 * a NULL image the op reads or writes, or one smaller than that.
 * cbas_debug_build_temporal (host only): tmat [3][T][T] and lin_vec [T] as a trainer with this T, ema_alpha and centre window
 * builds them (api_head_train.hip build_temporal); T in 3 .. 101, 0 <= lo < hi <= T. */
enum { CBAS_DEBUG_EXPAND_INFER = 0, CBAS_DEBUG_EXPAND_TRAIN_FWD = 1, CBAS_DEBUG_EXPAND_TRAIN_BWD = 2 };
typedef struct cbas_debug_head_expand_args {
    int64_t struct_bytes;        /* sizeof(cbas_debug_head_expand_args): a mismatch is rejected */
    int op;
    int T, Bn, NS, C, NPROJ;
    int lo, hi;                  /* INFER: the linear branch's centre window */
    int sliding;                 /* INFER */
    float alpha;                 /* INFER: the EMA weight */
    float scale;                 /* training: 1 / (1 - p) */
    uint32_t thr;                /* training: keep <=> top 24 hash bits >= thr */
    int64_t n_windows;
    int64_t w0, r0, n_frames;    /* INFER, sliding */
    uint64_t key[3];             /* training: the three streams' dropout keys */
    const void* in[9];
    int64_t in_bytes[9];
    void* out[3];                /* in / out */
    int64_t out_bytes[3];
} cbas_debug_head_expand_args;
int cbas_debug_head_expand_run(const cbas_debug_head_expand_args* a);
int cbas_debug_build_temporal(int T, float alpha, int lo, int hi, float* tmat, float* lin_vec);

/* Root-cause probe (round 5): run a kernel from a separately built code object IN PLACE of the library's head_expand_kernel
 * on this handle (same grid, block, dynamic LDS and arguments: scripts/probes/expand_r4/expand_r4.hip has the signature).
 * hsaco_path = NULL restores the library's kernel.  scripts/expand_rootcause.py builds instruction-level variants of the
 * round-4 kernel that returned wrong values beside MFMA-heavy neighbours and runs each one through the head this way. */
int cbas_head_debug_expand_module(cbas_head* h, const char* hsaco_path, const char* kernel_name);
/* Amplification for that probe.  mode 1: the next pass (run it on an idle device) copies its expand output to a reference
 * buffer; mode 2: every pass launches the probe kernel `repeat` times and compares every launch's rows bit for bit with
 * the reference ON THE DEVICE (differing rows are captured, 512 at most); mode 0: off.  cbas_head_debug_expand_stats:
 * counts4 = launches compared, launches with a differing row, differing rows, rows offered to the capture buffer;
 * rows_out receives up to max_rows captured rows of 2 + bottleneck_dim floats (row index = (window * T + t) * NS + stream,
 * launch number, the row's values); reset != 0 clears the counters and the capture buffer's fill. */
int cbas_head_debug_expand_repeat(cbas_head* h, int mode, int repeat);
int cbas_head_debug_expand_stats(cbas_head* h, uint64_t* counts4, float* rows_out, int max_rows, int reset);

/* Tests, host only (no device is touched): the position-table builder of cbas_enc_set_pos_interp.
 *   cbas_debug_pos_interp_matrix: W (out_size x in_size, row-major) = one axis' weights of `mode`'s filter.
 *   cbas_debug_pos_table: out (nh * nw, D) = the stored patch-position table src (G * G, D) resampled to nh x nw the way a
 *       handle in `mode` builds it (separable: width pass, then height pass; the stored table itself when nh = nw = G). */
int cbas_debug_pos_interp_matrix(int mode, int in_size, int out_size, float* W);
int cbas_debug_pos_table(int mode, const float* src, int G, int D, int nh, int nw, float* out);

#ifdef __cplusplus
}
#endif
#endif /* CBAS_MI355X_DEBUG_H */
