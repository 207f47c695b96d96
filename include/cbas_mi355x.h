/*
 * cbas_mi355x.h — C ABI of libcbas_mi355x.so, the MI355X (gfx950) implementation of the one hot
 * path of jones-lab-tamu/CBAS: streamed DINOv3-ViT frame encoding + sliding-window BiLSTM
 * classification.  Plain pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * What each entry point replaces in the reference (paths relative to the CBAS tree; "[tf]" =
 * transformers/models/dinov3_vit/modeling_dinov3_vit.py, the third-party file that holds the
 * encoder arithmetic the reference calls through AutoModel):
 *
 *   cbas_enc_create / cbas_enc_destroy     backend/cbas.py:651-670   DinoEncoder.__init__
 *                                          (AutoModel.from_pretrained(...).to(device), eval, freeze)
 *   cbas_enc_forward_f32                   backend/cbas.py:672-677   DinoEncoder.forward
 *                                          + [tf]:523-548 DINOv3ViTModel.forward (CLS row only)
 *   cbas_enc_forward_u8                    backend/cbas.py:431-436   green/255 preprocessing + encoder call
 *   cbas_enc_forward_u8_attn / _f32_attn   compare_encoders.py:36-49 the last layer's attention from the CLS token to
 *                                          the patch tokens, averaged over heads (output_attentions=True), beside the CLS rows
 *   cbas_enc_forward_u8_tokens / _f32_tokens   compare_encoders.py:36 / the golden scripts' model(pixel_values=x): the whole
 *                                          last_hidden_state (n, T, D) instead of row 0, and cosine maps over the patch rows
 *   cbas_enc_forward_u8_layers / _f32_layers   output_hidden_states=True / output_attentions=True of the same call: any layer's
 *                                          hidden state and CLS attention, and the attention rollout over the layers
 *   cbas_patch_pca_*                       (no counterpart: the reference draws attention only) PCA of the patch rows of that
 *                                          last_hidden_state, fitted and projected on the device
 *   cbas_patch_kmeans_*                    (no counterpart) k-means of the same patch rows: a cluster label per patch
 *   cbas_enc_submit_u8_host / cbas_enc_wait  backend/cbas.py:423-440 one iteration of the chunk loop
 *                                          (H2D copy, encode, D2H copy), made asynchronous
 *   cbas_head_create / cbas_head_destroy   backend/workthreads.py:427-447 ClassifierLSTMDeltas(...)
 *                                          + load_state_dict + .to(device).eval()
 *   cbas_head_forward_windows              backend/classifier_head.py:150-172 ClassifierLSTMDeltas.forward
 *   cbas_head_infer_f16                    backend/cbas.py:497-551   the window loop of infer_file
 *                                          (edge replicate padding, head, softmax(logits/max(1e-3,T)))
 *   cbas_fused_*                           backend/workthreads.py:316-328 + 488-498: EncodeThread -> _cls.h5 ->
 *                                          ClassificationThread, as one streaming session (rows stay in HBM)
 *   cbas_last_error                        Python exceptions raised on those paths
 *
 * Conventions
 *   - Every function returns 0 on success or a negative CBAS_E* code; no exception crosses the ABI.
 *     cbas_last_error() returns a thread-local, NUL-terminated description of the last failure.
 *   - "dev" pointers are HIP device pointers valid on the handle's device; "host" pointers are host
 *     memory owned by the caller.  The library owns its weights, workspaces, streams and pinned
 *     staging buffers; weights are copied during *_create.
 *   - `stream` is a hipStream_t passed as void* (NULL = HIP's null stream, as in the HIP API).  All
 *     *_forward_* / *_infer_* calls are asynchronous on that stream; the host-streamed
 *     submit/wait pair uses the handle's own copy and compute streams.
 *   - Handles are independent: distinct handles may be driven from distinct OS threads
 *     concurrently (the reference runs EncodeThread and ClassificationThread side by side,
 *     backend/workthreads.py:1256-1267).  One handle must not be used from two threads at once.
 */
#ifndef CBAS_MI355X_H
#define CBAS_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CBAS_OK            0
#define CBAS_EINVAL       -1   /* bad argument / unsupported configuration */
#define CBAS_EHIP         -2   /* a HIP runtime call failed */
#define CBAS_ENOMEM       -3
#define CBAS_ESTATE       -4   /* call sequence error (e.g. wait on an idle slot) */
#define CBAS_ERANGE       -5   /* a frame's CLS row came out NaN / infinite: an activation left the arithmetic mode's range */

/* Still 11 with cbas_rows_gather_windows / cbas_head_train_step_rows, with cbas_head_score_rows / cbas_logits_nll, with
 * cbas_enc_set_pos_interp, with cbas_enc_set_fp8_plan, with cbas_probs_top1 / cbas_disagreement_runs, with
 * cbas_labels_median / cbas_label_runs / cbas_activity_bins, with cbas_enc_forward_u8_attn / cbas_enc_forward_f32_attn, with
 * cbas_enc_forward_u8_tokens / cbas_enc_forward_f32_tokens, with cbas_patch_pca_* and with cbas_enc_forward_u8_layers /
 * cbas_enc_forward_f32_layers / cbas_enc_layers_scratch_bytes: they are additions.  No structure and no existing signature
 * changed, so a caller built against the earlier version 11 header runs unchanged. */
#define CBAS_ABI_VERSION   11

typedef struct cbas_enc  cbas_enc;
typedef struct cbas_head cbas_head;

/* ---- encoder ------------------------------------------------------------------------------ */

/* Mirrors the HF config.json fields of a DINOv3 ViT ([tf] configuration_dinov3_vit.py:74-101). */
typedef struct cbas_enc_config {
    int32_t hidden_size;          /* D: 384 / 768 / 1024 / 1280 (a multiple of 128, at most 1280; precision 2: at most 1024) */
    int32_t intermediate_size;    /* F: 4*D (a multiple of 128)                */
    int32_t num_layers;           /* L                                         */
    int32_t num_heads;            /* D / 64 (head_dim must be 64)              */
    int32_t num_register_tokens;  /* R (4 for the released checkpoints)        */
    int32_t patch_size;           /* 16 (DINOv3) or 14 (DINOv2)                */
    float   layer_norm_eps;       /* 1e-5                                      */
    float   rope_theta;           /* 100                                       */
    int32_t max_batch;            /* frames per encoder pass (workspace size)  */
    int32_t max_height;           /* largest frame the workspace must hold     */
    int32_t max_width;
    int32_t precision;            /* 0: fp16 operands, fp32 accumulate/residual (the fast mode; meets the 1e-3 CLS bar,
                                        not label identity - the host mirror's default is 4, see below)
                                     1: fp16 hi+lo split weights (2 MFMA/k-step)
                                     2: MX-fp8 throughput mode (BASELINE.json configs[4]): the QKV / o_proj / up / down
                                        GEMMs take e4m3 operands with one E8M0 scale per 32 k-elements - weights packed
                                        at create, activations quantised by the producing kernels (LayerNorm,
                                        attention, GELU epilogue) - on v_mfma_scale_f32_16x16x128_f8f6f4; accumulation,
                                        residual stream, attention, patch embedding and the CLS tail of the last
                                        layer are unchanged.  CLS error is a few 1e-2: held to label parity only.
                                        hidden_size and intermediate_size must be multiples of 256.
                                     3: fp32 end to end - the arithmetic of the reference's CPU path, which is the parity
                                        target (backend/cbas.py:433-434: autocast off on CPU; [tf]:523-548): fp32
                                        weights, activations, attention and LayerNorm, every contraction on
                                        v_mfma_f32_16x16x4_f32 (exact fp32 products and sums), the element-wise steps
                                        rounded where the reference's separate torch ops round.  CLS rows agree with
                                        the reference to a few 1e-6, so the fp16 rows written to _cls.h5 and the argmax
                                        labels are the reference's own.  ~1/7 of the default mode's frame rate.
                                     4: precision 3's buffers, element-wise arithmetic and attention, with every GEMM product
                                        formed on the fp16 matrix pipe from split operands: x = hi + lo (two fp16 halves, 22
                                        significant bits, stored in the GEMM's own tile order by the producing kernels and by
                                        the weight packer), a w ~ a_hi w_hi + a_hi w_lo + a_lo w_hi on
                                        v_mfma_f32_16x16x32_f16 with fp32 accumulation.  CLS rows are as close to the
                                        reference as precision 3's (measured: slightly closer - the MFMA sums each block of 32
                                        products before rounding into the accumulator); 2.4x its frame rate.  The split
                                        halves are fp16: after the fixed power-of-two scales an activation must stay below
                                        65 504 - LayerNorm rows as they are, |attention context| and |q| / 8 < 4 094, |k|, |v|
                                        and |GELU output| < 16 376 (far above what ViT checkpoints with "massive activation"
                                        channels produce: tests/test_gpu_fp32.py); precision 3 has no such bound.  A gated MLP
                                        (cbas_enc_create_mlp) stores silu(gate) * up where a GELU handle stores the GELU output,
                                        with the same scale of 4: |silu(gate) * up| < 16 376.  A value outside it becomes an
                                        infinite fp16 half, reaches the CLS row as a non-finite value and is reported as
                                        CBAS_ERANGE (cbas_enc_check_finite). */
    int32_t use_rope;             /* 1: DINOv3 (RoPE on patch rows, no additive position embedding)     */
    int32_t pos_embed_grid;       /* G > 0: DINOv2 (with registers, or plain with num_register_tokens = 0), learned (1+G*G, D)
                                     position embedding, bicubic-antialias interpolated to each frame's patch grid unless
                                     cbas_enc_set_pos_interp says otherwise; else 0 */
    /* ABI 11: the encoder family.  All-zero trailing fields keep the ViT behaviour of ABI 10. */
    int32_t family;               /* 0: ViT (the fields above); 1: DINOv3 ConvNeXt (transformers models/dinov3_convnext,
                                     DINOv3ConvNextModel: row 0 = LayerNorm(global mean pool of the last stage)).  ConvNeXt uses
                                     stage_widths / stage_depths, layer_norm_eps, max_batch, max_height, max_width and
                                     precision (3 or 4 only); hidden_size must equal stage_widths[3] (the row width), the
                                     other ViT fields are ignored.  Every width must be a multiple of 32, hidden_act exact-erf
                                     GELU (the caller checks the config; this struct has no activation field). */
    int32_t stage_widths[4];      /* ConvNeXt hidden_sizes: 96 192 384 768 (tiny / small)                          */
    int32_t stage_depths[4];      /* ConvNeXt depths: 3 3 9 3 (tiny), 3 3 27 3 (small)                               */
} cbas_enc_config;

/* Number of float32 elements cbas_enc_create expects in `weights`, in this order:
 *   cls_token[D], register_tokens[R*D], position_embeddings[(1+G*G)*D] (only when pos_embed_grid = G > 0),
 *   patch_weight[D*3*p*p], patch_bias[D],
 *   then per layer: norm1.w[D] norm1.b[D] q.w[D*D] q.b[D] k.w[D*D] k.b[D] (zeros for DINOv3) v.w[D*D] v.b[D] o.w[D*D] o.b[D]
 *                   ls1[D] norm2.w[D] norm2.b[D] up.w[F*D] up.b[F] down.w[D*F] down.b[D] ls2[D],
 *   then norm.w[D] norm.b[D].
 * Linear weights are (out_features, in_features) row-major, exactly the HF state_dict tensors.
 * family = 1 (ConvNeXt), with C_i = stage_widths[i] and the HF DINOv3ConvNextModel state-dict tensors as stored:
 *   stem: downsample_layers.0.weight[C0*3*4*4] .bias[C0], stem LayerNorm downsample_layers.1.weight[C0] .bias[C0],
 *   per stage i > 0: LayerNorm downsample_layers.0.weight[C_{i-1}] .bias[C_{i-1}], conv downsample_layers.1.weight[C_i*C_{i-1}*2*2]
 *                    .bias[C_i],
 *   per block of stage i (stage_depths[i] of them): depthwise_conv.weight[C*49] .bias[C], layer_norm.weight[C] .bias[C],
 *                    pointwise_conv1.weight[4C*C] .bias[4C], pointwise_conv2.weight[C*4C] .bias[C], gamma[C],
 *   then the final layer_norm.weight[C3] .bias[C3]. */
int64_t cbas_enc_weights_count(const cbas_enc_config* cfg);

int cbas_enc_create(const cbas_enc_config* cfg, const float* weights_host, int64_t n_weights,
                    int device_id, cbas_enc** out);

/* The MLP of a ViT layer.  cbas_enc_config has no field for it (its size is part of ABI 11), so the kind travels beside it:
 *   CBAS_MLP_GELU    down(gelu(up(x))): every ViT the two calls above build; cbas_enc_weights_count_mlp / cbas_enc_create_mlp with
 *                    this value ARE cbas_enc_weights_count / cbas_enc_create.
 *   CBAS_MLP_SWIGLU  down(silu(gate(x)) * up(x)): DINOv3ViTGatedMLP ([tf] modeling_dinov3_vit.py:360-373; use_gated_mlp = true,
 *                    hidden_act = "silu": ViT-S+/16 with D 384 / F 1536, ViT-H+/16 with D 1280 / F 5120).  family = 0, precision 0,
 *                    3 or 4.  Refused with CBAS_EINVAL and a message that says why: precision 2 (no MX-fp8 form of the gated
 *                    GEMM), precision 1 (no hi+lo form either - its use is bring-up, and no test would hold it to anything),
 *                    ConvNeXt, any other value of `mlp`.
 * Blob order for CBAS_MLP_SWIGLU: as documented above, with gate.w[F*D] gate.b[F] immediately before up.w[F*D] up.b[F] in every
 * layer (the HF state_dict order: mlp.gate_proj, mlp.up_proj, mlp.down_proj).  gate and up run as ONE GEMM of 2F columns whose
 * epilogue forms silu(gate) * up; neither is written to memory.  intermediate_size is F, as in the HF config.
 * cbas_enc_weights_count_mlp returns -1 (and sets cbas_last_error) where cbas_enc_create_mlp would refuse the combination. */
#define CBAS_MLP_GELU   0
#define CBAS_MLP_SWIGLU 1
int64_t cbas_enc_weights_count_mlp(const cbas_enc_config* cfg, int32_t mlp);
int cbas_enc_create_mlp(const cbas_enc_config* cfg, int32_t mlp, const float* weights_host, int64_t n_weights,
                        int device_id, cbas_enc** out);
/* The MLP kind the handle was created with. */
int cbas_enc_get_mlp(const cbas_enc* h, int32_t* mlp);
void cbas_enc_destroy(cbas_enc* h);

/* ConvNeXt handles take every forward / submit / wait / fused-session entry point below unchanged; frames must be at least
 * 32 x 32 (the stem and the three downsamples divide by 32; odd sizes drop the last row / column at each step, as PyTorch's
 * strided convolutions do).  cbas_enc_set_prune_last_layer is accepted and has no effect; cbas_enc_profile_read reports the
 * stem and downsample GEMMs as CBAS_PROF_PATCH, the LayerNorm / depthwise / pooling kernels as CBAS_PROF_LAYERNORM,
 * pointwise_conv1 as CBAS_PROF_UP and pointwise_conv2 as CBAS_PROF_DOWN. */

/* DinoEncoder.forward on a device tensor: x (n,1,H,W) float32 in [0,1] (gray; replicated to 3
 * identical channels by the reference, folded into the patch weights here).  Writes CLS rows:
 * cls_f32_dev (n,D) and/or cls_f16_dev (n,D) IEEE half; either may be NULL.  n <= max_batch. */
int cbas_enc_forward_f32(cbas_enc* h, const float* x_dev, int n, int height, int width,
                         float* cls_f32_dev, uint16_t* cls_f16_dev, void* stream);

/* Same from uint8 pixels already in HBM.  Pixel (f,y,x) is read at
 * frames_dev[f*frame_stride + y*row_stride + x*pixel_stride]; for decord-style (n,H,W,3) RGB pass
 * frames_dev = base+1, pixel_stride=3, row_stride=3*W, frame_stride=3*H*W (green channel,
 * backend/cbas.py:431); for a packed green plane pass 1, W, H*W.  value/255 is applied exactly. */
int cbas_enc_forward_u8(cbas_enc* h, const uint8_t* frames_dev, int n, int height, int width,
                        int64_t frame_stride, int64_t row_stride, int64_t pixel_stride,
                        float* cls_f32_dev, uint16_t* cls_f16_dev, void* stream);

/* The same two forwards with the last layer's CLS attention as extra outputs - what the reference's encoder comparison tool
 * shows (compare_encoders.py:36-49: outputs.attentions[-1][0, :, 0, NP:] averaged over the heads, :72-79 reshaped to the
 * patch grid).  For frame b, head k and token t < T (T = NP + P: CLS, registers, then the patches in row-major grid order):
 *     attn_heads_dev (n, NH, T) fp32:  softmax over ALL T tokens of q_cls . k_t / 8 of the last layer (rows sum to 1)
 *     attn_map_dev   (n, P)     fp32:  the mean over the heads (ascending) of columns NP .. T-1 of the above
 * Either may be NULL, not both (CBAS_EINVAL; the forms above are the calls without maps).  A ConvNeXt handle is CBAS_EINVAL:
 * it has no attention.  Every ViT precision is served; the scores are formed in fp32 from the query and keys the forward
 * itself uses (fp16 in precisions 0 - 2, fp32 in 3, 22-bit fp16 pairs in 4), in a fixed order, so a frame's map depends on
 * neither n nor its place in the batch.  The CLS rows are bit for bit those of the call without maps, and nothing else the
 * forward computes changes.  Precision 2 (and the LayerNorm-fold option) give the map of THAT encoder - MX-fp8 layers below
 * the last one - not of the fp16 one.  T may not exceed about 8 000 tokens (the kernel keeps one head's row in
 * 64 KiB of LDS); a larger frame is CBAS_EINVAL. */
int cbas_enc_forward_f32_attn(cbas_enc* h, const float* x_dev, int n, int height, int width,
                              float* cls_f32_dev, uint16_t* cls_f16_dev, void* stream,
                              float* attn_heads_dev, float* attn_map_dev);
int cbas_enc_forward_u8_attn(cbas_enc* h, const uint8_t* frames_dev, int n, int height, int width,
                             int64_t frame_stride, int64_t row_stride, int64_t pixel_stride,
                             float* cls_f32_dev, uint16_t* cls_f16_dev, void* stream,
                             float* attn_heads_dev, float* attn_map_dev);

/* The same two forwards returning what transformers calls the encoder's output: last_hidden_state, the final-LayerNorm'd row of
 * EVERY token, instead of the CLS rows.  For frame b and token t < T:
 *     tokens_f32_dev / tokens_f16_dev   row b T + t of an image of ld_tokens elements per row (ld_tokens >= D, a multiple of 4;
 *                                       columns D .. ld_tokens - 1 are not touched); either may be NULL, not both
 *   ViT:      T = NP + P - CLS, the registers, then the patches in row-major grid order
 *   ConvNeXt: T = 1 + (height / 32) (width / 32) - row 0 = LayerNorm(mean over the last stage's grid), row 1 + p = LayerNorm of
 *             grid pixel p (DINOv3ConvNextModel.forward: pool, concatenate, one LayerNorm)
 * Row 0 of each frame is bit for bit the fp32 / fp16 CLS row of cbas_enc_forward_u8 run with an unpruned last layer (ConvNeXt: of
 * any cbas_enc_forward_u8).  The call runs the last layer on every row FOR THIS CALL ONLY - cbas_enc_set_prune_last_layer's
 * setting and every other call's results are untouched.  sim_map_dev (optional) receives (n, T - NP) cosines of row
 * query_idx_dev[b] (a token index in [0, T), clamped; NULL: row 0) against each patch row, summed in fp32 from the fp32 image (the
 * fp16 one where only that is asked for); a row of norm 0 gives 0.  ViT handles of precision 0, 1, 3, 4 and ConvNeXt handles
 * (3, 4) are served; precision 2 is CBAS_EINVAL (its MX-fp8 layers serve the CLS row; their token rows are a different
 * encoder's).  The range guard counts every non-finite ROW here (cbas_enc_check_finite: CBAS_ERANGE). */
int cbas_enc_forward_f32_tokens(cbas_enc* h, const float* x_dev, int n, int height, int width,
                                float* tokens_f32_dev, uint16_t* tokens_f16_dev, int64_t ld_tokens,
                                const int32_t* query_idx_dev, float* sim_map_dev, void* stream);
int cbas_enc_forward_u8_tokens(cbas_enc* h, const uint8_t* frames_dev, int n, int height, int width,
                               int64_t frame_stride, int64_t row_stride, int64_t pixel_stride,
                               float* tokens_f32_dev, uint16_t* tokens_f16_dev, int64_t ld_tokens,
                               const int32_t* query_idx_dev, float* sim_map_dev, void* stream);

/* One unpruned forward on lane 0 that fills per-layer outputs - what transformers returns under output_hidden_states=True and
 * output_attentions=True ([tf] DINOv3ViTModel.forward / DINOv3ViTEncoder: all_hidden_states, all_self_attentions; DINOv2:
 * modeling_dinov2.py Dinov2Encoder.forward), DINO's get_intermediate_layers(n, norm=...), and the attention rollout of Abnar and
 * Zuidema built from the head-averaged attentions (compare_encoders.py:36-49 draws the last layer's CLS row only).  No CLS rows
 * are written: as in the ..._tokens forms the last layer runs on every row FOR THIS CALL ONLY, and no other call's results move.
 * Whatever group of destinations is non-NULL is filled; all NULL is CBAS_EINVAL.  T = NP + P tokens per frame.
 *   hidden states   hidden_layers (HOST array of n_hidden_layers indices): 0 = the embeddings output (prefix rows + patch
 *                   embeddings, the residual stream before block 0), l = the stream after block l, up to L - transformers'
 *                   hidden_states numbering.  Listed layer j goes to hidden_f32_dev / hidden_f16_dev + j * hidden_layer_stride
 *                   (elements) as rows b T + t of ld_hidden elements (>= D, a multiple of 4; the stride a multiple of 4).
 *                   hidden_norm = 0: the raw rows (fp16: rounded to nearest even); != 0: each through the encoder's final
 *                   LayerNorm - index L then is bit for bit cbas_enc_forward_*_tokens' image.  fp32 16-byte, fp16 8-byte aligned.
 *   CLS attention   attn_layers (HOST array of n_attn_layers layer numbers 1 .. L): listed layer j's attn_heads_dev
 *                   + j n NH T as (n, NH, T) and attn_map_dev + j n P as (n, P), as cbas_enc_forward_*_attn defines them.
 *   rollout         rollout_dev (n, P): with A_l the head mean (heads ascending) of layer l's softmax rows (T x T) and
 *                   A^_l = 0.5 A_l + 0.5 I, columns NP .. T - 1 of row rollout_query_dev[b] (device; a token index in [0, T),
 *                   clamped; NULL: row 0, the CLS token) of A^_L A^_(L-1) ... A^_(rollout_start_layer); no renormalisation.
 *                   scratch_dev: cbas_enc_layers_scratch_bytes(h, n, height, width) = 3 n T T 4 bytes, 16-byte aligned - A^ of
 *                   the current layer and the two products that alternate.  On return the query rows' product is in the second
 *                   (L - start even) or third (odd) n T T block.
 * All fp32 arithmetic in a fixed order, no atomics: a frame's outputs depend on neither n nor its place in the batch.
 * CBAS_EINVAL with a message, nothing queued: a ConvNeXt or precision-2 handle, a layer outside its range, a scratch too small,
 * a misaligned pointer, all destinations NULL, a frame whose token row does not fit the attention kernels' 64 KiB of LDS
 * (about 8 000 tokens), struct_bytes != sizeof(cbas_enc_layers_args).  A handle that never makes these calls allocates nothing
 * for them: every buffer is the caller's. */
typedef struct cbas_enc_layers_args {
    int64_t struct_bytes;              /* sizeof(cbas_enc_layers_args) */
    const int32_t* hidden_layers;      /* host */
    int32_t n_hidden_layers;
    int32_t hidden_norm;
    float* hidden_f32_dev;
    uint16_t* hidden_f16_dev;
    int64_t ld_hidden;
    int64_t hidden_layer_stride;
    const int32_t* attn_layers;        /* host */
    int32_t n_attn_layers;
    int32_t rollout_start_layer;
    float* attn_heads_dev;
    float* attn_map_dev;
    float* rollout_dev;
    const int32_t* rollout_query_dev;
    void* scratch_dev;
    int64_t scratch_bytes;
} cbas_enc_layers_args;
int64_t cbas_enc_layers_scratch_bytes(const cbas_enc* h, int n, int height, int width);      /* -1: refused (cbas_last_error) */
int cbas_enc_forward_f32_layers(cbas_enc* h, const float* x_dev, int n, int height, int width,
                                const cbas_enc_layers_args* args, void* stream);
int cbas_enc_forward_u8_layers(cbas_enc* h, const uint8_t* frames_dev, int n, int height, int width,
                               int64_t frame_stride, int64_t row_stride, int64_t pixel_stride,
                               const cbas_enc_layers_args* args, void* stream);

/* PCA of patch features: the picture that shows what an encoder separates (the top components of a frame's, or a batch's, patch
 * rows as colours), fitted and projected on the device.  The reference has no such tool; the arithmetic is the textbook one.
 * rows_dev is an image as cbas_enc_forward_*_tokens writes it (tokens_f32_dev): n frames of T rows of D floats, ld floats
 * apart; the first n_prefix rows of each frame (CLS and registers; ConvNeXt: the pooled row) are skipped, P = T - n_prefix
 * patch rows per frame take part.  Plain device pointers, no handle: any fp32 rows will do.
 *     scope CBAS_PCA_FRAME   n independent problems of M = P rows: bases (n, ...), frame b's basis has the bits it has when
 *                            fitted alone, whatever else shares the call
 *     scope CBAS_PCA_BATCH   one problem of M = n P rows: one basis
 * cbas_patch_pca_fit, per problem: mean_dev (D) = the column mean; the covariance C = (X - mean)^T (X - mean) / (M - 1) on the
 * exact-fp32 matrix pipe in row chunks of 1024 added in order; its k leading eigenvectors by `iters` rounds of subspace
 * iteration (fixed start, Z = C Q, modified Gram-Schmidt twice) and a Rayleigh-Ritz step: components_dev (k, D) with unit rows,
 * ordered by eigenvalues_dev (k) descending, each with its entry of largest magnitude positive (ties: the lowest index);
 * total_variance_dev (1) = trace C.  Every sum has a fixed order: two calls give the same bits.  The workspace
 * (cbas_patch_pca_workspace_bytes, -1 for a refused shape; 16-byte aligned) holds on return, first, the covariances: problem b's
 * D x D matrix, exactly symmetric, at float offset b * ceil(M / 1024) * D * D.
 * cbas_patch_pca_project: scores_dev (n, P, k), scores[b][p][j] = (x - mean) . component j, with frame b's own basis
 * (n_bases = n) or one basis for every frame (n_bases = 1) - from a fit, or the caller's.
 * CBAS_EINVAL with a message: D % 32 != 0 or D > 1536, k outside 1 .. 8 or k > min(M - 1, D), M < 2, ld < D, iters < 1, a
 * workspace too small, a NULL pointer, n outside 1 .. 65535, a pointer not 16-byte aligned or ld % 4 != 0, n_bases not 1 or n. */
#define CBAS_PCA_FRAME 0
#define CBAS_PCA_BATCH 1
int64_t cbas_patch_pca_workspace_bytes(int n, int T, int n_prefix, int D, int k, int scope);
int cbas_patch_pca_fit(const float* rows_dev, int n, int T, int n_prefix, int D, int64_t ld, int k, int scope, int iters,
                       float* mean_dev, float* components_dev, float* eigenvalues_dev, float* total_variance_dev,
                       void* workspace_dev, int64_t workspace_bytes, void* stream);
int cbas_patch_pca_project(const float* rows_dev, int n, int T, int n_prefix, int D, int64_t ld, int k, int n_bases,
                           const float* mean_dev, const float* components_dev, float* scores_dev, void* stream);

/* k-means of patch features: the discrete picture - a cluster label per patch - fitted and assigned on the device.  Rows, n_prefix,
 * P, ld and the two scopes are cbas_patch_pca_fit's (FRAME: nb = n problems of M = P rows; BATCH: nb = 1 problem of M = n P rows,
 * row m = patch m % P of frame m / P); rows are finite.  u = fp32, every sum below has the order stated and none uses an atomic:
 * two calls give the same bits, and a frame's FRAME-scope result has the bits it has when fitted alone.
 *   the working row   u = x (normalize = 0), or u = fl(x * rn), rn = fp32(1 / sqrt(s)), s = sum x_d^2 in fp64, rn = 0 when s = 0
 *                     (normalize = 1).  No normalised copy is written: rn is applied wherever a row is used.
 *   start             farthest-point seeding.  mean = the column mean of u (rows in chunks of CBAS_KMEANS_CHUNK added in ascending
 *                     order, the chunks in ascending order, / M).  d(m, t) = sum_d (u_md - t_d)^2: 64 fmaf chains over
 *                     d = l, l + 64, ... added by the xor tree 32, 16, .., 1.  Seed 0 = the row of largest d(m, mean); seed j = the
 *                     row of largest min_{i < j} d(m, seed i); ties to the lowest row.  init_index_dev (nb, k): the rows chosen, in
 *                     this order, an index within the problem (the frame's P rows, or the n P rows).  Seed centroids are u rows.
 *   a round           every row goes to the centroid of largest score_j = fmaf(rn, x . c_j, -h_j), h_j = |c_j|^2 / 2 (the form
 *                     u . c - |c|^2 / 2 of the squared distance; ties to the lowest j).  x . c_j is the sum, in this order, of four
 *                     fp32 fmaf chains: chain w runs over the columns d with (d / 16) % 4 = w, ascending in d / 16, within a block
 *                     of 16 in the order d % 4, then (d % 16) / 4 (v_mfma_f32_16x16x4_f32: exact products).  Its squared distance is
 *                     dist2 = max(0, fmaf(-2, score, |u|^2)), |u|^2 = fp32(s), or 1 (0 for a zero row) when normalize = 1.
 *                     New centroid j = (sum of rn x over its rows) / count_j: per chunk of CBAS_KMEANS_CHUNK rows one fmaf chain
 *                     per element in ascending row order, the chunks added in ascending order, one division.  A centroid without
 *                     rows keeps its value.  Exactly `iters` rounds: no tolerance, no host synchronisation.
 *   finish            one more assignment against the final centroids gives the counts; the clusters are then ordered by
 *                     descending count, ties by seeding order: centroids_dev (nb, k, D), counts_dev (nb, k).
 *   inertia_dev       (nb, iters + 1): inertia[t] = the sum of dist2 (per chunk in ascending row order, chunks in ascending order)
 *                     of the assignment against the centroids after t updates.
 * The workspace (cbas_patch_kmeans_workspace_bytes, -1 for a refused shape; 16-byte aligned) holds on return, first, the final
 * centroids in SEEDING order, nb * k * D floats, then (rounded up to 4 floats) nb * 16 int32: order[b][r] = the seeding position of
 * output cluster r (-1 past k).
 * cbas_patch_kmeans_assign: the round's assignment against given centroids, frame b's own set (n_sets = n) or one set for every
 * frame (n_sets = 1): labels_dev (n, P) int32 and, unless NULL, dist2_dev (n, P).
 * CBAS_EINVAL with a message, nothing queued: k outside 2 .. 16 or k > M, D % 32 != 0 or D > 1536, ld < D or ld % 4 != 0, rows,
 * centroids or workspace not 16-byte aligned, iters < 0 (0 returns the seeds), normalize not 0 or 1, n outside 1 .. 65535, n_sets
 * not 1 or n, a NULL pointer (dist2_dev may be NULL), a workspace too small, a problem of more than 65535 chunks. */
#define CBAS_KMEANS_FRAME CBAS_PCA_FRAME
#define CBAS_KMEANS_BATCH CBAS_PCA_BATCH
#define CBAS_KMEANS_CHUNK 64
#define CBAS_KMEANS_MAX_K 16
int64_t cbas_patch_kmeans_workspace_bytes(int n, int T, int n_prefix, int D, int k, int scope);
int cbas_patch_kmeans_fit(const float* rows_dev, int n, int T, int n_prefix, int D, int64_t ld, int k, int scope, int iters,
                          int normalize, float* centroids_dev, int32_t* counts_dev, float* inertia_dev, int32_t* init_index_dev,
                          void* workspace_dev, int64_t workspace_bytes, void* stream);
int cbas_patch_kmeans_assign(const float* rows_dev, int n, int T, int n_prefix, int D, int64_t ld, int k, int n_sets, int normalize,
                             const float* centroids_dev, int32_t* labels_dev, float* dist2_dev, void* stream);

/* Cosine search over resident CLS rows: "where else does a frame like this one occur?" - every row scored against a few query
 * vectors in one streaming pass, then the k best PEAKS of each query, so that a bout of near-identical neighbouring frames gives one
 * result.  Beyond the reference, which has no search over features.  rows_f16_dev (n_rows, dim) fp16 with row stride ld (in halves),
 * finite; queries_dev (n_queries, dim) fp32, contiguous, finite; clip_table_dev (n_clips, 2) int64 = (first row, rows) of every
 * clip, cbas_labels_median's table; clips do not overlap, and a row outside every clip is never a candidate.  mask_dev, unless NULL:
 * n_rows uint8, 0 = never return this row.  No atomics; every sum has the order stated: two calls give the same bytes, and a row's
 * score does not depend on n_rows, on the slot or group of 16 its query sits in, on where the row lies, or on the device.
 *   the score     trace_dev (n_queries, n_rows) fp32, all of it written: score[q][m] = fl(fl(dot(x_m, q) * rn_m) * rq_q), x = the
 *                 row widened to fp32 (exact).  dot = chain0 + chain1: chain p is the fp32 fmaf chain, from 0, over the columns d
 *                 with (d / 32) % 2 = p in ascending order of (d / 32, d % 8, (d % 32) / 8) (v_mfma_f32_16x16x4_f32: exact products).
 *                 rn_m = fp32(1 / sqrt((double)s_m)), 0 when s_m = 0; s_m = (l0 + l1) + (l2 + l3) in fp32, l_j the fmaf chain, from 0,
 *                 of x_d^2 over the columns d with (d % 32) / 8 = j, ascending.  rq_q = fp32(1 / sqrt(s)), 0 when s = 0, s the fp64 sum
 *                 of q_d^2: 64 fma chains over d = l, l + 64, ... added by the xor tree 32, 16, .., 1.  A zero row or a zero query
 *                 scores exactly 0.  |score - cosine| <= (2 dim + 8) 2^-24.
 *   the peaks     row m of a clip is a peak of query q iff every row m' of the SAME clip with 0 < |m - m'| <= min_gap has
 *                 score[m'] < score[m], or score[m'] == score[m] and m' > m.  min_gap = 0: every row is a peak (plain top-k).
 *                 Masked rows take part in the comparison (a labelled bout suppresses its neighbours) and are never returned.  With
 *                 use_threshold != 0 a result also has score >= threshold (fp32).  Two results of one clip are therefore more than
 *                 min_gap rows apart.  This is a rule on the scores alone, not greedy suppression: whether a row is returned does not
 *                 depend on k or on what else was returned.
 *   the result    per query the k best unmasked peaks by (score descending, row ascending): index_dev (n_queries, k) int64, the
 *                 row's index in rows_f16_dev, and score_dev (n_queries, k) fp32; fewer than k peaks: (-1, -inf) past the last.
 * The workspace (cbas_rows_search_workspace_bytes, -1 for a refused shape) is scratch: about 4 n_rows bytes and
 * 13 k n_queries n_rows / 1024 bytes of lists.  The clip table is checked on the device before anything is indexed with it and the
 * flags are read back: THE CALL SYNCHRONISES `stream` once, before the scores are queued.
 * CBAS_EINVAL with a message, nothing queued and no output written: dim % 32 != 0 or dim > 1536, ld < dim or ld % 8 != 0, rows,
 * queries, trace or workspace not 16-byte aligned, n_rows < 1, n_queries outside 1 .. 64, k outside 1 .. 64, min_gap outside
 * 0 .. 65535, n_clips < 1, a NULL pointer (mask_dev may be NULL), a workspace too small.  CBAS_EINVAL with a message, only the
 * workspace written: a clip table entry outside the rows, or two entries that overlap. */
int64_t cbas_rows_search_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t k);
int cbas_rows_search(const uint16_t* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, const float* queries_dev, int32_t n_queries,
                     const int64_t* clip_table_dev, int32_t n_clips, const uint8_t* mask_dev, int32_t min_gap, int32_t use_threshold,
                     float threshold, int32_t k, float* trace_dev, int64_t* index_dev, float* score_dev, void* workspace_dev,
                     int64_t workspace_bytes, void* stream);

/* Weighted k-nearest-neighbour labels for resident CLS rows: "I have labelled a few hundred bouts; what does that say about every
 * frame?" - the evaluation protocol of the self-supervised encoders (DINO, DINOv2, DINOv3).  Every store row takes its k most similar
 * labelled rows by cosine and each votes for its label with weight exp(cos / T).  Beyond the reference, whose pre-labels need a trained
 * head.  rows_f16_dev (N, D) fp16 with row stride ld (in halves); bank_f16_dev (M, D) fp16 with row stride bank_ld, the labelled rows;
 * bank_label_dev (M) int32 in [0, C); bank_group_dev (M) and row_group_dev (N) int32, either may be NULL; class_weight_dev (C) fp32 or
 * NULL = ones.  The (N, M) matrix of cosines is never in memory unless sims_dev asks for it (tests and small shapes).  No atomics.
 *   the cosine    cos[m][j] = fl(fl(dot * rn_row[m]) * rn_bank[j]); dot = the fp32-accumulated sum of the exact products of the two
 *                 fp16 rows on the fp16 matrix pipe (v_mfma_f32_16x16x32_f16), 32 columns an instruction in ascending order into one
 *                 accumulator; rn = fp32(1 / sqrt((double)s)), 0 when s = 0, s the fp32 sum of cbas_rows_search: (l0 + l1) + (l2 + l3),
 *                 l_j the fmaf chain, from 0, of x_d^2 over the columns d with (d % 32) / 8 = j, ascending.  A zero row scores exactly
 *                 0 with everything.  |cos - cosine| <= (2 D + 8) 2^-24.  sims_dev (N, M), unless NULL, receives every pair's cosine,
 *                 excluded ones included.
 *   excluded      bank entry j for row m when both group arrays are given and bank_group[j] == row_group[m] >= 0 (leave one instance
 *                 or one file out).
 *   neighbours    the k best entries that are not excluded: a beats b when cos[a] > cos[b], or cos[a] == cos[b] and a < b.
 *                 nn_index_dev (N, k) int32 and nn_score_dev (N, k) fp32, unless NULL, in that order; (-1, -inf) past the last.  A
 *                 function of the cosine bits and the bank indices alone: not of N, of where a row lies, or of the grid.
 *   the vote      s_0 = the best neighbour's score; w_r = fl(expf(fl(fl(s_r - s_0) / T)) * cw[label_r]); Z = the fp32 sum of w_r in
 *                 ascending rank, num_c that of the neighbours with label c; probs_dev[m][c] = num_c / Z, (N, C) fp32.  A row
 *                 without a neighbour gets zeros.
 * The workspace (cbas_rows_knn_workspace_bytes, -1 for a refused shape) holds the reciprocal norms: about 4 (N + M) bytes.  The labels
 * are checked on the device before one is used as an index and the flag is read back: THE CALL SYNCHRONISES `stream` once, before the
 * pass is queued.  N = 0: nothing is done.
 * CBAS_EINVAL with a message, nothing queued and no output written: D % 32 != 0 or D outside 32 .. 1536, ld or bank_ld < D or not a
 * multiple of 8, M outside 1 .. 65536, k outside 1 .. 64, C outside 1 .. 64, a temperature that is not finite or not greater than 0,
 * N < 0, rows, bank or workspace not 16-byte aligned, a NULL rows, bank, bank_label, probs or workspace, a workspace too small.
 * CBAS_EINVAL with a message, only the workspace written: a label outside [0, C). */
int64_t cbas_rows_knn_workspace_bytes(int64_t n_rows, int32_t n_bank, int32_t k);
int cbas_rows_knn(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, const void* bank_f16_dev, int32_t n_bank,
                  int64_t bank_ld, const int32_t* bank_label_dev, const int32_t* bank_group_dev, const int32_t* row_group_dev,
                  int32_t n_classes, const float* class_weight_dev, int32_t k, float temperature, float* probs_dev,
                  int32_t* nn_index_dev, float* nn_score_dev, float* sims_dev, void* workspace_dev, int64_t workspace_bytes,
                  void* stream);

/* k-means over resident CLS rows: "what behaviours are in these recordings at all?" - every frame of the store grouped into k motifs
 * before anything is labelled.  Beyond the reference, which has no unsupervised grouping.  rows_f16_dev (n_rows, dim) fp16 with row
 * stride ld (in halves), finite; centroids (k, dim) fp32, contiguous.  The definition is cbas_patch_kmeans_fit's with the sums of
 * this family; every sum below has the order stated, a function of (n_rows, dim, k) alone - not of the grid, the device or the
 * stream - and none uses an atomic: two calls give the same bytes.
 *   the working row   u = x widened to fp32 (normalize = 0), or u = fl(x * rn) (normalize = 1), rn cbas_rows_search's: rn = fp32(1 /
 *                     sqrt((double)s)), 0 when s = 0, s = (l0 + l1) + (l2 + l3) in fp32, l_j the fmaf chain, from 0, of x_d^2 over the
 *                     columns d with (d % 32) / 8 = j, ascending.  No normalised copy is written.
 *   start             farthest-point seeding, unless init_centroids_dev (k, dim) is given (then init_index_dev is -1 everywhere).
 *                     mean = the column mean of u: per SEGMENT of CBAS_ROWS_KMEANS_SEGMENT rows one fp32 sum per column in ascending
 *                     row order, the segments added in ascending order, / (float)n_rows.  d(m, t) = sum_d (u_md - t_d)^2: 64 fmaf
 *                     chains, chain l over the columns d with (d / 8) % 64 = l in ascending order, added by the xor tree 32, 16, .., 1.
 *                     Seed 0 = the row of largest d(m, mean); seed j = the row of largest min_{i < j} d(m, seed i); ties to the
 *                     lowest row.  init_index_dev (k) int64: the rows chosen, in this order.  Seed centroids are u rows.
 *   a round           every row goes to the centroid of largest score_j = fmaf(rn, x . c_j, -h_j) (rn = 1 without normalize); ties
 *                     to the lowest j.  x . c_j = chain0 + chain1, cbas_rows_search's dot: chain p is the fp32 fmaf chain, from 0, over
 *                     the columns d with (d / 32) % 2 = p in ascending order of (d / 32, d % 8, (d % 32) / 8) (v_mfma_f32_16x16x4_f32:
 *                     exact products).  h_j = 0.5 * |c_j|^2, |c_j|^2 one fp32 fmaf chain, from 0, over d ascending.
 *                     dist2 = max(0, fmaf(-2, score, |u|^2)), |u|^2 = s, or 1 (0 for a zero row) when normalize = 1.
 *                     New centroid j = (sum of u over its rows) / (float)count_j: per segment one fp32 sum per element in ascending
 *                     row order, the segments added in ascending order, one division.  A centroid without rows keeps its value.
 *                     Exactly `iters` rounds: no tolerance, no host synchronisation.
 *   finish            one more assignment against the final centroids gives the counts; the clusters are then numbered by descending
 *                     count, ties by seeding order: centroids_dev (k, dim), counts_dev (k) int64.  labels_dev (n_rows) int32 and
 *                     dist2_dev (n_rows), unless NULL, are that assignment in the output numbering.  They have the bytes of
 *                     cbas_rows_kmeans_assign against centroids_dev, except for a row whose two best scores are EQUAL in fp32: it keeps
 *                     the cluster of the lower seeding position (the one that was counted), which _assign gives only when that cluster
 *                     also has the lower output number.
 *   inertia_dev       (iters + 1): inertia[t] = the sum of dist2 (per segment one fp32 sum in ascending row order, the segments in
 *                     ascending order) of the assignment against the centroids after t updates.
 * The workspace (cbas_rows_kmeans_workspace_bytes, -1 for a refused shape; 16-byte aligned) takes, each part rounded up to 16 bytes,
 *   4 k dim + 512 + 4 dim + 16 n_rows + 12 ceil(n_rows / 64) + (4 k dim + 260) ceil(n_rows / CBAS_ROWS_KMEANS_SEGMENT)  bytes:
 * O(n_rows) plus one (k, dim) block of partial sums per segment.  On return it holds, first, the final centroids in SEEDING order,
 * k * dim floats, then 64 int32: order[r] = the seeding position of output cluster r (-1 past k) - what a caller passes as
 * init_centroids_dev to continue the fit.
 * cbas_rows_kmeans_assign: the round's assignment against given centroids: labels_dev (n_rows) int32 and, unless NULL, dist2_dev.  A
 * row's label and dist2 do not depend on n_rows or on where the row lies in the call; n_rows may be less than k.
 * CBAS_EINVAL with a message, nothing queued and no output written: k outside 2 .. 64 or (fit) k > n_rows, dim % 32 != 0 or dim
 * outside 32 .. 1536, ld < dim or ld % 8 != 0, n_rows < 1, iters < 0 (0 returns the start), normalize not 0 or 1, rows, centroids or
 * workspace not 16-byte aligned, a NULL pointer (init_centroids_dev, labels_dev of fit and dist2_dev may be NULL), a workspace too
 * small. */
#define CBAS_ROWS_KMEANS_SEGMENT 4096
int64_t cbas_rows_kmeans_workspace_bytes(int64_t n_rows, int32_t dim, int32_t k);
int cbas_rows_kmeans_fit(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, int32_t k, int32_t iters, int32_t normalize,
                         const float* init_centroids_dev, float* centroids_dev, int64_t* counts_dev, float* inertia_dev,
                         int64_t* init_index_dev, int32_t* labels_dev, float* dist2_dev, void* workspace_dev, int64_t workspace_bytes,
                         void* stream);
int cbas_rows_kmeans_assign(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, int32_t k, int32_t normalize,
                            const float* centroids_dev, int32_t* labels_dev, float* dist2_dev, void* stream);

/* A linear probe on resident CLS rows: softmax regression on the frozen, normalised rows - the second half of the evaluation protocol of
 * the self-supervised encoders (cbas_rows_knn is the first), and pre-labels for every frame from one (C, D) matrix.  Beyond the
 * reference, which has no probe.  train_f16_dev (n_train, dim) fp16 with row stride ld (in halves), finite; label_dev (n_train) int32
 * in [0, n_classes); sample_weight_dev (n_train) fp32, omega_m >= 0 and finite, NULL = ones.  Every sum below has the order stated, a
 * function of (n_train, dim, n_classes) alone - not of the grid, the device or the stream - and none uses an atomic: two calls give
 * the same bytes.
 *   the working row   u = fl(x * rn), rn cbas_rows_search's: rn = fp32(1 / sqrt((double)s)), 0 when s = 0 (a zero row has u = 0), s =
 *                     (l0 + l1) + (l2 + l3) in fp32, l_j the fmaf chain, from 0, of x_d^2 over the columns d with (d % 32) / 8 = j,
 *                     ascending.  There is no un-normalised mode: with |u| <= 1 the step size is known on the host, which keeps
 *                     the fit free of synchronisation.  No normalised copy is written.
 *   the model         W (C, dim) fp32, b (C) fp32; z_c = fmaf(rn, x . w_c, b_c), x . w_c = chain0 + chain1, cbas_rows_search's dot:
 *                     chain p is the fp32 fmaf chain, from 0, over the columns d with (d / 32) % 2 = p in ascending order of (d / 32,
 *                     d % 8, (d % 32) / 8) (v_mfma_f32_16x16x4_f32: exact products).  The logits of a zero row are the bias.
 *   the softmax       mx = the largest logit; e_c = expf(z_c - mx); S = (per j = c % 16 the e_c with c % 16 = j added in ascending c),
 *                     then these sixteen by the xor tree 1, 2, 4, 8 over j; p_c = e_c / S; lse = mx + logf(S).
 *   the objective     F(W, b) = (1 / Omega) sum_m omega_m (lse_m - z_{m, y_m}) + (l2 / 2) (|W|^2 + |b|^2): the bias is the weight of
 *                     a constant feature 1 and is regularised like every other weight.  Omega = sum_m omega_m: per SEGMENT of
 *                     CBAS_ROWS_PROBE_SEGMENT rows one fp32 sum in ascending row order, the segments added in ascending order; the
 *                     loss terms fl(omega_m * fl(lse_m - z_y)) are added the same way and divided by Omega.  |W|^2 + |b|^2 = the
 *                     |w_c|^2 (each one fmaf chain, from 0, over d ascending) added in ascending c, then |b|^2 (one fmaf chain over
 *                     c ascending); F = fmaf(0.5 l2, that, data term).
 *   the gradient      r_mc = fl(omega_m * (p_mc - [c = y_m])) (the subtraction rounds, then the product).  Per segment and element
 *                     one fmaf chain, from 0, of r_mc * u_md over the segment's rows in ascending order (the fp32 matrix pipe, its
 *                     k dimension over the rows); the bias' element is the plain fp32 sum of r_mc in that order.  The segments are
 *                     added in ascending order; g = fmaf(l2, v, sum * (1 / Omega)).
 *   the iteration     Nesterov's constant-step scheme for strongly convex functions, exactly `iters` steps, no tolerance, no host
 *                     synchronisation: L = 1 + l2 (the data term's Hessian is at most 1/2 max |(u, 1)|^2 = 1), q = l2 / L, beta =
 *                     (1 - sqrt q) / (1 + sqrt q); v_t = w_t + beta (w_t - w_{t-1}), w_{-1} = w_0; w_{t+1} = v_t - (1 / L) grad
 *                     F(v_t), as w_{t+1} = fmaf(-1/L, g, v_t), v_{t+1} = fmaf(beta, w_{t+1} - w_t, w_{t+1}).  beta and 1 / L are
 *                     computed on the host in double and rounded once to fp32.  w_0 = init_weights_dev (C, dim) / init_bias_dev
 *                     (C), zeros where NULL.  A fit continued from given weights restarts the momentum (v_0 = w_0): `a` steps and
 *                     then `b` more are not a + b steps.
 *   loss_dev          (iters + 1): loss[t] = F(v_t) for t < iters, a by-product of the gradient pass; loss[iters] = F(w_iters),
 *                     from one closing forward pass.  iters = 0 returns the start and loss[0] = F(w_0).
 * weights_dev (C, dim) and bias_dev (C) receive w_iters.  The call synchronises `stream` ONCE, before the iteration is queued, to
 * read back the checks of the labels, the sample weights and Omega; never after.
 * The workspace (cbas_rows_probe_workspace_bytes, -1 for a refused shape; 16-byte aligned) takes, each part rounded up to 16 bytes,
 *   32 + 2 (4 C dim + 256) + 320 + 8 n_train + 4 n_train C + (4 C dim + 264) ceil(n_train / CBAS_ROWS_PROBE_SEGMENT)  bytes:
 * O(n_train C) plus one (C, dim) block of partial sums per segment.
 * cbas_rows_probe_predict: probs_dev (n_rows, C) = p and, unless NULL, logits_dev (n_rows, C) = z of every row against given
 * weights.  A row's outputs do not depend on n_rows, on where the row lies in the call or on whether logits_dev is given; n_rows =
 * 0 does nothing.  Nothing is synchronised.
 * CBAS_EINVAL with a message, nothing queued and no output written: dim % 32 != 0 or dim outside 32 .. 1536, ld < dim or ld % 8 != 0,
 * n_classes outside 2 .. 64, n_train outside 1 .. 4 194 304, n_rows < 0, iters < 0, l2 not finite or not > 0, rows, weights or
 * workspace not 16-byte aligned, a NULL pointer (sample_weight_dev, init_weights_dev, init_bias_dev and logits_dev may be NULL), a
 * workspace too small.  CBAS_EINVAL with only the workspace written: a label outside [0, n_classes), a sample weight that is negative
 * or not finite, Omega = 0. */
#define CBAS_ROWS_PROBE_SEGMENT 1024
int64_t cbas_rows_probe_workspace_bytes(int64_t n_train, int32_t dim, int32_t n_classes);
int cbas_rows_probe_fit(const void* train_f16_dev, int64_t n_train, int32_t dim, int64_t ld, const int32_t* label_dev,
                        const float* sample_weight_dev, int32_t n_classes, float l2, int32_t iters,
                        const float* init_weights_dev, const float* init_bias_dev, float* weights_dev, float* bias_dev,
                        float* loss_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);
int cbas_rows_probe_predict(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, const float* weights_dev,
                            const float* bias_dev, int32_t n_classes, float* probs_dev, float* logits_dev, void* stream);

/* PCA over resident CLS rows: "what does the whole store look like?" - every frame a point in k <= 8 dimensions, and its squared
 * distance from that k-dimensional subspace.  Beyond the reference, which has no map of its features.  rows_f16_dev (n_rows, dim) fp16
 * with row stride ld (in halves), finite.  The definition is cbas_patch_pca_fit's with one problem; every sum below has the order
 * stated, a function of (n_rows, dim) alone - not of the grid, the device or the stream - and none uses an atomic: two calls give the
 * same bytes.
 *   the working row   u = x widened to fp32 (normalize = 0), or u = fl(x * rn) (normalize = 1), rn cbas_rows_search's: rn = fp32(1 /
 *                     sqrt((double)s)), 0 when s = 0 (a zero row has u = 0), s = (l0 + l1) + (l2 + l3) in fp32, l_j the fmaf chain,
 *                     from 0, of x_d^2 over the columns d with (d % 32) / 8 = j, ascending.  No normalised copy is written.
 *   the mean          mean_dev (dim): per CHUNK of CBAS_ROWS_PCA_CHUNK rows one fp32 sum per column in ascending row order, the
 *                     chunks added in ascending order, / (float)n_rows.
 *   the covariance    C = sum_m c_m c_m^T / (n_rows - 1), c_md = fl(u_md - mean_d).  The chunks are dealt to PARTS: a part is P =
 *                     ceil(ceil(n_rows / CBAS_ROWS_PCA_CHUNK) / CBAS_ROWS_PCA_MAX_PARTS) consecutive chunks, so there are
 *                     ceil(chunks / P) <= CBAS_ROWS_PCA_MAX_PARTS parts whatever n_rows.  Per element (i <= j) and chunk one fp32 fmaf
 *                     chain, from 0, over the chunk's rows in ascending order (v_mfma_f32_16x16x4_f32: exact products); within a part
 *                     the chunks' results are added in ascending order, from 0; the parts are added in ascending order, from part 0's
 *                     value; one division by (float)(n_rows - 1).  (i, j) and (j, i) are written from the same value: C is symmetric
 *                     bit for bit, and is left at the front of the workspace, dim * dim floats.
 *   the eigenvectors  cbas_patch_pca_fit's solver on that C, unchanged: `iters` rounds of subspace iteration from its fixed start,
 *                     Rayleigh-Ritz, eigenvalues descending, each component's entry of largest magnitude positive (ties to the lowest
 *                     index).  components_dev (k, dim), eigenvalues_dev (k), total_variance_dev (1) = the trace of C.
 * cbas_rows_pca_fit synchronises nothing.
 * The workspace (cbas_rows_pca_workspace_bytes, -1 for a refused shape; 16-byte aligned) takes, each part rounded up to 16 bytes,
 *   4 dim^2 parts + 4 k dim + 4 dim ceil(n_rows / CBAS_ROWS_PCA_CHUNK) + 4 n_rows  bytes:
 * at most CBAS_ROWS_PCA_MAX_PARTS dim x dim blocks whatever n_rows, one row of column sums per chunk, and the reciprocal norms.
 * cbas_rows_pca_project: scores_dev (n_rows, k) and, unless NULL, residual_dev (n_rows) of every row against a given mean (dim) and
 * components (k, dim), one streaming pass.
 *   score_mj          = chain0 + chain1, chain p the fp32 fmaf chain, from 0, of c_md * q_jd over the columns d with (d / 32) % 2 = p
 *                     in ascending order of (d / 32, d % 8, (d % 32) / 8) (cbas_rows_search's dot, with the centred value c_md = fl(u_md -
 *                     mean_d) in the row's place); then * scale_j, one rounding, when scale_dev (k) is given (whitening: the caller
 *                     passes 1 / sqrt(eigenvalue_j)).
 *   residual_m        = max(0, |c_m|^2 - sum_j score_mj^2) from the unscaled scores: |c_m|^2 = (n0 + n1) + (n2 + n3), n_j the fmaf
 *                     chain, from 0, of c_md^2 over the columns d with (d % 32) / 8 = j, ascending; the scores' squares one fmaf chain,
 *                     from 0, over j ascending.  The squared distance of the frame from the subspace.
 * A row's outputs do not depend on n_rows, on where the row lies in the call or on whether residual_dev is given; n_rows = 0 does
 * nothing.  Nothing is synchronised.
 * CBAS_EINVAL with a message, nothing queued and no output written: dim % 32 != 0 or dim outside 32 .. 1536, k outside 1 .. 8 or k >
 * dim, ld < dim or ld % 8 != 0, n_rows outside 2 .. 16 777 216 (fit) or < 0 (project), normalize not 0 or 1, iters < 1, rows, mean,
 * components or workspace not 16-byte aligned, a NULL pointer (scale_dev and residual_dev may be NULL), a workspace too small. */
#define CBAS_ROWS_PCA_CHUNK 1024
#define CBAS_ROWS_PCA_MAX_PARTS 64
int64_t cbas_rows_pca_workspace_bytes(int64_t n_rows, int32_t dim, int32_t k);
int cbas_rows_pca_fit(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, int32_t k, int32_t iters, int32_t normalize,
                      float* mean_dev, float* components_dev, float* eigenvalues_dev, float* total_variance_dev, void* workspace_dev,
                      int64_t workspace_bytes, void* stream);
int cbas_rows_pca_project(const void* rows_f16_dev, int64_t n_rows, int32_t dim, int64_t ld, int32_t k, int32_t normalize,
                          const float* mean_dev, const float* components_dev, const float* scale_dev, float* scores_dev,
                          float* residual_dev, void* stream);

/* Host-streamed form (one iteration of encode_file's chunk loop).  `slot` in [0, CBAS_ENC_SLOTS):
 * submit copies the pixels host->HBM on the handle's copy stream (from pinned staging), encodes
 * on the compute stream and copies the CLS rows back; wait blocks until that slot is done and
 * writes n*D halves (and/or floats).  Submitting to slot s while s is busy is CBAS_ESTATE.
 * Different slots overlap: copy(s+1) runs under compute(s).
 * The caller's bytes travel as they are (interleaved RGB included: 150 KB per 224x224 frame is nothing on PCIe 5)
 * and the consumed channel is picked on the device through the strides - the host does no per-pixel work.
 * Pageable memory is copied into the slot's pinned staging before the call returns.  If frames_host is itself
 * pinned (hipHostMalloc / hipHostRegister, e.g. a torch pin_memory() tensor) the H2D copy is a direct DMA from it and
 * the caller must leave those bytes untouched until cbas_enc_wait(slot). */
#define CBAS_ENC_SLOTS 3
int cbas_enc_submit_u8_host(cbas_enc* h, int slot, const uint8_t* frames_host, int n, int height,
                            int width, int64_t frame_stride, int64_t row_stride, int64_t pixel_stride);
int cbas_enc_wait(cbas_enc* h, int slot, uint16_t* cls_f16_host, float* cls_f32_host);

/* Asynchronous device-resident form (the chunk loop when the frames are already in HBM, and the live
 * encode -> head stream): like cbas_enc_forward_u8, but the batch runs on one of the handle's two compute
 * lanes (own workspace + stream; submissions alternate), ordered after everything queued so far on
 * `after_stream`.  Two consecutive submissions are therefore in flight together: one batch's partial tile
 * rounds, LayerNorm and attention run under the other batch's GEMMs (+10 % throughput on MI355X, outputs
 * bit-identical to the synchronous form).  cbas_enc_wait_stream makes `stream` wait for the slot's batch
 * (no host block) and frees the slot; until then frames_dev must stay valid and the outputs untouched.
 * The host-streamed form above alternates the same two lanes. */
int cbas_enc_submit_u8(cbas_enc* h, int slot, const uint8_t* frames_dev, int n, int height, int width,
                       int64_t frame_stride, int64_t row_stride, int64_t pixel_stride,
                       float* cls_f32_dev, uint16_t* cls_f16_dev, void* after_stream);
int cbas_enc_wait_stream(cbas_enc* h, int slot, void* stream);
/* Host frames in, device rows out: cbas_enc_submit_u8_host's ingest (pinned staging or direct DMA, copy stream)
 * with cbas_enc_submit_u8's outputs (rows written to cls_*_dev, slot released by cbas_enc_wait_stream).  The
 * batch is ordered after everything queued so far on `after_stream` (which may still read those rows). */
int cbas_enc_submit_u8_host_dev(cbas_enc* h, int slot, const uint8_t* frames_host, int n, int height, int width,
                                int64_t frame_stride, int64_t row_stride, int64_t pixel_stride,
                                float* cls_f32_dev, uint16_t* cls_f16_dev, void* after_stream);
/* The reference's fp32 arithmetic has no range limit; the fp16 activations of precision 0 (|value| < 65 504) and the
 * split-fp16 operands of precision 4 (power-of-two scaled, see cbas_enc_config.precision) do.  Every forward pass tests its
 * CLS rows (a non-finite value anywhere reaches them: every query attends to every key) and counts the frames that failed;
 * cbas_enc_wait, cbas_fused_finish and cbas_fused_wait return CBAS_ERANGE instead of handing out such rows, and a caller of
 * the stream-ordered forms (cbas_enc_forward_*, cbas_enc_submit_u8 + cbas_enc_wait_stream) asks here once its batches have
 * completed.  Returns CBAS_OK or CBAS_ERANGE (cbas_last_error names the mode and the way out); clears the count. */
int cbas_enc_check_finite(cbas_enc* h);
/* The handle's copy stream (a hipStream_t), for work that should be ordered with its host->HBM copies rather than get a stream
 * of its own.  The fused session runs the head there: a HIP process has FOUR hardware queues by default (GPU_MAX_HW_QUEUES)
 * and its streams share them round-robin; with the two compute lanes, the copy stream AND a head stream all active, the
 * pinned-host path measured 6 % slower than with three active queues (DESIGN.md, section 6 "hardware queues"). */
void* cbas_enc_copy_stream(cbas_enc* h);
/* The configuration the handle was created with. */
int cbas_enc_get_config(const cbas_enc* h, cbas_enc_config* out);
/* Use 1 or 2 compute lanes for the asynchronous forms (2 by default; 1 serialises the batches, e.g. to time
 * kernels without another batch's kernels running beside them).  No batch may be in flight. */
int cbas_enc_set_lanes(cbas_enc* h, int n_lanes);
/* The reference runs its last transformer layer on every token and then keeps row 0 ([tf]:540-541,
 * backend/cbas.py:677).  By default the last layer here projects K and V for all rows but computes the query,
 * attention, o_proj, LayerNorm 2 and the MLP for the n CLS rows only (rows are independent: the CLS output is
 * bit-identical).  enable = 0 restores the full last layer (used by the tests that prove the identity). */
int cbas_enc_set_prune_last_layer(cbas_enc* h, int enable);
/* How a handle with a learned position embedding (pos_embed_grid = G > 0) resamples its G x G table to a frame's nh x nw patch
 * grid.  The two HF DINOv2 families differ in exactly this:
 *   CBAS_POS_INTERP_BICUBIC_AA (the default of a new handle): Dinov2WithRegistersEmbeddings.interpolate_pos_encoding
 *       (transformers models/dinov2_with_registers/modeling_dinov2_with_registers.py:93-145) calls F.interpolate(mode="bicubic",
 *       align_corners=False, antialias=True): Keys kernel a = -0.5, support widened by the scale when downsampling, weights
 *       normalised per output.
 *   CBAS_POS_INTERP_BICUBIC: Dinov2Embeddings.interpolate_pos_encoding of plain DINOv2 ("facebook/dinov2-base"; transformers
 *       models/dinov2/modeling_dinov2.py:57-95, the call at :86-91) passes size=(nh, nw), mode="bicubic", align_corners=False and
 *       NO antialias: ATen's upsample_bicubic2d - source index (dst + 0.5) * G / n - 0.5 (scale from the sizes, not clamped), the
 *       four taps floor - 1 ... floor + 2 clamped to [0, G - 1], cubic convolution coefficients with a = -0.75.  At CBAS's 256 x 256
 *       video (18 x 18 from 37 x 37) the two tables differ in the first digit.
 * Both use the stored table as it is, bit for bit, when nh = nw = G (modeling_dinov2.py:71-72).  The tables are built on the
 * first batch of each grid, so call this between cbas_enc_create and the first forward / submit (a plain-DINOv2 handle is
 * cbas_enc_create with num_register_tokens = 0 followed by this); changing the mode once a table exists is CBAS_EINVAL.
 * Everything after the table - its cache per resolution, the patch GEMM epilogue that adds it - is the same for both. */
#define CBAS_POS_INTERP_BICUBIC_AA 0
#define CBAS_POS_INTERP_BICUBIC    1
int cbas_enc_set_pos_interp(cbas_enc* h, int mode);
/* Which projection GEMMs of a precision-2 (MX-fp8) ViT handle take MX-fp8 operands: a mask of CBAS_FP8_PLAN_* bits.  A new
 * handle has CBAS_FP8_PLAN_ALL - every earlier release's precision 2, bit for bit.  A GEMM outside the plan runs exactly as
 * precision 0 runs it (fp16 operands, fp32 accumulation), and every activation is stored in the format of the GEMM that
 * consumes it: LayerNorm 1 follows QKV, the attention context PROJ, LayerNorm 2 UP, the GELU output DOWN.  The pruned last
 * layer follows the same plan for its k | v projection; its CLS tail is fp16 in every plan.  Plan 0 is precision 0's rows.
 * Rows of different plans are different encoders' rows (as precision 2's are against precision 0's): train a head on the rows
 * of the plan it will be fed.  Costs no device memory: a precision-2 handle holds the fp16 weights beside the MX-fp8 ones.
 * Valid between cbas_enc_create and the handle's first forward / submit, on a precision-2 ViT handle; anything else - another
 * precision, a ConvNeXt handle, a mask outside 0..15, a handle that has run - is CBAS_EINVAL.  Applies to both compute lanes. */
#define CBAS_FP8_PLAN_QKV   1      /* q|k|v projection */
#define CBAS_FP8_PLAN_PROJ  2      /* o_proj */
#define CBAS_FP8_PLAN_UP    4      /* mlp.up_proj */
#define CBAS_FP8_PLAN_DOWN  8      /* mlp.down_proj */
#define CBAS_FP8_PLAN_ALL   15
int cbas_enc_set_fp8_plan(cbas_enc* h, int plan);

/* Bring-up, test and measurement-harness entry points (stage taps, implementation switches, stand-alone GEMM
 * harnesses, the MFMA neighbour) are NOT part of this boundary: include/cbas_mi355x_debug.h, built only into
 * libcbas_mi355x_debug.so (python -m cbas_amd.build --debug). */

/* Per-kernel timing for benchmarks: while enabled, every kernel launch of the forward pass is
 * bracketed by HIP events on the launch stream.  cbas_enc_profile_read synchronises the device
 * and sums elapsed milliseconds, launch counts and algorithmic FLOPs per category (arrays of
 * CBAS_PROF_NCAT entries); reset != 0 clears the records. */
enum { CBAS_PROF_PATCH = 0, CBAS_PROF_LAYERNORM = 1, CBAS_PROF_QKV = 2, CBAS_PROF_ATTENTION = 3,
       CBAS_PROF_OPROJ = 4, CBAS_PROF_UP = 5, CBAS_PROF_DOWN = 6,
       CBAS_PROF_OTHER = 7,      /* the CLS attention map kernel of the ..._attn forwards, the similarity map of ..._tokens */
       CBAS_PROF_NCAT = 8 };
int cbas_enc_profile(cbas_enc* h, int enable);
int cbas_enc_profile_read(cbas_enc* h, double* ms_by_cat, int64_t* launches_by_cat, double* flops_by_cat,
                          int reset);

/* ---- classifier head ---------------------------------------------------------------------- */

/* Mirrors ClassifierLSTMDeltas.__init__ (backend/classifier_head.py:62-64). */
typedef struct cbas_head_config {
    int32_t in_features;        /* 768 (D of the encoder)     */
    int32_t out_features;       /* C behaviours               */
    int32_t seq_len;            /* 31                         */
    int32_t bottleneck_dim;     /* 128                        */
    int32_t lin0_dim;           /* 256                        */
    int32_t lstm_hidden_size;   /* 64; any multiple of 16 up to 128 (inferred from the weights: workthreads.py:418-421) */
    int32_t center_window_size; /* 5                          */
    float   ema_alpha;          /* 0.3                        */
    int32_t lstm_layers;        /* 1 (stacked BiLSTM layers)  */
    int32_t use_acceleration;   /* 1: cls + delta + acc bottleneck streams; 0: cls + delta only
                                   (classifier_head.py:74-84, 158-162): the acc_* entries are then absent from the blob */
} cbas_head_config;

/* float32 elements expected by cbas_head_create, in this order (state_dict names):
 *   gate[1] attention_temp[1]
 *   cls_bottleneck.0.weight[Bn*I] .bias[Bn]  delta_bottleneck.0.weight .bias  acc_bottleneck.0.weight .bias
 *   cls_ln.weight[Bn] .bias[Bn]  delta_ln.weight .bias  acc_ln.weight .bias        (acc_* only when use_acceleration)
 *   lin0.0.weight[L0*NS*Bn] .bias[L0]                                                (NS = 3 or 2 streams)
 *   lin1.weight[C*I] .bias[C]
 *   per LSTM layer k = 0..lstm_layers-1 (input width L0 for k = 0, 2h above):
 *     lstm.weight_ih_lk[4h*in] weight_hh_lk[4h*h] bias_ih_lk[4h] bias_hh_lk[4h], then the same four _reverse
 *   attention_head.weight[2h] .bias[1]
 *   lin2.weight[C*2h] .bias[C]                                                                   */
int64_t cbas_head_weights_count(const cbas_head_config* cfg);

int cbas_head_create(const cbas_head_config* cfg, const float* weights_host, int64_t n_weights,
                     int device_id, cbas_head** out);
void cbas_head_destroy(cbas_head* h);

/* ClassifierLSTMDeltas.forward: x_dev (n_windows, seq_len, in_features) float32 ->
 * logits_dev (n_windows, C) and latent_dev (n_windows, 2h); either output may be NULL. */
int cbas_head_forward_windows(cbas_head* h, const float* x_dev, int64_t n_windows,
                              float* logits_dev, float* latent_dev, void* stream);

/* The window loop of infer_file over one clip: cls_f16_dev (n_frames, in_features) IEEE half rows
 * (what _cls.h5 holds) -> probs_dev (n_frames, C) = softmax(logits / max(1e-3, temperature)) and
 * optionally logits_dev (n_frames, C).  Window i = rows i-half .. i+half clamped to the clip
 * (replicate edge padding, backend/cbas.py:512-525). */
int cbas_head_infer_f16(cbas_head* h, const uint16_t* cls_f16_dev, int64_t n_frames, float temperature,
                        float* probs_dev, float* logits_dev, void* stream);

/* Same for the frames [first, first+count) of a clip of n_frames rows: outputs are count x C.
 * Windows still clamp to [0, n_frames), so a clip can be classified in segments while it is being
 * encoded (pass the number of rows encoded so far; a segment is final once first+count+seq_len/2
 * rows exist, or at the end of the clip). */
int cbas_head_infer_f16_range(cbas_head* h, const uint16_t* cls_f16_dev, int64_t n_frames, int64_t first,
                              int64_t count, float temperature, float* probs_dev, float* logits_dev,
                              void* stream);

/* The same over float32 rows: a `cls` dataset that is not IEEE half (the reference reads any dtype and converts with
 * .float(), backend/cbas.py:507-508). */
int cbas_head_infer_f32_range(cbas_head* h, const float* cls_f32_dev, int64_t n_frames, int64_t first,
                              int64_t count, float temperature, float* probs_dev, float* logits_dev,
                              void* stream);

int cbas_head_get_config(const cbas_head* h, cbas_head_config* out);

/* ---- fused streaming session: encode -> fp16 CLS -> head, rows never leave HBM ---------------------
 * The reference runs the two halves as two threads with a file in between (EncodeThread -> _cls.h5 ->
 * ClassificationThread: backend/workthreads.py:316-328, 488-498; chunk loop backend/cbas.py:423-440, window
 * loop :497-551).  A session owns a device clip buffer of `capacity_frames` rows (fp16 CLS + fp32
 * probabilities) and a stream for the head; pushes queue batches of <= max_batch frames on the encoder's
 * slots / compute lanes (splitting larger pushes), and every `classify_every` frames whose +-seq_len/2
 * context has been encoded are classified (windows clamp at the clip's ends exactly as infer_file's
 * replicate padding does).  Results are identical to cbas_enc_forward_u8 + cbas_head_infer_f16 over the
 * whole clip, bit for bit.  The encoder and head handles must outlive the session and must not be driven
 * through their own asynchronous entry points while a clip is open.
 * `head` may be NULL: an encode-only session (the chunk loop of encode_file with the rows kept in HBM until the clip
 * ends); probs_* outputs of cbas_fused_finish are then left untouched / NULL. */
typedef struct cbas_fused cbas_fused;
int cbas_fused_create(cbas_enc* enc, cbas_head* head, int64_t capacity_frames, float temperature,
                      int64_t classify_every /* 0: 1024 */, cbas_fused** out);
void cbas_fused_destroy(cbas_fused* f);
/* Start a new clip (waits for the previous clip's device work). */
int cbas_fused_reset(cbas_fused* f);
/* Append n frames from host memory (same layout / pinned-memory rules as cbas_enc_submit_u8_host). */
int cbas_fused_push_u8_host(cbas_fused* f, const uint8_t* frames_host, int n, int height, int width,
                            int64_t frame_stride, int64_t row_stride, int64_t pixel_stride);
/* Append n frames already in HBM, ready once everything queued on `after_stream` has run; they must stay
 * valid until the clip is finished. */
int cbas_fused_push_u8(cbas_fused* f, const uint8_t* frames_dev, int n, int height, int width,
                       int64_t frame_stride, int64_t row_stride, int64_t pixel_stride, void* after_stream);
/* Classify the tail and hand out the clip: any of cls_f16_host (N x D halves), probs_host (N x C floats) are filled;
 * cls_f16_dev / probs_dev receive the session's device buffers (valid until the next reset / push).  n_frames receives N.
 * stream == NULL: the call blocks until every output is complete.  stream != NULL: the host is NOT blocked - `stream` is
 * made to wait for the outputs instead (host buffers, which should then be page-locked, are complete when `stream` reaches
 * that point: record an event there and wait for it); the next clip may be pushed through another session meanwhile. */
int cbas_fused_finish(cbas_fused* f, uint16_t* cls_f16_host, float* probs_host, const uint16_t** cls_f16_dev,
                      const float** probs_dev, int64_t* n_frames, void* stream);
/* cbas_fused_finish for back-to-back clips: everything is QUEUED (last batches, tail classification, the copies into the
 * page-locked host buffers) and the call returns at once; cbas_fused_wait(f) blocks until that clip's results are complete
 * (a no-op when nothing is pending).  Push the next clip through ANOTHER session in between and the device never idles
 * at a clip boundary.  (Ordering another stream after the clip - the `stream` form above - is not used for this: handed the
 * legacy NULL stream, hipStreamWaitEvent blocks the HOST until the event has completed, 15 ms at the end of every clip.) */
int cbas_fused_finish_async(cbas_fused* f, uint16_t* cls_f16_host, float* probs_host, int64_t* n_frames);
int cbas_fused_wait(cbas_fused* f);
/* Rows out WHILE the clip runs - what encode_file's per-chunk `dset[...] = ...; f.flush()` is to the reference
 * (backend/cbas.py:436-440): called right after cbas_fused_reset with a page-locked buffer for the whole clip, it makes
 * the session copy CLS rows to it as their batches land (one device->host copy per 512 rows, queued behind the batches
 * that produce them); cbas_fused_finish then copies only the remainder (its cls_f16_host is ignored).  ONE consumer thread -
 * the file writer - follows with cbas_fused_rows_ready(f, block): the number R of leading rows that are complete in the
 * buffer (block != 0: waits for the next queued copy if there is one); it may run concurrently with pushes.  With this the
 * `_cls.h5` of a clip is all but written when its last batch ends (the file write was 21-26 ms of an 18 000-frame clip). */
int cbas_fused_stream_rows(cbas_fused* f, uint16_t* cls_f16_host);
int64_t cbas_fused_rows_ready(cbas_fused* f, int32_t block);

/* ---- head training -------------------------------------------------------------------------
 * Replaces the optimisation step inside train_lstm_model (backend/cbas.py:1326-1348):
 *   optimizer.zero_grad(); final_logits, rawm = model(d)          (model.train(): dropout active)
 *   loss = CrossEntropyLoss(weight, label_smoothing)(final_logits, l)
 *        + sum(off_diagonal(cov(rawm))^2);   loss.backward();   optimizer.step()
 * with optimizer = Adam([all but gate], [gate, weight_decay 1e-3], lr, weight_decay) (cbas.py:1305-1308).
 * Forward, loss, backward and the Adam update all run on the device in fp32.  Dropout keep-masks come
 * from a counter-based hash of (seed, step, layer, element), not from torch's RNG. */
typedef struct cbas_head_trainer cbas_head_trainer;

typedef struct cbas_train_config {
    float    lr;               /* 1e-4 (cbas.py:1275)                                   */
    float    weight_decay;     /* L2 added to the gradient, all parameters but gate     */
    float    label_smoothing;  /* nn.CrossEntropyLoss(label_smoothing=...)              */
    int32_t  max_batch;        /* largest number of windows per step (512)              */
    uint64_t seed;             /* dropout stream seed                                   */
    int32_t  dropout;          /* 1: Dropout(0.1) x3 + Dropout(0.15) as in train();  0: off */
} cbas_train_config;

/* weights_host: the same blob cbas_head_create takes.  class_weights_host: C floats or NULL.
 * Configurations: lstm_hidden_size 16, 32, ... 128; 3 or 2 bottleneck streams (use_acceleration); 1-4 LSTM layers;
 * seq_len 3..101; bottleneck_dim a multiple of 64; out_features <= 64. */
int cbas_head_train_create(const cbas_head_config* cfg, const cbas_train_config* tcfg, const float* weights_host,
                           int64_t n_weights, const float* class_weights_host, int device_id,
                           cbas_head_trainer** out);
void cbas_head_train_destroy(cbas_head_trainer* t);

/* One optimisation step on a batch of n_windows (<= max_batch) explicit windows:
 * x_dev (n_windows, seq_len, in_features) float32, labels_dev (n_windows) int32, both device pointers.
 * loss_host (optional, 3 floats: total, cross-entropy, covariance penalty) is filled after a stream
 * synchronisation; pass NULL to keep the step asynchronous.  update = 0 computes loss and gradients
 * only (no Adam step; the step counter and the dropout stream do not advance). */
int cbas_head_train_step(cbas_head_trainer* t, const float* x_dev, const int32_t* labels_dev, int32_t n_windows,
                         int32_t update, float* loss_host, void* stream);

/* Training and scoring from a store of CLS rows that stays in device memory.  The reference builds every window on the
 * host: one HDF5 slice of seq_len rows around the centre frame, `.float()`, stacked into the batch and copied to the device
 * (LazyStandardDataset / LazyBalancedDataset.__getitem__, backend/cbas.py:194-228, feeding the loop of cbas.py:1326-1348).
 * Here the half-precision rows of all `_cls.h5` files lie in one device array and a window is named by its first row:
 *   x_out[w][t][:] = float(rows[first_row[w] + t][:])        w < n_windows, t < seq_len      (f16 -> f32 is exact)
 * rows_f16_dev (n_rows, dim) IEEE half, first_row_dev (n_windows) int64, x_out_dev (n_windows, seq_len, dim) float32: all
 * device pointers, on the device `stream` belongs to.  A row outside [0, n_rows) is never read and comes out as zeros.
 * CBAS_EINVAL: a NULL pointer, n_rows < 0, dim / seq_len / n_windows < 1, seq_len > 65536, dim * seq_len > 2^23. */
int cbas_rows_gather_windows(const uint16_t* rows_f16_dev, int64_t n_rows, int32_t dim, const int64_t* first_row_dev,
                             int32_t n_windows, int32_t seq_len, float* x_out_dev, void* stream);
/* cbas_head_train_step on windows gathered from such a store: exactly cbas_rows_gather_windows into a buffer the trainer
 * has owned since cbas_head_train_create (max_batch windows), then cbas_head_train_step on it, both on `stream`.
 * CBAS_EINVAL also when dim != in_features, seq_len != the trainer's seq_len or n_windows > max_batch. */
int cbas_head_train_step_rows(cbas_head_trainer* t, const uint16_t* rows_f16_dev, int64_t n_rows, int32_t dim,
                              const int64_t* first_row_dev, const int32_t* labels_dev, int32_t n_windows, int32_t seq_len,
                              int32_t update, float* loss_host, void* stream);
/* One optimisation step (update = 1) for each of k trainers from ONE such store: the trials of a run (TrainingThread,
 * backend/workthreads.py:596-690, trains them one after another) differ in their random draws alone, and a step of this head
 * is launch latency and a serial LSTM recurrence more than arithmetic.  Trainer j steps on the n_windows[j] windows named by
 * first_row_dev[j] with labels labels_dev[j] (device pointers in host tables of k entries) and ends with the parameters, the
 * gradients and the Adam moments, bit for bit, that cbas_head_train_step_rows leaves for the same windows.
 *   - Every trainer has a stream of its own (made by its first call here, released by cbas_head_train_destroy) and owns every
 *     buffer its step writes; the store is only read.  The gather, the LSTM, expand and pool kernels, the transposes and the
 *     GEMMs of trainer j are queued on trainer j's stream, where they overlap with the other trainers'.
 *   - For k > 1 the small kernels (Adam, the column sums, the cross-entropy pair, the covariance off-diagonal, add / copy,
 *     GELU + dropout) are ONE launch for all k on trainer 0's stream, ordered against the others with events; per element
 *     and per reduction they are the single-trial kernels.  k = 1 queues exactly what cbas_head_train_step_rows queues.
 *   - Nothing is synchronised between trainers on the host.  losses_host (k x 3 floats: total, cross-entropy, covariance
 *     penalty per trainer) is filled after ONE wait at the end; NULL: no wait, the call returns with everything queued.
 * The caller orders these streams against its own: the pointers must be valid and their contents complete when the call is
 * made, and stay so until the trainers are read (cbas_head_train_read synchronises the device).  A trainer is stepped either
 * here or on a caller's stream; changing over needs a device synchronisation in between.
 * CBAS_EINVAL, with nothing queued and no trainer changed: k outside [1, CBAS_TRAIN_MULTI_MAX], a NULL table, trainer or
 * table entry, the same trainer twice, dim != in_features, trainers that differ in head configuration or device,
 * n_windows[j] outside [1, max_batch of trainer j], n_rows < 0. */
#define CBAS_TRAIN_MULTI_MAX 8
int cbas_head_train_step_rows_multi(cbas_head_trainer** trainers, int32_t k, const uint16_t* rows_f16_dev, int64_t n_rows,
                                    int32_t dim, const int64_t* const* first_row_dev, const int32_t* const* labels_dev,
                                    const int32_t* n_windows, float* losses_host);

/* The tail of a training job on the device: scoring a split and fitting the calibration temperature from such a store.
 *
 * cbas_head_score_rows replaces the loop of evaluate_on_split (backend/cbas.py:1235-1242) and the logit collection of
 * fit_temperature (backend/workthreads.py:115-120): per batch of 512 a host-built window tensor, its copy to the device,
 * model(x), `logits.argmax(1).cpu()`; then sklearn's confusion_matrix over the host lists (cbas.py:1250).  Here the
 * n_windows windows named by first_row_dev (int64, as for cbas_rows_gather_windows) are gathered and run through the head
 * 512 at a time, and per window w:
 *   logits_out_dev[w][:]  = the head's logits (float32, n_windows x C), bit-identical to cbas_rows_gather_windows +
 *                           cbas_head_forward_windows on any split of the windows into batches;        may be NULL
 *   pred_out_dev[w]       = index of the FIRST maximum of the logits, as torch.argmax (int32);          may be NULL
 *   confusion_dev[labels_dev[w]][pred] += 1   (int64, C x C, row = true label; ADDED to what the caller put there, with
 *                           integer atomics, so the matrix does not depend on the order of execution);  may be NULL
 * labels_dev (int32, n_windows) is needed with confusion_dev only.  All pointers are device pointers on the head's device.
 * The call synchronises `stream` once before it returns, to report: CBAS_ERANGE when a window's logits hold a NaN (such a
 * window gets prediction -1 and no count), CBAS_EINVAL for a label outside [0, C) (no count), a NULL rows / first_row,
 * dim != in_features, n_windows < 1 or no output requested. */
int cbas_head_score_rows(cbas_head* h, const uint16_t* rows_f16_dev, int64_t n_rows, int32_t dim,
                         const int64_t* first_row_dev, const int32_t* labels_dev, int64_t n_windows,
                         float* logits_out_dev, int32_t* pred_out_dev, int64_t* confusion_dev, void* stream);
/* The closure of fit_temperature (backend/workthreads.py:127-133, `criterion(all_logits / temp, all_labels)` and its
 * backward pass), one launch per evaluation:
 *   out2_dev[0] = mean over the n rows of -log_softmax(logits[r] / temp)[labels[r]]      (float32 row terms, as torch's)
 *   out2_dev[1] = d out2_dev[0] / d temp = mean of (logits[r][label] - sum_j softmax(logits[r] / temp)[j] * logits[r][j]) / temp^2
 * logits_dev (n, n_classes) float32, labels_dev (n) int32, out2_dev two floats: device pointers on one device; nothing is
 * copied or synchronised.  The rows are summed in a fixed order without floating-point atomics (per thread in ascending row
 * order, a tree per workgroup, a tree over the workgroups' partial sums in the workgroup that finishes last; the grid depends
 * on n alone), so equal inputs give equal bits on every launch.  The chain rule from temp to the fitted parameter
 * (softplus, clamp) is the caller's.  A label outside [0, n_classes) makes both results NaN.
 * CBAS_EINVAL: a NULL pointer, n < 1, n_classes outside [1, 64], temp <= 0 or NaN. */
int cbas_logits_nll(const float* logits_dev, const int32_t* labels_dev, int64_t n, int32_t n_classes, float temp,
                    float* out2_dev, void* stream);

/* The disagreement report of a training job (TrainingThread._generate_disagreement_report, backend/workthreads.py:728-811)
 * from probabilities that are on the device (cbas_head_infer_f16 over the resident rows of a training clip), instead of
 * writing `_outputs.csv`, reading it back with pandas and scanning it per instance.
 *
 * cbas_probs_top1 replaces :762-763 (`idxmax(axis=1)` and `max(axis=1)` over the behaviour columns): for each of the n rows
 * of probs_dev (n, n_classes) float32
 *   pred_dev[r] = index of the FIRST maximum (int32), conf_dev[r] = that maximum (float32).
 * A row that holds a NaN gets pred -1 and conf NaN, and CBAS_TOP1_FLAG_NAN is OR-ed into *flags_dev (a device word the caller
 * zeroes and reads; the reference's `except` at :764 drops such a clip).  Asynchronous on `stream`; nothing is copied.
 * CBAS_EINVAL: a NULL pointer, n < 1, n_classes outside [1, 64]. */
#define CBAS_TOP1_FLAG_NAN 1u
int cbas_probs_top1(const float* probs_dev, int64_t n, int32_t n_classes, int32_t* pred_dev, float* conf_dev,
                    uint32_t* flags_dev, void* stream);
/* cbas_disagreement_runs replaces :777-803, for all instances of all clips in one call.  pred_dev / conf_dev hold the frames of
 * all clips back to back (n_frames_total of them), clip_table_dev (n_clips, 2) int64 gives each clip's (first frame, frames).
 * Instance i is (inst_clip[i], inst_start[i], inst_end[i], inst_label[i]), all int32: its frames are
 * [start, min(end, frames - 1)] of its clip (`iloc[start:end+1]`; an empty range yields no record); label is the class index of
 * the human label, or -1 for a label that is no behaviour - then every frame is an error frame, as under the string
 * comparison of :781.  An error frame is one with pred != label.  One record per maximal run of consecutive error frames
 * INSIDE one instance (runs of abutting or overlapping instances never merge; overlapping instances each report theirs):
 *   model_prediction  the most frequent pred of the run; among equally frequent ones the class with the smallest
 *                     name_rank_dev[class] (int32[n_classes], the rank of the class NAME in sorted order: pandas mode()
 *                     returns sorted values and :794 takes [0]).  Frames with pred -1 are error frames but are not counted
 *                     here (mode() drops NaN); -1 when the run has no other frame.
 *   model_confidence  the mean of conf over the run in float64.  The sum is formed in a fixed order that depends on the run
 *                     alone (64 interleaved partial sums, each in ascending frame order, then a fixed tree), without
 *                     floating-point atomics; for top-1 probabilities (>= 1/64) of up to 2^22 frames every partial sum is
 *                     exact, so it is the sum in ascending frame order bit for bit.
 * Records are ordered by (instance, start_frame) whatever the order of execution (count, exclusive scan, emit; nothing is
 * appended with an atomic), so equal inputs give equal bytes.  Returns the number of records (>= 0) or a negative CBAS_E*
 * code; *needed_host (may be NULL) receives the number of records whenever the instances were accepted.  records_dev holds
 * `capacity` records; fewer than needed is CBAS_EINVAL and writes nothing (capacity 0 with records_dev NULL asks for the
 * count).  CBAS_EINVAL also for: a NULL pointer, n_clips / n_instances < 1, n_classes outside [1, 64], an instance whose clip
 * lies outside the table, whose label lies outside [-1, n_classes), with start < 0 or end < start, a table entry that reaches
 * outside the n_frames_total frames, a pred outside [-1, n_classes) - each checked on the device before anything is indexed
 * with it.  The call synchronises `stream`. */
typedef struct cbas_disagreement_run {
    int32_t instance;          /* index into the inst_* arrays */
    int32_t start_frame;       /* first and last frame of the run, in frames of the instance's clip */
    int32_t end_frame;
    int32_t model_prediction;
    double  model_confidence;
} cbas_disagreement_run;
int64_t cbas_disagreement_runs(const int32_t* pred_dev, const float* conf_dev, int64_t n_frames_total,
                               const int64_t* clip_table_dev, int32_t n_clips, const int32_t* inst_clip_dev,
                               const int32_t* inst_start_dev, const int32_t* inst_end_dev, const int32_t* inst_label_dev,
                               int32_t n_instances, const int32_t* name_rank_dev, int32_t n_classes,
                               cbas_disagreement_run* records_dev, int64_t capacity, int64_t* needed_host, void* stream);

/* What CBAS does with a clip's probabilities after inference - events, guided-labelling pre-labels, actogram bins
 * (backend/cbas.py:903-1000) - from per-frame values that are on the device, instead of reading `_outputs.csv` back with
 * pandas and walking it in Python.  The per-frame arrays hold the frames of all clips back to back (n_frames_total of them);
 * clip_table_dev (n_clips, 2) int64 gives each clip's (first frame, frames); clips must not overlap.  Every table entry and
 * label is checked on the device before anything is indexed with it.
 *
 * cbas_labels_median replaces :939, `medfilt(df['predicted_index'], kernel_size=smoothing_window)`, per clip: out_dev[f] is
 * the median of the kernel_size values around frame f of its clip.  As scipy does, every clip is padded with
 * kernel_size // 2 ZEROS at both ends, so the first and last frames of a clip are pulled towards class 0; windows never cross
 * clips.  Values lie in [-1, n_classes): -1 is the reference's `fillna(-1)` (:938) and takes part as -1.  kernel_size is
 * odd, >= 1 (1 copies) and may exceed a clip's length.  The result is an integer: the smallest value whose count in the
 * window, cumulated from -1 upwards with the padding zeros added to value 0, reaches (kernel_size + 1) / 2.
 * out_dev and pred_dev must not overlap at all (a window reads its neighbours; only out_dev == pred_dev is detected).
 * CBAS_EINVAL: a NULL pointer, out_dev == pred_dev, n_frames_total < 0, n_clips < 1, n_classes outside [1, 64], an even or
 * non-positive kernel_size, a table entry that reaches outside the n_frames_total frames, a value outside [-1, n_classes).
 * The call synchronises `stream` (it reads the refusals back). */
int cbas_labels_median(const int32_t* pred_dev, int64_t n_frames_total, const int64_t* clip_table_dev, int32_t n_clips,
                       int32_t n_classes, int32_t kernel_size, int32_t* out_dev, void* stream);
/* cbas_label_runs replaces the `df.iterrows()` state machine of Dataset.predictions_to_instances (:910-925) and the block
 * scan of Dataset.predictions_to_instances_with_confidence (:944-955).  key_dev is a label per frame (cbas_probs_top1's pred,
 * or cbas_labels_median's output), conf_dev the top-1 probability.  With use_threshold != 0 a frame's key counts as -1
 * unless (double)conf >= threshold (`row['max_prob'] >= threshold`, :912; a NaN is not).  One record per maximal run of
 * consecutive frames of ONE clip with equal key != -1, ordered by (clip, start_frame) whatever the order of execution (count,
 * exclusive scan, emit; nothing is appended with an atomic):
 *   with the threshold     the events of :910-925 - a run ends where the label changes or the probability drops below the
 *                          threshold, and a new one starts on the same frame when only the label changed;
 *   without                the blocks of :944-955; a block whose label is NaN there (key -1) is skipped, as at :950.
 *   confidence             the mean of conf over the run in float64 (:951), summed in the fixed order of
 *                          cbas_disagreement_runs' model_confidence (the same device function).
 * Returns the number of records (>= 0) or a negative CBAS_E* code; *needed_host (may be NULL) receives the number of records
 * whenever the arguments were accepted.  records_dev holds `capacity` records; with fewer than needed the call returns
 * CBAS_EINVAL and the buffer's contents are unspecified (capacity 0 with records_dev NULL asks for the count).  CBAS_EINVAL
 * also for: a NULL pointer, n_frames_total < 0, n_clips < 1, n_classes outside [1, 64], a NaN threshold, a table entry that
 * reaches outside the n_frames_total frames, a key outside [-1, n_classes).  The call synchronises `stream` once. */
typedef struct cbas_label_run {
    int32_t clip;              /* row of clip_table_dev */
    int32_t start_frame;       /* first and last frame of the run, in frames of the clip */
    int32_t end_frame;
    int32_t label;
    double  confidence;
} cbas_label_run;
int64_t cbas_label_runs(const int32_t* key_dev, const float* conf_dev, int64_t n_frames_total, const int64_t* clip_table_dev,
                        int32_t n_clips, int32_t n_classes, int32_t use_threshold, double threshold,
                        cbas_label_run* records_dev, int64_t capacity, int64_t* needed_host, void* stream);
/* cbas_activity_bins replaces :977-979 / :991-993 and :999 of Actogram.__init__.  probs_dev (n_total, n_classes) float32
 * holds the rows of all `_outputs.csv` files of a recording back to back, in the caller's order.  bins_dev[j] (int64,
 * n_bins = ceil(n_total / bin_frames) of them, zeroed by the call) counts the frames f of [j * bin_frames, (j + 1) *
 * bin_frames) with
 *   (double)p[f][behavior] * (is_max ? 1.0 : 0.0) >= threshold,      is_max = (max of the OTHER columns) < p[f][behavior].
 * The comparison is strict, so a tie is no maximum; the maximum skips NaN as pandas' does and over no value (n_classes == 1,
 * or every other column NaN) it is NaN, so is_max is false.  A threshold <= 0 therefore counts every frame whose own
 * probability is a number; a NaN probability counts nothing.  Bins run across file boundaries, as the reference's
 * concatenated list does.  Integer atomics only: equal inputs give equal bins.  Runs on the device probs_dev lives on,
 * asynchronously on `stream`.
 * CBAS_EINVAL: a NULL pointer, n_total < 1, n_classes outside [1, 64], behavior outside [0, n_classes), bin_frames < 1,
 * n_bins != ceil(n_total / bin_frames). */
int cbas_activity_bins(const float* probs_dev, int64_t n_total, int32_t n_classes, int32_t behavior, double threshold,
                       int64_t bin_frames, int64_t* bins_dev, int64_t n_bins, void* stream);

/* Copy the current parameters (what = 0), the gradients of the last step (what = 1) or Adam's first / second moment
 * (what = 2 / 3) to the host, in the blob order of cbas_head_create (n = cbas_head_weights_count).  Synchronises the device. */
int cbas_head_train_read(cbas_head_trainer* t, int32_t what, float* blob_host, int64_t n);
/* Logits (n_windows, C) and latent (n_windows, 2h) of the LAST step's forward pass (device -> host). */
int cbas_head_train_last_outputs(cbas_head_trainer* t, float* logits_host, float* latent_host, int32_t n_windows);

/* ---- output text ---------------------------------------------------------------------------
 * `<video>_<model>_outputs.csv` is written by the reference as
 *   pd.DataFrame(np.array(all_probs), columns=behaviors).to_csv(output_file, index=False)    backend/cbas.py:565
 * i.e. one header line, then per frame the float32 probabilities as numpy's str(np.float32): shortest decimal text that
 * round-trips in float32, positional for 1e-4 <= |x| < 1e16 (else scientific with a signed, >= 2-digit exponent),
 * NaN as an empty field, '\n' line ends.  These two calls produce exactly those bytes (host memory in, no GPU involved):
 * cbas_csv_format_f32 formats n_rows x n_cols values into `out` and returns the byte count (with out = NULL: an upper
 * bound for the buffer); cbas_csv_write_f32 writes `header_line` (already quoted, '\n'-terminated; may be NULL) and the
 * rows to `path`, formatting on up to n_threads threads. */
int64_t cbas_csv_format_f32(const float* values_host, int64_t n_rows, int32_t n_cols, char* out, int64_t cap);
int cbas_csv_write_f32(const char* path, const char* header_line, const float* values_host, int64_t n_rows,
                       int32_t n_cols, int32_t n_threads);

/* ---- frame source: Motion-JPEG decode ---------------------------------------------------------
 * The reference reads frames with decord.VideoReader(path, ctx=cpu(0)).get_batch(range(i, end)).asnumpy()
 * (backend/cbas.py:402,425) and keeps channel 1 (:431).  For Motion-JPEG streams this call is that decoder: frame k is the
 * JPEG at data[offsets[k] .. offsets[k] + sizes[k]); every frame must be height x width; channels = 1 writes the green
 * plane (n, H, W), channels = 3 the RGB frame (n, H, W, 3) - into `out` (host memory, e.g. a page-locked ring piece),
 * on up to n_threads threads.  Baseline / extended-sequential Huffman JPEG, 8 bit, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0,
 * restart intervals, Annex K tables when a frame has no DHT; pixel-identical to libjpeg-turbo's default decode (islow
 * IDCT, fancy upsampling).  Returns CBAS_EINVAL for a frame it cannot decode (cbas_last_error says whether the stream is
 * corrupt or "unsupported: ..."), with the index of the first such frame in *bad_frame (may be NULL). */
int cbas_mjpeg_decode(const uint8_t* data, const uint64_t* offsets, const uint32_t* sizes, int32_t n_frames,
                      int32_t height, int32_t width, int32_t channels, uint8_t* out, int32_t n_threads,
                      int32_t* bad_frame);

/* ---- frame source: keep the consumed channel ---------------------------------------------------
 * backend/cbas.py:431 keeps channel 1 of the decoded RGB frames (`frames_np[:, :, :, 1]`).  dst[i] = src[i * n_channels +
 * channel] for n_pixels pixels (any number of frames back to back), on up to n_threads host threads: what the decode-ahead
 * thread runs while it fills a page-locked ring piece, so that only the consumed plane is staged and copied to the device
 * (50 176 bytes per 224 x 224 frame instead of 150 528).  Host memory in and out, no GPU involved. */
int cbas_pick_channel_u8(const uint8_t* src, int64_t n_pixels, int32_t n_channels, int32_t channel, uint8_t* dst,
                         int32_t n_threads);

/* ---- misc --------------------------------------------------------------------------------- */

const char* cbas_last_error(void);
int cbas_abi_version(void);
/* Device facts for reports: writes the gfx arch name (e.g. "gfx950"), CU count and HBM bytes. */
int cbas_device_info(int device_id, char* arch_out, int arch_cap, int32_t* n_cu, int64_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CBAS_MI355X_H */
