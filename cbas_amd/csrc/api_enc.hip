// C-ABI: encoder handle (DinoEncoder replacement).  See include/cbas_mi355x.h for the contract and
// the reference lines each entry point stands in for.
#include <math.h>
#include <string.h>
#include <new>
#include <vector>
#include <algorithm>

#include "api_common.h"
#include "kernels.h"
#include <chrono>

thread_local char g_cbas_err[512] = {0};

extern "C" const char* cbas_last_error(void) { return g_cbas_err; }
extern "C" int cbas_abi_version(void) { return CBAS_ABI_VERSION; }

extern "C" int cbas_device_info(int device_id, char* arch_out, int arch_cap, int32_t* n_cu, int64_t* hbm_bytes) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    if (arch_out && arch_cap > 0) {
        strncpy(arch_out, prop.gcnArchName, arch_cap - 1);
        arch_out[arch_cap - 1] = 0;
    }
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    return CBAS_OK;
}

namespace {

struct LayerW {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *o_b, *ls1, *up_b, *down_b, *ls2;
    float* qkv_b;                       // [3D] = q.b | 0 | v.b
    f16 *wqkv, *wo, *wup, *wdown;       // fp16 (hi)
    f16 *wqkv_lo, *wo_lo, *wup_lo, *wdown_lo;
    // precision 2: MX-fp8 copies (e4m3 bytes, same [N][K] layout) + E8M0 block scales [K/128][N] dwords
    uint8_t *wqkv8 = nullptr, *wo8 = nullptr, *wup8 = nullptr, *wdown8 = nullptr;
    uint32_t *sqkv = nullptr, *so = nullptr, *sup = nullptr, *sdown = nullptr;
    // LayerNorm fold (precision 0): fp16(gamma o W) of the two GEMMs that consume a LayerNorm output, the column sums of
    // those rounded weights and the folded biases beta W^T + b
    f16 *wqkv_f = nullptr, *wup_f = nullptr;
    float *qkv_cs = nullptr, *qkv_bf = nullptr, *up_cs = nullptr, *up_bf = nullptr;
    // precision 3: the fp32 weights themselves ([N][K] as stored in the blob; q | k | v packed into one [3D][D] copy)
    const float *wqkv32 = nullptr, *wo32 = nullptr, *wup32 = nullptr, *wdown32 = nullptr;
    // precision 4: power-of-two scale per weight tensor that brings max |w| into [1, 2) before the fp16 split
    float sc_qkv = 1.f, sc_o = 1.f, sc_up = 1.f, sc_down = 1.f;
};

struct Slot {
    uint8_t* in_host = nullptr;   // pinned, green planes
    uint8_t* in_dev = nullptr;
    uint16_t* out16_host = nullptr;
    float* out32_host = nullptr;
    f16* out16_dev = nullptr;
    float* out32_dev = nullptr;
    hipEvent_t ev_copied = nullptr, ev_done = nullptr, ev_in = nullptr;
    int n = 0;
    bool busy = false;
    bool used = false;            // ev_copied / ev_done have been recorded at least once
    bool dev_mode = false;        // submitted by cbas_enc_submit_u8 (device in/out) rather than ..._host
};

// One compute lane: the activation workspace of one batch in flight and the stream its asynchronous batches run on.  The
// forward functions take the lane they work in as a parameter; nothing else in the handle points into a workspace.
// Precisions 3 / 4 and ConvNeXt keep floats in the buffers declared f16*.  A buffer the handle's mode has no use for is null.
struct Lane {
    f16 *A_patch = nullptr, *h16 = nullptr, *qkv16 = nullptr, *u16 = nullptr;
    float* x = nullptr;
    // compact per-frame rows of the pruned last layer (only the CLS row is consumed: [tf]:540-541, cbas.py:677):
    // cls16 = [q | ctx | LN2 | (pad)] x [max_batch][D] fp16, then GELU(up) [max_batch][F]: cls_rows()
    f16* cls16 = nullptr;
    uint32_t *sc_h = nullptr, *sc_u = nullptr; // precision 2: block scales of the fp8 activations in h16 / u16 ([K/128][rows_cap])
    f16* x16 = nullptr;                // LayerNorm fold: [rows_cap][D] fp16 copy of the residual stream (the folded GEMMs' A operand)
    float2* lnst = nullptr;            //                 [4][rows_cap] per-row LayerNorm statistics by 256-column block
    hipStream_t stream = nullptr;      // lane 0: the handle's `compute`; lane 1: its own
};

// bytes of each buffer of a lane, 0 for one the mode does not have: vit_lane_bytes / cnx_lane_bytes -> alloc_lane
struct LaneBytes { size_t A_patch = 0, h16 = 0, qkv16 = 0, u16 = 0, x = 0, cls16 = 0, sc_h = 0, sc_u = 0, x16 = 0, lnst = 0; };

}  // namespace

struct cbas_enc {
    cbas_enc_config cfg;
    int device;
    int D, F, L, NH, R, NP;            // NP = prefix tokens
    // CBAS_MLP_GELU / CBAS_MLP_SWIGLU (cbas_enc_create_mlp).  A gated handle keeps gate_proj | up_proj as ONE weight of 2F rows,
    // interleaved in blocks of 32 (EPI_SWIGLU, kernels.h): LayerW::wup / wup32 / up_b point at it and the up GEMM runs with N = 2F;
    // its output, the workspace u16 and the down projection are [rows][F] as for a GELU handle.
    int mlp = 0;
    float* gu_bias_all = nullptr;      // gated: [L][2F] interleaved gate | up biases
    float* gu_scratch = nullptr;       // gated, create only: one layer's interleaved fp32 weight on its way to the fp16 / split copy
    float* blob = nullptr;             // all fp32 parameters on device
    std::vector<LayerW> layers;
    const float *prefix, *patch_b, *norm_w, *norm_b;
    f16 *w16 = nullptr, *w16_lo = nullptr;     // all fp16 weights (hi / lo)
    uint8_t* w8 = nullptr;                     // precision 2: all MX-fp8 weights
    uint32_t* w8_sc = nullptr;                 //              and their block scales
    f16 *wpatch, *wpatch2, *wpatch_lo, *wpatch2_lo;
    float* w32 = nullptr;                      // precision 3 / 4: packed q|k|v weights of every layer + the (D,256) patch weight
    const float* wpatch32 = nullptr;
    float sc_patch = 1.f;                      // precision 4: scale of the patch weight (see LayerW)
    float* qkv_bias_all = nullptr;
    unsigned* nonfinite_dev = nullptr;  // frames whose CLS row came out non-finite since the last cbas_enc_check_finite
    float* prefix_dev = nullptr;        // (1+R, D): cls (+ its position embedding for DINOv2) | registers
    float* pos_tab = nullptr;           // DINOv2: (Pmax, D) position embedding interpolated to the current grid
    std::vector<float> pos_host;        // DINOv2: raw (1+G*G, D) table
    int pos_interp = CBAS_POS_INTERP_BICUBIC_AA;   // how it is resampled to a frame's grid (cbas_enc_set_pos_interp)
    // precision 2: which GEMMs of a layer take MX-fp8 operands (CBAS_FP8_PLAN_* bits; cbas_enc_set_fp8_plan).  A GEMM outside the
    // plan runs as precision 0 runs it, on the fp16 weights every precision-2 handle holds anyway (the CLS tail of the pruned
    // last layer uses them), in the same workspace: an fp8 activation is half the bytes of the fp16 one it replaces.
    int fp8_plan = CBAS_FP8_PLAN_ALL;
    bool vit_forward_seen = false;      // a ViT forward was queued: the plan is fixed from here on
    // RoPE (DINOv3) / interpolated position-embedding (DINOv2) tables, one set per patch grid seen so far.  A new
    // grid gets FRESH device buffers filled by a blocking copy, so no stream has to be drained when a queue mixes
    // resolutions; rope_cos / rope_sin / pos_tab point at the set of the batch being queued (kernel arguments are
    // captured at launch).  Only when POS_TABLES_MAX grids are cached is the oldest one recycled behind a device sync.
    struct PosTable { int nh = 0, nw = 0; float *cos = nullptr, *sin = nullptr, *fac = nullptr, *pos = nullptr; uint64_t last_use = 0; };
    static constexpr int POS_TABLES_MAX = 8;
    std::vector<PosTable> pos_tables;
    uint64_t pos_clock = 0;
    float *rope_cos = nullptr, *rope_sin = nullptr;
    float* rope_fac = nullptr;          // the same angles by axis, [nh + nw][cos(16) | sin(16)] (GemmParams::rope_fac)
    int rope_nh = 0, rope_nw = 0;
    int rope_cap = 0;
    int64_t rows_cap = 0, prow_cap = 0;      // token / patch rows a lane's workspace holds
    bool prune_last = true;
    bool rope_in_lds = true;           // cbas_enc_debug_option("rope_lds"): q|k|v epilogue reads the by-axis RoPE table from LDS
    // LayerNorm fold: see run_blocks.  fold_ok = the folded weights exist; ln_fold = use them (debug option "ln_fold").
    // Off by default: with two batches in flight it measured +0 ... +1 % (the LayerNorm kernels already hide under the other
    // lane's GEMMs, the fold moves their work into epilogues that do not); -5.4 % of kernel time with one batch in flight.
    bool fold_ok = false, ln_fold = false;
    f16* w16_fold = nullptr;
    float* fold_vec = nullptr;
    int last_rows = 0;
    hipStream_t compute = nullptr, copy = nullptr;
    hipStream_t aux = nullptr;          // cbas_enc_check_finite's 4-byte copies: not the NULL stream (torch's default stream is one: a copy there would wait for the caller's own work)
    Slot slots[CBAS_ENC_SLOTS];
    int64_t slot_bytes = 0;             // pinned staging / device input bytes per slot: max_batch x H x W x 4 channels
    // Two batches in flight: the asynchronous entry points (cbas_enc_submit_u8 / ..._host) alternate two
    // compute lanes, each a full workspace + its own stream, so that one batch's partial tile rounds,
    // LayerNorm and attention run under the other batch's GEMMs (+10 % measured; outputs bit-identical).
    // The lanes own every activation buffer of the handle (alloc_lane / free_lane).  The synchronous cbas_enc_forward_* and the
    // debug taps work in lanes[0] on the caller's stream / on `compute`; a handle created under CBAS_LANES=1 has no lanes[1].
    Lane lanes[2];
    int n_lanes = 1;
    uint64_t submit_count = 0;
    // ordering between the synchronous calls (lane 0 workspace on the CALLER's stream) and asynchronous batches
    // on lane 0's own stream, so that mixing the two forms on one handle never races on the workspace
    hipEvent_t lane0_async_done = nullptr, sync_done = nullptr;
    bool lane0_async_used = false, sync_used = false;
    // DINOv3 ConvNeXt (cfg.family == 1): weights, repacked at create into one device arena (precision 4: the GEMM weights
    // once more in the split format, at the same offsets in w32); the workspace is x (residual stream, row stride Cp),
    // h16 (every GEMM's A operand) and u16 (GELU(pointwise_conv1)), all fp32
    struct CnxBlock { const float *dw_t, *dw_b, *ln_w, *ln_b, *pw1_w, *pw1_b, *pw2_w, *pw2_b, *gamma; float sc1 = 1.f, sc2 = 1.f; };
    struct CnxStage {
        int C = 0, Cp = 0;                                         // width, width rounded up to the GEMM's 128-column tile
        const float *ds_ln_w = nullptr, *ds_ln_b = nullptr, *ds_w = nullptr, *ds_b = nullptr;   // stage 0: the stem
        float sc_ds = 1.f;
        std::vector<CnxBlock> blocks;
    };
    CnxStage cnx[4];
    const float *cnx_norm_w = nullptr, *cnx_norm_b = nullptr;
    float* cnx_arena = nullptr;
    int64_t cnx_x_cap = 0, cnx_a_cap = 0, cnx_u_cap = 0;      // floats per lane
    int cnx_tap = -1;                  // debug build: the point the last tapped ConvNeXt pass stopped at
    int cnx_tap_rows = 0;
    // optional per-kernel-category timing (HIP events on the launch stream)
    bool prof_on = false;
    struct ProfRec { hipEvent_t a, b; int cat; double flops; };
    std::vector<ProfRec> prof;
    size_t prof_used = 0;
};

namespace {

int64_t cnx_weights_count(const cbas_enc_config& c) {
    int64_t n = 0, prev = 0;
    for (int i = 0; i < 4; ++i) {
        const int64_t C = c.stage_widths[i];
        n += i == 0 ? C * 3 * 16 + C + 2 * C : 2 * prev + C * prev * 4 + C;
        n += (int64_t)c.stage_depths[i] * (49 * C + C + 2 * C + (4 * C * C + 4 * C) + (4 * C * C + C) + C);
        prev = C;
    }
    return n + 2 * prev;
}

int64_t weights_count(const cbas_enc_config& c, int mlp = CBAS_MLP_GELU) {
    if (c.family == 1) return cnx_weights_count(c);
    const int64_t D = c.hidden_size, F = c.intermediate_size, R = c.num_register_tokens, p = c.patch_size;
    const int64_t G = c.pos_embed_grid;
    int64_t n = D + R * D + (G > 0 ? (1 + G * G) * D : 0) + D * 3 * p * p + D;
    const int64_t per = 2 * D + (D * D + D) + (D * D + D) + (D * D + D) + (D * D + D) + D + 2 * D + (F * D + F) + (D * F + D) + D;
    n += (per + (mlp == CBAS_MLP_SWIGLU ? F * D + F : 0)) * c.num_layers;      // gated: + gate_proj weight and bias
    n += 2 * D;
    return n;
}

// Keys cubic kernel, a = -0.5: the coefficient ATen's ANTIALIASED bicubic uses (UpSampleKernel.cpp aa_filter)
static inline double cubic_aa(double x) {
    const double a = -0.5;
    x = fabs(x);
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
}

// (out, in) weights of F.interpolate(mode="bicubic", align_corners=False, antialias=True) along one axis
static std::vector<float> aa_bicubic_matrix(int in_size, int out_size) {
    std::vector<float> W((size_t)out_size * in_size, 0.f);
    const double scale = (double)in_size / out_size;
    const double support = scale >= 1.0 ? 2.0 * scale : 2.0, invscale = scale >= 1.0 ? 1.0 / scale : 1.0;
    for (int i = 0; i < out_size; ++i) {
        const double center = scale * (i + 0.5);
        int xmin = (int)(center - support + 0.5); if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5); if (xmax > in_size) xmax = in_size;
        double tot = 0.0;
        for (int j = xmin; j < xmax; ++j) tot += cubic_aa((j - center + 0.5) * invscale);
        for (int j = xmin; j < xmax; ++j) W[(size_t)i * in_size + j] = (float)(cubic_aa((j - center + 0.5) * invscale) / tot);
    }
    return W;
}

// Find or create the table set of an nh x nw patch grid and point the handle at it.
int acquire_pos_table(cbas_enc* h, int nh, int nw, cbas_enc::PosTable** out) {
    const int P = nh * nw;
    if (P > h->rope_cap) return cbas_fail(CBAS_EINVAL, "frame has %d patches, workspace holds %d", P, h->rope_cap);
    *out = nullptr;
    for (auto& t : h->pos_tables)
        if (t.nh == nh && t.nw == nw) { t.last_use = ++h->pos_clock; *out = &t; return CBAS_OK; }
    cbas_enc::PosTable* t = nullptr;
    if ((int)h->pos_tables.size() < cbas_enc::POS_TABLES_MAX) {
        h->pos_tables.emplace_back();
        t = &h->pos_tables.back();
        const size_t Pmax = (size_t)h->rope_cap;
        if (h->cfg.use_rope) {
            HIP_TRY(hipMalloc(&t->cos, Pmax * 64 * sizeof(float)));
            HIP_TRY(hipMalloc(&t->sin, Pmax * 64 * sizeof(float)));
            HIP_TRY(hipMalloc(&t->fac, (Pmax + 1) * 32 * sizeof(float)));     // nh + nw <= nh * nw + 1
        } else {
            HIP_TRY(hipMalloc(&t->pos, Pmax * h->D * sizeof(float)));
        }
    } else {                                   // recycle the least recently used set: its readers must have finished
        t = &h->pos_tables[0];
        for (auto& c : h->pos_tables) if (c.last_use < t->last_use) t = &c;
        HIP_TRY(hipDeviceSynchronize());
    }
    t->nh = -1; t->nw = -1;                    // not valid until filled
    t->last_use = ++h->pos_clock;
    *out = t;
    return 1;                                  // caller fills it
}

// ATen's cubic convolution coefficients, a = -0.75, in float like ATen (UpSample.h cubic_convolution1 / cubic_convolution2,
// get_cubic_upsample_coefficients).  The outer polynomial and the source index below are written with fmaf: ATen's x86 builds
// contract them, and the outer taps (a few 1e-4 after cancellation) then agree with torch's to 1.2e-7 instead of 7e-7.
static inline float cubic_conv1(float x, float A) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
static inline float cubic_conv2(float x, float A) { return fmaf(fmaf(fmaf(A, x, -5.f * A), x, 8.f * A), x, -4.f * A); }

// (out, in) weights of F.interpolate(size=, mode="bicubic", align_corners=False) - NO antialiasing - along one axis: ATen's
// upsample_bicubic2d (UpSampleKernel.cpp HelperInterpCubic::compute_indices_weights).  The scale comes from the sizes
// (HF passes size=), the source index (dst + 0.5) * in / out - 0.5 is not clamped, its four taps floor - 1 ... floor + 2 are
// clamped to [0, in - 1]; taps that clamp onto one index add up in the matrix.
static std::vector<float> bicubic_matrix(int in_size, int out_size) {
    std::vector<float> W((size_t)out_size * in_size, 0.f);
    const float scale = (float)in_size / (float)out_size, A = -0.75f;
    for (int i = 0; i < out_size; ++i) {
        const float real = fmaf(scale, (float)i + 0.5f, -0.5f);
        int idx = (int)floorf(real); if (idx > in_size - 1) idx = in_size - 1;
        float t = real - (float)idx; t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
        const float co[4] = {cubic_conv2(t + 1.f, A), cubic_conv1(t, A), cubic_conv1(1.f - t, A), cubic_conv2((1.f - t) + 1.f, A)};
        for (int k = 0; k < 4; ++k) {
            int j = idx - 1 + k; j = j < 0 ? 0 : (j > in_size - 1 ? in_size - 1 : j);
            W[(size_t)i * in_size + j] += co[k];
        }
    }
    return W;
}

}  // namespace

// DINOv2: the (nh*nw, D) position embedding of the patch tokens from the stored (G*G, D) one.  mode picks the filter:
// CBAS_POS_INTERP_BICUBIC_AA [v2] interpolate_pos_encoding :93-145 (with registers), CBAS_POS_INTERP_BICUBIC HF
// modeling_dinov2.py:57-95 (plain DINOv2).  Both skip the resampling at the stored grid (the stored table, bit for bit).
void cbas_build_pos_table(int mode, const float* src, int G, int D, int nh, int nw, float* out) {
    const size_t n_out = (size_t)nh * nw * D;
    if (nh == G && nw == G) {
        memcpy(out, src, n_out * 4);
        return;
    }
    const bool aa = mode == CBAS_POS_INTERP_BICUBIC_AA;
    const std::vector<float> Wh = aa ? aa_bicubic_matrix(G, nh) : bicubic_matrix(G, nh);
    const std::vector<float> Ww = aa ? aa_bicubic_matrix(G, nw) : bicubic_matrix(G, nw);
    std::vector<float> tmp((size_t)G * nw * D, 0.f);     // width pass, then height pass (separable)
    for (int i = 0; i < G; ++i)
        for (int x = 0; x < nw; ++x) {
            float* tp = &tmp[((size_t)i * nw + x) * D];
            for (int j = 0; j < G; ++j) {
                const float w = Ww[(size_t)x * G + j];
                if (w == 0.f) continue;
                const float* sp = src + ((size_t)i * G + j) * D;
                for (int d = 0; d < D; ++d) tp[d] += w * sp[d];
            }
        }
    std::fill(out, out + n_out, 0.f);
    for (int y = 0; y < nh; ++y)
        for (int i = 0; i < G; ++i) {
            const float w = Wh[(size_t)y * G + i];
            if (w == 0.f) continue;
            for (int x = 0; x < nw; ++x) {
                float* o = &out[((size_t)y * nw + x) * D];
                const float* tp = &tmp[((size_t)i * nw + x) * D];
                for (int d = 0; d < D; ++d) o[d] += w * tp[d];
            }
        }
}

// one axis' (out_size, in_size) weight matrix of either filter (the debug build's cbas_debug_pos_interp_matrix)
void cbas_pos_interp_matrix(int mode, int in_size, int out_size, float* W) {
    const std::vector<float> m = mode == CBAS_POS_INTERP_BICUBIC_AA ? aa_bicubic_matrix(in_size, out_size) : bicubic_matrix(in_size, out_size);
    memcpy(W, m.data(), m.size() * 4);
}

namespace {

// DINOv2: position embedding of the patch tokens for an nh x nw grid
int ensure_pos_embed(cbas_enc* h, int nh, int nw) {
    cbas_enc::PosTable* t = nullptr;
    const int rc = acquire_pos_table(h, nh, nw, &t);
    if (rc < 0) return rc;
    h->pos_tab = t->pos;
    if (rc == 0) return CBAS_OK;
    const int P = nh * nw, G = h->cfg.pos_embed_grid, D = h->D;
    std::vector<float> out((size_t)P * D);
    cbas_build_pos_table(h->pos_interp, h->pos_host.data() + D /* skip the cls position */, G, D, nh, nw, out.data());
    HIP_TRY(hipMemcpy(t->pos, out.data(), out.size() * 4, hipMemcpyHostToDevice));   // blocking; nothing reads t yet
    t->nh = nh; t->nw = nw;
    return CBAS_OK;
}

int ensure_rope(cbas_enc* h, int nh, int nw) {
    if (!h->cfg.use_rope) return ensure_pos_embed(h, nh, nw);
    cbas_enc::PosTable* t = nullptr;
    const int rc = acquire_pos_table(h, nh, nw, &t);
    if (rc < 0) return rc;
    h->rope_cos = t->cos; h->rope_sin = t->sin; h->rope_fac = t->fac; h->rope_nh = nh; h->rope_nw = nw;
    if (rc == 0) return CBAS_OK;
    const int P = nh * nw;
    // [tf]:96-121 patch-centre coordinates, :153-200 angles; float32 throughout like the reference
    std::vector<float> c((size_t)P * 64), s((size_t)P * 64);
    float inv_freq[16];
    for (int j = 0; j < 16; ++j) inv_freq[j] = 1.0f / powf(h->cfg.rope_theta, (float)j * (4.0f / 64.0f));
    const float two_pi = 6.283185307179586f;
    for (int iy = 0; iy < nh; ++iy)
        for (int ix = 0; ix < nw; ++ix) {
            const float cy = 2.0f * (((float)iy + 0.5f) / (float)nh) - 1.0f;
            const float cx = 2.0f * (((float)ix + 0.5f) / (float)nw) - 1.0f;
            float* cr = &c[(size_t)(iy * nw + ix) * 64];
            float* sr = &s[(size_t)(iy * nw + ix) * 64];
            for (int d = 0; d < 32; ++d) {
                const float coord = d < 16 ? cy : cx;
                const float ang = (two_pi * coord) * inv_freq[d & 15];
                cr[d] = cr[d + 32] = cosf(ang);
                sr[d] = sr[d + 32] = sinf(ang);
            }
        }
    HIP_TRY(hipMemcpy(t->cos, c.data(), c.size() * 4, hipMemcpyHostToDevice));       // blocking; nothing reads t yet
    HIP_TRY(hipMemcpy(t->sin, s.data(), s.size() * 4, hipMemcpyHostToDevice));
    // the same numbers by axis: columns 0-15 of patch (iy, ix) are those of any patch in row iy, 16-31 of column ix
    std::vector<float> fac((size_t)(nh + nw) * 32);
    for (int iy = 0; iy < nh; ++iy)
        for (int d = 0; d < 16; ++d) {
            fac[(size_t)iy * 32 + d] = c[(size_t)(iy * nw) * 64 + d];
            fac[(size_t)iy * 32 + 16 + d] = s[(size_t)(iy * nw) * 64 + d];
        }
    for (int ix = 0; ix < nw; ++ix)
        for (int d = 0; d < 16; ++d) {
            fac[(size_t)(nh + ix) * 32 + d] = c[(size_t)ix * 64 + 16 + d];
            fac[(size_t)(nh + ix) * 32 + 16 + d] = s[(size_t)ix * 64 + 16 + d];
        }
    HIP_TRY(hipMemcpy(t->fac, fac.data(), fac.size() * 4, hipMemcpyHostToDevice));
    t->nh = nh; t->nw = nw;
    return CBAS_OK;
}

// RoPE tables of the grid ensure_rope() selected, into a q|k|v GEMM's parameters (GemmParams or Gemm32VitParams)
template <typename Params>
void set_rope(const cbas_enc* h, Params& p) {
    if (!h->cfg.use_rope) return;
    p.rope_cos = h->rope_cos; p.rope_sin = h->rope_sin;
    p.rope_fac = h->rope_in_lds ? h->rope_fac : nullptr; p.rope_nh = h->rope_nh; p.rope_nw = h->rope_nw;
    p.rope_magic = (unsigned)((1ull << 32) / (unsigned)h->rope_nw) + 1u;
}

// ConvNeXt: floats of x, of the GEMM operand buffer and of the GELU buffer that n frames of height x width need
void cnx_sizes(const cbas_enc* h, int64_t n, int height, int width, int64_t* x, int64_t* a, int64_t* u) {
    int64_t hh = height / 4, ww = width / 4;
    *x = 0; *a = n * hh * ww * 32; *u = 0;
    for (int i = 0; i < 4; ++i) {
        const cbas_enc::CnxStage& S = h->cnx[i];
        if (i > 0) { hh /= 2; ww /= 2; *a = std::max(*a, n * hh * ww * 4 * h->cnx[i - 1].C); }
        const int64_t rows = n * hh * ww;
        *x = std::max(*x, rows * S.Cp);
        *a = std::max(*a, rows * S.C);
        *u = std::max(*u, rows * 4 * S.C);
    }
}

int check_frame(cbas_enc* h, int n, int height, int width) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null encoder handle");
    if (n <= 0 || n > h->cfg.max_batch) return cbas_fail(CBAS_EINVAL, "n=%d outside (0, max_batch=%d]", n, h->cfg.max_batch);
    if (h->cfg.family == 1) {
        if (height < 32 || width < 32) return cbas_fail(CBAS_EINVAL, "frame %dx%d: a ConvNeXt needs at least 32x32", height, width);
        int64_t x, a, u;
        cnx_sizes(h, n, height, width, &x, &a, &u);
        if (x > h->cnx_x_cap || a > h->cnx_a_cap || u > h->cnx_u_cap)
            return cbas_fail(CBAS_EINVAL, "%d frames of %dx%d exceed the workspace (max_batch=%d, %dx%d)", n, height, width,
                             h->cfg.max_batch, h->cfg.max_height, h->cfg.max_width);
        return CBAS_OK;
    }
    const int ps = h->cfg.patch_size;
    if (height < ps || width < ps) return cbas_fail(CBAS_EINVAL, "frame %dx%d smaller than one patch", height, width);
    const int64_t P = (int64_t)(height / ps) * (width / ps);
    if ((int64_t)n * (P + h->NP) > h->rows_cap || (int64_t)n * P > h->prow_cap)
        return cbas_fail(CBAS_EINVAL, "%d frames of %dx%d exceed the workspace (max_batch=%d, %dx%d)", n, height,
                         width, h->cfg.max_batch, h->cfg.max_height, h->cfg.max_width);
    return CBAS_OK;
}

// Bracket one launch with events when profiling is on (events are created lazily and reused).
struct ProfScope {
    cbas_enc* h; hipStream_t st; cbas_enc::ProfRec* r = nullptr;
    ProfScope(cbas_enc* h_, hipStream_t st_, int cat, double flops) : h(h_), st(st_) {
        if (!h->prof_on) return;
        if (h->prof_used == h->prof.size()) {
            cbas_enc::ProfRec n{};
            if (hipEventCreate(&n.a) != hipSuccess || hipEventCreate(&n.b) != hipSuccess) return;
            h->prof.push_back(n);
        }
        r = &h->prof[h->prof_used++];
        r->cat = cat; r->flops = flops;
        (void)hipEventRecord(r->a, st);
    }
    ~ProfScope() { if (r) (void)hipEventRecord(r->b, st); }
};
#define PROF(cat, flops) ProfScope _prof_scope_##cat(h, st, cat, flops)


// The ViT forward: the patch GEMM, then per layer ([tf]:404-445)
//     LayerNorm 1 -> q|k|v -> attention -> o_proj -> LayerNorm 2 -> up -> down
// (debug taps stop after stage 1..7 of a layer, in that order; layer 0, stage 0: after the patch GEMM), then the final norm of the
// CLS rows.  Written once per operand family: run_blocks on GemmParams / launch_gemm (precisions 0, 1, 2), run_blocks_f32 on
// Gemm32VitParams / launch_gemm_f32_vit (precisions 3, 4); in each, the row-wise part from o_proj on is vit_tail* on a RowView.
// The last layer feeds only the final norm of the CLS rows, so it is pruned unless a debug tap runs: K and V are still projected
// for every row (the CLS query attends to all tokens); the query, attention and the row-wise part run on the n CLS rows, read
// and written in place in the residual stream with a row stride of T*D (rows are independent: bit-identical CLS).
struct VitShape {
    int ps, nh, nw, P, T;      // patch size, patch grid, patches and tokens per frame
    int M, M_pad;              // token rows of the batch; rounded up to the GEMMs' 128-row tile
    int D, F, NU;              // NU = columns of the up GEMM: gate | up interleaved for a gated MLP
    GemmEpilogue EU;           // the up GEMM's epilogue
    bool prune;                // the last layer runs pruned
};

// the shape of this forward, and the position tables of its patch grid selected
int vit_begin(cbas_enc* h, int n, int height, int width, bool want_cls, int stop_layer, VitShape& s) {
    s.ps = h->cfg.patch_size; s.nh = height / s.ps; s.nw = width / s.ps; s.P = s.nh * s.nw; s.T = s.P + h->NP;
    s.M = n * s.T; s.M_pad = (int)round_up(s.M, 128);
    s.D = h->D; s.F = h->F; s.NU = h->mlp ? 2 * s.F : s.F;
    s.EU = h->mlp ? EPI_SWIGLU : EPI_GELU;
    s.prune = h->prune_last && stop_layer < 0 && want_cls;
    h->last_rows = s.M;
    return ensure_rope(h, s.nh, s.nw);
}

// The rows the row-wise part of a layer works on, E = f16 or float by family: every token row, or the CLS rows of the pruned last
// layer.  The CLS rows' operands are fp16 (+ lo halves) / fp32 (split) whatever the handle's mode: never MX-fp8, never folded.
template <typename E>
struct RowView {
    int M, M_pad;
    int64_t ldx;               // row stride of these rows in the residual stream
    E *ln, *ctx, *u;           // LayerNorm output, attention context, MLP activation (GELU(up) / silu(gate) * up)
    E* q;                      // CLS rows: their queries (bias added, scaled by 1/8; no RoPE on prefix rows); nullptr: every row
};

// Optional extra outputs of a forward (cbas_enc_forward_*_attn): the last layer's CLS attention, per head (n, NH, T) and / or
// averaged over the heads on the patch tokens (n, P).  Both null: none, the forward queues exactly what it queues without them.
struct AttnOut {
    float *heads = nullptr, *map = nullptr;
    explicit operator bool() const { return heads || map; }
};

// Per-layer outputs of a forward (cbas_enc_forward_*_layers), filled from the buffers the block loop holds at the right moments:
// the residual stream of every token after the patch GEMM (index 0) and after block l (index l), the CLS attention of any layer
// and the attention rollout chain.  Null: the forward queues exactly what it queues without them.
struct LayersOut {
    const int32_t* hs_layers = nullptr;   // host: n_hs indices 0 .. L
    int n_hs = 0, hs_norm = 0;
    float* hs_f32 = nullptr;
    f16* hs_f16 = nullptr;
    int64_t hs_ld = 0, hs_stride = 0;     // elements: row stride, distance between two listed layers' images
    const int32_t* at_layers = nullptr;   // host: n_at layer numbers 1 .. L
    int n_at = 0;
    float *at_heads = nullptr, *at_map = nullptr;      // (n_at, n, NH, T) / (n_at, n, P)
    float* roll = nullptr;                // (n, P)
    int roll_start = 1;                   // 1 .. L
    const int32_t* roll_query = nullptr;  // device: per-frame token index; NULL: row 0
    float* scratch = nullptr;             // 3 n T T floats: A^ of the current layer and the two products that alternate
};

// index 0: after the patch GEMM; index l: after block l
int layers_hidden(cbas_enc* h, const Lane& ws, const VitShape& s, const LayersOut* lo, int index, hipStream_t st) {
    if (!lo) return CBAS_OK;
    for (int j = 0; j < lo->n_hs; ++j) {
        if (lo->hs_layers[j] != index) continue;
        float* const o32 = lo->hs_f32 ? lo->hs_f32 + j * lo->hs_stride : nullptr;
        f16* const o16 = lo->hs_f16 ? lo->hs_f16 + j * lo->hs_stride : nullptr;
        PROF(CBAS_PROF_OTHER, 0.0);
        if (lo->hs_norm)
            LAUNCH_TRY(launch_final_norm_rows(ws.x, s.D, h->norm_w, h->norm_b, o32, o16, lo->hs_ld, s.M, s.D, h->cfg.layer_norm_eps, h->nonfinite_dev, st));
        else
            LAUNCH_TRY(launch_copy_rows(ws.x, s.D, o32, o16, lo->hs_ld, s.M, s.D, h->nonfinite_dev, st));
    }
    return CBAS_OK;
}

// after layer l's (0-based) attention launch, while q | k | v of every token is still in qkv
template <typename E>
int layers_attention(cbas_enc* h, const VitShape& s, const LayersOut* lo, int l, const E* qkv, int split, int n, hipStream_t st) {
    if (!lo) return CBAS_OK;
    const int T = s.T, D = s.D, NH = h->NH, NP = h->NP, layer = l + 1;
    for (int j = 0; j < lo->n_at; ++j) {
        if (lo->at_layers[j] != layer) continue;
        PROF(CBAS_PROF_OTHER, 2.0 * n * (double)T * D);
        LAUNCH_TRY(launch_cls_attention<E>(qkv, (int64_t)T * 3 * D, qkv + D, 3 * D, n, T, NH, NP, split,
                                           lo->at_heads ? lo->at_heads + (int64_t)j * n * NH * T : nullptr,
                                           lo->at_map ? lo->at_map + (int64_t)j * n * s.P : nullptr, st));
    }
    if (lo->roll && layer >= lo->roll_start) {
        const int64_t sz = (int64_t)n * T * T;
        const int k = layer - lo->roll_start;            // products so far: R lives in buffer 1 + (k & 1) ... see below
        float* const A = lo->scratch;
        float* const R0 = lo->scratch + sz;
        float* const R1 = lo->scratch + 2 * sz;
        // layer roll_start writes A^ straight into R0; step k >= 1 reads R[(k - 1) & 1] and writes R[k & 1]
        float* const cur = k == 0 ? R0 : ((k & 1) ? R1 : R0);
        { PROF(CBAS_PROF_OTHER, 2.0 * n * (double)T * T * D);
          LAUNCH_TRY(launch_attention_mean<E>(qkv, 3 * D, qkv + D, 3 * D, n, T, NH, split, 1, k == 0 ? R0 : A, st)); }
        if (k > 0) {
            PROF(CBAS_PROF_OTHER, 2.0 * n * (double)T * T * T);
            LAUNCH_TRY(launch_rollout_step(A, (k & 1) ? R0 : R1, cur, n, T, st));
        }
        if (layer == h->L) LAUNCH_TRY(launch_rollout_row(cur, n, T, NP, lo->roll_query, lo->roll, st));
    }
    return CBAS_OK;
}

template <typename E>
RowView<E> cls_rows(const cbas_enc* h, const VitShape& s, const Lane& ws, int n) {
    const int64_t cap = round_up(h->cfg.max_batch, 128);
    E* const q = reinterpret_cast<E*>(ws.cls16);
    return {n, n, (int64_t)s.T * s.D, q + 2 * cap * s.D, q + cap * s.D, q + 3 * cap * s.D, q};
}

// ---- half family: fp16 operands, fp32 residual stream ----
// The operand format of each GEMM of a layer; all false = fp16.
struct HalfFormats {
    bool split;                                // precision 1: weights as fp16 hi + lo
    // precision 2: the GEMMs with MX-fp8 operands (cbas_enc_set_fp8_plan).  An activation is stored in the format of the GEMM
    // that consumes it: LayerNorm 1 -> q|k|v, attention context -> o_proj, LayerNorm 2 -> up, MLP activation -> down; fp8
    // activations live in the fp16 buffers' memory.
    bool f8_qkv, f8_proj, f8_up, f8_down;
    // LayerNorm fold.  LN(x) W^T + b = rstd (x (gamma o W)^T - mean colsum(gamma o W)) + (beta W^T + b): the two GEMMs that
    // consume a LayerNorm output (q|k|v, up) run on the raw fp16 residual stream with gamma folded into their weights and apply
    // mean / rstd in their epilogues; the two that produce the residual stream (o_proj, down) write that fp16 copy and the row
    // statistics in theirs, as launch_ln_stats_x16 does once for layer 0.  The fold lives in the ping-pong kernel only, so all
    // four GEMMs run there at EVERY batch size: a frame's CLS row must not depend on how many frames shared its batch.
    bool fold;
};

// ping-pong tile of a folded handle's GEMMs: 128-row tiles for small problems, as precision 2 does
int pp_tile(int M, int N) { return (long)((M + 255) / 256) * (N / 256) >= 120 ? GEMM_TILE_PP_AUTO : GEMM_TILE_PP_128x256; }

// A and W of a GEMM as MX-fp8 bytes + block scales, or as fp16 (+ the weight's lo half under precision 1)
void set_operands(const cbas_enc* h, GemmParams& g, bool f8, bool split, const f16* A, const uint32_t* A_sc, const f16* W,
                  const f16* W_lo, const uint8_t* W8, const uint32_t* W_sc) {
    if (f8) { g.A8 = reinterpret_cast<const uint8_t*>(A); g.A_sc = A_sc; g.sc_lda = (int)h->rows_cap; g.W8 = W8; g.W_sc = W_sc; }
    else { g.A = A; g.W = W; g.W_lo = split ? W_lo : nullptr; }
}

// LayerNorm fold: the operands and statistics of a consumer GEMM, the extra outputs of a producer GEMM
void fold_consumer(const cbas_enc* h, const Lane& ws, GemmParams& g, const f16* W_folded, const float* colsum) {
    g.A = ws.x16; g.W = W_folded;
    g.ln_in = ws.lnst; g.ln_colsum = colsum; g.ln_parts = h->D / 256; g.ln_ld = (int)h->rows_cap; g.ln_eps = h->cfg.layer_norm_eps;
}
void fold_producer(const cbas_enc* h, const Lane& ws, GemmParams& g) { g.x16_out = ws.x16; g.ln_out = ws.lnst; g.ln_ld = (int)h->rows_cap; }

// q|k|v of every token row, from section sec0 of the fused weight on: 0 = q | k | v, 1 = k | v (the pruned last layer)
int vit_qkv(cbas_enc* h, const Lane& ws, const LayerW& w, const VitShape& s, const HalfFormats& f, int sec0, hipStream_t st) {
    const int D = s.D, M = s.M, N = (3 - sec0) * D;
    const size_t w0 = (size_t)sec0 * D * D;
    GemmParams q{};
    if (f.fold) {
        fold_consumer(h, ws, q, w.wqkv_f + w0, w.qkv_cs + sec0 * D);
        q.tile = pp_tile(M, N);
    } else if (f.f8_qkv) {
        q.A8 = reinterpret_cast<const uint8_t*>(ws.h16); q.A_sc = ws.sc_h; q.sc_lda = (int)h->rows_cap;
        q.W8 = w.wqkv8 + w0; q.W_sc = w.sqkv + sec0 * D;
        if (sec0) q.sc_ldw = 3 * D;
    } else {
        q.A = ws.h16; q.W = w.wqkv + w0; q.W_lo = f.split ? w.wqkv_lo + w0 : nullptr;
    }
    q.M = M; q.M_pad = s.M_pad; q.N = N; q.K = D; q.bias = (f.fold ? w.qkv_bf : w.qkv_b) + sec0 * D;
    q.out_f16 = ws.qkv16 + sec0 * D; q.ldo = 3 * D;
    q.tokens_per_frame = s.T; q.n_prefix = h->NP; q.D = D; q.sec0 = sec0;
    set_rope(h, q);
    PROF(CBAS_PROF_QKV, 2.0 * M * (3.0 - sec0) * D * D);
    LAUNCH_TRY(launch_gemm(f.fold ? EPI_QKV_LN : EPI_QKV, q, st));
    return CBAS_OK;
}

// o_proj -> LayerNorm 2 -> up -> down on the rows of v; returns after stage `stop` (4..7) when a debug tap asks for one.
// more = a layer follows this one.
int vit_tail(cbas_enc* h, const Lane& ws, const LayerW& w, const VitShape& s, const HalfFormats& all, const RowView<f16>& v,
             bool more, int stop, hipStream_t st) {
    const HalfFormats f = v.q ? HalfFormats{all.split} : all;
    const int D = s.D, F = s.F, NU = s.NU, M = v.M, sc_ld = (int)h->rows_cap;
    const float eps = h->cfg.layer_norm_eps;
    GemmParams o{};
    set_operands(h, o, f.f8_proj, f.split, v.ctx, ws.sc_h, w.wo, w.wo_lo, w.wo8, w.so);
    o.M = M; o.M_pad = v.M_pad; o.N = D; o.K = D; o.bias = w.o_b; o.lambda = w.ls1; o.out_f32 = ws.x; o.ldo = (int)v.ldx;
    if (f.fold) { o.tile = pp_tile(M, D); fold_producer(h, ws, o); }
    { PROF(CBAS_PROF_OPROJ, 2.0 * M * (double)D * D); LAUNCH_TRY(launch_gemm(f.fold ? EPI_RESID_LN : EPI_RESID, o, st)); }
    if (stop == 4) return CBAS_OK;

    if (f.f8_up) { PROF(CBAS_PROF_LAYERNORM, 0.0); LAUNCH_TRY(launch_layernorm_f8(ws.x, v.ldx, w.ln2_w, w.ln2_b, reinterpret_cast<uint8_t*>(v.ln), ws.sc_h, sc_ld, M, D, eps, st)); }
    else if (!f.fold) { PROF(CBAS_PROF_LAYERNORM, 0.0); LAUNCH_TRY(launch_layernorm_f16(ws.x, v.ldx, w.ln2_w, w.ln2_b, v.ln, M, D, eps, st)); }
    if (stop == 5) return CBAS_OK;

    GemmParams u{};                         // operands in the format of `up`, the result in the format `down` consumes
    if (f.fold) { fold_consumer(h, ws, u, w.wup_f, w.up_cs); u.tile = pp_tile(M, NU); }
    else set_operands(h, u, f.f8_up, f.split, v.ln, ws.sc_h, w.wup, w.wup_lo, w.wup8, w.sup);
    if (f.f8_down) { u.out_f8 = reinterpret_cast<uint8_t*>(v.u); u.out_sc = ws.sc_u; u.sc_ldo = sc_ld; }
    else u.out_f16 = v.u;
    u.M = M; u.M_pad = v.M_pad; u.N = NU; u.K = D; u.bias = f.fold ? w.up_bf : w.up_b; u.ldo = F;
    const GemmEpilogue eu = f.fold ? EPI_GELU_LN : f.f8_down && s.EU == EPI_GELU ? EPI_GELU_F8 : s.EU;
    { PROF(CBAS_PROF_UP, 2.0 * M * (double)NU * D); LAUNCH_TRY(launch_gemm(eu, u, st)); }
    if (stop == 6) return CBAS_OK;

    GemmParams d{};
    set_operands(h, d, f.f8_down, f.split, v.u, ws.sc_u, w.wdown, w.wdown_lo, w.wdown8, w.sdown);
    d.M = M; d.M_pad = v.M_pad; d.N = D; d.K = F; d.bias = w.down_b; d.lambda = w.ls2; d.out_f32 = ws.x; d.ldo = (int)v.ldx;
    const bool stats = f.fold && more;      // the last layer's down_proj feeds the final norm only
    if (f.fold) { d.tile = pp_tile(M, D); if (stats) fold_producer(h, ws, d); }
    { PROF(CBAS_PROF_DOWN, 2.0 * M * (double)F * D); LAUNCH_TRY(launch_gemm(stats ? EPI_RESID_LN : EPI_RESID, d, st)); }
    return CBAS_OK;
}

// ---- fp32 family (vit_f32.hip): every buffer and every contraction in fp32; the workspace pointers (A_patch, h16, qkv16, u16,
// cls16) are allocated at 4 bytes per element and hold floats.  Precision 4: every GEMM's products on the fp16 pipe as
// three-term splits of scaled operands: LayerNorm rows and pixels as they are, weights by their per-tensor power of two, the
// attention context and the MLP activation by these (typical magnitudes ~0.05 / ~0.3: keeps their low halves out of fp16's
// subnormal range) ----
constexpr float P4_CTX_SCALE = 16.f, P4_ACT_SCALE = 4.f;

void set_split(const cbas_enc* h, Gemm32VitParams& g, float a_scale, float w_scale) { g.split = h->cfg.precision == 4; g.a_scale = a_scale; g.w_scale = w_scale; }

// o_proj -> LayerNorm 2 -> up -> down on the rows of v (see vit_tail)
int vit_tail_f32(cbas_enc* h, const Lane& ws, const LayerW& w, const VitShape& s, const RowView<float>& v, int stop, hipStream_t st) {
    const int D = s.D, F = s.F, NU = s.NU, M = v.M;
    Gemm32VitParams o{};
    set_split(h, o, P4_CTX_SCALE, w.sc_o);
    o.A = v.ctx; o.lda = D; o.W = w.wo32; o.M = M; o.N = D; o.K = D; o.bias = w.o_b; o.lambda = w.ls1; o.out = ws.x; o.ldo = v.ldx;
    { PROF(CBAS_PROF_OPROJ, 2.0 * M * (double)D * D); LAUNCH_TRY(launch_gemm_f32_vit(EPI_RESID, o, st)); }
    if (stop == 4) return CBAS_OK;

    { PROF(CBAS_PROF_LAYERNORM, 0.0);
      LAUNCH_TRY(launch_layernorm_f32(ws.x, v.ldx, w.ln2_w, w.ln2_b, v.ln, M, D, h->cfg.layer_norm_eps, h->cfg.precision == 4, st)); }
    if (stop == 5) return CBAS_OK;

    Gemm32VitParams u{};
    set_split(h, u, 1.f, w.sc_up);
    u.out_scale = P4_ACT_SCALE;
    u.A = v.ln; u.lda = D; u.W = w.wup32; u.M = M; u.N = NU; u.K = D; u.bias = w.up_b; u.out = v.u; u.ldo = F;
    { PROF(CBAS_PROF_UP, 2.0 * M * (double)NU * D); LAUNCH_TRY(launch_gemm_f32_vit(s.EU, u, st)); }
    if (stop == 6) return CBAS_OK;

    Gemm32VitParams d{};
    set_split(h, d, P4_ACT_SCALE, w.sc_down);
    d.A = v.u; d.lda = F; d.W = w.wdown32; d.M = M; d.N = D; d.K = F; d.bias = w.down_b; d.lambda = w.ls2; d.out = ws.x; d.ldo = v.ldx;
    { PROF(CBAS_PROF_DOWN, 2.0 * M * (double)F * D); LAUNCH_TRY(launch_gemm_f32_vit(EPI_RESID, d, st)); }
    return CBAS_OK;
}

int run_blocks_f32(cbas_enc* h, const Lane& ws, int n, int height, int width, float* cls_f32, f16* cls_f16, hipStream_t st,
                   int stop_layer, int stop_stage, const AttnOut& attn = AttnOut{}, const LayersOut* lo = nullptr) {
    VitShape s{};
    int rc = vit_begin(h, n, height, width, cls_f32 || cls_f16, stop_layer, s);
    if (rc) return rc;
    const int D = s.D, T = s.T, M = s.M;
    float* const h32 = reinterpret_cast<float*>(ws.h16);
    float* const qkv32 = reinterpret_cast<float*>(ws.qkv16);
    const float eps = h->cfg.layer_norm_eps;
    const int split = h->cfg.precision == 4;

    Gemm32VitParams g{};
    set_split(h, g, 1.f, h->sc_patch);
    g.A = reinterpret_cast<float*>(ws.A_patch); g.lda = 256; g.W = h->wpatch32; g.M = n * s.P; g.N = D; g.K = 256;
    g.bias = h->patch_b; g.out = ws.x; g.ldo = D;
    g.patches_per_frame = s.P; g.tokens_per_frame = T; g.n_prefix = h->NP; g.pos = h->cfg.use_rope ? nullptr : h->pos_tab;
    { PROF(CBAS_PROF_PATCH, 2.0 * g.M * g.N * g.K); LAUNCH_TRY(launch_gemm_f32_vit(EPI_PATCH, g, st)); }
    if (stop_layer == 0 && stop_stage == 0) return CBAS_OK;
    if ((rc = layers_hidden(h, ws, s, lo, 0, st))) return rc;

    const RowView<float> all{M, s.M_pad, D, h32, h32, reinterpret_cast<float*>(ws.u16), nullptr}, cls = cls_rows<float>(h, s, ws, n);
    for (int l = 0; l < h->L; ++l) {
        const LayerW& w = h->layers[l];
        const int stop = stop_layer == l ? stop_stage : -1;
        const bool cls_only = s.prune && l == h->L - 1;
        const RowView<float>& v = cls_only ? cls : all;
        { PROF(CBAS_PROF_LAYERNORM, 0.0); LAUNCH_TRY(launch_layernorm_f32(ws.x, D, w.ln1_w, w.ln1_b, h32, M, D, eps, split, st)); }
        if (stop == 1) return CBAS_OK;

        const int sec0 = cls_only ? 1 : 0;  // q|k|v of every token row from this section of the packed weight on (see vit_qkv)
        Gemm32VitParams qkv{};
        set_split(h, qkv, 1.f, w.sc_qkv);
        qkv.A = h32; qkv.lda = D; qkv.W = w.wqkv32 + (size_t)sec0 * D * D; qkv.M = M; qkv.N = (3 - sec0) * D; qkv.K = D;
        qkv.bias = w.qkv_b + sec0 * D; qkv.out = qkv32 + sec0 * D; qkv.ldo = 3 * D;
        qkv.tokens_per_frame = T; qkv.n_prefix = h->NP; qkv.D = D; qkv.sec0 = sec0;
        set_rope(h, qkv);
        { PROF(CBAS_PROF_QKV, 2.0 * M * (3.0 - sec0) * D * D); LAUNCH_TRY(launch_gemm_f32_vit(EPI_QKV, qkv, st)); }
        if (stop == 2) return CBAS_OK;

        if (cls_only) {
            Gemm32VitParams q{};            // q section, CLS rows only (row b*T of h32)
            set_split(h, q, 1.f, w.sc_qkv);
            q.A = h32; q.lda = (int64_t)T * D; q.W = w.wqkv32; q.M = n; q.N = D; q.K = D; q.bias = w.qkv_b; q.out = cls.q; q.ldo = D;
            q.tokens_per_frame = 1; q.n_prefix = 1; q.D = D; q.sec0 = 0;      // every row is token 0: no RoPE
            set_rope(h, q);
            { PROF(CBAS_PROF_QKV, 2.0 * n * (double)D * D); LAUNCH_TRY(launch_gemm_f32_vit(EPI_QKV, q, st)); }
        }
        { PROF(CBAS_PROF_ATTENTION, 4.0 * n * (double)T * (cls_only ? 1 : T) * D);      // the view's queries against every key
          LAUNCH_TRY(launch_attention_f32(qkv32, v.q, v.ctx, n, T, D, h->NH, split ? P4_CTX_SCALE : 0.f, st)); }
        if (attn && l == h->L - 1) {        // the CLS queries and K are still live: compact rows, or row b*T of q|k|v when nothing is pruned
            PROF(CBAS_PROF_OTHER, 2.0 * n * (double)T * D);
            LAUNCH_TRY(launch_cls_attention<float>(cls_only ? cls.q : qkv32, cls_only ? D : (int64_t)T * 3 * D, qkv32 + D, 3 * D, n, T,
                                                   h->NH, h->NP, split, attn.heads, attn.map, st));
        }
        if (!cls_only && (rc = layers_attention<float>(h, s, lo, l, qkv32, split, n, st))) return rc;
        if (stop == 3) return CBAS_OK;

        rc = vit_tail_f32(h, ws, w, s, v, stop, st);
        if (rc || (stop >= 4 && stop <= 7)) return rc;
        if ((rc = layers_hidden(h, ws, s, lo, l + 1, st))) return rc;
    }
    if (cls_f32 || cls_f16)
        LAUNCH_TRY(launch_final_norm_cls(ws.x, h->norm_w, h->norm_b, cls_f32, cls_f16, n, T, D, eps, st, h->nonfinite_dev));
    return CBAS_OK;
}

// Everything after ingest: patch GEMM, L transformer blocks, final CLS norm.
int run_blocks(cbas_enc* h, const Lane& ws, int n, int height, int width, int patch_k, float in_scale, float* cls_f32,
               f16* cls_f16, hipStream_t st, int stop_layer, int stop_stage, const AttnOut& attn = AttnOut{},
               const LayersOut* lo = nullptr) {
    if (h->cfg.precision >= 3) return run_blocks_f32(h, ws, n, height, width, cls_f32, cls_f16, st, stop_layer, stop_stage, attn, lo);
    VitShape s{};
    int rc = vit_begin(h, n, height, width, cls_f32 || cls_f16, stop_layer, s);
    if (rc) return rc;
    const int D = s.D, T = s.T, M = s.M;
    const float eps = h->cfg.layer_norm_eps;
    const int sc_ld = (int)h->rows_cap;

    GemmParams g{};
    g.A = ws.A_patch;
    g.W = patch_k == 256 ? h->wpatch : h->wpatch2;
    g.W_lo = h->cfg.precision == 1 ? (patch_k == 256 ? h->wpatch_lo : h->wpatch2_lo) : nullptr;
    g.M = n * s.P; g.M_pad = (int)round_up(n * s.P, 128); g.N = D; g.K = patch_k;
    g.bias = h->patch_b; g.out_f32 = ws.x; g.ldo = D;
    g.patches_per_frame = s.P; g.tokens_per_frame = T; g.n_prefix = h->NP; g.in_scale = in_scale;
    g.pos = h->cfg.use_rope ? nullptr : h->pos_tab;
    { PROF(CBAS_PROF_PATCH, 2.0 * g.M * g.N * g.K); LAUNCH_TRY(launch_gemm(EPI_PATCH, g, st)); }
    if (stop_layer == 0 && stop_stage == 0) return CBAS_OK;
    if ((rc = layers_hidden(h, ws, s, lo, 0, st))) return rc;

    const int plan = h->cfg.precision == 2 ? h->fp8_plan : 0;
    const HalfFormats f{h->cfg.precision == 1, bool(plan & CBAS_FP8_PLAN_QKV), bool(plan & CBAS_FP8_PLAN_PROJ), bool(plan & CBAS_FP8_PLAN_UP),
                        bool(plan & CBAS_FP8_PLAN_DOWN), h->ln_fold && h->fold_ok && stop_layer < 0 && !lo};      // debug taps and the per-layer outputs keep the LayerNorm kernels
    h->vit_forward_seen = true;
    if (f.fold) { PROF(CBAS_PROF_LAYERNORM, 0.0); LAUNCH_TRY(launch_ln_stats_x16(ws.x, ws.x16, ws.lnst, sc_ld, M, D, st)); }
    if (h->cfg.precision == 2 && stop_layer >= 0)
        return cbas_fail(CBAS_EINVAL, "debug taps read fp16 buffers; not available with precision 2");

    const RowView<f16> all{M, s.M_pad, D, ws.h16, ws.h16, ws.u16, nullptr}, cls = cls_rows<f16>(h, s, ws, n);
    for (int l = 0; l < h->L; ++l) {
        const LayerW& w = h->layers[l];
        const int stop = stop_layer == l ? stop_stage : -1;
        const bool cls_only = s.prune && l == h->L - 1;
        const RowView<f16>& v = cls_only ? cls : all;
        if (f.f8_qkv) { PROF(CBAS_PROF_LAYERNORM, 0.0); LAUNCH_TRY(launch_layernorm_f8(ws.x, D, w.ln1_w, w.ln1_b, reinterpret_cast<uint8_t*>(ws.h16), ws.sc_h, sc_ld, M, D, eps, st)); }
        else if (!f.fold) { PROF(CBAS_PROF_LAYERNORM, 0.0); LAUNCH_TRY(launch_layernorm_f16(ws.x, D, w.ln1_w, w.ln1_b, ws.h16, M, D, eps, st)); }
        if (stop == 1) return CBAS_OK;

        // the CLS query is an fp16 GEMM on the unfolded weight in every mode: where LayerNorm 1 of every row is MX-fp8 or folded
        // away, the n CLS rows get one of their own (in the view's LayerNorm 2 rows for now)
        const bool compact_q = cls_only && (f.f8_qkv || f.fold);
        if (compact_q) { PROF(CBAS_PROF_LAYERNORM, 0.0); LAUNCH_TRY(launch_layernorm_f16(ws.x, cls.ldx, w.ln1_w, w.ln1_b, cls.ln, n, D, eps, st)); }
        rc = vit_qkv(h, ws, w, s, f, cls_only ? 1 : 0, st);
        if (rc) return rc;
        if (stop == 2) return CBAS_OK;

        if (cls_only) {
            GemmParams q{};                 // q section, CLS rows only (row b*T of h16, or the compact rows)
            q.A = compact_q ? cls.ln : ws.h16; q.lda = compact_q ? D : T * D; q.W = w.wqkv; q.W_lo = f.split ? w.wqkv_lo : nullptr;
            q.M = n; q.M_pad = n; q.N = D; q.K = D; q.bias = w.qkv_b; q.out_f16 = cls.q; q.ldo = D;
            q.tokens_per_frame = 1; q.n_prefix = 1; q.D = D; q.sec0 = 0;      // every row is token 0: no RoPE
            { PROF(CBAS_PROF_QKV, 2.0 * n * (double)D * D); LAUNCH_TRY(launch_gemm(EPI_QKV, q, st)); }
        }
        { PROF(CBAS_PROF_ATTENTION, 4.0 * n * (double)T * (cls_only ? 1 : T) * D);      // the view's queries against every key
          LAUNCH_TRY(launch_attention(ws.qkv16, v.q, v.ctx, f.f8_proj && !cls_only ? ws.sc_h : nullptr, cls_only ? 0 : sc_ld, n, T, D, h->NH, st)); }
        if (attn && l == h->L - 1) {        // q and K are fp16 in every mode of this family (see run_blocks_f32 for the two query layouts)
            PROF(CBAS_PROF_OTHER, 2.0 * n * (double)T * D);
            LAUNCH_TRY(launch_cls_attention<f16>(cls_only ? cls.q : ws.qkv16, cls_only ? D : (int64_t)T * 3 * D, ws.qkv16 + D, 3 * D, n, T,
                                                 h->NH, h->NP, 0, attn.heads, attn.map, st));
        }
        if (!cls_only && (rc = layers_attention<f16>(h, s, lo, l, ws.qkv16, 0, n, st))) return rc;
        if (stop == 3) return CBAS_OK;

        rc = vit_tail(h, ws, w, s, f, v, l + 1 < h->L, stop, st);
        if (rc || (stop >= 4 && stop <= 7)) return rc;
        if ((rc = layers_hidden(h, ws, s, lo, l + 1, st))) return rc;
    }
    if (cls_f32 || cls_f16)
        LAUNCH_TRY(launch_final_norm_cls(ws.x, h->norm_w, h->norm_b, cls_f32, cls_f16, n, T, D, eps, st, h->nonfinite_dev));
    return CBAS_OK;
}

// DINOv3 ConvNeXt ([cx] = transformers models/dinov3_convnext/modeling_dinov3_convnext.py, DINOv3ConvNextModel.forward), after
// the stem's im2col has been written to h16: the whole network on the fp32 GEMMs of the ViT (precision 4: split operands) and
// the kernels of convnext_f32.hip.  stop >= 0 (debug taps): 0 ends after the stem's LayerNorm, 1 + i after stage i.
int run_cnx(cbas_enc* h, const Lane& ws, int n, int height, int width, float* cls_f32, f16* cls_f16, hipStream_t st, int stop) {
    const int split = h->cfg.precision == 4;
    const float eps = h->cfg.layer_norm_eps;
    float* const A32 = reinterpret_cast<float*>(ws.h16);
    float* const u32 = reinterpret_cast<float*>(ws.u16);
    auto gemm = [&](const float* A, int64_t lda, const float* W, int M, int N, int K, const float* bias,
                    float* out, int64_t ldo, float a_scale, float w_scale) {
        Gemm32VitParams g{};
        g.A = A; g.lda = lda; g.W = W; g.M = M; g.N = N; g.K = K; g.bias = bias; g.out = out; g.ldo = ldo;
        g.patches_per_frame = M; g.tokens_per_frame = M; g.n_prefix = 0;      // EPI_PATCH: output row m = A row m
        g.split = split; g.a_scale = a_scale; g.w_scale = w_scale;
        return g;
    };
    int hh = height / 4, ww = width / 4;
    int M = n * hh * ww;
    const cbas_enc::CnxStage& S0 = h->cnx[0];
    {
        Gemm32VitParams g = gemm(A32, 32, S0.ds_w, M, S0.Cp, 32, S0.ds_b, ws.x, S0.Cp, 1.f, S0.sc_ds);
        { PROF(CBAS_PROF_PATCH, 2.0 * M * S0.C * 48); LAUNCH_TRY(launch_gemm_f32_vit(EPI_PATCH, g, st)); }
        { PROF(CBAS_PROF_LAYERNORM, 0.0); LAUNCH_TRY(launch_cnx_ln_rows(ws.x, S0.Cp, S0.ds_ln_w, S0.ds_ln_b, M, S0.C, eps, st)); }
    }
    h->cnx_tap_rows = M;
    if (stop == 0) return CBAS_OK;
    for (int i = 0; i < 4; ++i) {
        const cbas_enc::CnxStage& S = h->cnx[i];
        const int C = S.C;
        if (i > 0) {
            const cbas_enc::CnxStage& P = h->cnx[i - 1];
            { PROF(CBAS_PROF_LAYERNORM, 0.0);
              LAUNCH_TRY(launch_cnx_downsample(ws.x, P.Cp, n, hh, ww, S.ds_ln_w, S.ds_ln_b, P.C, eps, A32, split, st)); }
            hh /= 2; ww /= 2;
            M = n * hh * ww;
            Gemm32VitParams g = gemm(A32, 4 * P.C, S.ds_w, M, S.Cp, 4 * P.C, S.ds_b, ws.x, S.Cp, 1.f, S.sc_ds);
            { PROF(CBAS_PROF_PATCH, 2.0 * M * C * 4.0 * P.C); LAUNCH_TRY(launch_gemm_f32_vit(EPI_PATCH, g, st)); }
        }
        for (const cbas_enc::CnxBlock& b : S.blocks) {
            { PROF(CBAS_PROF_LAYERNORM, 0.0);
              LAUNCH_TRY(launch_cnx_dwconv_ln(ws.x, S.Cp, n, hh, ww, b.dw_t, b.dw_b, b.ln_w, b.ln_b, C, eps, A32, split, st)); }
            Gemm32VitParams u = gemm(A32, C, b.pw1_w, M, 4 * C, C, b.pw1_b, u32, 4 * C, 1.f, b.sc1);
            u.out_scale = P4_ACT_SCALE;                               // the GELU output as pointwise_conv2's split A operand
            { PROF(CBAS_PROF_UP, 2.0 * M * 4.0 * C * C); LAUNCH_TRY(launch_gemm_f32_vit(EPI_GELU, u, st)); }
            Gemm32VitParams d = gemm(u32, 4 * C, b.pw2_w, M, S.Cp, 4 * C, b.pw2_b, ws.x, S.Cp, P4_ACT_SCALE, b.sc2);
            d.lambda = b.gamma;                                       // x += (pointwise_conv2 + b) * gamma
            { PROF(CBAS_PROF_DOWN, 2.0 * M * 4.0 * C * C); LAUNCH_TRY(launch_gemm_f32_vit(EPI_RESID, d, st)); }
        }
        h->cnx_tap_rows = M;
        if (stop == 1 + i) return CBAS_OK;
    }
    if (cls_f32 || cls_f16) {
        PROF(CBAS_PROF_LAYERNORM, 0.0);
        LAUNCH_TRY(launch_cnx_pool_ln(ws.x, h->cnx[3].Cp, n, hh * ww, h->cnx_norm_w, h->cnx_norm_b, h->cnx[3].C, eps, cls_f32,
                                      cls_f16, h->nonfinite_dev, st));
    }
    return CBAS_OK;
}

int forward_u8_one(cbas_enc* h, const Lane& ws, const uint8_t* frames_dev, int n, int height, int width, int64_t frame_stride,
                   int64_t row_stride, int64_t pixel_stride, float* cls_f32, f16* cls_f16, hipStream_t st,
                   int stop_layer, int stop_stage, const AttnOut& attn = AttnOut{}, const LayersOut* lo = nullptr) {
    if (h->cfg.family == 1) {
        LAUNCH_TRY(launch_cnx_stem_im2col_u8(frames_dev, n, height, width, frame_stride, row_stride, pixel_stride,
                                             reinterpret_cast<float*>(ws.h16), h->cfg.precision == 4, st));
        h->cnx_tap = stop_layer;
        return run_cnx(h, ws, n, height, width, cls_f32, cls_f16, st, stop_layer);
    }
    const int ps = h->cfg.patch_size;
    const int T = (height / ps) * (width / ps) + h->NP;
    if (h->cfg.precision >= 3)
        LAUNCH_TRY(launch_im2col_u8_f32(frames_dev, n, height, width, frame_stride, row_stride, pixel_stride,
                                        reinterpret_cast<float*>(ws.A_patch), ws.x, h->prefix, h->NP, h->D, T, ps,
                                        h->cfg.precision == 4, st));
    else
        LAUNCH_TRY(launch_im2col_u8(frames_dev, n, height, width, frame_stride, row_stride, pixel_stride, ws.A_patch,
                                    ws.x, h->prefix, h->NP, h->D, T, ps, st));
    return run_blocks(h, ws, n, height, width, 256, 1.0f / 255.0f, cls_f32, cls_f16, st, stop_layer, stop_stage, attn, lo);
}

int forward_u8(cbas_enc* h, const Lane& ws, const uint8_t* frames_dev, int n, int height, int width, int64_t frame_stride,
               int64_t row_stride, int64_t pixel_stride, float* cls_f32, f16* cls_f16, hipStream_t st,
               int stop_layer, int stop_stage, const AttnOut& attn = AttnOut{}, const LayersOut* lo = nullptr) {
    int rc = check_frame(h, n, height, width);
    if (rc) return rc;
    if (!frames_dev) return cbas_fail(CBAS_EINVAL, "frames_dev is NULL");
    HIP_TRY(hipSetDevice(h->device));
    return forward_u8_one(h, ws, frames_dev, n, height, width, frame_stride, row_stride, pixel_stride, cls_f32, cls_f16, st,
                          stop_layer, stop_stage, attn, lo);
}

// The buffers of lanes[lane], each zero-filled whole on `st` (the handle's compute stream: see the note at qkv_bias_all in
// vit_build).  ConvNeXt's padding columns of x stay zero from here on.
int alloc_lane(cbas_enc* h, int lane, const LaneBytes& sz, hipStream_t st) {
    Lane& ws = h->lanes[lane];
#define LANE_BUF(name)                                              \
    if (sz.name) {                                                  \
        ALLOC_TRY(hipMalloc(&ws.name, sz.name));                    \
        ALLOC_TRY(hipMemsetAsync(ws.name, 0, sz.name, st));         \
    }
    LANE_BUF(A_patch); LANE_BUF(x); LANE_BUF(h16); LANE_BUF(qkv16); LANE_BUF(u16); LANE_BUF(cls16);
    LANE_BUF(sc_h); LANE_BUF(sc_u); LANE_BUF(x16); LANE_BUF(lnst);
#undef LANE_BUF
    return CBAS_OK;
}

// Safe on a lane that was never or only partly allocated (a failed create); lane 0's stream belongs to the handle.
void free_lane(cbas_enc* h, int lane) {
    Lane& ws = h->lanes[lane];
    if (ws.stream && ws.stream != h->compute) { (void)hipStreamSynchronize(ws.stream); (void)hipStreamDestroy(ws.stream); }
    void* bufs[] = {ws.A_patch, ws.x, ws.h16, ws.qkv16, ws.u16, ws.cls16, ws.sc_h, ws.sc_u, ws.x16, ws.lnst};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    ws = Lane{};
}

}  // namespace

extern "C" int64_t cbas_enc_weights_count(const cbas_enc_config* cfg) { return cfg ? weights_count(*cfg) : -1; }

namespace {
// why a gated MLP cannot be built for this configuration, or nullptr
const char* mlp_refusal(const cbas_enc_config& c, int mlp) {
    if (mlp == CBAS_MLP_GELU) return nullptr;
    if (mlp != CBAS_MLP_SWIGLU) return "mlp must be CBAS_MLP_GELU (0) or CBAS_MLP_SWIGLU (1)";
    if (c.family != 0) return "a gated MLP (CBAS_MLP_SWIGLU) exists for ViT handles only; ConvNeXt blocks have none";
    if (c.precision == 2) return "precision 2 (MX-fp8) has no gated-MLP GEMM; a gated handle runs in precision 0, 3 or 4";
    if (c.precision == 1) return "precision 1 (fp16 hi+lo weights) has no gated-MLP GEMM; a gated handle runs in precision 0, 3 or 4";
    return nullptr;
}
}  // namespace

extern "C" int64_t cbas_enc_weights_count_mlp(const cbas_enc_config* cfg, int32_t mlp) {
    if (!cfg) return -1;
    if (const char* why = mlp_refusal(*cfg, mlp)) { cbas_fail(CBAS_EINVAL, "%s", why); return -1; }
    return weights_count(*cfg, mlp);
}

extern "C" int cbas_enc_get_mlp(const cbas_enc* h, int32_t* mlp) {
    if (!h || !mlp) return cbas_fail(CBAS_EINVAL, "null argument");
    *mlp = h->mlp;
    return CBAS_OK;
}

extern "C" void cbas_enc_destroy(cbas_enc* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->compute) (void)hipStreamSynchronize(h->compute);
    if (h->copy) (void)hipStreamSynchronize(h->copy);
    if (h->nonfinite_dev) (void)hipFree(h->nonfinite_dev);
    for (Slot& s : h->slots) {
        if (s.in_host) (void)hipHostFree(s.in_host);
        if (s.out16_host) (void)hipHostFree(s.out16_host);
        if (s.out32_host) (void)hipHostFree(s.out32_host);
        if (s.in_dev) (void)hipFree(s.in_dev);
        if (s.out16_dev) (void)hipFree(s.out16_dev);
        if (s.out32_dev) (void)hipFree(s.out32_dev);
        if (s.ev_copied) (void)hipEventDestroy(s.ev_copied);
        if (s.ev_done) (void)hipEventDestroy(s.ev_done);
        if (s.ev_in) (void)hipEventDestroy(s.ev_in);
    }
    for (auto& r : h->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (int l = 0; l < 2; ++l) free_lane(h, l);
    if (h->lane0_async_done) (void)hipEventDestroy(h->lane0_async_done);
    if (h->sync_done) (void)hipEventDestroy(h->sync_done);
    for (auto& t : h->pos_tables) { if (t.cos) (void)hipFree(t.cos); if (t.sin) (void)hipFree(t.sin); if (t.fac) (void)hipFree(t.fac); if (t.pos) (void)hipFree(t.pos); }
    void* bufs[] = {h->blob, h->w16, h->w16_lo, h->qkv_bias_all, h->prefix_dev, h->w8, h->w8_sc,
                    h->w16_fold, h->fold_vec, h->w32, h->cnx_arena, h->gu_bias_all, h->gu_scratch};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (h->compute) (void)hipStreamDestroy(h->compute);
    if (h->copy) (void)hipStreamDestroy(h->copy);
    if (h->aux) (void)hipStreamDestroy(h->aux);
    delete h;
}

namespace {

// host-streaming slots (both families)
int create_slots(cbas_enc* h) {
    const cbas_enc_config& c = h->cfg;
    h->slot_bytes = (int64_t)c.max_batch * c.max_height * c.max_width * 4;
    for (Slot& s : h->slots) {
        ALLOC_TRY(hipHostMalloc(&s.in_host, h->slot_bytes, hipHostMallocDefault));
        ALLOC_TRY(hipHostMalloc(&s.out16_host, (int64_t)c.max_batch * h->D * 2, hipHostMallocDefault));
        ALLOC_TRY(hipHostMalloc(&s.out32_host, (int64_t)c.max_batch * h->D * 4, hipHostMallocDefault));
        ALLOC_TRY(hipMalloc(&s.in_dev, h->slot_bytes));
        ALLOC_TRY(hipMalloc(&s.out16_dev, (int64_t)c.max_batch * h->D * 2));
        ALLOC_TRY(hipMalloc(&s.out32_dev, (int64_t)c.max_batch * h->D * 4));
        ALLOC_TRY(hipEventCreateWithFlags(&s.ev_copied, hipEventDisableTiming));
        ALLOC_TRY(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
        ALLOC_TRY(hipEventCreateWithFlags(&s.ev_in, hipEventDisableTiming));
    }
    return CBAS_OK;
}

int cnx_check_config(const cbas_enc_config& c) {
    if (c.precision != 3 && c.precision != 4)
        return cbas_fail(CBAS_EINVAL, "precision=%d: ConvNeXt encoders run in precision 3 (fp32) or 4 (fp32 storage, split-fp16 "
                                      "GEMM products) only", c.precision);
    for (int i = 0; i < 4; ++i) {
        if (c.stage_widths[i] <= 0 || c.stage_widths[i] % 32 || c.stage_widths[i] > 1536)
            return cbas_fail(CBAS_EINVAL, "ConvNeXt stage_widths[%d]=%d must be a positive multiple of 32 up to 1536", i,
                             c.stage_widths[i]);
        if (c.stage_depths[i] < 1 || c.stage_depths[i] > 64)
            return cbas_fail(CBAS_EINVAL, "ConvNeXt stage_depths[%d]=%d outside [1, 64]", i, c.stage_depths[i]);
    }
    if (c.hidden_size != c.stage_widths[3])
        return cbas_fail(CBAS_EINVAL, "hidden_size=%d must be the last stage's width %d (the row width)", c.hidden_size,
                         c.stage_widths[3]);
    if (!(c.layer_norm_eps > 0.f)) return cbas_fail(CBAS_EINVAL, "layer_norm_eps must be positive");
    if (c.max_batch <= 0 || c.max_height < 32 || c.max_width < 32)
        return cbas_fail(CBAS_EINVAL, "bad batch/frame-size field (a ConvNeXt needs frames of at least 32x32)");
    return CBAS_OK;
}

// ConvNeXt weights and workspaces.  The blob (include/cbas_mi355x.h) is read on the host and repacked into one arena:
//   stem weight [Cp0][32]: the 3 identical input channels summed in double and rounded once (launch_pack_patch_weight_f32's
//   rule), k = 4 i + j; downsample weights [Cp][4 C_prev] with k = (2 kh + kw) C_prev + c (the operand order of
//   launch_cnx_downsample); depthwise taps [49][C]; pointwise_conv2, its bias, gamma and the stem / downsample biases padded to
//   Cp rows with zeros (padding columns of the residual stream stay 0).  Rows past C of a GEMM weight are zero.
int cnx_build(cbas_enc* h, const float* wh) {
    const cbas_enc_config& c = h->cfg;
    const bool split = c.precision == 4;
    std::vector<float> ar;
    struct Gw { int64_t off, N, K; float* sc; };
    std::vector<Gw> gw;                                     // GEMM weights (split-packed in precision 4)
    std::vector<std::pair<const float**, int64_t>> fix;     // pointers into the arena, set after the upload
    auto take = [&](int64_t n) { const int64_t o = (int64_t)ar.size(); ar.resize(ar.size() + n, 0.f); return o; };
    auto pow2_scale = [](float maxabs) {                    // as cbas_enc_create's
        if (!(maxabs > 0.f) || !std::isfinite(maxabs)) return 1.0f;
        int e = 0;
        (void)frexpf(maxabs, &e);
        e = std::min(20, std::max(-20, 1 - e));
        return ldexpf(1.0f, e);
    };
    auto gemm_w = [&](int64_t off, int64_t N, int64_t K, float* sc, const float** ptr) {
        float m = 0.f;
        for (int64_t i = 0; i < N * K; ++i) m = std::max(m, fabsf(ar[off + i]));
        *sc = split ? pow2_scale(m) : 1.f;
        gw.push_back({off, N, K, sc});
        fix.push_back({ptr, off});
    };
    auto vec = [&](const float* src, int64_t n, int64_t n_pad, const float** ptr) {
        const int64_t o = take(n_pad);
        std::copy(src, src + n, ar.begin() + o);
        fix.push_back({ptr, o});
    };
    const float* p = wh;
    int prev = 0, prevp = 0;
    for (int i = 0; i < 4; ++i) {
        cbas_enc::CnxStage& S = h->cnx[i];
        const int C = c.stage_widths[i], Cp = (int)round_up(C, 128);
        S.C = C; S.Cp = Cp;
        if (i == 0) {
            const int64_t o = take((int64_t)Cp * 32);
            for (int co = 0; co < C; ++co)
                for (int k = 0; k < 16; ++k) {
                    const float* b = p + (int64_t)co * 48 + k;
                    ar[o + (int64_t)co * 32 + k] = (float)(((double)b[0] + (double)b[16]) + (double)b[32]);
                }
            p += (int64_t)C * 48;
            gemm_w(o, Cp, 32, &S.sc_ds, &S.ds_w);
            vec(p, C, Cp, &S.ds_b); p += C;
            vec(p, C, C, &S.ds_ln_w); p += C;
            vec(p, C, C, &S.ds_ln_b); p += C;
        } else {
            vec(p, prev, prev, &S.ds_ln_w); p += prev;
            vec(p, prev, prev, &S.ds_ln_b); p += prev;
            const int64_t K = 4 * (int64_t)prev, o = take((int64_t)Cp * K);
            for (int co = 0; co < C; ++co)                 // HF (C, C_prev, 2, 2) -> [co][(2 kh + kw) C_prev + ci]
                for (int ci = 0; ci < prev; ++ci)
                    for (int q = 0; q < 4; ++q) ar[o + co * K + (int64_t)q * prev + ci] = p[((int64_t)co * prev + ci) * 4 + q];
            p += (int64_t)C * K;
            gemm_w(o, Cp, K, &S.sc_ds, &S.ds_w);
            vec(p, C, Cp, &S.ds_b); p += C;
        }
        S.blocks.resize(c.stage_depths[i]);
        for (cbas_enc::CnxBlock& b : S.blocks) {
            const int64_t o = take(49 * (int64_t)C);
            for (int ch = 0; ch < C; ++ch)
                for (int t = 0; t < 49; ++t) ar[o + (int64_t)t * C + ch] = p[(int64_t)ch * 49 + t];
            fix.push_back({&b.dw_t, o});
            p += 49 * (int64_t)C;
            vec(p, C, C, &b.dw_b); p += C;
            vec(p, C, C, &b.ln_w); p += C;
            vec(p, C, C, &b.ln_b); p += C;
            const int64_t o1 = take(4 * (int64_t)C * C);
            std::copy(p, p + 4 * (int64_t)C * C, ar.begin() + o1);
            p += 4 * (int64_t)C * C;
            gemm_w(o1, 4 * C, C, &b.sc1, &b.pw1_w);
            vec(p, 4 * C, 4 * C, &b.pw1_b); p += 4 * C;
            const int64_t o2 = take((int64_t)Cp * 4 * C);
            std::copy(p, p + 4 * (int64_t)C * C, ar.begin() + o2);
            p += 4 * (int64_t)C * C;
            gemm_w(o2, Cp, 4 * C, &b.sc2, &b.pw2_w);
            vec(p, C, Cp, &b.pw2_b); p += C;
            vec(p, C, Cp, &b.gamma); p += C;
        }
        prev = C; prevp = Cp;
    }
    (void)prevp;
    vec(p, prev, prev, &h->cnx_norm_w); p += prev;
    vec(p, prev, prev, &h->cnx_norm_b); p += prev;
    if (p - wh != cnx_weights_count(c)) return cbas_fail(CBAS_EHIP, "ConvNeXt weight repack consumed %lld floats",
                                                         (long long)(p - wh));
    hipStream_t st = h->compute;
    HIP_TRY(hipMalloc(&h->cnx_arena, ar.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(h->cnx_arena, ar.data(), ar.size() * sizeof(float), hipMemcpyHostToDevice));
    for (auto& f : fix) *f.first = h->cnx_arena + f.second;
    if (split) {
        // the GEMM weights once more in the split format, at the same offsets
        HIP_TRY(hipMalloc(&h->w32, ar.size() * sizeof(float)));
        for (const Gw& g : gw) {
            if (launch_pack_split_weight(h->cnx_arena + g.off, h->w32 + g.off, g.N, (int)g.K, *g.sc, st))
                return cbas_fail(CBAS_EHIP, "split packing of a ConvNeXt weight failed");
            for (auto& f : fix)
                if (f.second == g.off) *f.first = h->w32 + g.off;
        }
    }
    return CBAS_OK;
}

// floats per lane of a ConvNeXt handle's three buffers (kept for check_frame) and their bytes
LaneBytes cnx_lane_bytes(cbas_enc* h) {
    const cbas_enc_config& c = h->cfg;
    cnx_sizes(h, c.max_batch, c.max_height, c.max_width, &h->cnx_x_cap, &h->cnx_a_cap, &h->cnx_u_cap);
    LaneBytes sz;
    sz.x = h->cnx_x_cap * sizeof(float);
    sz.h16 = h->cnx_a_cap * sizeof(float);
    sz.u16 = h->cnx_u_cap * sizeof(float);
    return sz;
}

int vit_check_config(const cbas_enc_config& c) {
    if (c.family != 0) return cbas_fail(CBAS_EINVAL, "family=%d: 0 (ViT) or 1 (DINOv3 ConvNeXt)", c.family);
    if (c.hidden_size <= 0 || c.hidden_size % 128 || c.num_heads * 64 != c.hidden_size)
        return cbas_fail(CBAS_EINVAL, "hidden_size=%d must be a multiple of 128 with head_dim 64 (num_heads=%d)",
                         c.hidden_size, c.num_heads);
    if (c.intermediate_size <= 0 || c.intermediate_size % 128)
        return cbas_fail(CBAS_EINVAL, "intermediate_size=%d must be a multiple of 128", c.intermediate_size);
    if (c.hidden_size > 1280) return cbas_fail(CBAS_EINVAL, "hidden_size > 1280 not supported");
    if (c.patch_size != 16 && c.patch_size != 14) return cbas_fail(CBAS_EINVAL, "patch_size must be 14 or 16");
    if (c.precision < 0 || c.precision > 4)
        return cbas_fail(CBAS_EINVAL, "precision=%d: 0 (fp16), 1 (fp16 hi+lo weights), 2 (MX-fp8), 3 (fp32, the reference's CPU arithmetic) "
                                      "or 4 (fp32 storage, GEMM products as three-term fp16 splits)", c.precision);
    if (c.precision == 2 && (c.hidden_size % 256 || c.intermediate_size % 256))
        return cbas_fail(CBAS_EINVAL, "precision 2 (MX-fp8) needs hidden_size and intermediate_size to be multiples of 256 "
                                      "(K-tiles of 128 consumed in pairs); got %d / %d", c.hidden_size, c.intermediate_size);
    if (c.precision == 2 && c.hidden_size > 1024)
        return cbas_fail(CBAS_EINVAL, "precision 2 (MX-fp8) stops at hidden_size 1024 (its LayerNorm has no wider form); got %d", c.hidden_size);
    if ((c.use_rope != 0) == (c.pos_embed_grid > 0))
        return cbas_fail(CBAS_EINVAL, "exactly one of use_rope / pos_embed_grid must be set");
    if (c.num_layers <= 0 || c.num_register_tokens < 0 || c.max_batch <= 0 || c.max_height < c.patch_size || c.max_width < c.patch_size)
        return cbas_fail(CBAS_EINVAL, "bad layer/register/batch/frame-size field");
    return CBAS_OK;
}

// ViT weights: the blob on the device as it is, and every GEMM weight once more in the format the handle's precision
// multiplies in (packing kernels on the compute stream)
int vit_build(cbas_enc* h, const float* weights_host, int64_t n_weights) {
    const cbas_enc_config& c = h->cfg;
    h->F = c.intermediate_size; h->L = c.num_layers; h->NH = c.num_heads;
    h->R = c.num_register_tokens; h->NP = 1 + h->R;
    const int64_t D = h->D, F = h->F;
    ALLOC_TRY(hipMalloc(&h->blob, n_weights * sizeof(float)));
    ALLOC_TRY(hipMemcpy(h->blob, weights_host, n_weights * sizeof(float), hipMemcpyHostToDevice));

    // fp16 weight arena: patch (D*256 + D*512) + per layer (3DD + DD + FD + DF); a gated MLP's gate | up weight is 2FD
    const bool gated = h->mlp == CBAS_MLP_SWIGLU;
    const int64_t FU = gated ? 2 * F : F;      // rows of the up GEMM's weight
    const int64_t n16 = D * 256 + D * 512 + (int64_t)h->L * (4 * D * D + FU * D + F * D);
    const bool p3 = c.precision >= 3;         // fp32 end to end (3: fp32 MFMA; 4: three-term fp16 split of the same operands): no fp16 copies, every workspace 4 bytes per element
    if (!p3) ALLOC_TRY(hipMalloc(&h->w16, n16 * sizeof(f16)));
    if (c.precision == 1) ALLOC_TRY(hipMalloc(&h->w16_lo, n16 * sizeof(f16)));
    float* w32p = nullptr;
    if (c.precision == 4) {
        // every weight once more in the split hi | lo format (same byte size as fp32) + a scratch patch weight
        ALLOC_TRY(hipMalloc(&h->w32, (2 * D * 256 + (int64_t)h->L * (4 * D * D + FU * D + F * D)) * sizeof(float)));
        w32p = h->w32;
    } else if (p3) {
        // (gated: + the interleaved gate | up weight of every layer, which precision 3 reads as it is)
        ALLOC_TRY(hipMalloc(&h->w32, (D * 256 + (int64_t)h->L * (3 * D * D + (gated ? FU * D : 0))) * sizeof(float)));
        w32p = h->w32;
    }
    uint8_t* w8p = nullptr;
    uint32_t* s8p = nullptr;
    if (c.precision == 2) {
        const int64_t n8 = (int64_t)h->L * (4 * D * D + 2 * F * D);
        ALLOC_TRY(hipMalloc(&h->w8, n8));
        ALLOC_TRY(hipMalloc(&h->w8_sc, n8 / 32));              // one E8M0 byte per 32 elements
        w8p = h->w8; s8p = h->w8_sc;
    }
    ALLOC_TRY(hipMalloc(&h->qkv_bias_all, (int64_t)h->L * 3 * D * sizeof(float)));
    // on the stream the packing kernels and copies below run on: a null-stream hipMemset may still be in flight when work on a
    // NON-BLOCKING stream (every stream of this library) touches the buffer - found by running training beside the encoder (r5)
    ALLOC_TRY(hipMemsetAsync(h->qkv_bias_all, 0, (int64_t)h->L * 3 * D * sizeof(float), h->compute));

    if (gated) {
        ALLOC_TRY(hipMalloc(&h->gu_bias_all, (int64_t)h->L * FU * sizeof(float)));
        if (c.precision != 3) ALLOC_TRY(hipMalloc(&h->gu_scratch, FU * D * sizeof(float)));
    }

    // LayerNorm fold: folded copies of the q|k|v and up_proj weights (+ column sums and biases), fp16 path only; not for a
    // gated MLP (no folded EPI_SWIGLU) or D > 1024 (the statistics are pooled over at most four 256-column blocks)
    h->fold_ok = c.precision == 0 && !gated && D % 256 == 0 && D <= 1024 && F % 256 == 0;
    f16* wf = nullptr;
    float* fv = nullptr;
    if (h->fold_ok) {
        ALLOC_TRY(hipMalloc(&h->w16_fold, (int64_t)h->L * (3 * D * D + F * D) * sizeof(f16)));
        ALLOC_TRY(hipMalloc(&h->fold_vec, (int64_t)h->L * 2 * (3 * D + F) * sizeof(float)));
        wf = h->w16_fold; fv = h->fold_vec;
    }

    hipStream_t st = h->compute;
    const float* p = h->blob;
    f16* w = h->w16;
    f16* wl = h->w16_lo;
    auto lo = [&](f16* hi_ptr) -> f16* { return wl ? wl + (hi_ptr - h->w16) : nullptr; };

    // prefix rows of every frame: cls_token (+ its position embedding, DINOv2 [v2]:158-161) | register_tokens
    {
        const int64_t G = c.pos_embed_grid;
        std::vector<float> pre(weights_host, weights_host + (1 + h->R) * D);
        if (G > 0) {
            const float* pos = weights_host + (1 + h->R) * D;
            h->pos_host.assign(pos, pos + (1 + G * G) * D);
            for (int64_t d = 0; d < D; ++d) pre[d] += pos[d];
        }
        ALLOC_TRY(hipMalloc(&h->prefix_dev, pre.size() * sizeof(float)));
        ALLOC_TRY(hipMemcpy(h->prefix_dev, pre.data(), pre.size() * sizeof(float), hipMemcpyHostToDevice));
        h->prefix = h->prefix_dev;
        p += (1 + h->R) * D + (G > 0 ? (1 + G * G) * D : 0);
    }
    const float* patch_w = p; p += D * 3 * c.patch_size * c.patch_size;
    h->patch_b = p; p += D;
    h->wpatch = w; w += D * 256;
    h->wpatch2 = w; w += D * 512;
    h->wpatch_lo = lo(h->wpatch); h->wpatch2_lo = lo(h->wpatch2);
    // precision 4: per-tensor power-of-two scales from the HOST copy of the weights (same offsets as the device blob)
    auto host_max = [&](const float* dev_ptr, int64_t n) {
        const float* hp = weights_host + (dev_ptr - h->blob);
        float m = 0.f;
        for (int64_t i = 0; i < n; ++i) m = std::max(m, fabsf(hp[i]));
        return m;
    };
    auto pow2_scale = [](float maxabs) {                     // 2^s with maxabs * 2^s in [1, 2); 1 for an all-zero tensor
        if (!(maxabs > 0.f) || !std::isfinite(maxabs)) return 1.0f;
        int e = 0;
        (void)frexpf(maxabs, &e);                            // maxabs = f * 2^e, f in [0.5, 1)
        e = std::min(20, std::max(-20, 1 - e));
        return ldexpf(1.0f, e);
    };
    int rc = 0;
    if (c.precision == 4) {
        const int pp = c.patch_size * c.patch_size;
        const float* hw = weights_host + (patch_w - h->blob);
        float m = 0.f;
        for (int64_t d = 0; d < D; ++d)
            for (int k = 0; k < pp; ++k)
                m = std::max(m, fabsf((hw[d * 3 * pp + k] + hw[d * 3 * pp + pp + k]) + hw[d * 3 * pp + 2 * pp + k]));
        h->sc_patch = pow2_scale(m);
    }
    if (c.precision == 4) {
        h->wpatch32 = w32p;
        rc = launch_pack_patch_weight_f32(patch_w, w32p + D * 256, (int)D, c.patch_size, st);      // fp32 sum over channels
        rc |= launch_pack_split_weight(w32p + D * 256, w32p, D, 256, h->sc_patch, st);
        w32p += 2 * D * 256;
    } else if (p3) {
        h->wpatch32 = w32p;
        rc = launch_pack_patch_weight_f32(patch_w, w32p, (int)D, c.patch_size, st);
        w32p += D * 256;
    } else {
        rc = launch_pack_patch_weight(patch_w, h->wpatch, h->wpatch_lo, h->wpatch2, h->wpatch2_lo, (int)D, c.patch_size, st);
    }

    h->layers.resize(h->L);
    for (int l = 0; l < h->L && !rc; ++l) {
        LayerW& lw = h->layers[l];
        lw.qkv_b = h->qkv_bias_all + (int64_t)l * 3 * D;
        lw.ln1_w = p; p += D;
        lw.ln1_b = p; p += D;
        const float* qw = p; p += D * D;
        const float* qb = p; p += D;
        const float* kw = p; p += D * D;
        const float* kb = p; p += D;
        const float* vw = p; p += D * D;
        const float* vb = p; p += D;
        const float* ow = p; p += D * D;
        lw.o_b = p; p += D;
        lw.ls1 = p; p += D;
        lw.ln2_w = p; p += D;
        lw.ln2_b = p; p += D;
        const float *gw = nullptr, *gb = nullptr;      // gated: gate_proj sits immediately before up_proj
        if (gated) { gw = p; p += F * D; gb = p; p += F; }
        const float* uw = p; p += F * D;
        lw.up_b = p; p += F;
        const float* dw = p; p += D * F;
        lw.down_b = p; p += D;
        lw.ls2 = p; p += D;
        lw.wqkv = w; w += 3 * D * D;
        lw.wo = w; w += D * D;
        lw.wup = w; w += FU * D;
        lw.wdown = w; w += D * F;
        lw.wqkv_lo = lo(lw.wqkv); lw.wo_lo = lo(lw.wo); lw.wup_lo = lo(lw.wup); lw.wdown_lo = lo(lw.wdown);
        if (c.precision == 4) {
            lw.sc_qkv = pow2_scale(std::max(host_max(qw, D * D), std::max(host_max(kw, D * D), host_max(vw, D * D))));
            lw.sc_o = pow2_scale(host_max(ow, D * D));
            lw.sc_up = pow2_scale(gated ? std::max(host_max(gw, F * D), host_max(uw, F * D)) : host_max(uw, F * D));
            lw.sc_down = pow2_scale(host_max(dw, D * F));
        }
        if (c.precision == 4) {
            rc |= launch_pack_split_weight(qw, w32p, D, (int)D, lw.sc_qkv, st);
            rc |= launch_pack_split_weight(kw, w32p + D * D, D, (int)D, lw.sc_qkv, st);
            rc |= launch_pack_split_weight(vw, w32p + 2 * D * D, D, (int)D, lw.sc_qkv, st);
            lw.wqkv32 = w32p; w32p += 3 * D * D;
            rc |= launch_pack_split_weight(ow, w32p, D, (int)D, lw.sc_o, st);
            lw.wo32 = w32p; w32p += D * D;
            if (gated) rc |= launch_interleave_gate_up(gw, uw, h->gu_scratch, F, (int)D, st);      // same stream: the scratch is reused per layer
            rc |= launch_pack_split_weight(gated ? h->gu_scratch : uw, w32p, FU, (int)D, lw.sc_up, st);
            lw.wup32 = w32p; w32p += FU * D;
            rc |= launch_pack_split_weight(dw, w32p, D, (int)F, lw.sc_down, st);
            lw.wdown32 = w32p; w32p += D * F;
        } else if (p3) {
            // q, k, v sit in the blob with their biases between them: one packed [3D][D] copy; the rest is used in place
            ALLOC_TRY(hipMemcpyAsync(w32p, qw, D * D * sizeof(float), hipMemcpyDeviceToDevice, st));
            ALLOC_TRY(hipMemcpyAsync(w32p + D * D, kw, D * D * sizeof(float), hipMemcpyDeviceToDevice, st));
            ALLOC_TRY(hipMemcpyAsync(w32p + 2 * D * D, vw, D * D * sizeof(float), hipMemcpyDeviceToDevice, st));
            lw.wqkv32 = w32p; w32p += 3 * D * D;
            lw.wo32 = ow; lw.wup32 = uw; lw.wdown32 = dw;
            if (gated) {
                rc |= launch_interleave_gate_up(gw, uw, w32p, F, (int)D, st);
                lw.wup32 = w32p; w32p += FU * D;
            }
        } else {
            rc |= launch_convert_f16(qw, lw.wqkv, lw.wqkv_lo, D * D, st);
            rc |= launch_convert_f16(kw, lw.wqkv + D * D, lw.wqkv_lo ? lw.wqkv_lo + D * D : nullptr, D * D, st);
            rc |= launch_convert_f16(vw, lw.wqkv + 2 * D * D, lw.wqkv_lo ? lw.wqkv_lo + 2 * D * D : nullptr, D * D, st);
            rc |= launch_convert_f16(ow, lw.wo, lw.wo_lo, D * D, st);
            if (gated) rc |= launch_interleave_gate_up(gw, uw, h->gu_scratch, F, (int)D, st);      // same stream: the scratch is reused per layer
            rc |= launch_convert_f16(gated ? h->gu_scratch : uw, lw.wup, lw.wup_lo, FU * D, st);
            rc |= launch_convert_f16(dw, lw.wdown, lw.wdown_lo, D * F, st);
        }
        if (c.precision == 2) {
            lw.wqkv8 = w8p; w8p += 3 * D * D;  lw.sqkv = s8p; s8p += 3 * D * D / 128;
            lw.wo8 = w8p; w8p += D * D;        lw.so = s8p; s8p += D * D / 128;
            lw.wup8 = w8p; w8p += F * D;       lw.sup = s8p; s8p += F * D / 128;
            lw.wdown8 = w8p; w8p += D * F;     lw.sdown = s8p; s8p += D * F / 128;
            rc |= launch_pack_fp8_weight(qw, lw.wqkv8, lw.sqkv, (int)D, (int)D, (int)(3 * D), 0, st);
            rc |= launch_pack_fp8_weight(kw, lw.wqkv8 + D * D, lw.sqkv, (int)D, (int)D, (int)(3 * D), (int)D, st);
            rc |= launch_pack_fp8_weight(vw, lw.wqkv8 + 2 * D * D, lw.sqkv, (int)D, (int)D, (int)(3 * D), (int)(2 * D), st);
            rc |= launch_pack_fp8_weight(ow, lw.wo8, lw.so, (int)D, (int)D, (int)D, 0, st);
            rc |= launch_pack_fp8_weight(uw, lw.wup8, lw.sup, (int)F, (int)D, (int)F, 0, st);
            rc |= launch_pack_fp8_weight(dw, lw.wdown8, lw.sdown, (int)D, (int)F, (int)D, 0, st);
        }
        if (h->fold_ok) {
            lw.wqkv_f = wf; wf += 3 * D * D;
            lw.wup_f = wf; wf += F * D;
            lw.qkv_cs = fv; fv += 3 * D;
            lw.qkv_bf = fv; fv += 3 * D;
            lw.up_cs = fv; fv += F;
            lw.up_bf = fv; fv += F;
            rc |= launch_fold_ln_weight(qw, lw.ln1_w, lw.ln1_b, qb, lw.wqkv_f, lw.qkv_cs, lw.qkv_bf, (int)D, (int)D, st);
            rc |= launch_fold_ln_weight(kw, lw.ln1_w, lw.ln1_b, kb, lw.wqkv_f + D * D, lw.qkv_cs + D, lw.qkv_bf + D, (int)D, (int)D, st);
            rc |= launch_fold_ln_weight(vw, lw.ln1_w, lw.ln1_b, vb, lw.wqkv_f + 2 * D * D, lw.qkv_cs + 2 * D, lw.qkv_bf + 2 * D, (int)D, (int)D, st);
            rc |= launch_fold_ln_weight(uw, lw.ln2_w, lw.ln2_b, lw.up_b, lw.wup_f, lw.up_cs, lw.up_bf, (int)F, (int)D, st);
        }
        if (gated) {
            float* gub = h->gu_bias_all + (int64_t)l * FU;
            rc |= launch_interleave_gate_up(gb, lw.up_b, gub, F, 1, st);
            lw.up_b = gub;
        }
        ALLOC_TRY(hipMemcpyAsync(lw.qkv_b, qb, D * sizeof(float), hipMemcpyDeviceToDevice, st));
        ALLOC_TRY(hipMemcpyAsync(lw.qkv_b + D, kb, D * sizeof(float), hipMemcpyDeviceToDevice, st));
        ALLOC_TRY(hipMemcpyAsync(lw.qkv_b + 2 * D, vb, D * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    h->norm_w = p; p += D;
    h->norm_b = p; p += D;
    if (rc || (p - h->blob) != n_weights)
        return cbas_fail(CBAS_EHIP, "weight packing failed (rc=%d, consumed %lld of %lld)", rc, (long long)(p - h->blob),
                         (long long)n_weights);
    return CBAS_OK;
}

// rows a ViT lane holds (kept for check_frame and the scale / statistics strides) and the bytes of its buffers
LaneBytes vit_lane_bytes(cbas_enc* h) {
    const cbas_enc_config& c = h->cfg;
    const int64_t D = h->D, F = h->F;
    const int64_t Pmax = (int64_t)(c.max_height / c.patch_size) * (c.max_width / c.patch_size);
    const int64_t Tmax = Pmax + h->NP;
    h->rows_cap = round_up((int64_t)c.max_batch * Tmax, 128);
    h->prow_cap = round_up((int64_t)c.max_batch * Pmax, 128);
    h->rope_cap = (int)Pmax;
    h->pos_tables.reserve(cbas_enc::POS_TABLES_MAX);     // entries are handed out by pointer: never reallocate
    const size_t esz = c.precision >= 3 ? sizeof(float) : sizeof(f16);      // activation element size (A_patch is 512 f16 = 256 f32 per row)
    LaneBytes sz;
    sz.A_patch = h->prow_cap * 512 * sizeof(f16);
    sz.x = h->rows_cap * D * sizeof(float);
    sz.h16 = h->rows_cap * D * esz;
    sz.qkv16 = h->rows_cap * 3 * D * esz;
    sz.u16 = h->rows_cap * F * esz;
    sz.cls16 = round_up(c.max_batch, 128) * (3 * D + F) * esz;
    if (c.precision == 2) {
        sz.sc_h = (D / 128) * h->rows_cap * 4;      // dwords
        sz.sc_u = (F / 128) * h->rows_cap * 4;
    }
    if (h->fold_ok) {
        sz.x16 = h->rows_cap * D * sizeof(f16);
        sz.lnst = 4 * h->rows_cap * sizeof(float2);
    }
    return sz;
}

// Everything cbas_enc_create_mlp puts on the device; on a non-zero return the caller destroys the handle.
int enc_init(cbas_enc* h, const float* weights_host, int64_t n_weights) {
    const bool cnx = h->cfg.family == 1;
    ALLOC_TRY(hipStreamCreateWithFlags(&h->compute, hipStreamNonBlocking));
    ALLOC_TRY(hipStreamCreateWithFlags(&h->copy, hipStreamNonBlocking));
    ALLOC_TRY(hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking));
    hipStream_t st = h->compute;
    ALLOC_TRY(hipMalloc(&h->nonfinite_dev, sizeof(unsigned)));
    ALLOC_TRY(hipMemsetAsync(h->nonfinite_dev, 0, sizeof(unsigned), st));

    int rc = cnx ? cnx_build(h, weights_host) : vit_build(h, weights_host, n_weights);
    if (rc) return rc;

    // compute lanes (see cbas_enc::lanes); CBAS_LANES=1 (read here, once per handle) keeps a single lane
    const LaneBytes sz = cnx ? cnx_lane_bytes(h) : vit_lane_bytes(h);
    const char* e = getenv("CBAS_LANES");
    h->n_lanes = (e && atoi(e) == 1) ? 1 : 2;
    for (int l = 0; l < h->n_lanes; ++l) {
        rc = alloc_lane(h, l, sz, st);
        if (rc) return rc;
        if (l == 0) h->lanes[l].stream = h->compute;
        else ALLOC_TRY(hipStreamCreateWithFlags(&h->lanes[l].stream, hipStreamNonBlocking));
    }
    ALLOC_TRY(hipEventCreateWithFlags(&h->lane0_async_done, hipEventDisableTiming));
    ALLOC_TRY(hipEventCreateWithFlags(&h->sync_done, hipEventDisableTiming));
    rc = create_slots(h);
    if (rc) return rc;
    ALLOC_TRY(hipStreamSynchronize(st));
    if (h->gu_scratch) { (void)hipFree(h->gu_scratch); h->gu_scratch = nullptr; }
    return CBAS_OK;
}

}  // namespace

extern "C" int cbas_enc_create(const cbas_enc_config* cfg, const float* weights_host, int64_t n_weights,
                               int device_id, cbas_enc** out) {
    return cbas_enc_create_mlp(cfg, CBAS_MLP_GELU, weights_host, n_weights, device_id, out);
}

extern "C" int cbas_enc_create_mlp(const cbas_enc_config* cfg, int32_t mlp, const float* weights_host, int64_t n_weights,
                                   int device_id, cbas_enc** out) {
    if (!cfg || !weights_host || !out) return cbas_fail(CBAS_EINVAL, "null argument");
    *out = nullptr;
    const cbas_enc_config& c = *cfg;
    if (const char* why = mlp_refusal(c, mlp)) return cbas_fail(CBAS_EINVAL, "%s", why);
    int rc = c.family == 1 ? cnx_check_config(c) : vit_check_config(c);
    if (rc) return rc;
    if (n_weights != weights_count(c, mlp))
        return cbas_fail(CBAS_EINVAL, "weights blob has %lld floats, config needs %lld", (long long)n_weights,
                         (long long)weights_count(c, mlp));
    HIP_TRY(hipSetDevice(device_id));
    cbas_enc* h = new (std::nothrow) cbas_enc();
    if (!h) return cbas_fail(CBAS_ENOMEM, "out of host memory");
    h->cfg = c; h->device = device_id; h->mlp = mlp;
    h->D = c.hidden_size;
    rc = enc_init(h, weights_host, n_weights);
    if (rc) {
        cbas_enc_destroy(h);      // never touches the error text: the failing step's message stands
        return rc;
    }
    *out = h;
    return CBAS_OK;
}

// a synchronous call is about to use lane 0's workspace on stream st
static int sync_enter(cbas_enc* h, hipStream_t st) {
    if (h->lane0_async_used) HIP_TRY(hipStreamWaitEvent(st, h->lane0_async_done, 0));
    // two synchronous calls on DIFFERENT caller streams share lane 0's workspace too (free when st is the same stream)
    if (h->sync_used) HIP_TRY(hipStreamWaitEvent(st, h->sync_done, 0));
    return CBAS_OK;
}
static int sync_leave(cbas_enc* h, hipStream_t st) {
    HIP_TRY(hipEventRecord(h->sync_done, st));
    h->sync_used = true;
    return CBAS_OK;
}
// an asynchronous batch is about to use `lane` on its own stream ls / has been queued there
static int async_enter(cbas_enc* h, int lane, hipStream_t ls) {
    if (lane == 0 && h->sync_used) HIP_TRY(hipStreamWaitEvent(ls, h->sync_done, 0));
    return CBAS_OK;
}
static int async_leave(cbas_enc* h, int lane, hipStream_t ls) {
    if (lane == 0) { HIP_TRY(hipEventRecord(h->lane0_async_done, ls)); h->lane0_async_used = true; }
    return CBAS_OK;
}

// The all-token outputs of cbas_enc_forward_*_tokens: the final LayerNorm of every row of the residual stream instead of the CLS
// rows, and optionally the cosine map of one row against the patch rows.  Such a forward runs with null CLS pointers, which
// leaves the last layer unpruned for that call (vit_begin) and queues no CLS tail; tokens_tail then reads lane 0's stream.
struct TokOut {
    float* f32 = nullptr;
    f16* h16 = nullptr;
    int64_t ld = 0;               // row stride of both images, elements
    const int* query = nullptr;   // per-frame token index of the similarity map's query row; NULL: row 0
    float* sim = nullptr;         // (n, T - prefix rows); NULL: no map
    explicit operator bool() const { return f32 || h16; }
};

static int check_tokens(const cbas_enc* h, const TokOut& t) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null encoder handle");
    if (h->cfg.family != 1 && h->cfg.precision == 2)
        return cbas_fail(CBAS_EINVAL, "precision 2 serves CLS rows only: the token rows of its MX-fp8 layers are a different encoder's (use precision 0)");
    if (!t) return cbas_fail(CBAS_EINVAL, "tokens_f32_dev and tokens_f16_dev are both NULL");
    const int D = h->cfg.family == 1 ? h->cnx[3].C : h->D;
    if (t.ld < D || t.ld % 4) return cbas_fail(CBAS_EINVAL, "ld_tokens = %lld: at least the width %d and a multiple of 4", (long long)t.ld, D);
    if (((uintptr_t)t.f32 | (uintptr_t)t.sim) % 16 || (uintptr_t)t.h16 % 8 || (uintptr_t)t.query % 4)
        return cbas_fail(CBAS_EINVAL, "token outputs must be 16-byte aligned (fp16: 8)");
    return CBAS_OK;
}

// after a forward that kept every row: rows -> t.f32 / t.h16, then the map
static int tokens_tail(cbas_enc* h, const Lane& ws, int n, int height, int width, const TokOut& t, hipStream_t st) {
    const float eps = h->cfg.layer_norm_eps;
    int T, D, P0;
    if (h->cfg.family == 1) {
        const int hw = (height / 32) * (width / 32);      // stage 3's grid: the stem's / 4, then three floor halvings
        T = hw + 1; D = h->cnx[3].C; P0 = 1;
        PROF(CBAS_PROF_LAYERNORM, 0.0);
        LAUNCH_TRY(launch_cnx_token_rows(ws.x, h->cnx[3].Cp, n, hw, h->cnx_norm_w, h->cnx_norm_b, D, eps, t.f32, t.h16, t.ld,
                                         h->nonfinite_dev, st));
    } else {
        const int ps = h->cfg.patch_size;
        T = (height / ps) * (width / ps) + h->NP; D = h->D; P0 = h->NP;
        PROF(CBAS_PROF_LAYERNORM, 0.0);
        LAUNCH_TRY(launch_final_norm_rows(ws.x, D, h->norm_w, h->norm_b, t.f32, t.h16, t.ld, (int64_t)n * T, D, eps, h->nonfinite_dev, st));
    }
    if (t.sim) {
        PROF(CBAS_PROF_OTHER, 6.0 * n * (double)(T - P0) * D);
        if (t.f32) LAUNCH_TRY(launch_token_similarity<float>(t.f32, t.ld, n, T, D, P0, t.query, t.sim, st));
        else LAUNCH_TRY(launch_token_similarity<f16>(t.h16, t.ld, n, T, D, P0, t.query, t.sim, st));
    }
    return CBAS_OK;
}

// the two synchronous forwards: the CLS rows, with or without the attention outputs, or (tok) every token's row instead
static int enc_forward_u8(cbas_enc* h, const uint8_t* frames_dev, int n, int height, int width, int64_t frame_stride,
                          int64_t row_stride, int64_t pixel_stride, float* cls_f32_dev, uint16_t* cls_f16_dev, void* stream,
                          const AttnOut& attn, const TokOut& tok = TokOut{}, const LayersOut* lo = nullptr) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null encoder handle");
    hipStream_t st = (hipStream_t)stream;
    int rc = sync_enter(h, st);
    if (rc) return rc;
    rc = forward_u8(h, h->lanes[0], frames_dev, n, height, width, frame_stride, row_stride, pixel_stride, cls_f32_dev,
                    (f16*)cls_f16_dev, st, -1, -1, attn, lo);
    if (!rc && tok) rc = tokens_tail(h, h->lanes[0], n, height, width, tok, st);
    if (rc) return rc;
    return sync_leave(h, st);
}

// the refusals of the ..._attn forms
static int check_attn(const cbas_enc* h, const AttnOut& attn) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null encoder handle");
    if (h->cfg.family == 1) return cbas_fail(CBAS_EINVAL, "a ConvNeXt encoder has no attention: CLS attention maps exist for the ViT families only");
    if (!attn) return cbas_fail(CBAS_EINVAL, "attn_heads_dev and attn_map_dev are both NULL (cbas_enc_forward_u8 / _f32 are the forms without maps)");
    return CBAS_OK;
}
// ... and of a frame whose token row does not fit the map kernel's LDS: refused before anything is queued
static int check_attn_frame(const cbas_enc* h, int height, int width) {
    const int ps = h->cfg.patch_size;
    if (ps <= 0 || height < ps || width < ps) return CBAS_OK;      // check_frame names these
    const int64_t T = (int64_t)(height / ps) * (width / ps) + h->NP;
    if ((2 * T - h->NP) * (int64_t)sizeof(float) > CLS_ATTENTION_LDS_BYTES)
        return cbas_fail(CBAS_EINVAL, "frame %dx%d has %lld tokens: the CLS attention map kernel holds at most %lld", height, width,
                         (long long)T, (long long)((CLS_ATTENTION_LDS_BYTES / (int64_t)sizeof(float) + h->NP) / 2));
    return CBAS_OK;
}

extern "C" int cbas_enc_forward_u8(cbas_enc* h, const uint8_t* frames_dev, int n, int height, int width,
                                   int64_t frame_stride, int64_t row_stride, int64_t pixel_stride,
                                   float* cls_f32_dev, uint16_t* cls_f16_dev, void* stream) {
    return enc_forward_u8(h, frames_dev, n, height, width, frame_stride, row_stride, pixel_stride, cls_f32_dev, cls_f16_dev, stream,
                          AttnOut{});
}

extern "C" int cbas_enc_forward_u8_attn(cbas_enc* h, const uint8_t* frames_dev, int n, int height, int width,
                                        int64_t frame_stride, int64_t row_stride, int64_t pixel_stride,
                                        float* cls_f32_dev, uint16_t* cls_f16_dev, void* stream, float* attn_heads_dev,
                                        float* attn_map_dev) {
    AttnOut attn;
    attn.heads = attn_heads_dev; attn.map = attn_map_dev;
    int rc = check_attn(h, attn);
    if (!rc) rc = check_attn_frame(h, height, width);
    if (rc) return rc;
    return enc_forward_u8(h, frames_dev, n, height, width, frame_stride, row_stride, pixel_stride, cls_f32_dev, cls_f16_dev, stream, attn);
}

static int enc_forward_f32(cbas_enc* h, const float* x_dev, int n, int height, int width, float* cls_f32_dev,
                           uint16_t* cls_f16_dev, void* stream, const AttnOut& attn, const TokOut& tok = TokOut{},
                           const LayersOut* lo = nullptr) {
    int rc = check_frame(h, n, height, width);
    if (rc) return rc;
    if (!x_dev) return cbas_fail(CBAS_EINVAL, "x_dev is NULL");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int ps = h->cfg.patch_size;
    const int T = ps > 0 ? (height / ps) * (width / ps) + h->NP : 0;
    rc = sync_enter(h, st);
    if (rc) return rc;
    const Lane& ws = h->lanes[0];
    if (h->cfg.family == 1) {
        LAUNCH_TRY(launch_cnx_stem_im2col_f32(x_dev, n, height, width, reinterpret_cast<float*>(ws.h16), h->cfg.precision == 4, st));
        rc = run_cnx(h, ws, n, height, width, cls_f32_dev, (f16*)cls_f16_dev, st, -1);
        if (!rc && tok) rc = tokens_tail(h, ws, n, height, width, tok, st);
        if (rc) return rc;
        return sync_leave(h, st);
    }
    if (h->cfg.precision >= 3)
        LAUNCH_TRY(launch_im2col_f32_f32(x_dev, n, height, width, reinterpret_cast<float*>(ws.A_patch), ws.x, h->prefix, h->NP, h->D, T, ps,
                                         h->cfg.precision == 4, st));
    else
        LAUNCH_TRY(launch_im2col_f32(x_dev, n, height, width, ws.A_patch, ws.x, h->prefix, h->NP, h->D, T, ps, st));
    rc = run_blocks(h, ws, n, height, width, 512, 1.0f, cls_f32_dev, (f16*)cls_f16_dev, st, -1, -1, attn, lo);
    if (!rc && tok) rc = tokens_tail(h, ws, n, height, width, tok, st);
    if (rc) return rc;
    return sync_leave(h, st);
}

extern "C" int cbas_enc_forward_f32(cbas_enc* h, const float* x_dev, int n, int height, int width,
                                    float* cls_f32_dev, uint16_t* cls_f16_dev, void* stream) {
    return enc_forward_f32(h, x_dev, n, height, width, cls_f32_dev, cls_f16_dev, stream, AttnOut{});
}

extern "C" int cbas_enc_forward_f32_attn(cbas_enc* h, const float* x_dev, int n, int height, int width,
                                         float* cls_f32_dev, uint16_t* cls_f16_dev, void* stream, float* attn_heads_dev,
                                         float* attn_map_dev) {
    AttnOut attn;
    attn.heads = attn_heads_dev; attn.map = attn_map_dev;
    int rc = check_attn(h, attn);
    if (!rc) rc = check_attn_frame(h, height, width);
    if (rc) return rc;
    return enc_forward_f32(h, x_dev, n, height, width, cls_f32_dev, cls_f16_dev, stream, attn);
}

extern "C" int cbas_enc_forward_u8_tokens(cbas_enc* h, const uint8_t* frames_dev, int n, int height, int width,
                                          int64_t frame_stride, int64_t row_stride, int64_t pixel_stride,
                                          float* tokens_f32_dev, uint16_t* tokens_f16_dev, int64_t ld_tokens,
                                          const int32_t* query_idx_dev, float* sim_map_dev, void* stream) {
    TokOut tok;
    tok.f32 = tokens_f32_dev; tok.h16 = (f16*)tokens_f16_dev; tok.ld = ld_tokens; tok.query = query_idx_dev; tok.sim = sim_map_dev;
    const int rc = check_tokens(h, tok);
    if (rc) return rc;
    return enc_forward_u8(h, frames_dev, n, height, width, frame_stride, row_stride, pixel_stride, nullptr, nullptr, stream, AttnOut{}, tok);
}

extern "C" int cbas_enc_forward_f32_tokens(cbas_enc* h, const float* x_dev, int n, int height, int width,
                                           float* tokens_f32_dev, uint16_t* tokens_f16_dev, int64_t ld_tokens,
                                           const int32_t* query_idx_dev, float* sim_map_dev, void* stream) {
    TokOut tok;
    tok.f32 = tokens_f32_dev; tok.h16 = (f16*)tokens_f16_dev; tok.ld = ld_tokens; tok.query = query_idx_dev; tok.sim = sim_map_dev;
    const int rc = check_tokens(h, tok);
    if (rc) return rc;
    return enc_forward_f32(h, x_dev, n, height, width, nullptr, nullptr, stream, AttnOut{}, tok);
}

// ---- per-layer outputs: cbas_enc_forward_*_layers ----
extern "C" int64_t cbas_enc_layers_scratch_bytes(const cbas_enc* h, int n, int height, int width) {
    if (!h) { cbas_fail(CBAS_EINVAL, "null encoder handle"); return -1; }
    if (h->cfg.family == 1) { cbas_fail(CBAS_EINVAL, "a ConvNeXt encoder has no attention: attention rollout exists for the ViT families only"); return -1; }
    const int ps = h->cfg.patch_size;
    if (n <= 0 || height < ps || width < ps) { cbas_fail(CBAS_EINVAL, "n = %d frames of %dx%d", n, height, width); return -1; }
    const int64_t T = (int64_t)(height / ps) * (width / ps) + h->NP;
    return 3 * (int64_t)n * T * T * (int64_t)sizeof(float);
}

// every refusal of the ..._layers forms, before anything is queued
static int check_layers(const cbas_enc* h, const cbas_enc_layers_args* a, int n, int height, int width, LayersOut& lo) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null encoder handle");
    if (!a || a->struct_bytes != (int64_t)sizeof(cbas_enc_layers_args))
        return cbas_fail(CBAS_EINVAL, "cbas_enc_layers_args: struct_bytes %lld, library expects %lld", a ? (long long)a->struct_bytes : -1ll,
                         (long long)sizeof(cbas_enc_layers_args));
    if (h->cfg.family == 1)
        return cbas_fail(CBAS_EINVAL, "a ConvNeXt encoder has no transformer layers: per-layer hidden states, attention and rollout exist for the ViT families only");
    if (h->cfg.precision == 2)
        return cbas_fail(CBAS_EINVAL, "precision 2 serves CLS rows only: the token rows of its MX-fp8 layers are a different encoder's (use precision 0)");
    const bool want_hs = a->hidden_f32_dev || a->hidden_f16_dev, want_at = a->attn_heads_dev || a->attn_map_dev, want_roll = a->rollout_dev != nullptr;
    if (!want_hs && !want_at && !want_roll)
        return cbas_fail(CBAS_EINVAL, "hidden_f32_dev, hidden_f16_dev, attn_heads_dev, attn_map_dev and rollout_dev are all NULL");
    const int L = h->L, D = h->D;
    if (want_hs) {
        if (!a->hidden_layers || a->n_hidden_layers <= 0) return cbas_fail(CBAS_EINVAL, "hidden-state outputs without a list of layers");
        for (int j = 0; j < a->n_hidden_layers; ++j)
            if (a->hidden_layers[j] < 0 || a->hidden_layers[j] > L)
                return cbas_fail(CBAS_EINVAL, "hidden_layers[%d] = %d: hidden states are numbered 0 .. %d", j, a->hidden_layers[j], L);
        if (a->ld_hidden < D || a->ld_hidden % 4) return cbas_fail(CBAS_EINVAL, "ld_hidden = %lld: at least the width %d and a multiple of 4", (long long)a->ld_hidden, D);
        if (a->hidden_layer_stride % 4 || (a->n_hidden_layers > 1 && a->hidden_layer_stride < ((int64_t)n * (height / h->cfg.patch_size) * (width / h->cfg.patch_size) + (int64_t)n * h->NP - 1) * a->ld_hidden + D))
            return cbas_fail(CBAS_EINVAL, "hidden_layer_stride = %lld: a multiple of 4 that holds one layer's image", (long long)a->hidden_layer_stride);
        if ((uintptr_t)a->hidden_f32_dev % 16 || (uintptr_t)a->hidden_f16_dev % 8)
            return cbas_fail(CBAS_EINVAL, "hidden-state outputs must be 16-byte aligned (fp16: 8)");
    }
    if (want_at) {
        if (!a->attn_layers || a->n_attn_layers <= 0) return cbas_fail(CBAS_EINVAL, "attention outputs without a list of layers");
        for (int j = 0; j < a->n_attn_layers; ++j)
            if (a->attn_layers[j] < 1 || a->attn_layers[j] > L)
                return cbas_fail(CBAS_EINVAL, "attn_layers[%d] = %d: attention layers are numbered 1 .. %d", j, a->attn_layers[j], L);
        if (((uintptr_t)a->attn_heads_dev | (uintptr_t)a->attn_map_dev) % 4) return cbas_fail(CBAS_EINVAL, "attention outputs must be 4-byte aligned");
    }
    if (want_roll) {
        if (a->rollout_start_layer < 1 || a->rollout_start_layer > L)
            return cbas_fail(CBAS_EINVAL, "rollout_start_layer = %d: layers are numbered 1 .. %d", a->rollout_start_layer, L);
        if (((uintptr_t)a->rollout_dev | (uintptr_t)a->rollout_query_dev) % 4) return cbas_fail(CBAS_EINVAL, "rollout outputs must be 4-byte aligned");
        if (!a->scratch_dev || (uintptr_t)a->scratch_dev % 16) return cbas_fail(CBAS_EINVAL, "the rollout scratch must be a 16-byte aligned device pointer");
    }
    int rc = check_frame(const_cast<cbas_enc*>(h), n, height, width);
    if (rc) return rc;
    if (want_at && (rc = check_attn_frame(h, height, width))) return rc;
    if (want_roll) {
        const int ps = h->cfg.patch_size;
        const int64_t T = (int64_t)(height / ps) * (width / ps) + h->NP;
        if (!attention_mean_rows_per_block(T))
            return cbas_fail(CBAS_EINVAL, "frame %dx%d has %lld tokens: one row of the attention rollout kernel does not fit 64 KiB of LDS", height, width, (long long)T);
        const int64_t need = 3 * (int64_t)n * T * T * (int64_t)sizeof(float);
        if (a->scratch_bytes < need)
            return cbas_fail(CBAS_EINVAL, "rollout scratch of %lld bytes: %d frames of %lld tokens need %lld (cbas_enc_layers_scratch_bytes)",
                             (long long)a->scratch_bytes, n, (long long)T, (long long)need);
    }
    if (want_hs) {
        lo.hs_layers = a->hidden_layers; lo.n_hs = a->n_hidden_layers; lo.hs_norm = a->hidden_norm != 0;
        lo.hs_f32 = a->hidden_f32_dev; lo.hs_f16 = (f16*)a->hidden_f16_dev; lo.hs_ld = a->ld_hidden; lo.hs_stride = a->hidden_layer_stride;
    }
    if (want_at) { lo.at_layers = a->attn_layers; lo.n_at = a->n_attn_layers; lo.at_heads = a->attn_heads_dev; lo.at_map = a->attn_map_dev; }
    if (want_roll) {
        lo.roll = a->rollout_dev; lo.roll_start = a->rollout_start_layer; lo.roll_query = a->rollout_query_dev; lo.scratch = (float*)a->scratch_dev;
    }
    return CBAS_OK;
}

extern "C" int cbas_enc_forward_u8_layers(cbas_enc* h, const uint8_t* frames_dev, int n, int height, int width,
                                          int64_t frame_stride, int64_t row_stride, int64_t pixel_stride,
                                          const cbas_enc_layers_args* args, void* stream) {
    LayersOut lo;
    const int rc = check_layers(h, args, n, height, width, lo);
    if (rc) return rc;
    return enc_forward_u8(h, frames_dev, n, height, width, frame_stride, row_stride, pixel_stride, nullptr, nullptr, stream, AttnOut{}, TokOut{}, &lo);
}

extern "C" int cbas_enc_forward_f32_layers(cbas_enc* h, const float* x_dev, int n, int height, int width,
                                           const cbas_enc_layers_args* args, void* stream) {
    LayersOut lo;
    const int rc = check_layers(h, args, n, height, width, lo);
    if (rc) return rc;
    return enc_forward_f32(h, x_dev, n, height, width, nullptr, nullptr, stream, AttnOut{}, TokOut{}, &lo);
}

#if CBAS_BUILD_DEBUG      // stage taps: debug build only (include/cbas_mi355x_debug.h)
extern "C" int cbas_enc_debug_forward_u8(cbas_enc* h, const uint8_t* frames_dev, int n, int height, int width,
                                         int64_t frame_stride, int64_t row_stride, int64_t pixel_stride,
                                         int stop_layer, int stop_stage) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null encoder handle");
    int rc = forward_u8(h, h->lanes[0], frames_dev, n, height, width, frame_stride, row_stride, pixel_stride, nullptr, nullptr,
                        h->compute, stop_layer, stop_stage);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->compute));
    return CBAS_OK;
}

extern "C" int cbas_enc_debug_read(cbas_enc* h, int which, void* host_out, int64_t n_bytes) {
    if (!h || !host_out) return cbas_fail(CBAS_EINVAL, "null argument");
    const void* src = nullptr;
    int64_t cap = 0;
    const Lane& ws = h->lanes[0];      // the taps run there (cbas_enc_debug_forward_u8)
    if (h->cfg.family == 1) {
        // the tensor the last tapped pass stopped at: rows of C floats out of the residual stream's Cp-float rows
        if (which < 4 || which > 8) return cbas_fail(CBAS_EINVAL, "ConvNeXt taps are which = 4 (stem) .. 8 (stage 3); got %d", which);
        if (h->cnx_tap != which - 4) return cbas_fail(CBAS_ESTATE, "the last tapped pass stopped at %d, not %d", h->cnx_tap, which - 4);
        const cbas_enc::CnxStage& S = h->cnx[which == 4 ? 0 : which - 5];
        const int64_t need = (int64_t)h->cnx_tap_rows * S.C * 4;
        if (n_bytes != need) return cbas_fail(CBAS_EINVAL, "tap %d holds %lld bytes, asked for %lld", which, (long long)need, (long long)n_bytes);
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->compute));
        HIP_TRY(hipMemcpy2D(host_out, (size_t)S.C * 4, ws.x, (size_t)S.Cp * 4, (size_t)S.C * 4, (size_t)h->cnx_tap_rows,
                            hipMemcpyDeviceToHost));
        return CBAS_OK;
    }
    switch (which) {
        case 0: src = ws.x; cap = h->rows_cap * h->D * 4; break;
        // precision 3 keeps these as fp32 (4 bytes per element)
        case 1: src = ws.h16; cap = h->rows_cap * h->D * (h->cfg.precision >= 3 ? 4 : 2); break;
        case 2: src = ws.qkv16; cap = h->rows_cap * 3 * h->D * (h->cfg.precision >= 3 ? 4 : 2); break;
        case 3: src = ws.u16; cap = h->rows_cap * h->F * (h->cfg.precision >= 3 ? 4 : 2); break;
        default: return cbas_fail(CBAS_EINVAL, "unknown buffer %d", which);
    }
    if (n_bytes < 0 || n_bytes > cap) return cbas_fail(CBAS_EINVAL, "read of %lld bytes exceeds buffer (%lld)", (long long)n_bytes, (long long)cap);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->compute));
    HIP_TRY(hipMemcpy(host_out, src, n_bytes, hipMemcpyDeviceToHost));
    return CBAS_OK;
}
#endif

// cls_*_dev == nullptr: rows go to the slot's own buffers and on to pinned host memory (cbas_enc_wait);
// otherwise rows are written to the caller's device buffers and the slot is released by cbas_enc_wait_stream.
static int submit_u8_host_impl(cbas_enc* h, int slot, const uint8_t* frames_host, int n, int height, int width,
                               int64_t frame_stride, int64_t row_stride, int64_t pixel_stride, float* cls_f32_dev,
                               f16* cls_f16_dev, bool to_device) {
    int rc = check_frame(h, n, height, width);
    if (rc) return rc;
    if (slot < 0 || slot >= CBAS_ENC_SLOTS) return cbas_fail(CBAS_EINVAL, "slot %d out of range", slot);
    if (!frames_host) return cbas_fail(CBAS_EINVAL, "frames_host is NULL");
    Slot& s = h->slots[slot];
    if (s.busy) return cbas_fail(CBAS_ESTATE, "slot %d is busy; call cbas_enc_wait first", slot);
    const int64_t plane = (int64_t)height * width;
    if (frame_stride < 0 || row_stride < 0 || pixel_stride < 1) return cbas_fail(CBAS_EINVAL, "negative stride");
    HIP_TRY(hipSetDevice(h->device));
    // Bytes of the caller's layout are shipped AS THEY ARE (for decord's (n,H,W,3) RGB: 3 bytes per pixel, trivial on
    // PCIe 5) and the consumed channel is picked by the ingest kernel through the strides, so the host does no
    // per-pixel work.  `ext` = bytes from a frame's first consumed pixel to its last.
    if (s.used) {
        // A slot released by cbas_enc_wait_stream was never waited for on the HOST: its previous H2D copy may still be
        // reading the pinned staging, and its previous batch may still be reading in_dev.
        HIP_TRY(hipEventSynchronize(s.ev_copied));
        HIP_TRY(hipStreamWaitEvent(h->copy, s.ev_done, 0));
    }
    const int64_t ext = (int64_t)(height - 1) * row_stride + (int64_t)(width - 1) * pixel_stride + 1;
    const bool dense = n == 1 || frame_stride >= ext;               // frames do not interleave
    int64_t dev_frame_stride = plane, dev_row_stride = width, dev_pixel_stride = 1, bytes = (int64_t)n * plane;
    const uint8_t* src_host = s.in_host;
    if (dense && frame_stride <= ext + 64 && (int64_t)(n - 1) * frame_stride + ext <= h->slot_bytes) {
        // one contiguous span holds the whole chunk
        bytes = (int64_t)(n - 1) * frame_stride + ext;
        dev_frame_stride = frame_stride; dev_row_stride = row_stride; dev_pixel_stride = pixel_stride;
        hipPointerAttribute_t attr;
        const bool pinned = hipPointerGetAttributes(&attr, frames_host) == hipSuccess && attr.type == hipMemoryTypeHost;
        if (!pinned) (void)hipGetLastError();                         // pageable memory: the query fails, clear it
        if (pinned) src_host = frames_host;                           // direct DMA; caller keeps it valid until wait
        else memcpy(s.in_host, frames_host, bytes);
    } else if (dense && (int64_t)n * ext <= h->slot_bytes) {
        // strided frames: one span per frame, packed back to back
        for (int f = 0; f < n; ++f) memcpy(s.in_host + (int64_t)f * ext, frames_host + (int64_t)f * frame_stride, ext);
        bytes = (int64_t)n * ext;
        dev_frame_stride = ext; dev_row_stride = row_stride; dev_pixel_stride = pixel_stride;
    } else {
        // sparse layouts (huge strides): gather the consumed channel into packed planes on the host
        if ((int64_t)n * plane > h->slot_bytes) return cbas_fail(CBAS_EINVAL, "chunk exceeds slot staging size");
        for (int f = 0; f < n; ++f) {
            const uint8_t* src = frames_host + (int64_t)f * frame_stride;
            uint8_t* dst = s.in_host + (int64_t)f * plane;
            for (int y = 0; y < height; ++y) {
                const uint8_t* r = src + (int64_t)y * row_stride;
                uint8_t* d = dst + (int64_t)y * width;
                if (pixel_stride == 1) memcpy(d, r, width);
                else for (int xx = 0; xx < width; ++xx) d[xx] = r[(int64_t)xx * pixel_stride];
            }
        }
    }
    HIP_TRY(hipMemcpyAsync(s.in_dev, src_host, bytes, hipMemcpyHostToDevice, h->copy));
    HIP_TRY(hipEventRecord(s.ev_copied, h->copy));
    const int lane = (int)(h->submit_count++ % (uint64_t)h->n_lanes);
    const Lane& ws = h->lanes[lane];
    hipStream_t ls = ws.stream;
    HIP_TRY(hipStreamWaitEvent(ls, s.ev_copied, 0));
    rc = async_enter(h, lane, ls);
    if (rc) return rc;
    rc = forward_u8(h, ws, s.in_dev, n, height, width, dev_frame_stride, dev_row_stride, dev_pixel_stride,
                    to_device ? cls_f32_dev : s.out32_dev, to_device ? cls_f16_dev : s.out16_dev, ls, -1, -1);
    if (rc) return rc;
    rc = async_leave(h, lane, ls);
    if (rc) return rc;
    if (!to_device) {
        HIP_TRY(hipMemcpyAsync(s.out16_host, s.out16_dev, (int64_t)n * h->D * 2, hipMemcpyDeviceToHost, ls));
        HIP_TRY(hipMemcpyAsync(s.out32_host, s.out32_dev, (int64_t)n * h->D * 4, hipMemcpyDeviceToHost, ls));
    }
    HIP_TRY(hipEventRecord(s.ev_done, ls));
    s.n = n;
    s.busy = true;
    s.used = true;
    s.dev_mode = to_device;
    return CBAS_OK;
}

extern "C" int cbas_enc_submit_u8_host(cbas_enc* h, int slot, const uint8_t* frames_host, int n, int height,
                                       int width, int64_t frame_stride, int64_t row_stride, int64_t pixel_stride) {
    return submit_u8_host_impl(h, slot, frames_host, n, height, width, frame_stride, row_stride, pixel_stride, nullptr,
                               nullptr, false);
}

extern "C" int cbas_enc_submit_u8_host_dev(cbas_enc* h, int slot, const uint8_t* frames_host, int n, int height,
                                           int width, int64_t frame_stride, int64_t row_stride, int64_t pixel_stride,
                                           float* cls_f32_dev, uint16_t* cls_f16_dev, void* after_stream) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null encoder handle");
    if (!cls_f32_dev && !cls_f16_dev) return cbas_fail(CBAS_EINVAL, "no output requested");
    if (slot >= 0 && slot < CBAS_ENC_SLOTS && !h->slots[slot].busy) {
        // the output rows may still be read by work queued on after_stream (e.g. the head over an earlier clip)
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipEventRecord(h->slots[slot].ev_in, (hipStream_t)after_stream));
        HIP_TRY(hipStreamWaitEvent(h->copy, h->slots[slot].ev_in, 0));
    }
    return submit_u8_host_impl(h, slot, frames_host, n, height, width, frame_stride, row_stride, pixel_stride,
                               cls_f32_dev, (f16*)cls_f16_dev, true);
}

extern "C" void* cbas_enc_copy_stream(cbas_enc* h) { return h ? (void*)h->copy : nullptr; }

extern "C" int cbas_enc_get_config(const cbas_enc* h, cbas_enc_config* out) {
    if (!h || !out) return cbas_fail(CBAS_EINVAL, "null argument");
    *out = h->cfg;
    return CBAS_OK;
}

extern "C" int cbas_enc_submit_u8(cbas_enc* h, int slot, const uint8_t* frames_dev, int n, int height, int width,
                                  int64_t frame_stride, int64_t row_stride, int64_t pixel_stride, float* cls_f32_dev,
                                  uint16_t* cls_f16_dev, void* after_stream) {
    int rc = check_frame(h, n, height, width);
    if (rc) return rc;
    if (slot < 0 || slot >= CBAS_ENC_SLOTS) return cbas_fail(CBAS_EINVAL, "slot %d out of range", slot);
    if (!frames_dev) return cbas_fail(CBAS_EINVAL, "frames_dev is NULL");
    if (!cls_f32_dev && !cls_f16_dev) return cbas_fail(CBAS_EINVAL, "no output requested");
    Slot& s = h->slots[slot];
    if (s.busy) return cbas_fail(CBAS_ESTATE, "slot %d is busy; call cbas_enc_wait_stream first", slot);
    HIP_TRY(hipSetDevice(h->device));
    const int lane = (int)(h->submit_count++ % (uint64_t)h->n_lanes);
    const Lane& ws = h->lanes[lane];
    hipStream_t ls = ws.stream;
    HIP_TRY(hipEventRecord(s.ev_in, (hipStream_t)after_stream));      // the frames (and the output rows) are ready
    HIP_TRY(hipStreamWaitEvent(ls, s.ev_in, 0));
    rc = async_enter(h, lane, ls);
    if (rc) return rc;
    rc = forward_u8(h, ws, frames_dev, n, height, width, frame_stride, row_stride, pixel_stride, cls_f32_dev,
                    (f16*)cls_f16_dev, ls, -1, -1);
    if (rc) return rc;
    rc = async_leave(h, lane, ls);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(s.ev_done, ls));
    s.n = n;
    s.busy = true;
    s.dev_mode = true;
    return CBAS_OK;
}

extern "C" int cbas_enc_set_lanes(cbas_enc* h, int n_lanes) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null encoder handle");
    if (n_lanes < 1 || n_lanes > 2 || (n_lanes == 2 && !h->lanes[1].stream))
        return cbas_fail(CBAS_EINVAL, "n_lanes=%d not available (handle was created with %s)", n_lanes,
                         h->lanes[1].stream ? "2 lanes" : "CBAS_LANES=1");
    for (const Slot& s : h->slots)
        if (s.busy) return cbas_fail(CBAS_ESTATE, "cbas_enc_set_lanes with a batch in flight");
    h->n_lanes = n_lanes;
    h->submit_count = 0;
    return CBAS_OK;
}

extern "C" int cbas_enc_set_pos_interp(cbas_enc* h, int mode) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null handle");
    if (h->cfg.family != 0 || h->cfg.pos_embed_grid <= 0)
        return cbas_fail(CBAS_EINVAL, "cbas_enc_set_pos_interp: the handle has no learned position embedding");
    if (mode != CBAS_POS_INTERP_BICUBIC_AA && mode != CBAS_POS_INTERP_BICUBIC)
        return cbas_fail(CBAS_EINVAL, "cbas_enc_set_pos_interp: mode=%d: 0 (bicubic, antialiased) or 1 (bicubic)", mode);
    if (mode != h->pos_interp && !h->pos_tables.empty())
        return cbas_fail(CBAS_EINVAL, "cbas_enc_set_pos_interp: call it before the first batch (tables of %d grid(s) are built)",
                         (int)h->pos_tables.size());
    h->pos_interp = mode;
    return CBAS_OK;
}

extern "C" int cbas_enc_set_fp8_plan(cbas_enc* h, int plan) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null handle");
    if (h->cfg.family != 0 || h->cfg.precision != 2)
        return cbas_fail(CBAS_EINVAL, "cbas_enc_set_fp8_plan: only a precision-2 (MX-fp8) ViT handle has a plan (this one: %s, precision %d)",
                         h->cfg.family == 0 ? "ViT" : "ConvNeXt", h->cfg.precision);
    if (plan < 0 || plan > CBAS_FP8_PLAN_ALL)
        return cbas_fail(CBAS_EINVAL, "cbas_enc_set_fp8_plan: plan=%d: a mask of 1 (qkv), 2 (proj), 4 (up), 8 (down)", plan);
    if (h->vit_forward_seen)
        return cbas_fail(CBAS_EINVAL, "cbas_enc_set_fp8_plan: call it before the handle's first forward / submit (rows of one handle "
                                      "come from one plan)");
    // nothing to allocate or repack: the handle holds the fp16 weights of every GEMM beside the MX-fp8 ones, and both lanes'
    // workspaces fit either format of every activation (the plan is read per launch sequence, whichever lane runs it)
    h->fp8_plan = plan;
    return CBAS_OK;
}

extern "C" int cbas_enc_set_prune_last_layer(cbas_enc* h, int enable) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null encoder handle");
    h->prune_last = enable != 0;
    return CBAS_OK;
}

#if CBAS_BUILD_DEBUG
extern "C" int cbas_enc_debug_option(cbas_enc* h, const char* name, int value) {
    if (!h || !name) return cbas_fail(CBAS_EINVAL, "null argument");
    if (!strcmp(name, "rope_lds")) { h->rope_in_lds = value != 0; return CBAS_OK; }
    if (!strcmp(name, "ln_fold")) { h->ln_fold = value != 0; return CBAS_OK; }
    if (!strcmp(name, "split_kernels")) { vit32_split_set_forms(value); return CBAS_OK; }       // process-wide (precision 4)
    return cbas_fail(CBAS_EINVAL, "unknown debug option '%s'", name);
}
#endif

extern "C" int cbas_enc_wait_stream(cbas_enc* h, int slot, void* stream) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null encoder handle");
    if (slot < 0 || slot >= CBAS_ENC_SLOTS) return cbas_fail(CBAS_EINVAL, "slot %d out of range", slot);
    Slot& s = h->slots[slot];
    if (!s.busy) return cbas_fail(CBAS_ESTATE, "slot %d has no submitted work", slot);
    if (!s.dev_mode) return cbas_fail(CBAS_ESTATE, "slot %d holds a host submission; use cbas_enc_wait", slot);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, s.ev_done, 0));
    s.busy = false;
    return CBAS_OK;
}

// Frames whose CLS row came out NaN / infinite since the last call (the counter is cleared): CBAS_ERANGE when there are any.
// Meaningful after the batches in question have completed (cbas_enc_wait and the fused session's waits call it themselves).
extern "C" int cbas_enc_check_finite(cbas_enc* h) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null encoder handle");
    HIP_TRY(hipSetDevice(h->device));
    unsigned n = 0;
    HIP_TRY(hipMemcpyAsync(&n, h->nonfinite_dev, sizeof(n), hipMemcpyDeviceToHost, h->aux));
    HIP_TRY(hipStreamSynchronize(h->aux));
    if (!n) return CBAS_OK;
    HIP_TRY(hipMemsetAsync(h->nonfinite_dev, 0, sizeof(unsigned), h->aux));
    HIP_TRY(hipStreamSynchronize(h->aux));
    return cbas_fail(CBAS_ERANGE, "%u frame(s) produced a non-finite CLS row: an activation left the range of precision %d%s",
                     n, h->cfg.precision,
                     h->cfg.precision == 4 ? " (operands are split into fp16 halves after power-of-two scaling: |GELU / gated-MLP output| < 16 376, "
                                             "|k|, |v| < 16 376, ... - include/cbas_mi355x.h); precision 3 (CBAS_PRECISION=3) computes "
                                             "the same rows in fp32 without a range limit"
                                           : h->cfg.precision == 3 ? "" : " (fp16 activations: |value| < 65 504); precisions 3 / 4 keep them in fp32");
}

extern "C" int cbas_enc_wait(cbas_enc* h, int slot, uint16_t* cls_f16_host, float* cls_f32_host) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null encoder handle");
    if (slot < 0 || slot >= CBAS_ENC_SLOTS) return cbas_fail(CBAS_EINVAL, "slot %d out of range", slot);
    Slot& s = h->slots[slot];
    if (!s.busy) return cbas_fail(CBAS_ESTATE, "slot %d has no submitted work", slot);
    if (s.dev_mode) return cbas_fail(CBAS_ESTATE, "slot %d holds a device submission; use cbas_enc_wait_stream", slot);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipEventSynchronize(s.ev_done));
    if (cls_f16_host) memcpy(cls_f16_host, s.out16_host, (int64_t)s.n * h->D * 2);
    if (cls_f32_host) memcpy(cls_f32_host, s.out32_host, (int64_t)s.n * h->D * 4);
    s.busy = false;
    return cbas_enc_check_finite(h);
}

extern "C" int cbas_enc_profile(cbas_enc* h, int enable) {
    if (!h) return cbas_fail(CBAS_EINVAL, "null encoder handle");
    h->prof_on = enable != 0;
    return CBAS_OK;
}

extern "C" int cbas_enc_profile_read(cbas_enc* h, double* ms_by_cat, int64_t* launches_by_cat, double* flops_by_cat,
                                     int reset) {
    if (!h || !ms_by_cat || !launches_by_cat || !flops_by_cat) return cbas_fail(CBAS_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    for (int c = 0; c < CBAS_PROF_NCAT; ++c) { ms_by_cat[c] = 0; launches_by_cat[c] = 0; flops_by_cat[c] = 0; }
    for (size_t i = 0; i < h->prof_used; ++i) {
        const auto& r = h->prof[i];
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        ms_by_cat[r.cat] += ms;
        launches_by_cat[r.cat] += 1;
        flops_by_cat[r.cat] += r.flops;
    }
    if (reset) h->prof_used = 0;
    return CBAS_OK;
}
