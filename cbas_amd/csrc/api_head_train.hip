// C-ABI: classifier-head trainer (one optimisation step of train_lstm_model, backend/cbas.py:1326-1348).
// See include/cbas_mi355x.h for the contract.  Kernels: head_train_kernels.hip, GEMMs: gemm_f32.hip.
//
// Parameters, gradients and the two Adam moments live in four device arrays of one "train layout":
//   w_proj [NPROJ][I] (rows: cls | delta | acc bottleneck weights, lin1 weight, zero rows)
//   b_bott [3Bn]  ln_w [3Bn]  ln_b [3Bn]  b_lin1 [C^]            (^ = padded to a multiple of 4)
//   w_lin0 [L0][3Bn]  b_lin0 [L0]
//   per LSTM layer: w_ih [8h][in]  b_ih [8h]  b_hh [8h]  w_hh [2][4h][h]   (forward rows, then reverse)
//   w_att [2h]  b_att [4]  gate [4]  att_temp [4]  w_lin2 [C][2h]  b_lin2 [C^]
// so that every weight gradient is the direct output of one GEMM or one column sum.  Padding elements
// have zero gradients and stay zero.  `map` translates to and from the state-dict blob order.
#include <math.h>
#include <string.h>
#include <new>
#include <vector>

#include "api_common.h"
#include "kernels.h"

namespace {
struct MapEntry { int64_t blob_off, train_off, n; };
inline int64_t pad4(int64_t n) { return (n + 3) / 4 * 4; }
inline unsigned long long mix64h(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
}  // namespace

struct cbas_head_trainer {
    cbas_head_config cfg;
    cbas_train_config tcfg;
    int device = 0;
    int I, C, T, Bn, L0, h, NL, lo, hi, NPROJ, F, H2, NS;
    int64_t n_blob = 0, n_train = 0;
    std::vector<MapEntry> map;
    // segment offsets (floats) in the train layout
    int64_t o_wproj, o_bbott, o_lnw, o_lnb, o_blin1, o_wlin0, o_blin0, o_wih[4], o_bih[4], o_bhh[4], o_whh[4], o_watt, o_batt,
        o_gate, o_temp, o_wlin2, o_blin2;
    float *P = nullptr, *G = nullptr, *M = nullptr, *V = nullptr;       // parameters, gradients, Adam moments
    float* cw = nullptr;                                                 // class weights or nullptr
    float *tmat = nullptr, *lin_vec = nullptr;
    int step = 0;
    int64_t Bcap = 0, Rcap = 0, Rp = 0, Bp = 0;
    // activations kept for the backward pass
    float *proj, *Y, *aug, *Z, *xl, *gin, *act[4], *cst[4], *hout[4], *attw, *scores, *latent, *lstm_logits, *final_logits,
        *lin_logits, *b_gate;
    // backward workspaces
    float *terms, *sums, *dfinal, *dlstm, *dlin, *part_pool, *part_exp, *cs_tmp, *dhA, *dhB, *dgin, *hprev, *dxl, *daug, *dproj,
        *XT, *dprojT, *augT, *dZT, *dginT, *xinT, *hprevT, *latentT, *dlogT, *Rc, *RcT, *cov, *Gm, *sq, *dlat_cov, *wlin0T, *wihT,
        *skbuf;                                                          // split-K partial tiles
    float* xg = nullptr;             // [max_batch][T][I] windows gathered by cbas_head_train_step_rows (the step's operand)
    // cbas_head_train_step_rows_multi: the trainer's own stream and the event that orders it against the other trainers of a
    // call; made by the first such call (a trainer stepped on its caller's stream never has them)
    hipStream_t own = nullptr;
    hipEvent_t ev = nullptr;
    std::vector<void*> allocs;
};

namespace {

int gemm_nt(const float* A, int64_t lda, const float* W, int n_alloc, const float* bias, float* out, int64_t ldo, int64_t M,
            int N, int K, hipStream_t st) {
    Gemm32Params g{};
    g.A = A; g.lda = lda; g.W = W; g.bias = bias; g.out = out; g.ldo = ldo; g.M = M; g.N = N; g.N_alloc = n_alloc; g.K = K;
    return launch_gemm_f32(g, 0, st);
}

// Weight-gradient GEMM out[M][N] = A[M][K] W[N][K]^T with K = (windows x seq_len) and a handful of output
// tiles: split K over grid.z and add the partial tiles in a fixed order (deterministic).  K % (32*splits) == 0.
constexpr int K_PAD = 512;             // transposed activations are zero-padded to a multiple of this
int gemm_nt_longk(const float* A, const float* W, int n_alloc, float* out, int M, int N, int64_t K, float* skbuf,
                  hipStream_t st) {
    int splits = 1;
    while (splits < 16 && K / (splits * 2) >= 512 && K % (64 * splits) == 0) splits *= 2;
    if (splits == 1) return gemm_nt(A, K, W, n_alloc, nullptr, out, N, M, N, (int)K, st);
    Gemm32Params g{};
    g.A = A; g.lda = K; g.W = W; g.ldw = K; g.bias = nullptr; g.out = skbuf; g.ldo = N; g.M = M; g.N = N; g.N_alloc = n_alloc;
    g.K = (int)(K / splits); g.splits = splits; g.split_stride = (int64_t)M * N;
    int rc = launch_gemm_f32(g, 0, st);
    if (rc) return rc;
    return launch_splitk_reduce(skbuf, splits, (int64_t)M * N, (int64_t)M * N, out, st);
}

int build_layout(cbas_head_trainer* t) {
    const int64_t I = t->I, C = t->C, Bn = t->Bn, L0 = t->L0, h = t->h;
    int64_t o = 0;
    auto seg = [&](int64_t n) { const int64_t at = o; o += pad4(n); return at; };
    t->o_wproj = seg((int64_t)t->NPROJ * I);
    const int64_t NS = t->NS;
    // b_bott | ln_w | ln_b must be contiguous (one column sum over part_exp fills all three gradients): NS * Bn is a multiple of 4
    t->o_bbott = seg(NS * Bn); t->o_lnw = seg(NS * Bn); t->o_lnb = seg(NS * Bn); t->o_blin1 = seg(C);
    t->o_wlin0 = seg(L0 * NS * Bn); t->o_blin0 = seg(L0);
    for (int l = 0; l < t->NL; ++l) {
        const int64_t in = l == 0 ? L0 : 2 * h;
        t->o_wih[l] = seg(8 * h * in); t->o_bih[l] = seg(8 * h); t->o_bhh[l] = seg(8 * h); t->o_whh[l] = seg(8 * h * h);
    }
    t->o_watt = seg(2 * h); t->o_batt = seg(1); t->o_gate = seg(1); t->o_temp = seg(1);
    t->o_wlin2 = seg(C * 2 * h); t->o_blin2 = seg(C);
    t->n_train = o;
    // blob order (include/cbas_mi355x.h, cbas_head_create) -> train layout
    int64_t b = 0;
    auto put = [&](int64_t train_off, int64_t n) { t->map.push_back({b, train_off, n}); b += n; };
    put(t->o_gate, 1); put(t->o_temp, 1);
    for (int s = 0; s < NS; ++s) { put(t->o_wproj + s * Bn * I, Bn * I); put(t->o_bbott + s * Bn, Bn); }
    for (int s = 0; s < NS; ++s) { put(t->o_lnw + s * Bn, Bn); put(t->o_lnb + s * Bn, Bn); }
    put(t->o_wlin0, L0 * NS * Bn); put(t->o_blin0, L0);
    put(t->o_wproj + NS * Bn * I, C * I); put(t->o_blin1, C);
    for (int l = 0; l < t->NL; ++l) {
        const int64_t in = l == 0 ? L0 : 2 * h;
        for (int dir = 0; dir < 2; ++dir) {
            put(t->o_wih[l] + dir * 4 * h * in, 4 * h * in);
            put(t->o_whh[l] + dir * 4 * h * h, 4 * h * h);
            put(t->o_bih[l] + dir * 4 * h, 4 * h);
            put(t->o_bhh[l] + dir * 4 * h, 4 * h);
        }
    }
    put(t->o_watt, 2 * h); put(t->o_batt, 1); put(t->o_wlin2, C * 2 * h); put(t->o_blin2, C);
    t->n_blob = b;
    return 0;
}

// temporal operators of _calculate_robust_deltas (classifier_head.py:102-117) as T x T matrices, in double
void build_temporal(int T, double alpha, int lo, int hi, std::vector<float>& tmat, std::vector<float>& lin_vec) {
    std::vector<double> E((size_t)T * T, 0.0), D((size_t)T * T, 0.0), A((size_t)T * T, 0.0);
    E[0] = 1.0;
    for (int t = 1; t < T; ++t) {
        for (int s = 0; s < T; ++s) E[(size_t)t * T + s] = (1.0 - alpha) * E[(size_t)(t - 1) * T + s];
        E[(size_t)t * T + t] += alpha;
    }
    auto row = [&](std::vector<double>& m, int t) { return &m[(size_t)t * T]; };
    for (int s = 0; s < T; ++s) {
        row(D, 0)[s] = row(E, 0)[s] - row(E, 1)[s];                                     // reflect pad: s0 - s1
        row(A, 0)[s] = row(E, 0)[s] - 2.0 * row(E, 1)[s] + row(E, 2)[s];
        row(A, 1)[s] = 2.0 * (row(E, 1)[s] - row(E, 0)[s]);
        for (int t = 1; t < T; ++t) row(D, t)[s] = row(E, t)[s] - row(E, t - 1)[s];
        for (int t = 2; t < T; ++t) row(A, t)[s] = row(E, t)[s] - 2.0 * row(E, t - 1)[s] + row(E, t - 2)[s];
    }
    tmat.resize(3 * (size_t)T * T);
    for (size_t i = 0; i < (size_t)T * T; ++i) { tmat[i] = (float)E[i]; tmat[(size_t)T * T + i] = (float)D[i]; tmat[2 * (size_t)T * T + i] = (float)A[i]; }
    lin_vec.assign(T, 0.f);
    for (int s = 0; s < T; ++s) {
        double v = 0.0;
        for (int t = lo; t < hi; ++t) v += E[(size_t)t * T + s];
        lin_vec[s] = (float)(v / (double)(hi - lo));
    }
}

// Device side of cbas_head_train_create: every buffer of the handle, zero-filled, and the parameters in the train layout.
// On a non-zero return the caller destroys the handle, which frees what t->allocs holds by then.
int trainer_init(cbas_head_trainer* t, const float* weights_host, const float* class_weights_host) {
    auto dalloc = [&](float** p, int64_t n) -> hipError_t {
        hipError_t e = hipMalloc((void**)p, (size_t)(n > 0 ? n : 1) * sizeof(float));
        if (e == hipSuccess) { t->allocs.push_back(*p); e = hipMemset(*p, 0, (size_t)(n > 0 ? n : 1) * sizeof(float)); }
        return e;
    };
    const int T = t->T;
    const int64_t B = t->tcfg.max_batch, R = B * T, Rp = round_up(R, K_PAD), Bp = round_up(B, 32);
    t->Bcap = B; t->Rcap = R; t->Rp = Rp; t->Bp = Bp;
    const int64_t I = t->I, C = t->C, F = t->F, L0 = t->L0, h = t->h, H2 = t->H2, NP = t->NPROJ, nc = t->hi - t->lo;
    ALLOC_TRY(dalloc(&t->P, t->n_train)); ALLOC_TRY(dalloc(&t->G, t->n_train)); ALLOC_TRY(dalloc(&t->M, t->n_train)); ALLOC_TRY(dalloc(&t->V, t->n_train));
    {   // parameters: blob -> train layout
        std::vector<float> host((size_t)t->n_train, 0.f);
        for (const MapEntry& e : t->map) memcpy(host.data() + e.train_off, weights_host + e.blob_off, (size_t)e.n * sizeof(float));
        ALLOC_TRY(hipMemcpy(t->P, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (class_weights_host) {
        ALLOC_TRY(dalloc(&t->cw, C));
        ALLOC_TRY(hipMemcpy(t->cw, class_weights_host, (size_t)C * sizeof(float), hipMemcpyHostToDevice));
    }
    {
        std::vector<float> tm, lv;
        build_temporal(T, (double)t->cfg.ema_alpha, t->lo, t->hi, tm, lv);
        ALLOC_TRY(dalloc(&t->tmat, (int64_t)tm.size())); ALLOC_TRY(dalloc(&t->lin_vec, T));
        ALLOC_TRY(hipMemcpy(t->tmat, tm.data(), tm.size() * sizeof(float), hipMemcpyHostToDevice));
        ALLOC_TRY(hipMemcpy(t->lin_vec, lv.data(), lv.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    ALLOC_TRY(dalloc(&t->proj, R * NP)); ALLOC_TRY(dalloc(&t->Y, R * F)); ALLOC_TRY(dalloc(&t->aug, R * F));
    ALLOC_TRY(dalloc(&t->Z, R * L0)); ALLOC_TRY(dalloc(&t->xl, R * L0)); ALLOC_TRY(dalloc(&t->gin, R * 8 * h));
    for (int l = 0; l < t->NL; ++l) {
        ALLOC_TRY(dalloc(&t->act[l], R * 8 * h)); ALLOC_TRY(dalloc(&t->cst[l], R * H2)); ALLOC_TRY(dalloc(&t->hout[l], R * H2));
    }
    ALLOC_TRY(dalloc(&t->attw, B * nc)); ALLOC_TRY(dalloc(&t->scores, B * nc)); ALLOC_TRY(dalloc(&t->latent, B * H2));
    ALLOC_TRY(dalloc(&t->lstm_logits, B * C)); ALLOC_TRY(dalloc(&t->final_logits, B * C)); ALLOC_TRY(dalloc(&t->lin_logits, B * C));
    ALLOC_TRY(dalloc(&t->b_gate, 8 * h));
    ALLOC_TRY(dalloc(&t->terms, B * 2)); ALLOC_TRY(dalloc(&t->sums, 8)); ALLOC_TRY(dalloc(&t->dfinal, B * C)); ALLOC_TRY(dalloc(&t->dlstm, B * C));
    ALLOC_TRY(dalloc(&t->dlin, B * C)); ALLOC_TRY(dalloc(&t->part_pool, B * (H2 + 12))); ALLOC_TRY(dalloc(&t->part_exp, B * 3 * F));
    const int64_t max_cols = 8 * h > 3 * F ? 8 * h : 3 * F;
    ALLOC_TRY(dalloc(&t->cs_tmp, COLSUM_CHUNKS * max_cols));
    ALLOC_TRY(dalloc(&t->dhA, R * H2)); ALLOC_TRY(dalloc(&t->dhB, R * H2)); ALLOC_TRY(dalloc(&t->dgin, R * 8 * h)); ALLOC_TRY(dalloc(&t->hprev, R * H2));
    ALLOC_TRY(dalloc(&t->dxl, R * L0)); ALLOC_TRY(dalloc(&t->daug, R * F)); ALLOC_TRY(dalloc(&t->dproj, R * NP));
    ALLOC_TRY(dalloc(&t->XT, I * Rp)); ALLOC_TRY(dalloc(&t->dprojT, NP * Rp)); ALLOC_TRY(dalloc(&t->augT, F * Rp)); ALLOC_TRY(dalloc(&t->dZT, L0 * Rp));
    ALLOC_TRY(dalloc(&t->dginT, 8 * h * Rp)); ALLOC_TRY(dalloc(&t->xinT, (L0 > H2 ? L0 : H2) * Rp)); ALLOC_TRY(dalloc(&t->hprevT, H2 * Rp));
    ALLOC_TRY(dalloc(&t->latentT, H2 * Bp)); ALLOC_TRY(dalloc(&t->dlogT, pad4(C) * Bp)); ALLOC_TRY(dalloc(&t->Rc, B * H2)); ALLOC_TRY(dalloc(&t->RcT, H2 * Bp));
    ALLOC_TRY(dalloc(&t->cov, H2 * H2)); ALLOC_TRY(dalloc(&t->Gm, H2 * H2)); ALLOC_TRY(dalloc(&t->sq, H2)); ALLOC_TRY(dalloc(&t->dlat_cov, B * H2));
    ALLOC_TRY(dalloc(&t->wlin0T, F * L0)); ALLOC_TRY(dalloc(&t->wihT, (L0 > H2 ? L0 : H2) * 8 * h));
    {
        int64_t mx = (int64_t)NP * I;
        if (L0 * F > mx) mx = L0 * F;
        if (8 * h * (L0 > H2 ? L0 : H2) > mx) mx = 8 * h * (L0 > H2 ? L0 : H2);
        ALLOC_TRY(dalloc(&t->skbuf, 16 * mx));
    }
    ALLOC_TRY(dalloc(&t->xg, R * I));    // filled below like every other buffer: ordered before the handle is handed out
    // dalloc zero-fills with hipMemset on the NULL stream, which may return before the fill has run, and the training step is
    // queued on the caller's stream - in CBAS a torch stream, NON-BLOCKING, hence not ordered after the null stream: beside a
    // busy encoder the fills of G / M / V landed after the first steps had written them (r5: 114 of 125 forty-step runs
    // beside encoder passes ended with other weights than the idle-device run; scripts/train_beside_encoder.py).  The handle
    // is only handed out once every fill has completed.
    ALLOC_TRY(hipStreamSynchronize(nullptr));
    return CBAS_OK;
}

}  // namespace

// build_temporal for the debug harness (kernels.h): tmat [3][T][T] and lin_vec [T] as a trainer of this shape uploads them
void head_build_temporal(int T, double alpha, int lo, int hi, float* tmat, float* lin_vec) {
    std::vector<float> tm, lv;
    build_temporal(T, alpha, lo, hi, tm, lv);
    memcpy(tmat, tm.data(), tm.size() * sizeof(float));
    memcpy(lin_vec, lv.data(), lv.size() * sizeof(float));
}

extern "C" void cbas_head_train_destroy(cbas_head_trainer* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    (void)hipDeviceSynchronize();
    if (t->ev) (void)hipEventDestroy(t->ev);
    if (t->own) (void)hipStreamDestroy(t->own);
    for (void* p : t->allocs)
        if (p) (void)hipFree(p);
    delete t;
}

extern "C" int cbas_head_train_create(const cbas_head_config* cfg, const cbas_train_config* tcfg, const float* weights_host,
                                      int64_t n_weights, const float* class_weights_host, int device_id,
                                      cbas_head_trainer** out) {
    if (!cfg || !tcfg || !weights_host || !out) return cbas_fail(CBAS_EINVAL, "null argument");
    *out = nullptr;
    const cbas_head_config& c = *cfg;
    if (c.in_features <= 0 || c.in_features % 32) return cbas_fail(CBAS_EINVAL, "in_features=%d must be a positive multiple of 32", c.in_features);
    if (c.out_features <= 0 || c.out_features > 64) return cbas_fail(CBAS_EINVAL, "out_features=%d outside [1,64]", c.out_features);
    if (c.bottleneck_dim % 64 || c.bottleneck_dim <= 0 || c.bottleneck_dim > 256) return cbas_fail(CBAS_EINVAL, "bottleneck_dim=%d unsupported", c.bottleneck_dim);
    if (c.lin0_dim % 32 || c.lin0_dim <= 0) return cbas_fail(CBAS_EINVAL, "lin0_dim=%d must be a multiple of 32", c.lin0_dim);
    if (c.lstm_hidden_size < 16 || c.lstm_hidden_size > 128 || c.lstm_hidden_size % 16)
        return cbas_fail(CBAS_EINVAL, "lstm_hidden_size=%d: multiples of 16 from 16 to 128 are built", c.lstm_hidden_size);
    if (c.seq_len < 3 || c.seq_len > 101) return cbas_fail(CBAS_EINVAL, "seq_len=%d outside [3,101]", c.seq_len);
    if (c.lstm_layers < 1 || c.lstm_layers > 4) return cbas_fail(CBAS_EINVAL, "lstm_layers=%d outside [1,4]", c.lstm_layers);
    if (tcfg->max_batch < 1 || tcfg->max_batch > 65536) return cbas_fail(CBAS_EINVAL, "max_batch=%d outside [1,65536]", tcfg->max_batch);
    if (!(tcfg->lr > 0.f) || tcfg->weight_decay < 0.f || tcfg->label_smoothing < 0.f || tcfg->label_smoothing >= 1.f)
        return cbas_fail(CBAS_EINVAL, "bad hyper-parameters (lr=%g weight_decay=%g label_smoothing=%g)", tcfg->lr, tcfg->weight_decay, tcfg->label_smoothing);
    const int T = c.seq_len, hsl = T / 2, sw = c.center_window_size;
    const int lo = hsl - sw > 0 ? hsl - sw : 0, hi = hsl + sw + 1 < T ? hsl + sw + 1 : T;
    if (lo >= hi) return cbas_fail(CBAS_EINVAL, "empty centre window (seq_len=%d, center_window_size=%d)", T, sw);
    if (n_weights != cbas_head_weights_count(cfg))
        return cbas_fail(CBAS_EINVAL, "weights blob has %lld floats, config needs %lld", (long long)n_weights, (long long)cbas_head_weights_count(cfg));
    HIP_TRY(hipSetDevice(device_id));

    cbas_head_trainer* t = new (std::nothrow) cbas_head_trainer();
    if (!t) return cbas_fail(CBAS_ENOMEM, "out of host memory");
    t->cfg = c; t->tcfg = *tcfg; t->device = device_id;
    t->I = c.in_features; t->C = c.out_features; t->T = T; t->Bn = c.bottleneck_dim; t->L0 = c.lin0_dim; t->h = c.lstm_hidden_size;
    t->NS = c.use_acceleration ? 3 : 2;                        // bottleneck streams (classifier_head.py:74-84)
    t->NL = c.lstm_layers; t->lo = lo; t->hi = hi; t->F = t->NS * t->Bn; t->H2 = 2 * t->h;
    t->NPROJ = (int)round_up(t->F + t->C, 4);
    build_layout(t);
    if (t->n_blob != n_weights) { delete t; return cbas_fail(CBAS_EINVAL, "internal blob layout mismatch"); }
    if (train_expand_lds_bytes(T, t->Bn, t->NPROJ) > 160 * 1024) {
        delete t;
        return cbas_fail(CBAS_EINVAL, "seq_len=%d too long for the training kernels (window does not fit the 160 KiB LDS)", T);
    }

    const int rc = trainer_init(t, weights_host, class_weights_host);
    if (rc != CBAS_OK) {
        cbas_head_train_destroy(t);      // never touches the error text: the failing call's message stands
        return rc;
    }
    *out = t;
    return CBAS_OK;
}

namespace {

// One trainer's part of a step.  cbas_head_train_step runs one Job on the caller's stream; cbas_head_train_step_rows_multi
// runs k of them in lockstep, each on its trainer's own stream.
struct Job {
    cbas_head_trainer* t;
    const float* x;                  // [B][T][I]
    const int32_t* labels;
    hipStream_t st;
    int64_t B, R, Rp, Bp;
    bool use_cov;                    // cbas.py:1340
    float cov_inv;                   // 1 / (B - 1)
    unsigned long long key[4];       // dropout streams of this step (oracle/head_train_oracle.py: dropout_keep)
    unsigned thr_b, thr_l;
    float sc_b, sc_l;
    TrainExpandParams ep;
    TrainPoolParams pp;
    float *dh_cur, *dh_next;
};

void bind_job(Job& c) {
    cbas_head_trainer* t = c.t;
    c.R = c.B * t->T; c.Rp = round_up(c.R, K_PAD); c.Bp = round_up(c.B, 32); c.use_cov = c.B > 1;
    c.cov_inv = c.use_cov ? 1.0f / (float)(c.B - 1) : 0.f;
    const bool drop = t->tcfg.dropout != 0;
    for (int s = 0; s < 4; ++s) c.key[s] = mix64h(t->tcfg.seed ^ mix64h((unsigned long long)t->step * 4ull + (unsigned long long)s));
    c.thr_b = drop ? (unsigned)floor(0.1 * 16777216.0) : 0u; c.thr_l = drop ? (unsigned)floor(0.15 * 16777216.0) : 0u;
    c.sc_b = drop ? (float)(1.0 / (1.0 - 0.1)) : 1.0f; c.sc_l = drop ? (float)(1.0 / (1.0 - 0.15)) : 1.0f;
    float* P = t->P;
    TrainExpandParams& ep = c.ep;
    ep = TrainExpandParams{};
    ep.proj = t->proj; ep.tmat = t->tmat; ep.lin_vec = t->lin_vec; ep.b_bott = P + t->o_bbott; ep.ln_w = P + t->o_lnw;
    ep.ln_b = P + t->o_lnb; ep.b_lin1 = P + t->o_blin1; ep.T = t->T; ep.Bn = t->Bn; ep.NPROJ = t->NPROJ; ep.C = t->C; ep.NS = t->NS;
    for (int s = 0; s < 3; ++s) ep.key[s] = c.key[s];
    ep.thr = c.thr_b; ep.scale = c.sc_b;
    TrainPoolParams& pp = c.pp;
    pp = TrainPoolParams{};
    pp.hout = t->hout[t->NL - 1]; pp.lin_logits = t->lin_logits; pp.w_att = P + t->o_watt; pp.b_att = P + t->o_batt;
    pp.att_temp = P + t->o_temp; pp.w_lin2 = P + t->o_wlin2; pp.b_lin2 = P + t->o_blin2; pp.gate = P + t->o_gate;
    pp.T = t->T; pp.H2 = t->H2; pp.C = t->C; pp.lo = t->lo; pp.hi = t->hi;
    c.dh_cur = t->dhA; c.dh_next = t->dhB;
}

// The k jobs of one step and the two ways their launches are queued.  The LSTM, expand and pool kernels, the transposes and
// the GEMMs go out per trainer on jobs[j].st and overlap there (`each`).  The small kernels - Adam, the column sums, the
// cross-entropy pair, cov_offdiag, add / copy, GELU + dropout - go out as ONE launch for all k on the leading stream
// jobs[0].st, with trainer j's operands in entry j of the kernel's table (`batched`).  `join` orders the leading stream
// behind every trainer's with one event each, `fork` orders every trainer's stream behind it again; launches of one kind
// that follow each other need neither, and for k = 1 both do nothing: everything is queued on the one stream.
// A table of one goes out through the single-trial launcher of head_train_kernels.hip, whose kernel takes the operands as
// plain arguments: measured 0.012 ms per solo step (0.75 %) faster than the table form at k = 1, same bytes.
// Every call returns the step's status and queues nothing once that is not CBAS_OK: a step is a list of calls.
struct Step {
    Job* jobs;
    int k;
    int rc = CBAS_OK;
    bool joined = false;
    hipStream_t lead() const { return jobs[0].st; }

    int join() {
        if (joined || k == 1) return CBAS_OK;
        for (int j = 1; j < k; ++j) {
            HIP_TRY(hipEventRecord(jobs[j].t->ev, jobs[j].st));
            HIP_TRY(hipStreamWaitEvent(lead(), jobs[j].t->ev, 0));
        }
        joined = true;
        return CBAS_OK;
    }
    int fork() {
        if (!joined) return CBAS_OK;
        HIP_TRY(hipEventRecord(jobs[0].t->ev, lead()));
        for (int j = 1; j < k; ++j) HIP_TRY(hipStreamWaitEvent(jobs[j].st, jobs[0].t->ev, 0));
        joined = false;
        return CBAS_OK;
    }
    // launches(job, job.t), once per trainer, queue on job.st
    template <class Launches>
    int each(Launches launches) {
        if (rc == CBAS_OK) rc = fork();
        for (int j = 0; j < k && rc == CBAS_OK; ++j) rc = launches(jobs[j], jobs[j].t);
        return rc;
    }
    // fill(j, job) writes entry j of a table (an entry left alone has the count 0 and takes no part); launch() queues the
    // table's kernel on the leading stream
    template <class Fill, class Launch>
    int batched(Fill fill, Launch launch) {
        if (rc == CBAS_OK) rc = join();
        if (rc != CBAS_OK) return rc;
        for (int j = 0; j < k; ++j) fill(j, jobs[j]);
        return rc = launch();
    }
};

// ---- the small kernels of a step: one table per launch, the operands spelled once ----
int gelu_dropout(Step& s, int backward) {        // lin0's activation: xl = dropout(gelu(Z)); backward: dxl becomes dZ in place
    GeluBatch b{};
    return s.batched(
        [&](int j, Job& c) {
            b.Z[j] = c.t->Z; b.io[j] = backward ? c.t->dxl : c.t->xl; b.n[j] = c.R * c.t->L0;
            b.key[j] = c.key[3]; b.thr[j] = c.thr_l; b.scale[j] = c.sc_l;
        },
        [&]() -> int {
            if (s.k > 1) LAUNCH_TRY(launch_gelu_dropout_multi(b, s.k, backward, s.lead()));
            else LAUNCH_TRY(launch_gelu_dropout(b.Z[0], b.io[0], b.n[0], b.key[0], b.thr[0], b.scale[0], backward, s.lead()));
            return CBAS_OK;
        });
}

int cross_entropy(Step& s, int grad) {           // final_logits -> terms; grad: final_logits, sums[0..1] -> dfinal
    CeBatch b{};
    return s.batched(
        [&](int j, Job& c) {
            b.logits[j] = c.t->final_logits; b.labels[j] = c.labels; b.cw[j] = c.t->cw; b.sums[j] = c.t->sums; b.n[j] = c.B;
            b.C[j] = c.t->C; b.eps[j] = c.t->tcfg.label_smoothing; b.out[j] = grad ? c.t->dfinal : c.t->terms;
        },
        [&]() -> int {
            if (s.k > 1) LAUNCH_TRY(launch_ce_multi(b, s.k, grad, s.lead()));
            else if (grad) LAUNCH_TRY(launch_ce_grad(b.logits[0], b.labels[0], b.cw[0], b.sums[0], b.n[0], b.C[0], b.eps[0], b.out[0], s.lead()));
            else LAUNCH_TRY(launch_ce_terms(b.logits[0], b.labels[0], b.cw[0], b.n[0], b.C[0], b.eps[0], b.out[0], s.lead()));
            return CBAS_OK;
        });
}

int cov_offdiag(Step& s) {                       // cov -> Gm, sq; only the trainers with a covariance penalty
    CovBatch b{};
    return s.batched(
        [&](int j, Job& c) {
            if (!c.use_cov) return;
            b.cov[j] = c.t->cov; b.n[j] = c.t->H2; b.cscale[j] = c.cov_inv; b.gscale[j] = 4.0f * c.cov_inv; b.G[j] = c.t->Gm;
            b.sq[j] = c.t->sq;
        },
        [&]() -> int {
            if (s.k > 1) LAUNCH_TRY(launch_cov_offdiag_multi(b, s.k, s.lead()));
            else if (b.n[0]) LAUNCH_TRY(launch_cov_offdiag(b.cov[0], b.n[0], b.cscale[0], b.gscale[0], b.G[0], b.sq[0], s.lead()));
            return CBAS_OK;
        });
}

struct Cols { const float* src; int64_t rows; int cols; float* dst; };      // cols = 0: the trainer takes no part
template <class Of>
int colsum(Step& s, Of of) {                     // of(job, job.t): that trainer's column sum, dst [cols] = sum_r src [r][cols]
    ColsumBatch b{};
    return s.batched(
        [&](int j, Job& c) {
            const Cols o = of(c, c.t);
            if (!o.cols) return;
            b.src[j] = o.src; b.rows[j] = o.rows; b.cols[j] = o.cols; b.ld[j] = o.cols; b.tmp[j] = c.t->cs_tmp; b.dst[j] = o.dst;
        },
        [&]() -> int {
            if (s.k > 1) LAUNCH_TRY(launch_colsum_multi(b, s.k, s.lead()));
            else if (b.cols[0]) LAUNCH_TRY(launch_colsum(b.src[0], b.rows[0], b.cols[0], b.ld[0], 1.0f, b.tmp[0], b.dst[0], s.lead()));
            return CBAS_OK;
        });
}

int add_lstm_biases(Step& s, int l, int backward) {   // b_gate = b_ih + b_hh; backward: d b_hh = d b_ih
    VecBatch b{};
    return s.batched(
        [&](int j, Job& c) {
            cbas_head_trainer* t = c.t;
            b.a[j] = (backward ? t->G : t->P) + t->o_bih[l]; b.b[j] = backward ? nullptr : t->P + t->o_bhh[l];
            b.out[j] = backward ? t->G + t->o_bhh[l] : t->b_gate; b.n[j] = 8 * t->h;
        },
        [&]() -> int {
            if (s.k > 1) LAUNCH_TRY(launch_add_vec_multi(b, s.k, s.lead()));
            else LAUNCH_TRY(launch_add_vec(b.a[0], b.b[0], b.out[0], b.n[0], s.lead()));
            return CBAS_OK;
        });
}

int adam(Step& s) {
    AdamBatch b{};
    b.wd_special = 1e-3f;                                                                       // cbas.py:1307
    return s.batched(
        [&](int j, Job& c) {
            cbas_head_trainer* t = c.t;
            b.p[j] = t->P; b.g[j] = t->G; b.m[j] = t->M; b.v[j] = t->V; b.n[j] = t->n_train; b.wd[j] = t->tcfg.weight_decay;
            b.wd_lo[j] = t->o_gate; b.wd_hi[j] = t->o_gate + 1;
            adam_bias_corrections(t->tcfg.lr, t->step + 1, &b.lr_c1[j], &b.inv_sqrt_c2[j]);
        },
        [&]() -> int {
            const cbas_head_trainer* t = s.jobs[0].t;
            if (s.k > 1) LAUNCH_TRY(launch_adam_step_multi(b, s.k, s.lead()));
            else LAUNCH_TRY(launch_adam_step(b.p[0], b.g[0], b.m[0], b.v[0], b.n[0], t->tcfg.lr, b.wd[0], b.wd_lo[0], b.wd_hi[0], b.wd_special,
                                             t->step + 1, s.lead()));
            return CBAS_OK;
        });
}

// The step of k trainers that share one head configuration (k = 1: the one trainer of cbas_head_train_step, on the caller's
// stream).  The call returns forked, so each stream alone orders the next step.
int step_jobs(Job* jobs, const int k, const int update) {
    const cbas_head_trainer* cfg = jobs[0].t;
    const int I = cfg->I, C = cfg->C, T = cfg->T, L0 = cfg->L0, h = cfg->h, F = cfg->F, H2 = cfg->H2, NP = cfg->NPROJ, NL = cfg->NL;
    Step s{jobs, k};

    // ---------------- forward ----------------
    s.each([&](Job& c, cbas_head_trainer* t) -> int {
        LAUNCH_TRY(gemm_nt(c.x, I, t->P + t->o_wproj, NP, nullptr, t->proj, NP, c.R, NP, I, c.st));
        LAUNCH_TRY(launch_train_expand_fwd(c.ep, c.B, t->Y, t->aug, t->lin_logits, c.st));
        LAUNCH_TRY(gemm_nt(t->aug, F, t->P + t->o_wlin0, L0, t->P + t->o_blin0, t->Z, L0, c.R, L0, F, c.st));
        return CBAS_OK;
    });
    gelu_dropout(s, 0);
    s.each([&](Job& c, cbas_head_trainer* t) -> int { LAUNCH_TRY(launch_head_centre(t->xl, c.B, T, L0, c.st)); return CBAS_OK; });
    for (int l = 0; l < NL; ++l) {
        const int in = l == 0 ? L0 : H2;
        add_lstm_biases(s, l, 0);
        s.each([&](Job& c, cbas_head_trainer* t) -> int {
            LAUNCH_TRY(gemm_nt(l == 0 ? t->xl : t->hout[l - 1], in, t->P + t->o_wih[l], 8 * h, t->b_gate, t->gin, 8 * h, c.R, 8 * h, in, c.st));
            LAUNCH_TRY(launch_lstm_train_fwd(t->gin, t->P + t->o_whh[l], h, T, c.B, t->act[l], t->cst[l], t->hout[l], c.st));
            return CBAS_OK;
        });
    }
    s.each([&](Job& c, cbas_head_trainer* t) -> int {
        LAUNCH_TRY(launch_pool_train_fwd(c.pp, c.B, t->attw, t->scores, t->latent, t->lstm_logits, t->final_logits, c.st));
        return CBAS_OK;
    });

    // ---------------- loss ----------------
    cross_entropy(s, 0);
    colsum(s, [&](Job& c, cbas_head_trainer* t) { return Cols{t->terms, c.B, 2, t->sums}; });                  // sums[0..1]
    cross_entropy(s, 1);
    colsum(s, [&](Job& c, cbas_head_trainer* t) { return c.use_cov ? Cols{t->latent, c.B, H2, t->sq} : Cols{}; });     // column sums (sq as scratch)
    s.each([&](Job& c, cbas_head_trainer* t) -> int {
        if (!c.use_cov) return CBAS_OK;
        LAUNCH_TRY(launch_sub_colmean(t->latent, t->sq, c.B, H2, t->Rc, c.st));
        LAUNCH_TRY(launch_transpose_pad(t->Rc, c.B, H2, H2, t->RcT, c.Bp, c.st));
        LAUNCH_TRY(gemm_nt(t->RcT, c.Bp, t->RcT, H2, nullptr, t->cov, H2, H2, H2, (int)c.Bp, c.st));
        return CBAS_OK;
    });
    cov_offdiag(s);
    colsum(s, [&](Job& c, cbas_head_trainer* t) { return c.use_cov ? Cols{t->sq, H2, 1, t->sums + 2} : Cols{}; });     // sums[2] = covariance penalty
    s.each([&](Job& c, cbas_head_trainer* t) -> int {
        if (c.use_cov) LAUNCH_TRY(gemm_nt(t->Rc, H2, t->Gm, H2, nullptr, t->dlat_cov, H2, c.B, H2, H2, c.st));
        else HIP_TRY(hipMemsetAsync(t->sums + 2, 0, sizeof(float), c.st));
        return CBAS_OK;
    });

    // ---------------- backward ----------------
    s.each([&](Job& c, cbas_head_trainer* t) -> int {
        LAUNCH_TRY(launch_pool_train_bwd(c.pp, c.B, t->attw, t->scores, t->lstm_logits, t->dfinal, c.use_cov ? t->dlat_cov : nullptr,
                                         t->dhA, t->dlstm, t->dlin, t->part_pool, c.st));
        return CBAS_OK;
    });
    // w_att | b_att | gate | att_temp are contiguous in the layout and in part_pool's row
    colsum(s, [&](Job& c, cbas_head_trainer* t) { return Cols{t->part_pool, c.B, H2 + 12, t->G + t->o_watt}; });
    colsum(s, [&](Job& c, cbas_head_trainer* t) { return Cols{t->dlstm, c.B, C, t->G + t->o_blin2}; });
    colsum(s, [&](Job& c, cbas_head_trainer* t) { return Cols{t->dlin, c.B, C, t->G + t->o_blin1}; });
    s.each([&](Job& c, cbas_head_trainer* t) -> int {
        LAUNCH_TRY(launch_transpose_pad(t->dlstm, c.B, C, C, t->dlogT, c.Bp, c.st));
        LAUNCH_TRY(launch_transpose_pad(t->latent, c.B, H2, H2, t->latentT, c.Bp, c.st));
        LAUNCH_TRY(gemm_nt(t->dlogT, c.Bp, t->latentT, H2, nullptr, t->G + t->o_wlin2, H2, C, H2, (int)c.Bp, c.st));
        return CBAS_OK;
    });

    for (int l = NL - 1; l >= 0; --l) {
        const int in = l == 0 ? L0 : H2;
        s.each([&](Job& c, cbas_head_trainer* t) -> int {
            LAUNCH_TRY(launch_lstm_train_bwd(c.dh_cur, t->act[l], t->cst[l], t->hout[l], t->P + t->o_whh[l], h, T, c.B, t->dgin, t->hprev, c.st));
            return CBAS_OK;
        });
        colsum(s, [&](Job& c, cbas_head_trainer* t) { return Cols{t->dgin, c.R, 8 * h, t->G + t->o_bih[l]}; });
        add_lstm_biases(s, l, 1);
        s.each([&](Job& c, cbas_head_trainer* t) -> int {
            const float* xin = l == 0 ? t->xl : t->hout[l - 1];
            LAUNCH_TRY(launch_transpose_pad(t->dgin, c.R, 8 * h, 8 * h, t->dginT, c.Rp, c.st));
            LAUNCH_TRY(launch_transpose_pad(t->hprev, c.R, H2, H2, t->hprevT, c.Rp, c.st));
            LAUNCH_TRY(launch_transpose_pad(xin, c.R, in, in, t->xinT, c.Rp, c.st));
            for (int dir = 0; dir < 2; ++dir)
                LAUNCH_TRY(gemm_nt_longk(t->dginT + (int64_t)dir * 4 * h * c.Rp, t->hprevT + (int64_t)dir * h * c.Rp, h,
                                         t->G + t->o_whh[l] + (int64_t)dir * 4 * h * h, 4 * h, h, c.Rp, t->skbuf, c.st));
            LAUNCH_TRY(gemm_nt_longk(t->dginT, t->xinT, in, t->G + t->o_wih[l], 8 * h, in, c.Rp, t->skbuf, c.st));
            LAUNCH_TRY(launch_transpose_pad(t->P + t->o_wih[l], 8 * h, in, in, t->wihT, 8 * h, c.st));      // [in][8h]
            LAUNCH_TRY(gemm_nt(t->dgin, 8 * h, t->wihT, in, nullptr, l == 0 ? t->dxl : c.dh_next, in, c.R, in, 8 * h, c.st));
            float* tmp = c.dh_cur; c.dh_cur = c.dh_next; c.dh_next = tmp;
            return CBAS_OK;
        });
    }
    // centring (classifier_head.py:166-167) is its own adjoint: d x = d xc - mean_t(d xc)
    s.each([&](Job& c, cbas_head_trainer* t) -> int { LAUNCH_TRY(launch_head_centre(t->dxl, c.B, T, L0, c.st)); return CBAS_OK; });
    gelu_dropout(s, 1);                                                                         // dxl is now dZ
    colsum(s, [&](Job& c, cbas_head_trainer* t) { return Cols{t->dxl, c.R, L0, t->G + t->o_blin0}; });
    s.each([&](Job& c, cbas_head_trainer* t) -> int {
        LAUNCH_TRY(launch_transpose_pad(t->dxl, c.R, L0, L0, t->dZT, c.Rp, c.st));
        LAUNCH_TRY(launch_transpose_pad(t->aug, c.R, F, F, t->augT, c.Rp, c.st));
        LAUNCH_TRY(gemm_nt_longk(t->dZT, t->augT, F, t->G + t->o_wlin0, L0, F, c.Rp, t->skbuf, c.st));
        LAUNCH_TRY(launch_transpose_pad(t->P + t->o_wlin0, L0, F, F, t->wlin0T, L0, c.st));      // [F][L0]
        LAUNCH_TRY(gemm_nt(t->dxl, L0, t->wlin0T, F, nullptr, t->daug, F, c.R, F, L0, c.st));
        LAUNCH_TRY(launch_train_expand_bwd(c.ep, c.B, t->Y, t->daug, t->dlin, t->dproj, t->part_exp, c.st));
        return CBAS_OK;
    });
    // b_bott | ln_w | ln_b are contiguous in the layout and in part_exp's row
    colsum(s, [&](Job& c, cbas_head_trainer* t) { return Cols{t->part_exp, c.B, 3 * F, t->G + t->o_bbott}; });
    s.each([&](Job& c, cbas_head_trainer* t) -> int {
        LAUNCH_TRY(launch_transpose_pad(t->dproj, c.R, NP, NP, t->dprojT, c.Rp, c.st));
        LAUNCH_TRY(launch_transpose_pad(c.x, c.R, I, I, t->XT, c.Rp, c.st));
        LAUNCH_TRY(gemm_nt_longk(t->dprojT, t->XT, I, t->G + t->o_wproj, NP, I, c.Rp, t->skbuf, c.st));
        return CBAS_OK;
    });

    if (update && adam(s) == CBAS_OK)
        for (int j = 0; j < k; ++j) jobs[j].t->step += 1;
    if (s.rc == CBAS_OK) s.rc = s.fork();
    return s.rc;
}

void read_loss(const float* s, float* loss_host) {
    loss_host[1] = s[0] / s[1];
    loss_host[2] = s[2];
    loss_host[0] = loss_host[1] + loss_host[2];
}

}  // namespace

extern "C" int cbas_head_train_step(cbas_head_trainer* t, const float* x_dev, const int32_t* labels_dev, int32_t n_windows,
                                    int32_t update, float* loss_host, void* stream) {
    if (!t) return cbas_fail(CBAS_EINVAL, "null trainer handle");
    if (!x_dev || !labels_dev) return cbas_fail(CBAS_EINVAL, "x_dev / labels_dev NULL");
    if (n_windows < 1 || n_windows > t->Bcap) return cbas_fail(CBAS_EINVAL, "n_windows=%d outside [1, max_batch=%lld]", n_windows, (long long)t->Bcap);
    HIP_TRY(hipSetDevice(t->device));
    hipStream_t st = (hipStream_t)stream;
    Job job{};
    job.t = t; job.x = x_dev; job.labels = labels_dev; job.st = st; job.B = n_windows;
    bind_job(job);
    const int rc = step_jobs(&job, 1, update);
    if (rc != CBAS_OK) return rc;
    if (loss_host) {
        float s[3];
        HIP_TRY(hipMemcpyAsync(s, t->sums, sizeof(s), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        read_loss(s, loss_host);
    }
    return CBAS_OK;
}

extern "C" int cbas_rows_gather_windows(const uint16_t* rows_f16_dev, int64_t n_rows, int32_t dim, const int64_t* first_row_dev,
                                        int32_t n_windows, int32_t seq_len, float* x_out_dev, void* stream) {
    if (!rows_f16_dev || !first_row_dev || !x_out_dev) return cbas_fail(CBAS_EINVAL, "rows_f16_dev / first_row_dev / x_out_dev NULL");
    if (n_rows < 0) return cbas_fail(CBAS_EINVAL, "n_rows=%lld is negative", (long long)n_rows);
    if (dim < 1 || seq_len < 1 || seq_len > ROWS_GATHER_MAX_SEQ || (int64_t)dim * seq_len > ROWS_GATHER_MAX_WINDOW)
        return cbas_fail(CBAS_EINVAL, "dim=%d, seq_len=%d: both at least 1, seq_len <= %d and dim * seq_len <= %lld", dim, seq_len,
                         ROWS_GATHER_MAX_SEQ, (long long)ROWS_GATHER_MAX_WINDOW);
    if (n_windows < 1) return cbas_fail(CBAS_EINVAL, "n_windows=%d must be at least 1", n_windows);
    LAUNCH_TRY(launch_rows_gather(rows_f16_dev, n_rows, dim, first_row_dev, n_windows, seq_len, x_out_dev, (hipStream_t)stream));
    return CBAS_OK;
}

extern "C" int cbas_head_train_step_rows(cbas_head_trainer* t, const uint16_t* rows_f16_dev, int64_t n_rows, int32_t dim,
                                         const int64_t* first_row_dev, const int32_t* labels_dev, int32_t n_windows,
                                         int32_t seq_len, int32_t update, float* loss_host, void* stream) {
    if (!t) return cbas_fail(CBAS_EINVAL, "null trainer handle");
    if (!rows_f16_dev || !first_row_dev || !labels_dev) return cbas_fail(CBAS_EINVAL, "rows_f16_dev / first_row_dev / labels_dev NULL");
    if (dim != t->I || seq_len != t->T)
        return cbas_fail(CBAS_EINVAL, "rows of width %d in windows of %d: the trainer was created for in_features=%d, seq_len=%d", dim,
                         seq_len, t->I, t->T);
    if (n_windows < 1 || n_windows > t->Bcap) return cbas_fail(CBAS_EINVAL, "n_windows=%d outside [1, max_batch=%lld]", n_windows, (long long)t->Bcap);
    HIP_TRY(hipSetDevice(t->device));
    // t->xg holds max_batch windows and was filled before cbas_head_train_create returned; the gather and the step that
    // reads it are queued on the same stream
    const int rc = cbas_rows_gather_windows(rows_f16_dev, n_rows, dim, first_row_dev, n_windows, seq_len, t->xg, stream);
    if (rc != CBAS_OK) return rc;
    return cbas_head_train_step(t, t->xg, labels_dev, n_windows, update, loss_host, stream);
}

extern "C" int cbas_head_train_step_rows_multi(cbas_head_trainer** trainers, int32_t k, const uint16_t* rows_f16_dev,
                                               int64_t n_rows, int32_t dim, const int64_t* const* first_row_dev,
                                               const int32_t* const* labels_dev, const int32_t* n_windows, float* losses_host) {
    static_assert(CBAS_TRAIN_MULTI_MAX == TRAIN_MULTI_MAX, "the header's cap is the batched kernels' table size");
    if (!trainers || !rows_f16_dev || !first_row_dev || !labels_dev || !n_windows)
        return cbas_fail(CBAS_EINVAL, "trainers / rows_f16_dev / first_row_dev / labels_dev / n_windows NULL");
    if (k < 1 || k > CBAS_TRAIN_MULTI_MAX) return cbas_fail(CBAS_EINVAL, "k=%d outside [1, %d]", k, CBAS_TRAIN_MULTI_MAX);
    if (n_rows < 0) return cbas_fail(CBAS_EINVAL, "n_rows=%lld is negative", (long long)n_rows);
    // everything is checked before anything is queued: a refused call leaves every trainer as it was
    for (int j = 0; j < k; ++j) {
        const cbas_head_trainer* t = trainers[j];
        if (!t) return cbas_fail(CBAS_EINVAL, "trainer %d is NULL", j);
        if (!first_row_dev[j] || !labels_dev[j]) return cbas_fail(CBAS_EINVAL, "first_row_dev[%d] / labels_dev[%d] NULL", j, j);
        if (dim != t->I) return cbas_fail(CBAS_EINVAL, "rows of width %d: trainer %d was created for in_features=%d", dim, j, t->I);
        if (n_windows[j] < 1 || n_windows[j] > t->Bcap)
            return cbas_fail(CBAS_EINVAL, "n_windows[%d]=%d outside [1, max_batch=%lld]", j, n_windows[j], (long long)t->Bcap);
        const cbas_head_trainer* a = trainers[0];
        if (t->device != a->device || t->C != a->C || t->T != a->T || t->Bn != a->Bn || t->L0 != a->L0 || t->h != a->h ||
            t->NS != a->NS || t->NL != a->NL || t->lo != a->lo || t->hi != a->hi)
            return cbas_fail(CBAS_EINVAL, "trainer %d has another head configuration or device than trainer 0", j);
        for (int i = 0; i < j; ++i)
            if (trainers[i] == t) return cbas_fail(CBAS_EINVAL, "trainer %d is trainer %d again", j, i);
    }
    HIP_TRY(hipSetDevice(trainers[0]->device));
    Job jobs[CBAS_TRAIN_MULTI_MAX] = {};
    for (int j = 0; j < k; ++j) {
        cbas_head_trainer* t = trainers[j];
        if (!t->own) HIP_TRY(hipStreamCreateWithFlags(&t->own, hipStreamNonBlocking));
        if (!t->ev) HIP_TRY(hipEventCreateWithFlags(&t->ev, hipEventDisableTiming));
        jobs[j].t = t; jobs[j].x = t->xg; jobs[j].labels = labels_dev[j]; jobs[j].st = t->own; jobs[j].B = n_windows[j];
        bind_job(jobs[j]);
    }
    for (int j = 0; j < k; ++j) {
        const int rc = cbas_rows_gather_windows(rows_f16_dev, n_rows, dim, first_row_dev[j], n_windows[j], jobs[j].t->T, jobs[j].t->xg,
                                                jobs[j].st);
        if (rc != CBAS_OK) return rc;
    }
    const int rc = step_jobs(jobs, k, 1);
    if (rc != CBAS_OK) return rc;
    if (losses_host) {
        // the one wait of the call: the leading stream behind every trainer's, the k copies on it, one synchronisation
        float s[CBAS_TRAIN_MULTI_MAX][3];
        const hipStream_t lead = jobs[0].st;
        for (int j = 1; j < k; ++j) {
            HIP_TRY(hipEventRecord(jobs[j].t->ev, jobs[j].st));
            HIP_TRY(hipStreamWaitEvent(lead, jobs[j].t->ev, 0));
        }
        for (int j = 0; j < k; ++j) HIP_TRY(hipMemcpyAsync(s[j], jobs[j].t->sums, sizeof(s[j]), hipMemcpyDeviceToHost, lead));
        HIP_TRY(hipStreamSynchronize(lead));
        for (int j = 0; j < k; ++j) read_loss(s[j], losses_host + 3 * j);
    }
    return CBAS_OK;
}

extern "C" int cbas_head_train_read(cbas_head_trainer* t, int32_t what, float* blob_host, int64_t n) {
    if (!t || !blob_host) return cbas_fail(CBAS_EINVAL, "null argument");
    if (n != t->n_blob) return cbas_fail(CBAS_EINVAL, "blob has %lld floats, config needs %lld", (long long)n, (long long)t->n_blob);
    if (what < 0 || what > 3) return cbas_fail(CBAS_EINVAL, "what=%d (0 parameters, 1 gradients, 2 / 3 Adam's first / second moment)", what);
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<float> host((size_t)t->n_train);
    const float* const src[4] = {t->P, t->G, t->M, t->V};
    HIP_TRY(hipMemcpy(host.data(), src[what], host.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (const MapEntry& e : t->map) memcpy(blob_host + e.blob_off, host.data() + e.train_off, (size_t)e.n * sizeof(float));
    return CBAS_OK;
}

extern "C" int cbas_head_train_last_outputs(cbas_head_trainer* t, float* logits_host, float* latent_host, int32_t n_windows) {
    if (!t) return cbas_fail(CBAS_EINVAL, "null trainer handle");
    if (n_windows < 1 || n_windows > t->Bcap) return cbas_fail(CBAS_EINVAL, "n_windows=%d outside [1, max_batch]", n_windows);
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipDeviceSynchronize());
    if (logits_host) HIP_TRY(hipMemcpy(logits_host, t->final_logits, (size_t)n_windows * t->C * sizeof(float), hipMemcpyDeviceToHost));
    if (latent_host) HIP_TRY(hipMemcpy(latent_host, t->latent, (size_t)n_windows * t->H2 * sizeof(float), hipMemcpyDeviceToHost));
    return CBAS_OK;
}
