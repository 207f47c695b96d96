// C ABI of the patch-feature PCA (include/cbas_mi355x.h: cbas_patch_pca_*): argument checks and the launch sequence over the
// kernels of patch_pca.hip.  Plain device pointers, no handle: the rows may come from cbas_enc_forward_*_tokens or from anywhere.
#include "api_common.h"
#include "kernels.h"

namespace {

struct PcaShape {
    PcaRows rows;
    int nprob;
    int64_t nch, nmc;                      // partial covariances / partial column sums per problem
    int64_t cov_floats, z_floats, tmp_floats;
    int64_t floats() const { return cov_floats + z_floats + tmp_floats; }
};

// 0, or CBAS_EINVAL with the message set
int pca_shape(const char* what, int n, int T, int n_prefix, int D, int k, int scope, PcaShape* s) {
    if (n < 1 || n > 65535) return cbas_fail(CBAS_EINVAL, "%s: n = %d frames (1 .. 65535)", what, n);
    if (n_prefix < 0 || T <= n_prefix) return cbas_fail(CBAS_EINVAL, "%s: T = %d rows with n_prefix = %d leaves no patch row", what, T, n_prefix);
    if (D < 32 || D % 32 != 0 || D > PCA_MAX_D)
        return cbas_fail(CBAS_EINVAL, "%s: D = %d (the width is a multiple of 32 up to %d)", what, D, PCA_MAX_D);
    if (scope != CBAS_PCA_FRAME && scope != CBAS_PCA_BATCH)
        return cbas_fail(CBAS_EINVAL, "%s: scope %d (CBAS_PCA_FRAME or CBAS_PCA_BATCH)", what, scope);
    const int P = T - n_prefix;
    const int64_t M = scope == CBAS_PCA_BATCH ? (int64_t)n * P : P;
    if (M < 2) return cbas_fail(CBAS_EINVAL, "%s: M = %lld rows per problem: a covariance needs at least 2 rows", what, (long long)M);
    if (k < 1 || k > PCA_MAX_K) return cbas_fail(CBAS_EINVAL, "%s: k = %d components (1 .. %d)", what, k, PCA_MAX_K);
    if (k > M - 1 || k > D)
        return cbas_fail(CBAS_EINVAL, "%s: k = %d components exceed min(M - 1, D) = %lld", what, k, (long long)(M - 1 < D ? M - 1 : D));
    s->rows = PcaRows{nullptr, 0, T, n_prefix, P, M, scope == CBAS_PCA_BATCH ? n : 1};
    s->nprob = scope == CBAS_PCA_BATCH ? 1 : n;
    s->nch = pca_cov_chunks(M);
    s->nmc = pca_mean_chunks(M);
    if (s->nch > 65535 || s->nmc > 65535) return cbas_fail(CBAS_EINVAL, "%s: M = %lld rows per problem is more than one call takes", what, (long long)M);
    s->cov_floats = (int64_t)s->nprob * s->nch * D * D;
    s->z_floats = (int64_t)s->nprob * k * D;
    s->tmp_floats = (int64_t)s->nprob * s->nmc * D;
    return CBAS_OK;
}

}  // namespace

extern "C" int64_t cbas_patch_pca_workspace_bytes(int n, int T, int n_prefix, int D, int k, int scope) {
    PcaShape s;
    if (pca_shape("cbas_patch_pca_workspace_bytes", n, T, n_prefix, D, k, scope, &s) != CBAS_OK) return CBAS_EINVAL;
    return s.floats() * (int64_t)sizeof(float);
}

extern "C" int cbas_patch_pca_fit(const float* rows_dev, int n, int T, int n_prefix, int D, int64_t ld, int k, int scope, int iters,
                                  float* mean_dev, float* components_dev, float* eigenvalues_dev, float* total_variance_dev,
                                  void* workspace_dev, int64_t workspace_bytes, void* stream) {
    PcaShape s;
    if (pca_shape("cbas_patch_pca_fit", n, T, n_prefix, D, k, scope, &s) != CBAS_OK) return CBAS_EINVAL;
    if (!rows_dev || !mean_dev || !components_dev || !eigenvalues_dev || !total_variance_dev || !workspace_dev)
        return cbas_fail(CBAS_EINVAL, "cbas_patch_pca_fit: a NULL pointer");
    if (ld < D || ld % 4 != 0) return cbas_fail(CBAS_EINVAL, "cbas_patch_pca_fit: ld = %lld (at least D = %d, a multiple of 4)", (long long)ld, D);
    if (iters < 1) return cbas_fail(CBAS_EINVAL, "cbas_patch_pca_fit: iters = %d (at least 1)", iters);
    if (workspace_bytes < s.floats() * (int64_t)sizeof(float))
        return cbas_fail(CBAS_EINVAL, "cbas_patch_pca_fit: workspace of %lld bytes, %lld needed (cbas_patch_pca_workspace_bytes)",
                         (long long)workspace_bytes, (long long)(s.floats() * (int64_t)sizeof(float)));
    if (((uintptr_t)rows_dev | (uintptr_t)mean_dev | (uintptr_t)components_dev | (uintptr_t)workspace_dev) % 16)
        return cbas_fail(CBAS_EINVAL, "cbas_patch_pca_fit: rows, mean, components and workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    s.rows.x = rows_dev;
    s.rows.ld = ld;
    float* const cov = (float*)workspace_dev;
    float* const Z = cov + s.cov_floats;
    float* const tmp = Z + s.z_floats;
    LAUNCH_TRY(launch_pca_mean(s.rows, s.nprob, D, tmp, mean_dev, st));
    LAUNCH_TRY(launch_pca_cov(s.rows, s.nprob, D, mean_dev, cov, st));
    LAUNCH_TRY(launch_pca_eig(cov, s.nch * D * D, s.nprob, D, k, iters, Z, components_dev, eigenvalues_dev, total_variance_dev, st));
    return CBAS_OK;
}

extern "C" int cbas_patch_pca_project(const float* rows_dev, int n, int T, int n_prefix, int D, int64_t ld, int k, int n_bases,
                                      const float* mean_dev, const float* components_dev, float* scores_dev, void* stream) {
    if (n < 1 || n > 65535) return cbas_fail(CBAS_EINVAL, "cbas_patch_pca_project: n = %d frames (1 .. 65535)", n);
    if (n_prefix < 0 || T <= n_prefix)
        return cbas_fail(CBAS_EINVAL, "cbas_patch_pca_project: T = %d rows with n_prefix = %d leaves no patch row", T, n_prefix);
    if (D < 32 || D % 32 != 0 || D > PCA_MAX_D)
        return cbas_fail(CBAS_EINVAL, "cbas_patch_pca_project: D = %d (the width is a multiple of 32 up to %d)", D, PCA_MAX_D);
    if (k < 1 || k > PCA_MAX_K || k > D) return cbas_fail(CBAS_EINVAL, "cbas_patch_pca_project: k = %d components (1 .. %d)", k, PCA_MAX_K);
    if (n_bases != 1 && n_bases != n) return cbas_fail(CBAS_EINVAL, "cbas_patch_pca_project: n_bases = %d (1, or n = %d)", n_bases, n);
    if (!rows_dev || !mean_dev || !components_dev || !scores_dev) return cbas_fail(CBAS_EINVAL, "cbas_patch_pca_project: a NULL pointer");
    if (ld < D || ld % 4 != 0)
        return cbas_fail(CBAS_EINVAL, "cbas_patch_pca_project: ld = %lld (at least D = %d, a multiple of 4)", (long long)ld, D);
    if (((uintptr_t)rows_dev | (uintptr_t)mean_dev | (uintptr_t)components_dev) % 16)
        return cbas_fail(CBAS_EINVAL, "cbas_patch_pca_project: rows, mean and components must be 16-byte aligned");
    LAUNCH_TRY(launch_pca_project(rows_dev, ld, n, T, n_prefix, D, k, n_bases == 1 ? 0 : 1, mean_dev, components_dev, scores_dev,
                                  (hipStream_t)stream));
    return CBAS_OK;
}

// ---- k-means of patch features (cbas_patch_kmeans_*): the launch sequence over the kernels of patch_kmeans.hip -----------------------
namespace {

struct KmeansShape {
    PcaRows rows;
    int nprob;
    int64_t nch;
    // float offsets into the workspace, each a multiple of 4: the layout the header documents (cur and order first)
    int64_t cur, order, psum, pcount, pinertia, rn, mind, tmp, mean, bestv, besti, total;
};

int64_t round4(int64_t v) { return (v + 3) / 4 * 4; }

// the checks cbas_patch_kmeans_fit and _assign share; 0, or CBAS_EINVAL with the message set
int kmeans_rows(const char* what, int n, int T, int n_prefix, int D, int k, PcaRows* rows) {
    if (n < 1 || n > 65535) return cbas_fail(CBAS_EINVAL, "%s: n = %d frames (1 .. 65535)", what, n);
    if (n_prefix < 0 || T <= n_prefix) return cbas_fail(CBAS_EINVAL, "%s: T = %d rows with n_prefix = %d leaves no patch row", what, T, n_prefix);
    if (D < 32 || D % 32 != 0 || D > PCA_MAX_D)
        return cbas_fail(CBAS_EINVAL, "%s: D = %d (the width is a multiple of 32 up to %d)", what, D, PCA_MAX_D);
    if (k < 2 || k > KMEANS_MAX_K) return cbas_fail(CBAS_EINVAL, "%s: k = %d clusters (2 .. %d)", what, k, KMEANS_MAX_K);
    *rows = PcaRows{nullptr, 0, T, n_prefix, T - n_prefix, T - n_prefix, 1};
    return CBAS_OK;
}

int kmeans_shape(const char* what, int n, int T, int n_prefix, int D, int k, int scope, KmeansShape* s) {
    if (kmeans_rows(what, n, T, n_prefix, D, k, &s->rows) != CBAS_OK) return CBAS_EINVAL;
    if (scope != CBAS_PCA_FRAME && scope != CBAS_PCA_BATCH)
        return cbas_fail(CBAS_EINVAL, "%s: scope %d (CBAS_KMEANS_FRAME or CBAS_KMEANS_BATCH)", what, scope);
    const int64_t P = s->rows.P, M = scope == CBAS_PCA_BATCH ? (int64_t)n * P : P;
    if (k > M) return cbas_fail(CBAS_EINVAL, "%s: k = %d clusters exceed the M = %lld rows of a problem", what, k, (long long)M);
    if (kmeans_chunks(M) > 65535) return cbas_fail(CBAS_EINVAL, "%s: M = %lld rows per problem is more than one call takes", what, (long long)M);
    s->rows.M = M;
    s->rows.frames_per_problem = scope == CBAS_PCA_BATCH ? n : 1;
    s->nprob = scope == CBAS_PCA_BATCH ? 1 : n;
    s->nch = kmeans_chunks(M);
    const int64_t nb = s->nprob, nch = s->nch;
    int64_t at = 0;
    auto take = [&](int64_t floats) { const int64_t o = at; at += round4(floats); return o; };
    s->cur = take(nb * k * D);
    s->order = take(nb * 16);
    s->psum = take(nb * nch * k * D);
    s->pcount = take(nb * nch * 16);
    s->pinertia = take(nb * nch);
    s->rn = take(nb * M);
    s->mind = take(nb * M);
    s->tmp = take(nb * nch * D);
    s->mean = take(nb * D);
    s->bestv = take(nb * nch);
    s->besti = take(nb * nch);
    s->total = at;
    return CBAS_OK;
}

}  // namespace

extern "C" int64_t cbas_patch_kmeans_workspace_bytes(int n, int T, int n_prefix, int D, int k, int scope) {
    KmeansShape s;
    if (kmeans_shape("cbas_patch_kmeans_workspace_bytes", n, T, n_prefix, D, k, scope, &s) != CBAS_OK) return CBAS_EINVAL;
    return s.total * (int64_t)sizeof(float);
}

extern "C" int cbas_patch_kmeans_fit(const float* rows_dev, int n, int T, int n_prefix, int D, int64_t ld, int k, int scope, int iters,
                                     int normalize, float* centroids_dev, int32_t* counts_dev, float* inertia_dev, int32_t* init_index_dev,
                                     void* workspace_dev, int64_t workspace_bytes, void* stream) {
    KmeansShape s;
    if (kmeans_shape("cbas_patch_kmeans_fit", n, T, n_prefix, D, k, scope, &s) != CBAS_OK) return CBAS_EINVAL;
    if (!rows_dev || !centroids_dev || !counts_dev || !inertia_dev || !init_index_dev || !workspace_dev)
        return cbas_fail(CBAS_EINVAL, "cbas_patch_kmeans_fit: a NULL pointer");
    if (ld < D || ld % 4 != 0) return cbas_fail(CBAS_EINVAL, "cbas_patch_kmeans_fit: ld = %lld (at least D = %d, a multiple of 4)", (long long)ld, D);
    if (iters < 0) return cbas_fail(CBAS_EINVAL, "cbas_patch_kmeans_fit: iters = %d (at least 0)", iters);
    if (normalize != 0 && normalize != 1) return cbas_fail(CBAS_EINVAL, "cbas_patch_kmeans_fit: normalize = %d (0 or 1)", normalize);
    if (workspace_bytes < s.total * (int64_t)sizeof(float))
        return cbas_fail(CBAS_EINVAL, "cbas_patch_kmeans_fit: workspace of %lld bytes, %lld needed (cbas_patch_kmeans_workspace_bytes)",
                         (long long)workspace_bytes, (long long)(s.total * (int64_t)sizeof(float)));
    if (((uintptr_t)rows_dev | (uintptr_t)centroids_dev | (uintptr_t)workspace_dev) % 16)
        return cbas_fail(CBAS_EINVAL, "cbas_patch_kmeans_fit: rows, centroids and workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    s.rows.x = rows_dev;
    s.rows.ld = ld;
    float* const ws = (float*)workspace_dev;
    float* const cur = ws + s.cur;
    int32_t* const pcount = (int32_t*)(ws + s.pcount);
    LAUNCH_TRY(launch_kmeans_seed(s.rows, s.nprob, D, k, normalize, cur, init_index_dev, ws + s.rn, ws + s.mind, ws + s.tmp, ws + s.mean,
                                  ws + s.bestv, (int32_t*)(ws + s.besti), st));
    for (int t = 0; t <= iters; ++t) {
        LAUNCH_TRY(launch_kmeans_pass(s.rows, s.nprob, D, k, normalize, cur, (int64_t)k * D, ws + s.psum, pcount, ws + s.pinertia, nullptr,
                                      nullptr, st));
        if (t < iters)
            LAUNCH_TRY(launch_kmeans_update(ws + s.psum, pcount, ws + s.pinertia, s.nch, s.nprob, D, k, cur, inertia_dev + t, iters + 1, st));
    }
    LAUNCH_TRY(launch_kmeans_finish(pcount, ws + s.pinertia, s.nch, s.nprob, D, k, cur, inertia_dev + iters, iters + 1, centroids_dev,
                                    counts_dev, (int32_t*)(ws + s.order), st));
    return CBAS_OK;
}

extern "C" int cbas_patch_kmeans_assign(const float* rows_dev, int n, int T, int n_prefix, int D, int64_t ld, int k, int n_sets, int normalize,
                                        const float* centroids_dev, int32_t* labels_dev, float* dist2_dev, void* stream) {
    PcaRows rows;
    if (kmeans_rows("cbas_patch_kmeans_assign", n, T, n_prefix, D, k, &rows) != CBAS_OK) return CBAS_EINVAL;
    if (n_sets != 1 && n_sets != n) return cbas_fail(CBAS_EINVAL, "cbas_patch_kmeans_assign: n_sets = %d (1, or n = %d)", n_sets, n);
    if (!rows_dev || !centroids_dev || !labels_dev) return cbas_fail(CBAS_EINVAL, "cbas_patch_kmeans_assign: a NULL pointer");
    if (ld < D || ld % 4 != 0)
        return cbas_fail(CBAS_EINVAL, "cbas_patch_kmeans_assign: ld = %lld (at least D = %d, a multiple of 4)", (long long)ld, D);
    if (normalize != 0 && normalize != 1) return cbas_fail(CBAS_EINVAL, "cbas_patch_kmeans_assign: normalize = %d (0 or 1)", normalize);
    if (((uintptr_t)rows_dev | (uintptr_t)centroids_dev) % 16)
        return cbas_fail(CBAS_EINVAL, "cbas_patch_kmeans_assign: rows and centroids must be 16-byte aligned");
    rows.x = rows_dev;
    rows.ld = ld;
    LAUNCH_TRY(launch_kmeans_pass(rows, n, D, k, normalize, centroids_dev, n_sets == 1 ? 0 : (int64_t)k * D, nullptr, nullptr, nullptr, labels_dev,
                                  dist2_dev, (hipStream_t)stream));
    return CBAS_OK;
}
