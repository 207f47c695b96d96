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
