// What the entry points over resident fp16 rows (rows_search / rows_knn / rows_kmeans / rows_probe / rows_pca .hip) share on the host:
// the workspace offsets, the checks on the width and the row stride, and the opt-in to more than 64 KB of LDS.
#pragma once
#include "api_common.h"

static inline int64_t rows_round16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

// a workspace laid out piece after piece: take(bytes) is the piece's byte offset, a multiple of 16; at, in the end, the total
struct RowsTake {
    int64_t at = 0;
    int64_t operator()(int64_t bytes) {
        const int64_t o = at;
        at += rows_round16(bytes);
        return o;
    }
};

// 0, or CBAS_EINVAL with the message set; name and ld_name are the parameters' spellings in the entry point (dim or D, ld or bank_ld)
static inline int rows_width_ok(const char* what, const char* name, int32_t dim, int max_dim) {
    if (dim < 32 || dim % 32 != 0 || dim > max_dim)
        return cbas_fail(CBAS_EINVAL, "%s: %s = %d (the width is a multiple of 32 up to %d)", what, name, dim, max_dim);
    return CBAS_OK;
}

static inline int rows_ld_ok(const char* what, const char* ld_name, int64_t ld, const char* name, int32_t dim) {
    if (ld < dim || ld % 8 != 0)
        return cbas_fail(CBAS_EINVAL, "%s: %s = %lld (at least %s = %d, a multiple of 8)", what, ld_name, (long long)ld, name, dim);
    return CBAS_OK;
}

// a launch with more than 64 KB of dynamic LDS has to opt its kernel in to the CU's 160 KB first: every time, nothing is remembered
template <typename Kernel>
static inline int rows_lds_opt_in(Kernel* kernel, size_t lds_bytes) {
    if (lds_bytes > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return CBAS_OK;
}
