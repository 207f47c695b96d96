// Window gather for head training and scoring from a resident store of half-precision CLS rows:
//   x_out[w][t][:] = float(rows[first_row[w] + t][:])            (w < n_windows, t < seq_len)
// which is what the reference's datasets build on the host, one HDF5 slice and one `.float()` per window
// (backend/cbas.py:194-228), before the batch is stacked and copied to the device.  The f16 -> f32 conversion is exact.
//
// A window is seq_len consecutive rows of the store, so its source is ONE contiguous run of seq_len * dim halves and its
// destination one contiguous run of floats.  One block column (blockIdx.x) per window; a lane takes 8 consecutive halves
// (one 16-byte load) and writes them as two 16-byte stores, consecutive lanes on consecutive addresses.  That form needs
// every row to start on a 16-byte boundary: dim % 8 == 0 and 16-byte aligned base pointers.  Any other dim (or base) takes
// the element-wise kernel, still with consecutive lanes on consecutive addresses.
//
// Every read is predicated on 0 <= row < n_rows, written so that no first_row value can overflow the comparison; a row
// outside the store comes out as zeros.  The callers validate their indices on the host: the predicate is a guard.
#include "kernels.h"

namespace {

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -2)

constexpr int GATHER_BLOCK = 256;

// t < seq_len <= 2^20, n_rows >= 0: neither side of either comparison can overflow for any int64 first
__device__ __forceinline__ bool row_in_store(int64_t first, int t, int64_t n_rows) { return first >= -(int64_t)t && first < n_rows - t; }

__global__ void __launch_bounds__(GATHER_BLOCK)
rows_gather_vec8_kernel(const f16x8* __restrict__ rows, int64_t n_rows, int dim8, const int64_t* __restrict__ first_row,
                        int chunks, int seq_len, f32x4* __restrict__ out) {
    const int c = blockIdx.y * GATHER_BLOCK + threadIdx.x;           // 8-half chunk of this window
    if (c >= chunks) return;
    const int64_t first = first_row[blockIdx.x];
    f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (first >= 0 && first <= n_rows - seq_len) {                   // the whole window is inside the store (block-uniform)
        v = rows[first * dim8 + c];
    } else {
        const int t = c / dim8;
        if (row_in_store(first, t, n_rows)) v = rows[(first + t) * dim8 + (c - t * dim8)];
    }
    f32x4 lo, hi;
    lo.x = (float)v[0]; lo.y = (float)v[1]; lo.z = (float)v[2]; lo.w = (float)v[3];
    hi.x = (float)v[4]; hi.y = (float)v[5]; hi.z = (float)v[6]; hi.w = (float)v[7];
    f32x4* o = out + ((int64_t)blockIdx.x * chunks + c) * 2;
    o[0] = lo;
    o[1] = hi;
}

__global__ void __launch_bounds__(GATHER_BLOCK)
rows_gather_scalar_kernel(const f16* __restrict__ rows, int64_t n_rows, int dim, const int64_t* __restrict__ first_row,
                          int elems, float* __restrict__ out) {
    const int e = blockIdx.y * GATHER_BLOCK + threadIdx.x;           // element of this window
    if (e >= elems) return;
    const int64_t first = first_row[blockIdx.x];
    const int t = e / dim;
    float v = 0.f;
    if (row_in_store(first, t, n_rows)) v = (float)rows[(first + t) * dim + (e - t * dim)];
    out[(int64_t)blockIdx.x * elems + e] = v;
}

}  // namespace

int launch_rows_gather(const uint16_t* rows_f16, int64_t n_rows, int dim, const int64_t* first_row, int n_windows, int seq_len,
                       float* x_out, hipStream_t st) {
    if (!rows_f16 || !first_row || !x_out || n_rows < 0 || dim < 1 || seq_len < 1 || n_windows < 1) return -1;
    const int64_t elems = (int64_t)seq_len * dim;
    if (seq_len > ROWS_GATHER_MAX_SEQ || elems > ROWS_GATHER_MAX_WINDOW) return -1;
    const bool vec = dim % 8 == 0 && ((uintptr_t)rows_f16 % 16) == 0 && ((uintptr_t)x_out % 16) == 0;
    if (vec) {
        const int chunks = (int)(elems / 8);
        const dim3 grid((unsigned)n_windows, (unsigned)((chunks + GATHER_BLOCK - 1) / GATHER_BLOCK));
        hipLaunchKernelGGL(rows_gather_vec8_kernel, grid, dim3(GATHER_BLOCK), 0, st, reinterpret_cast<const f16x8*>(rows_f16),
                           n_rows, dim / 8, first_row, chunks, seq_len, reinterpret_cast<f32x4*>(x_out));
    } else {
        const dim3 grid((unsigned)n_windows, (unsigned)((elems + GATHER_BLOCK - 1) / GATHER_BLOCK));
        hipLaunchKernelGGL(rows_gather_scalar_kernel, grid, dim3(GATHER_BLOCK), 0, st, reinterpret_cast<const f16*>(rows_f16),
                           n_rows, dim, first_row, (int)elems, x_out);
    }
    return CHECK_LAUNCH();
}
