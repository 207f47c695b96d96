// Error plumbing shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include "../../include/cbas_mi355x.h"
#ifndef CBAS_BUILD_DEBUG
#define CBAS_BUILD_DEBUG 0
#endif
#if CBAS_BUILD_DEBUG
#include "../../include/cbas_mi355x_debug.h"      // bring-up / test entry points: debug build only
#endif

extern thread_local char g_cbas_err[512];

// api_enc.hip: the host-side builder of the DINOv2 position tables (mode: CBAS_POS_INTERP_*), shared with the debug entries
void cbas_build_pos_table(int mode, const float* src, int G, int D, int nh, int nw, float* out);
void cbas_pos_interp_matrix(int mode, int in_size, int out_size, float* W);

static inline int cbas_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_cbas_err, sizeof(g_cbas_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return cbas_fail(CBAS_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                             __FILE__, __LINE__);                                              \
    } while (0)

// HIP_TRY for the calls of a create path: running out of memory is CBAS_ENOMEM, every other failure CBAS_EHIP
#define ALLOC_TRY(expr)                                                                                            \
    do {                                                                                                           \
        hipError_t _e = (expr);                                                                                    \
        if (_e != hipSuccess)                                                                                      \
            return cbas_fail(_e == hipErrorOutOfMemory ? CBAS_ENOMEM : CBAS_EHIP, "%s failed: %s (%s:%d)", #expr,  \
                             hipGetErrorString(_e), __FILE__, __LINE__);                                           \
    } while (0)

// makes the device that owns dev_ptr the calling thread's, as every entry point that takes device pointers and no handle does before
// its first launch; 0, or CBAS_EHIP with the message set.  device: where to leave its number, or NULL
static inline int cbas_use_device_of(const void* dev_ptr, int* device = nullptr) {
    hipPointerAttribute_t attr;
    HIP_TRY(hipPointerGetAttributes(&attr, dev_ptr));
    HIP_TRY(hipSetDevice(attr.device));
    if (device) *device = attr.device;
    return CBAS_OK;
}

#define LAUNCH_TRY(expr)                                                                      \
    do {                                                                                       \
        int _r = (expr);                                                                       \
        if (_r != 0)                                                                           \
            return cbas_fail(_r == -1 ? CBAS_EINVAL : CBAS_EHIP, "%s failed (%d; hip: %s) (%s:%d)", \
                             #expr, _r, hipGetErrorString(hipGetLastError()), __FILE__, __LINE__); \
    } while (0)
