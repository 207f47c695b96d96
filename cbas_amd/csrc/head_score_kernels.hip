// The two kernels behind the tail of a training job (test split, calibration temperature): what the reference does on the
// host once per batch after the head's forward pass.
//
//   head_score_kernel   logits (n, C) -> argmax per window (first maximum, as torch.argmax) and a C x C confusion matrix
//                       (backend/cbas.py:1240-1250: logits.argmax(1).cpu() per batch, then sklearn's confusion_matrix).
//   logits_nll_kernel   logits (n, C), labels, temp -> mean cross-entropy of logits / temp and its derivative with respect to
//                       temp (backend/workthreads.py:127-133: the closure torch.optim.LBFGS evaluates up to 51 times).
//
// Both are bandwidth-trivial (tens of thousands of rows of 2-64 floats).  What they buy is the absence of a host round trip
// per batch, and a calibration loss whose bits do not depend on the run:
//   * the confusion matrix is summed with INTEGER atomics (per-workgroup counts in LDS, then one 64-bit global add per
//     non-zero cell): integer addition is associative, so any arrival order gives the same matrix;
//   * the loss is summed in a FIXED order and with no float atomic: a thread adds its rows in ascending order (row =
//     block * 256 + thread + k * grid * 256), a workgroup combines its 256 threads by a binary tree in LDS, the workgroup
//     that arrives last combines the per-workgroup partials by the same tree.  The grid is a function of n alone, so the
//     same (logits, labels, temp) give the same two floats on every launch, on any placement of workgroups.
//
// Hand-off of the partials inside the launch: thread 0 of a workgroup writes its (loss, derivative) pair as ONE 8-byte
// agent-scope atomic store and then takes a ticket with an acquire-release agent-scope fetch_add (the release orders the
// store before the ticket, both by the same thread); thread 0 of the last arriver has thereby acquired every other
// workgroup's pair, the workgroup barrier passes that on to its other threads, and those read the pairs with agent-scope
// atomic loads (which do not hit a stale line of this CU's L1).  The ticket word is zeroed by the launcher before every launch.
#include "kernels.h"

namespace {

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -2)

constexpr int SCORE_BLOCK = 256;
constexpr int NLL_BLOCK = 256;

__global__ void __launch_bounds__(SCORE_BLOCK)
head_score_kernel(const float* __restrict__ logits, const int* __restrict__ labels, int64_t n, int C, int* __restrict__ pred,
                  unsigned long long* confusion, unsigned* flags) {
    extern __shared__ unsigned score_hist[];                   // [C][C] counts of this workgroup (<= 256 in total)
    const int cells = confusion ? C * C : 0;
    for (int i = threadIdx.x; i < cells; i += SCORE_BLOCK) score_hist[i] = 0u;
    __syncthreads();
    const int64_t w = (int64_t)blockIdx.x * SCORE_BLOCK + threadIdx.x;
    if (w < n) {
        const float* z = logits + w * C;
        float best = z[0];
        int arg = 0;
        bool nan = best != best;
        for (int c = 1; c < C; ++c) {
            const float v = z[c];
            nan |= v != v;
            if (v > best) { best = v; arg = c; }               // strict: the first of equal maxima stays
        }
        if (nan) atomicOr(flags, HEAD_SCORE_FLAG_NAN);
        if (pred) pred[w] = nan ? -1 : arg;
        if (confusion && !nan) {
            const int y = labels[w];
            if (y < 0 || y >= C) atomicOr(flags, HEAD_SCORE_FLAG_LABEL);
            else atomicAdd(&score_hist[y * C + arg], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += SCORE_BLOCK) {
        const unsigned k = score_hist[i];
        if (k) atomicAdd(&confusion[i], (unsigned long long)k);
    }
}

__device__ __forceinline__ void nll_tree(float (*sh)[NLL_BLOCK], float& a, float& b) {
    sh[0][threadIdx.x] = a;
    sh[1][threadIdx.x] = b;
    __syncthreads();
    for (int s = NLL_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    a = sh[0][0];
    b = sh[1][0];
    __syncthreads();                                           // sh is reused by the caller
}

// Row terms as torch forms them in fp32: x = z / temp; log_softmax(x)[y] = (x[y] - max) - log(sum exp(x - max)).
//   loss_row  = -log_softmax(x)[y]
//   dloss_row / dtemp = (z[y] - sum_j softmax(x)[j] * z[j]) / temp^2
// A label outside [0, C) makes both results NaN (torch raises there; nothing is read outside the row).
__global__ void __launch_bounds__(NLL_BLOCK)
logits_nll_kernel(const float* __restrict__ logits, const int* __restrict__ labels, int64_t n, int C, float temp,
                  unsigned long long* partials, unsigned* ticket, float* __restrict__ out2) {
    __shared__ float sh[2][NLL_BLOCK];
    __shared__ int is_last;
    float loss = 0.f, dt = 0.f;
    const int64_t stride = (int64_t)gridDim.x * NLL_BLOCK;
    for (int64_t r = (int64_t)blockIdx.x * NLL_BLOCK + threadIdx.x; r < n; r += stride) {
        const float* z = logits + r * C;
        const int y = labels[r];
        float m = z[0] / temp;
        for (int c = 1; c < C; ++c) m = fmaxf(m, z[c] / temp);
        float se = 0.f, sz = 0.f;
        for (int c = 0; c < C; ++c) {
            const float e = expf(z[c] / temp - m);
            se += e;
            sz += e * z[c];
        }
        if (y < 0 || y >= C) {
            loss = __builtin_nanf("");
            dt = loss;
        } else {
            loss += logf(se) - (z[y] / temp - m);
            dt += (z[y] - sz / se) / (temp * temp);
        }
    }
    nll_tree(sh, loss, dt);
    if (threadIdx.x == 0) {
        const unsigned long long pair = ((unsigned long long)__float_as_uint(dt) << 32) | __float_as_uint(loss);
        __hip_atomic_store(&partials[blockIdx.x], pair, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        is_last = drawn == gridDim.x - 1;
    }
    __syncthreads();
    if (!is_last) return;
    loss = 0.f;
    dt = 0.f;
    if (threadIdx.x < gridDim.x) {                             // gridDim.x <= NLL_BLOCK: one partial per thread
        const unsigned long long pair = __hip_atomic_load(&partials[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        loss = __uint_as_float((unsigned)pair);
        dt = __uint_as_float((unsigned)(pair >> 32));
    }
    nll_tree(sh, loss, dt);
    if (threadIdx.x == 0) {
        out2[0] = loss / (float)n;
        out2[1] = dt / (float)n;
    }
}

}  // namespace

int launch_head_score(const float* logits, const int* labels, int64_t n, int C, int* pred, unsigned long long* confusion,
                      unsigned* flags, hipStream_t st) {
    if (!logits || !flags || n < 1 || C < 1 || C > HEAD_SCORE_MAX_CLASSES || (confusion && !labels)) return -1;
    const int64_t blocks = (n + SCORE_BLOCK - 1) / SCORE_BLOCK;
    if (blocks > 0x7fffffff) return -1;
    const size_t lds = confusion ? (size_t)C * C * sizeof(unsigned) : 0;
    hipLaunchKernelGGL(head_score_kernel, dim3((unsigned)blocks), dim3(SCORE_BLOCK), lds, st, logits, labels, n, C, pred, confusion,
                       flags);
    return CHECK_LAUNCH();
}

int logits_nll_blocks(int64_t n) {
    const int64_t b = (n + NLL_BLOCK - 1) / NLL_BLOCK;
    return (int)(b < LOGITS_NLL_MAX_BLOCKS ? b : LOGITS_NLL_MAX_BLOCKS);
}

int launch_logits_nll(const float* logits, const int* labels, int64_t n, int C, float temp, unsigned long long* partials,
                      unsigned* ticket, float* out2, hipStream_t st) {
    if (!logits || !labels || !partials || !ticket || !out2 || n < 1 || C < 1 || C > HEAD_SCORE_MAX_CLASSES) return -1;
    static_assert(LOGITS_NLL_MAX_BLOCKS <= NLL_BLOCK, "the last workgroup reads one partial per thread");
    if (hipMemsetAsync(ticket, 0, 16, st) != hipSuccess) return -2;          // the ticket's 16-byte block (see api_head.hip)
    hipLaunchKernelGGL(logits_nll_kernel, dim3((unsigned)logits_nll_blocks(n)), dim3(NLL_BLOCK), 0, st, logits, labels, n, C, temp,
                       partials, ticket, out2);
    return CHECK_LAUNCH();
}
