// Forward-backward (include/cbas_mi355x_ext.h): the posterior marginals gamma of every clip under a
// first-order transition model, the expected transition counts Xi, the expected first states Pi and the log-likelihood, from
// per-frame probabilities that are already on the device.  The floating-point sibling of seq_viterbi.hip: the same pieces of
// CBASX_HMM_CHUNK frames relative to a clip's own first frame, one transfer operator per piece, a walk over pieces, then the
// pieces side by side.
//
//   hm_check_kernel      the refusals that need device data - table entries, transitions, prior - and, per clip, its number of
//                        pieces.  Writes into the workspace only.
//   hm_transfer_kernel   (clips of more than one piece) per piece and start state s one forward run without storing: row s of
//                        F_k = prod_t (A diag(b_t)), as a float vector with its largest entry in [1, 2) and an integer exponent.
//                        The first piece of a clip has one run, from the prior.
//   hm_scan_kernel       (the same clips) one wave per clip and direction walks the pieces, not the frames: forward
//                        alpha_start ~ alpha_start F_k for every piece's start vector, backward beta_end ~ F_k beta_end for
//                        every piece's end vector.  Rows enter with their own exponents, so they combine exactly in scale.
//   hm_forward_kernel    per piece the serial forward pass from its start vector; writes alpha_t (up to a power of two) into
//                        gamma_dev, which doubles as the store, and the piece's share of the log-likelihood.
//   hm_backward_kernel   per piece the serial backward pass from its end vector; turns the stored alpha_t into gamma_t in place
//                        and forms the piece's partial Xi, the step across the seam into the piece BEFORE it included (from
//                        that piece's start vector of the scan, so no piece reads a row another piece rewrites).
//   hm_reduce_kernel     Xi, Pi and loglik: partials added per clip in ascending piece order, then in ascending clip order, in
//                        float64, one thread per output element.
//
// A state is a lane (C <= 64 = one wave).  Forward, lane j keeps column j of A in registers and alpha_{t-1}[i] arrives through
// v_readlane; backward, lane i keeps row i and b_{t+1}[j] beta_{t+1}[j] arrives the same way.  Neither recursion is normalised
// by a sum: the values read for the broadcast are uniform, their largest exponent is a scalar maximum beside the vector work,
// and the step is scaled by that power of two - exact, and no cross-lane reduction on the serial chain.  Both recursions
// run in float64 (hm_dot says why); what is stored - alpha, gamma, the transfer rows - is float32.  The exponents are
// summed as integers; a piece's log-likelihood is that sum plus log2 of the sum of its last vector.  No atomic but the flag word.
#include <limits.h>
#include <math.h>
#include "api_common.h"
#include "kernels.h"
#include "../../include/cbas_mi355x_ext.h"

#pragma clang fp contract(off)                             // every fused multiply-add below is written as one

namespace {

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -2)

constexpr int HM_CHUNK = CBASX_HMM_CHUNK;
constexpr int HM_MAXC = CBASX_HMM_MAX_CLASSES;
constexpr int HM_BLOCK = 256;                              // the checking and the reducing kernel
constexpr int HM_LD = HM_MAXC + 1;                         // hm_scan_kernel: row pitch of a transfer matrix in LDS
constexpr int HM_MAX_STREAM_BLOCKS = 2048;
constexpr int64_t HM_MAX_FRAMES = (int64_t)1 << 40;
constexpr float HM_FLOOR = 0x1p-32f;
constexpr unsigned HM_BAD_TABLE = 1u, HM_BAD_TRANS = 2u, HM_BAD_PRIOR = 4u;
static_assert(HM_MAXC == 64 && HM_CHUNK % 8 == 0, "a state is a lane; the passes load 8 frames ahead");

// the workspace: byte offsets of its parts (all multiples of 256) and its size
struct HmLayout {
    int64_t pieces, long_pieces;                           // capacities: all pieces; pieces of clips of more than one
    size_t flags, counts, lcounts, offsets, loffsets, t_d, t_exp, vstart, bend, xi_part, ll_part, total;
};

bool hm_layout(int64_t n_total, int n_clips, int C, HmLayout* L) {
    if (n_total < 0 || n_total > HM_MAX_FRAMES || n_clips < 1 || C < 1 || C > HM_MAXC) return false;
    // as cbasx_viterbi_workspace_bytes: sum over clips of ceil(n_c / CHUNK) <= n_total / CHUNK + n_clips for clips that do not
    // overlap; a clip of more than one piece has ceil(n_c / CHUNK) < 2 n_c / CHUNK
    L->pieces = n_total / HM_CHUNK + n_clips;
    L->long_pieces = 2 * (n_total / HM_CHUNK) + 1;
    if (L->pieces > INT_MAX) return false;
    size_t at = 0;
    auto part = [&at](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) / 256 * 256;
        return here;
    };
    const size_t K = (size_t)L->pieces, KT = (size_t)L->long_pieces, c = (size_t)C;
    L->flags = part(256);
    L->counts = part((size_t)n_clips * 4);
    L->lcounts = part((size_t)n_clips * 4);
    L->offsets = part(((size_t)n_clips + 1) * 8);
    L->loffsets = part(((size_t)n_clips + 1) * 8);
    L->t_d = part(KT * c * c * 4);
    L->t_exp = part(KT * c * 4);
    L->vstart = part(KT * c * 4);
    L->bend = part(KT * c * 4);
    L->xi_part = part(K * c * c * 8);
    L->ll_part = part(K * 8);
    L->total = at;
    return true;
}

struct HmArgs {
    const float* probs;
    int64_t n_total;
    const int64_t* table;
    int n_clips, C;
    const float* trans;
    const float* prior;                                    // may be null: uniform
    float* gamma;
    double* xi;                                            // may be null
    double* pi;                                            // may be null
    double* loglik;                                        // may be null
    unsigned* flags;                                       // the caller's
    const long long* offsets;
    const long long* loffsets;
    float* t_d;
    int* t_exp;
    float* vstart;
    float* bend;
    double* xi_part;
    double* ll_part;
};

// frames of clip c, or -1 for an entry that reaches outside [0, n_total); *base = its first frame
__device__ __forceinline__ int64_t hm_clip(const int64_t* __restrict__ table, int c, int64_t n_total, int64_t* base) {
    const int64_t b = table[2 * (int64_t)c], n = table[2 * (int64_t)c + 1];
    if (b < 0 || n < 0 || n > 0x7fffffff || b > n_total || n > n_total - b) return -1;
    *base = b;
    return n;
}

// finite, at least 0, and summing to 1 within CBASX_HMM_ROW_TOL
__device__ __forceinline__ bool hm_stochastic(const float* __restrict__ row, int C) {
    double s = 0.0;
    bool ok = true;
    for (int j = 0; j < C; ++j) {
        const float v = row[j];
        ok &= v >= 0.f && v < INFINITY;                    // false for a NaN
        s += (double)v;
    }
    return ok && fabs(s - 1.0) <= (double)CBASX_HMM_ROW_TOL;
}

__global__ void __launch_bounds__(HM_BLOCK)
hm_check_kernel(int64_t n_total, const int64_t* __restrict__ table, int n_clips, int C, const float* __restrict__ trans,
                const float* __restrict__ prior, int* __restrict__ counts, int* __restrict__ lcounts, unsigned* flags) {
    const int64_t tid = (int64_t)blockIdx.x * HM_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * HM_BLOCK;
    unsigned bad = 0;
    for (int64_t c = tid; c < n_clips; c += stride) {
        int64_t base = 0;
        const int64_t n = hm_clip(table, (int)c, n_total, &base);
        const int pieces = n < 0 ? 0 : (int)((n + HM_CHUNK - 1) / HM_CHUNK);
        if (n < 0) bad |= HM_BAD_TABLE;
        counts[c] = pieces;
        lcounts[c] = pieces > 1 ? pieces : 0;
    }
    for (int64_t i = tid; i < C; i += stride)
        if (!hm_stochastic(trans + i * C, C)) bad |= HM_BAD_TRANS;
    if (prior && tid == 0 && !hm_stochastic(prior, C)) bad |= HM_BAD_PRIOR;
    if (bad) atomicOr(flags, bad);
}

// the largest c with offsets[c] <= g, for 0 <= g < offsets[n]: the clip that owns piece g
__device__ __forceinline__ int hm_find(const long long* __restrict__ offsets, int n, long long g) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// a piece: clip, number within the clip, pieces of the clip, first frame in the call's arrays, frames
struct HmPiece {
    int clip, k, pieces, len;
    int64_t t0;
};

__device__ __forceinline__ bool hm_piece(const HmArgs& p, const long long* __restrict__ offsets, long long g, HmPiece* q) {
    q->clip = hm_find(offsets, p.n_clips, g);
    const long long k = g - offsets[q->clip];
    int64_t base = 0;
    const int64_t n = hm_clip(p.table, q->clip, p.n_total, &base);      // checked again: nothing is indexed with an unchecked entry
    if (n < 0 || k < 0 || k * HM_CHUNK >= n) return false;
    q->k = (int)k;
    q->pieces = (int)((n + HM_CHUNK - 1) / HM_CHUNK);
    q->t0 = base + k * HM_CHUNK;
    q->len = (int)(n - k * HM_CHUNK < HM_CHUNK ? n - k * HM_CHUNK : HM_CHUNK);
    return true;
}

// b = max(p, 2^-32); a NaN and a negative count as 2^-32 and are reported
__device__ __forceinline__ float hm_emission(float p, bool& bad) {
    bad |= !(p >= 0.f);
    return p >= HM_FLOOR ? p : HM_FLOOR;
}

// the exponent of the largest of the magnitudes whose bit patterns were maximised into bits
__device__ __forceinline__ int hm_exponent(unsigned bits) { return (int)(bits >> 23) - 127; }

__device__ __forceinline__ double hm_wave_sum_d(double v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int hm_wave_max(int v) {
    for (int o = 32; o; o >>= 1) {
        const int w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

// a vector of non-negative entries brought to a largest entry in [1, 2): returns the exponent taken out
__device__ __forceinline__ int hm_normalise(float& v) {
    const int e = hm_exponent((unsigned)hm_wave_max(__float_as_int(v) & 0x7fffffff));
    v = ldexpf(v, -e);
    return e;
}

// the same for float64, whose exponent lies in the high word
__device__ __forceinline__ int hm_exponent_d(unsigned hi) { return (int)(hi >> 20) - 1023; }

__device__ __forceinline__ int hm_normalise_d(double& v) {
    const int e = hm_exponent_d((unsigned)hm_wave_max(__double2hiint(v) & 0x7fffffff));
    v = ldexp(v, -e);
    return e;
}

// v[lane i], uniform
__device__ __forceinline__ double hm_lane(double v, int i, unsigned& hi) {
    const int h = __builtin_amdgcn_readlane(__double2hiint(v), i);
    hi = (unsigned)h & 0x7fffffffu;
    return __hiloint2double(h, __builtin_amdgcn_readlane(__double2loint(v), i));
}

// sum_i v[lane i] * a[i] in four partial sums of a fixed order, and the largest high word among the |v[lane i]|: both from the
// same uniform reads.  Lanes C .. 63 hold v = 0.  The recursions run in float64: under emissions that say little, alpha and
// beta forget a rounding error only at the rate the chain mixes, and a bout's frames repeat the same rounding step after step;
// in float32 that reached 14 ulp of gamma and Xi on uniform rows, where the serial float32 restatement happened to stay at 1.
template <int CP>
__device__ __forceinline__ double hm_dot(const float (&a)[CP], int C, double v, unsigned& bits) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < CP; ++i) {
        if (i < C) {                                           // uniform
            unsigned hi;
            const double x = hm_lane(v, i, hi);
            m = hi > m ? hi : m;
            s[i & 3] = fma(x, (double)a[i], s[i & 3]);
        }
    }
    bits = m;
    return (s[0] + s[1]) + (s[2] + s[3]);
}

// `steps` frames from p_rows: u <- ((u A) o b_t) / 2^E with E the exponent of the largest entry of the u that went in, so u
// stays in range without a reduction; the E are added to esum.  With STORE every u goes to out_rows, as float32.
template <int CP, bool STORE>
__device__ __forceinline__ void hm_forward_run(const float (&acol)[CP], int C, int lane, const float* __restrict__ p_rows,
                                               float* out_rows, int steps, double& u, int& esum, bool& bad) {
    constexpr int U = 8;
    for (int t0 = 0; t0 < steps; t0 += U) {
        float p[U];
#pragma unroll
        for (int k = 0; k < U; ++k) p[k] = (t0 + k < steps && lane < C) ? p_rows[(int64_t)(t0 + k) * C + lane] : 1.f;
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (t0 + k < steps) {                              // uniform
                unsigned bits;
                const double d = hm_dot<CP>(acol, C, u, bits);
                const int E = hm_exponent_d(bits);
                const float b = lane < C ? hm_emission(p[k], bad) : 0.f;
                u = d * ldexp((double)b, -E);
                esum += E;
                if (STORE && lane < C) out_rows[(int64_t)(t0 + k) * C + lane] = (float)u;
            }
        }
    }
}

template <int CP>
__device__ __forceinline__ void hm_load_column(float (&a)[CP], const float* __restrict__ trans, int C, int lane) {
#pragma unroll
    for (int i = 0; i < CP; ++i) a[i] = (i < C && lane < C) ? trans[i * C + lane] : 0.f;
}

template <int CP>
__device__ __forceinline__ void hm_load_row(float (&a)[CP], const float* __restrict__ trans, int C, int lane) {
#pragma unroll
    for (int j = 0; j < CP; ++j) a[j] = (j < C && lane < C) ? trans[lane * C + j] : 0.f;
}

__device__ __forceinline__ float hm_prior(const HmArgs& p, int lane) { return p.prior ? p.prior[lane] : 1.f / (float)p.C; }

template <int CP>
__global__ void __launch_bounds__(64) hm_transfer_kernel(HmArgs p) {
    const int lane = threadIdx.x, C = p.C, s = blockIdx.y;
    HmPiece q;
    if (!hm_piece(p, p.loffsets, blockIdx.x, &q)) return;
    if (q.k == 0 && s != 0) return;                            // the first piece starts from the prior: one run
    float acol[CP];
    hm_load_column<CP>(acol, p.trans, C, lane);
    const float* p_rows = p.probs + q.t0 * C;
    bool bad = false;
    double u = 0.0;
    if (lane < C) u = (double)(q.k == 0 ? hm_prior(p, lane) : p.trans[s * C + lane]) * (double)hm_emission(p_rows[lane], bad);
    int esum = 0;
    hm_forward_run<CP, false>(acol, C, lane, p_rows + C, nullptr, q.len - 1, u, esum, bad);
    esum += hm_normalise_d(u);
    const int64_t row = (int64_t)blockIdx.x * C + s;
    if (lane < C) p.t_d[row * C + lane] = (float)u;
    if (lane == 0) p.t_exp[row] = esum;
}

// the transfer matrix of a slot into LDS, rows HM_LD apart (the backward walk reads a row per lane), and its row exponents
__device__ __forceinline__ void hm_stage_transfer(const HmArgs& p, int64_t slot, float* T, int* tx) {
    const int lane = threadIdx.x, C = p.C;
    for (int i = lane; i < C * C; i += 64) T[(i / C) * HM_LD + i % C] = p.t_d[slot * C * C + i];
    if (lane < C) tx[lane] = p.t_exp[slot * C + lane];
    __syncthreads();
}

// r[lane] * 2^tx[lane] over the lanes below C, brought to a largest entry in [1, 2): the rows' exponents enter as integers
__device__ __forceinline__ float hm_scaled(float r, int tx, bool live) {
    live = live && r > 0.f;
    const int x = live ? tx + hm_exponent((unsigned)__float_as_int(r)) : INT_MIN / 2;
    const int X = hm_wave_max(x);
    const int shift = tx - X;                                  // at most 127 - the exponent of r is at least -127
    return live ? ldexpf(r, shift < -400 ? -400 : shift) : 0.f;
}

__global__ void __launch_bounds__(64) hm_scan_kernel(HmArgs p) {
    __shared__ float T[HM_MAXC * HM_LD];
    __shared__ int tx[HM_MAXC];
    const int lane = threadIdx.x, C = p.C, c = blockIdx.x;
    const bool live = lane < C;
    int64_t base = 0;
    const int64_t n = hm_clip(p.table, c, p.n_total, &base);
    if (n <= HM_CHUNK) return;
    const int pieces = (int)((n + HM_CHUNK - 1) / HM_CHUNK);
    const int64_t slot0 = p.loffsets[c];
    if (blockIdx.y == 0) {
        // forward: the vector at the last frame of piece 0 is row 0 of its slot; v <- v F_k
        float v = live ? p.t_d[slot0 * C * C + lane] : 0.f;
        for (int k = 1; k < pieces; ++k) {
            if (live) p.vstart[(slot0 + k) * C + lane] = v;
            if (k == pieces - 1) break;
            hm_stage_transfer(p, slot0 + k, T, tx);
            const int coef = __float_as_int(hm_scaled(v, live ? tx[lane] : 0, live));
            float acc = 0.f;
            for (int s = 0; s < C; ++s) acc = fmaf(__int_as_float(__builtin_amdgcn_readlane(coef, s)), T[s * HM_LD + (live ? lane : 0)], acc);
            v = live ? acc : 0.f;
            hm_normalise(v);
            __syncthreads();
        }
    } else {
        // backward: beta at the last frame of the last piece is 1; e <- F_k e is beta at the last frame of piece k - 1
        float e = live ? 1.f : 0.f;
        for (int k = pieces - 1; k >= 1; --k) {
            hm_stage_transfer(p, slot0 + k, T, tx);
            const int ei = __float_as_int(e);
            float r = 0.f;
            for (int j = 0; j < C; ++j) r = fmaf(T[(live ? lane : 0) * HM_LD + j], __int_as_float(__builtin_amdgcn_readlane(ei, j)), r);
            e = hm_scaled(r, live ? tx[lane] : 0, live);
            if (live) p.bend[(slot0 + k - 1) * C + lane] = e;
            __syncthreads();
        }
    }
}

template <int CP>
__global__ void __launch_bounds__(64) hm_forward_kernel(HmArgs p) {
    const int lane = threadIdx.x, C = p.C;
    HmPiece q;
    if (!hm_piece(p, p.offsets, blockIdx.x, &q)) return;
    float acol[CP];
    hm_load_column<CP>(acol, p.trans, C, lane);
    const float* p_rows = p.probs + q.t0 * C;
    float* rows = p.gamma + q.t0 * C;
    bool bad = false;
    double u = 0.0;
    int esum = 0;
    double start = 0.0;                                        // log2 of the sum of the vector the piece starts from
    if (q.k == 0) {
        if (lane < C) {
            u = (double)hm_prior(p, lane) * (double)hm_emission(p_rows[lane], bad);
            rows[lane] = (float)u;
        }
        hm_forward_run<CP, true>(acol, C, lane, p_rows + C, rows + C, q.len - 1, u, esum, bad);
    } else {
        if (lane < C) u = (double)p.vstart[(p.loffsets[q.clip] + q.k) * C + lane];
        start = log2(hm_wave_sum_d(u));
        hm_forward_run<CP, true>(acol, C, lane, p_rows, rows, q.len, u, esum, bad);
    }
    const double end = hm_wave_sum_d(u);
    if (lane == 0) p.ll_part[blockIdx.x] = (double)esum + (log2(end) - start);
    if (__any(bad) && lane == 0) atomicOr(p.flags, CBASX_HMM_FLAG_EMISSION);
}

// one backward step at frame t, on lane i: w = b_t o beta_t; beta_{t-1}[i] = sum_j A[i][j] w[j]; g = alpha_{t-1} o beta_{t-1}
// and its sum Z give gamma_{t-1} = g / Z (returned) and, with XI, S[j] += alpha_{t-1}[i] / Z * w[j] - the expected count of
// i -> j at this step is A[i][j] times that, and A is multiplied in once per piece.  S is float64 in registers: a product of two
// floats is exact there, and a bout's steps add nearly the same term again and again, which a float32 sum rounds the same way
// every time.  beta leaves scaled by the power of two of the largest w.
template <int CP, bool XI>
__device__ __forceinline__ float hm_backward_step(const float (&arow)[CP], int C, int lane, float prob, float a_prev, double& beta,
                                                  double (&S)[CP], bool& bad) {
    bool ignored = false;
    const float b = lane < C ? hm_emission(prob, ignored) : 0.f;
    const double w = (double)b * beta;
    unsigned bits;
    const double raw = hm_dot<CP>(arow, C, w, bits);
    const double g = (double)a_prev * raw;
    const double Z = hm_wave_sum_d(g);
    const bool ok = Z > 0.0 && Z < (double)INFINITY;
    bad |= !ok;
    const double inv = 1.0 / Z;
    if (XI) {
        const double coef = ok ? (double)a_prev * inv : 0.0;   // a step without a posterior counts nothing: its w may be
        const double wc = ok ? w : 0.0;                        // infinite, and 0 * inf would be a NaN
#pragma unroll
        for (int j = 0; j < CP; ++j) {
            if (j < C) {
                unsigned hi;
                S[j] = fma(coef, hm_lane(wc, j, hi), S[j]);
            }
        }
    }
    beta = ldexp(raw, -hm_exponent_d(bits));
    return ok ? (float)(g * inv) : NAN;
}

template <int CP, bool XI>
__global__ void __launch_bounds__(64) hm_backward_kernel(HmArgs p) {
    const int lane = threadIdx.x, C = p.C;
    HmPiece q;
    if (!hm_piece(p, p.offsets, blockIdx.x, &q)) return;
    float arow[CP];
    double S[CP];
    hm_load_row<CP>(arow, p.trans, C, lane);
#pragma unroll
    for (int j = 0; j < CP; ++j) S[j] = 0.0;
    const float* p_rows = p.probs + q.t0 * C;
    float* rows = p.gamma + q.t0 * C;                          // alpha in, gamma out: a row is read before it is written
    const int64_t slot = q.pieces > 1 ? p.loffsets[q.clip] + q.k : 0;
    const int top = q.len - 1;
    bool bad = false;
    double beta = 0.0;
    if (lane < C) beta = q.k == q.pieces - 1 ? 1.0 : (double)p.bend[slot * C + lane];
    {
        const double g = lane < C ? (double)rows[(int64_t)top * C + lane] * beta : 0.0;
        const double Z = hm_wave_sum_d(g);
        const bool ok = Z > 0.0 && Z < (double)INFINITY;
        bad |= !ok;
        if (lane < C) rows[(int64_t)top * C + lane] = ok ? (float)(g / Z) : NAN;
    }
    constexpr int U = 8;
    for (int r0 = 0; r0 < top; r0 += U) {                      // step r handles frame t = top - r and writes row t - 1
        float pe[U], al[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const bool in = r0 + k < top && lane < C;
            const int64_t t = top - (r0 + k);
            pe[k] = in ? p_rows[t * C + lane] : 1.f;
            al[k] = in ? rows[(t - 1) * C + lane] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (r0 + k < top) {                                // uniform
                const float gam = hm_backward_step<CP, XI>(arow, C, lane, pe[k], al[k], beta, S, bad);
                if (lane < C) rows[(int64_t)(top - (r0 + k) - 1) * C + lane] = gam;
            }
        }
    }
    if (XI) {
        if (q.k > 0) {                                         // the seam: from the last frame of the piece before into this one
            const float a_prev = lane < C ? p.vstart[slot * C + lane] : 0.f;
            hm_backward_step<CP, true>(arow, C, lane, lane < C ? p_rows[lane] : 1.f, a_prev, beta, S, bad);
        }
        if (lane < C) {
            double* out = p.xi_part + ((int64_t)blockIdx.x * C + lane) * C;
#pragma unroll
            for (int j = 0; j < CP; ++j)
                if (j < C) out[j] = (double)arow[j] * S[j];
        }
    }
    if (bad && lane == 0) atomicOr(p.flags, CBASX_HMM_FLAG_POSTERIOR);
}

__global__ void __launch_bounds__(HM_BLOCK) hm_reduce_kernel(HmArgs p) {
    const int C = p.C, CC = C * C;
    const int64_t idx = (int64_t)blockIdx.x * HM_BLOCK + threadIdx.x;
    if (idx < CC) {
        if (!p.xi) return;
        double total = 0.0;
        for (int c = 0; c < p.n_clips; ++c) {
            const long long g0 = p.offsets[c], g1 = p.offsets[c + 1];
            if (g1 <= g0) continue;
            double s = 0.0;
            for (long long g = g0; g < g1; ++g) s += p.xi_part[g * CC + idx];
            total += s;
        }
        p.xi[idx] = total;
    } else if (idx < CC + C) {
        if (!p.pi) return;
        const int j = (int)(idx - CC);
        double total = 0.0;
        for (int c = 0; c < p.n_clips; ++c) {
            int64_t base = 0;
            if (hm_clip(p.table, c, p.n_total, &base) > 0) total += (double)p.gamma[base * C + j];
        }
        p.pi[j] = total;
    } else if (idx < (int64_t)CC + C + p.n_clips) {
        if (!p.loglik) return;
        const int c = (int)(idx - CC - C);
        double s = 0.0;
        for (long long g = p.offsets[c]; g < p.offsets[c + 1]; ++g) s += p.ll_part[g];
        p.loglik[c] = s;
    }
}

template <int CP>
int hm_launch_cp(const HmArgs& a, long long pieces, long long long_pieces, hipStream_t st) {
    if (long_pieces > 0) {
        hipLaunchKernelGGL(hm_transfer_kernel<CP>, dim3((unsigned)long_pieces, (unsigned)a.C), dim3(64), 0, st, a);
        if (CHECK_LAUNCH()) return -2;
        hipLaunchKernelGGL(hm_scan_kernel, dim3((unsigned)a.n_clips, 2), dim3(64), 0, st, a);
        if (CHECK_LAUNCH()) return -2;
    }
    hipLaunchKernelGGL(hm_forward_kernel<CP>, dim3((unsigned)pieces), dim3(64), 0, st, a);
    if (CHECK_LAUNCH()) return -2;
    if (a.xi) hipLaunchKernelGGL((hm_backward_kernel<CP, true>), dim3((unsigned)pieces), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((hm_backward_kernel<CP, false>), dim3((unsigned)pieces), dim3(64), 0, st, a);
    return CHECK_LAUNCH();
}

int hm_launch(const HmArgs& a, long long pieces, long long long_pieces, hipStream_t st) {
    const int C = a.C;
    if (C <= 2) return hm_launch_cp<2>(a, pieces, long_pieces, st);
    if (C <= 4) return hm_launch_cp<4>(a, pieces, long_pieces, st);
    if (C <= 8) return hm_launch_cp<8>(a, pieces, long_pieces, st);
    if (C <= 16) return hm_launch_cp<16>(a, pieces, long_pieces, st);
    if (C <= 32) return hm_launch_cp<32>(a, pieces, long_pieces, st);
    return hm_launch_cp<64>(a, pieces, long_pieces, st);
}

unsigned hm_stream_blocks(int64_t items) {
    int64_t blocks = (items + HM_BLOCK - 1) / HM_BLOCK;
    return (unsigned)(blocks < 1 ? 1 : blocks > HM_MAX_STREAM_BLOCKS ? HM_MAX_STREAM_BLOCKS : blocks);
}

}  // namespace

extern "C" int64_t cbasx_hmm_workspace_bytes(int64_t n_total, int32_t n_clips, int32_t C) {
    HmLayout L;
    if (!hm_layout(n_total, n_clips, C, &L)) {
        cbas_fail(CBAS_EINVAL, "cbasx_hmm_workspace_bytes: n_total=%lld, n_clips=%d, C=%d: 0 <= n_total <= 2^40, n_clips >= 1, 1 <= C <= %d "
                  "and at most 2^31 - 1 pieces", (long long)n_total, n_clips, C, HM_MAXC);
        return -1;
    }
    return (int64_t)L.total;
}

extern "C" int cbasx_hmm_posteriors(const float* probs_dev, int64_t n_total, const int64_t* clip_table_dev, int32_t n_clips, int32_t C,
                                    const float* trans_dev, const float* prior_dev, float* gamma_dev, double* xi_dev, double* pi_dev,
                                    double* loglik_dev, uint32_t* flags_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (!probs_dev || !clip_table_dev || !trans_dev || !gamma_dev || !flags_dev || !workspace_dev)
        return cbas_fail(CBAS_EINVAL, "cbasx_hmm_posteriors: a NULL pointer among probs / clip_table / trans / gamma / flags / workspace");
    HmLayout L;
    if (!hm_layout(n_total, n_clips, C, &L))
        return cbas_fail(CBAS_EINVAL, "cbasx_hmm_posteriors: n_total=%lld, n_clips=%d, C=%d: 0 <= n_total <= 2^40, n_clips >= 1, 1 <= C <= %d "
                         "and at most 2^31 - 1 pieces", (long long)n_total, n_clips, C, HM_MAXC);
    if (workspace_bytes < (int64_t)L.total)
        return cbas_fail(CBAS_EINVAL, "cbasx_hmm_posteriors: the workspace holds %lld bytes, %lld are needed (cbasx_hmm_workspace_bytes)",
                         (long long)workspace_bytes, (long long)L.total);
    if ((uintptr_t)workspace_dev % 256) return cbas_fail(CBAS_EINVAL, "cbasx_hmm_posteriors: the workspace must be 256-byte aligned");
    if (((uintptr_t)probs_dev | (uintptr_t)trans_dev | (uintptr_t)prior_dev | (uintptr_t)gamma_dev | (uintptr_t)flags_dev) % 4 ||
        ((uintptr_t)clip_table_dev | (uintptr_t)xi_dev | (uintptr_t)pi_dev | (uintptr_t)loglik_dev) % 8)
        return cbas_fail(CBAS_EINVAL, "cbasx_hmm_posteriors: probs, trans, prior, gamma and flags must be 4-byte aligned, clip_table, xi, pi "
                         "and loglik 8-byte aligned");
    if (cbas_use_device_of(gamma_dev) != CBAS_OK) return CBAS_EHIP;
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace_dev);
    unsigned* bad_dev = reinterpret_cast<unsigned*>(ws + L.flags);
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    int* lcounts = reinterpret_cast<int*>(ws + L.lcounts);
    long long* offsets = reinterpret_cast<long long*>(ws + L.offsets);
    long long* loffsets = reinterpret_cast<long long*>(ws + L.loffsets);

    // the checking pass: writes into the workspace only
    HIP_TRY(hipMemsetAsync(bad_dev, 0, 256, st));
    const int64_t items = n_clips > C ? n_clips : C;
    hipLaunchKernelGGL(hm_check_kernel, dim3(hm_stream_blocks(items)), dim3(HM_BLOCK), 0, st, n_total, clip_table_dev, n_clips, C, trans_dev,
                       prior_dev, counts, lcounts, bad_dev);
    LAUNCH_TRY(CHECK_LAUNCH());
    LAUNCH_TRY(launch_runs_scan(counts, n_clips, offsets, st));
    LAUNCH_TRY(launch_runs_scan(lcounts, n_clips, loffsets, st));
    unsigned bad = 0;
    long long pieces = 0, long_pieces = 0;
    HIP_TRY(hipMemcpyAsync(&bad, bad_dev, sizeof(bad), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&pieces, offsets + n_clips, sizeof(pieces), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&long_pieces, loffsets + n_clips, sizeof(long_pieces), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad & HM_BAD_TABLE)
        return cbas_fail(CBAS_EINVAL, "cbasx_hmm_posteriors: a clip table entry reaches outside the %lld frames of probs", (long long)n_total);
    if (bad & HM_BAD_TRANS)
        return cbas_fail(CBAS_EINVAL, "cbasx_hmm_posteriors: a row of the transitions is not finite, negative or does not sum to 1 within 1e-4");
    if (bad & HM_BAD_PRIOR)
        return cbas_fail(CBAS_EINVAL, "cbasx_hmm_posteriors: the prior is not finite, negative or does not sum to 1 within 1e-4");
    if (pieces > L.pieces || long_pieces > L.long_pieces)
        return cbas_fail(CBAS_EINVAL, "cbasx_hmm_posteriors: the clips hold more frames than the %lld of probs: clips must not overlap",
                         (long long)n_total);

    if (n_total > 0) HIP_TRY(hipMemsetAsync(gamma_dev, 0, (size_t)n_total * C * sizeof(float), st));      // rows owned by no clip
    const HmArgs a{probs_dev, n_total, clip_table_dev, n_clips, C, trans_dev, prior_dev, gamma_dev, xi_dev, pi_dev, loglik_dev, flags_dev,
                   offsets, loffsets, reinterpret_cast<float*>(ws + L.t_d), reinterpret_cast<int*>(ws + L.t_exp),
                   reinterpret_cast<float*>(ws + L.vstart), reinterpret_cast<float*>(ws + L.bend), reinterpret_cast<double*>(ws + L.xi_part),
                   reinterpret_cast<double*>(ws + L.ll_part)};
    if (pieces > 0) LAUNCH_TRY(hm_launch(a, pieces, long_pieces, st));
    if (xi_dev || pi_dev || loglik_dev) {
        hipLaunchKernelGGL(hm_reduce_kernel, dim3((unsigned)(((int64_t)C * C + C + n_clips + HM_BLOCK - 1) / HM_BLOCK)), dim3(HM_BLOCK), 0, st, a);
        LAUNCH_TRY(CHECK_LAUNCH());
    }
    return CBAS_OK;
}
