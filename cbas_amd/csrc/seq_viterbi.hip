// Sequence decoding (include/cbas_mi355x_ext.h): the Viterbi path of every clip under a first-order
// transition model, from per-frame probabilities that are already on the device.
//
//   vt_scores_kernel     p -> clamp(rint(256 * log2 p), -8192, 0) as int32: the only floating point of this file.
//   vt_check_kernel      the refusals that need device data - table entries, transitions, prior, scores - and, per clip, its
//                        number of pieces of CBASX_VITERBI_CHUNK frames.  Writes into the workspace only.
//   vt_transfer_kernel   (clips of more than one piece) per piece and start state s one forward run without back-pointers: row
//                        s of the piece's max-plus transfer matrix.  The first piece of a clip has one run, from the prior.
//   vt_scan_kernel       (the same clips) one wave per clip walks the pieces, not the frames: the exact d at every piece's
//                        start, kept as an int32 vector below its own maximum and that maximum in int64.
//   vt_forward_kernel    per piece the serial forward pass from its start vector; writes uint8 back-pointers; the last piece
//                        of a clip finds the end state and the clip's score.
//   vt_backmap_kernel    per piece, from LDS, the map end state -> end state of the piece before, for all C end states.
//   vt_compose_kernel    per clip the composition of those maps, last piece to first: every piece's end state.
//   vt_emit_kernel       per piece the path from its end state, from LDS, and the labels in one coalesced write.
//
// A state is a lane (C <= 64 = one wave); lane j keeps column j of the transition matrix in registers, d_{t-1}[i] comes through
// v_readlane.  All arithmetic after the scores is integer, hence associative: cutting a clip into pieces changes no bit.  d is
// brought below its maximum every VT_RENORM steps (64 * (2^20 + 8192) < 2^27: no int32 overflow between two of them) and the
// maxima are summed in int64.  No atomic but the integer flag; no floating point after vt_scores_kernel.
#include <limits.h>
#include "api_common.h"
#include "kernels.h"
#include "../../include/cbas_mi355x_ext.h"

namespace {

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -2)

constexpr int VT_CHUNK = CBASX_VITERBI_CHUNK;
constexpr int VT_MAXC = CBASX_VITERBI_MAX_CLASSES;
constexpr int VT_LIMIT = CBASX_VITERBI_TRANS_LIMIT;
constexpr int VT_EMIN = CBASX_VITERBI_SCORE_MIN;
constexpr int VT_RENORM = 64;                          // forward steps between two renormalisations
constexpr int VT_BLOCK = 256;                          // the streaming and the LDS kernels
constexpr int VT_SEGS = 16;                            // vt_compose_kernel: segments of pieces composed side by side
constexpr int VT_MAX_STREAM_BLOCKS = 2048;
constexpr int64_t VT_MAX_FRAMES = (int64_t)1 << 40;
constexpr unsigned VT_FLAG_TABLE = 1u, VT_FLAG_TRANS = 2u, VT_FLAG_PRIOR = 4u, VT_FLAG_SCORE = 8u;
static_assert(VT_MAXC == 64 && VT_CHUNK % 8 == 0 && VT_CHUNK >= 8, "a state is a lane; the forward pass loads 8 frames ahead");

// the workspace: byte offsets of its parts (all multiples of 256) and its size
struct VtLayout {
    int64_t pieces, long_pieces;                       // capacities: all pieces; pieces of clips of more than one
    size_t flags, counts, lcounts, offsets, loffsets, end, map, t_rel, t_off, vstart, vbase, bp, total;
};

bool vt_layout(int64_t n_total, int n_clips, int C, VtLayout* L) {
    if (n_total < 0 || n_total > VT_MAX_FRAMES || n_clips < 1 || C < 1 || C > VT_MAXC) return false;
    // sum over clips of ceil(n_c / CHUNK) <= n_total / CHUNK + n_clips for clips that do not overlap; a clip of more than one
    // piece has ceil(n_c / CHUNK) < 2 n_c / CHUNK
    L->pieces = n_total / VT_CHUNK + n_clips;
    L->long_pieces = 2 * (n_total / VT_CHUNK) + 1;
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
    L->end = part(K * 4);
    L->map = part(K * c);
    L->t_rel = part(KT * c * c * 4);
    L->t_off = part(KT * c * 8);
    L->vstart = part(KT * c * 4);
    L->vbase = part(KT * 8);
    L->bp = part((size_t)n_total * c + 16);
    L->total = at;
    return true;
}

struct VtArgs {
    const int* scores;
    int64_t n_total;
    const int64_t* table;
    int n_clips, C;
    const int* trans;
    const int* prior;                                  // may be null
    int* labels;
    long long* clip_score;                             // may be null
    const int* counts;
    const int* lcounts;
    const long long* offsets;
    const long long* loffsets;
    int* end;
    uint8_t* map;
    int* t_rel;
    long long* t_off;
    int* vstart;
    long long* vbase;
    uint8_t* bp;
};

__global__ void __launch_bounds__(VT_BLOCK)
vt_scores_kernel(const float* __restrict__ probs, int64_t n, int* __restrict__ scores, unsigned* flags) {
    bool nan = false;
    for (int64_t i = (int64_t)blockIdx.x * VT_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * VT_BLOCK) {
        const float p = probs[i];
        nan |= p != p;
        const float q = p >= 0x1p-32f ? p : 0x1p-32f;          // a NaN, a negative and a denormal: 2^-32
        const int bits = __float_as_int(q);
        int e;
        if ((bits & 0x7fffff) == 0) e = (((bits >> 23) & 0xff) - 127) * CBASX_VITERBI_UNIT;      // a power of two: exact
        else e = (int)rintf((float)CBASX_VITERBI_UNIT * log2f(q));
        scores[i] = e < VT_EMIN ? VT_EMIN : e > 0 ? 0 : e;
    }
    if (nan) atomicOr(flags, CBASX_VITERBI_FLAG_NAN);
}

// frames of clip c, or -1 for an entry that reaches outside [0, n_total); *base = its first frame
__device__ __forceinline__ int64_t vt_clip(const int64_t* __restrict__ table, int c, int64_t n_total, int64_t* base) {
    const int64_t b = table[2 * (int64_t)c], n = table[2 * (int64_t)c + 1];
    if (b < 0 || n < 0 || n > 0x7fffffff || b > n_total || n > n_total - b) return -1;
    *base = b;
    return n;
}

__global__ void __launch_bounds__(VT_BLOCK)
vt_check_kernel(const int* __restrict__ scores, int64_t n_total, const int64_t* __restrict__ table, int n_clips, int C,
                const int* __restrict__ trans, const int* __restrict__ prior, int* __restrict__ counts, int* __restrict__ lcounts,
                unsigned* flags) {
    const int64_t tid = (int64_t)blockIdx.x * VT_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * VT_BLOCK;
    unsigned bad = 0;
    for (int64_t c = tid; c < n_clips; c += stride) {
        int64_t base = 0;
        const int64_t n = vt_clip(table, (int)c, n_total, &base);
        const int pieces = n < 0 ? 0 : (int)((n + VT_CHUNK - 1) / VT_CHUNK);
        if (n < 0) bad |= VT_FLAG_TABLE;
        counts[c] = pieces;
        lcounts[c] = pieces > 1 ? pieces : 0;
    }
    for (int64_t i = tid; i < C * C; i += stride)
        if (trans[i] < -VT_LIMIT || trans[i] > VT_LIMIT) bad |= VT_FLAG_TRANS;
    if (prior)
        for (int64_t i = tid; i < C; i += stride)
            if (prior[i] < -VT_LIMIT || prior[i] > VT_LIMIT) bad |= VT_FLAG_PRIOR;
    for (int64_t i = tid; i < n_total * C; i += stride)
        if (scores[i] < VT_EMIN || scores[i] > 0) bad |= VT_FLAG_SCORE;
    if (bad) atomicOr(flags, bad);
}

// the largest c with offsets[c] <= g, for 0 <= g < offsets[n]: the clip that owns piece g (clips without pieces share the
// offset of the next one and are stepped over)
__device__ __forceinline__ int vt_find(const long long* __restrict__ offsets, int n, long long g) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// a piece: clip, number within the clip, pieces of the clip, first frame in the call's arrays, frames
struct VtPiece {
    int clip, k, pieces, len;
    int64_t t0;
};

__device__ __forceinline__ bool vt_piece(const VtArgs& p, const long long* __restrict__ offsets, long long g, VtPiece* q) {
    q->clip = vt_find(offsets, p.n_clips, g);
    const long long k = g - offsets[q->clip];
    int64_t base = 0;
    const int64_t n = vt_clip(p.table, q->clip, p.n_total, &base);      // checked again: nothing is indexed with an unchecked entry
    if (n < 0 || k < 0 || k * VT_CHUNK >= n) return false;
    q->k = (int)k;
    q->pieces = (int)((n + VT_CHUNK - 1) / VT_CHUNK);
    q->t0 = base + k * VT_CHUNK;
    q->len = (int)(n - k * VT_CHUNK < VT_CHUNK ? n - k * VT_CHUNK : VT_CHUNK);
    return true;
}

__device__ __forceinline__ int vt_wave_max(int d, int lane, int C) {
    int v = lane < C ? d : INT_MIN;
    for (int o = 32; o; o >>= 1) {
        const int w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

__device__ __forceinline__ long long vt_wave_max64(long long d, int lane, int C) {
    long long v = lane < C ? d : LLONG_MIN;
    for (int o = 32; o; o >>= 1) {
        const long long w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

template <int CP>
__device__ __forceinline__ void vt_load_column(int (&a)[CP], const int* __restrict__ trans, int C, int lane) {
#pragma unroll
    for (int i = 0; i < CP; ++i) a[i] = (i < C && lane < C) ? trans[i * C + lane] : 0;
}

// one step: d[j] = max_i (d[i] + a[i]) + e, arg = the lowest i that attains it
template <int CP>
__device__ __forceinline__ void vt_step(const int (&a)[CP], int C, int e, int& d, int& arg) {
    int best = __builtin_amdgcn_readlane(d, 0) + a[0];
    arg = 0;
#pragma unroll
    for (int i = 1; i < CP; ++i) {
        if (i < C) {                                           // uniform
            const int cand = __builtin_amdgcn_readlane(d, i) + a[i];
            arg = cand > best ? i : arg;
            best = cand > best ? cand : best;
        }
    }
    d = best + e;
}

// `steps` frames from e_rows (and, with BP, their back-pointers to bp_rows); d is brought below its maximum every VT_RENORM
// steps and the maxima are added to acc
template <int CP, bool BP>
__device__ __forceinline__ void vt_run(const int (&a)[CP], int C, int lane, const int* __restrict__ e_rows, uint8_t* __restrict__ bp_rows,
                                       int steps, int& d, long long& acc) {
    constexpr int U = 8;
    int since = 0;
    for (int t0 = 0; t0 < steps; t0 += U) {
        int e[U];
#pragma unroll
        for (int u = 0; u < U; ++u) e[u] = (t0 + u < steps && lane < C) ? e_rows[(int64_t)(t0 + u) * C + lane] : 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t0 + u < steps) {                              // uniform
                int arg;
                vt_step<CP>(a, C, e[u], d, arg);
                if (BP && lane < C) bp_rows[(int64_t)(t0 + u) * C + lane] = (uint8_t)arg;
            }
        }
        since += U;
        if (since >= VT_RENORM) {
            const int m = vt_wave_max(d, lane, C);
            d -= m;
            acc += m;
            since = 0;
        }
    }
}

template <int CP>
__global__ void __launch_bounds__(64) vt_transfer_kernel(VtArgs p) {
    const int lane = threadIdx.x, C = p.C, s = blockIdx.y;
    VtPiece q;
    if (!vt_piece(p, p.loffsets, blockIdx.x, &q)) return;
    if (q.k == q.pieces - 1 || (q.k == 0 && s != 0)) return;   // nothing follows the last piece; the first starts from the prior
    int a[CP];
    vt_load_column<CP>(a, p.trans, C, lane);
    const int* e_rows = p.scores + q.t0 * C;
    int d = 0;
    if (lane < C) d = (q.k == 0 ? (p.prior ? p.prior[lane] : 0) : p.trans[s * C + lane]) + e_rows[lane];
    long long acc = 0;
    vt_run<CP, false>(a, C, lane, e_rows + C, nullptr, q.len - 1, d, acc);
    const int m = vt_wave_max(d, lane, C);
    const int64_t row = (int64_t)blockIdx.x * C + s;
    if (lane < C) p.t_rel[row * C + lane] = d - m;
    if (lane == 0) p.t_off[row] = acc + m;
}

__global__ void __launch_bounds__(64) vt_scan_kernel(VtArgs p) {
    __shared__ int T[VT_MAXC * VT_MAXC];
    __shared__ long long toff[VT_MAXC];
    const int lane = threadIdx.x, C = p.C, c = blockIdx.x;
    int64_t base = 0;
    const int64_t n = vt_clip(p.table, c, p.n_total, &base);
    if (n <= VT_CHUNK) return;
    const int pieces = (int)((n + VT_CHUNK - 1) / VT_CHUNK);
    const int64_t slot0 = p.loffsets[c];
    // d at the last frame of piece 0: row 0 of its slot
    long long v = lane < C ? p.t_off[slot0 * C] + p.t_rel[slot0 * C * C + lane] : 0;
    for (int k = 1; k < pieces; ++k) {
        const int64_t slot = slot0 + k;
        const long long m = vt_wave_max64(v, lane, C);
        if (lane < C) p.vstart[slot * C + lane] = (int)(v - m);
        if (lane == 0) p.vbase[slot] = m;
        if (k == pieces - 1) break;
        for (int i = lane; i < C * C; i += 64) T[i] = p.t_rel[slot * C * C + i];
        if (lane < C) toff[lane] = p.t_off[slot * C + lane];
        __syncthreads();
        const long long u = lane < C ? v + toff[lane] : 0;
        const int ulo = (int)(unsigned)(u & 0xffffffffll), uhi = (int)(u >> 32);
        long long best = LLONG_MIN;
        for (int s = 0; s < C; ++s) {
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane(ulo, s);
            const long long us = ((long long)__builtin_amdgcn_readlane(uhi, s) << 32) | (long long)lo;
            const long long cand = us + T[s * C + (lane < C ? lane : 0)];
            best = cand > best ? cand : best;
        }
        v = best;
        __syncthreads();
    }
}

template <int CP>
__global__ void __launch_bounds__(64) vt_forward_kernel(VtArgs p) {
    const int lane = threadIdx.x, C = p.C;
    VtPiece q;
    if (!vt_piece(p, p.offsets, blockIdx.x, &q)) return;
    int a[CP];
    vt_load_column<CP>(a, p.trans, C, lane);
    const int* e_rows = p.scores + q.t0 * C;
    uint8_t* bp_rows = p.bp + q.t0 * C;
    int d = 0;
    long long acc = 0, start = 0;
    if (q.k == 0) {
        if (lane < C) d = (p.prior ? p.prior[lane] : 0) + e_rows[lane];
        vt_run<CP, true>(a, C, lane, e_rows + C, bp_rows + C, q.len - 1, d, acc);
    } else {
        const int64_t slot = p.loffsets[q.clip] + q.k;
        if (lane < C) d = p.vstart[slot * C + lane];
        start = p.vbase[slot];
        vt_run<CP, true>(a, C, lane, e_rows, bp_rows, q.len, d, acc);
    }
    if (q.k == q.pieces - 1) {
        const int m = vt_wave_max(d, lane, C);
        const unsigned long long at = __ballot(lane < C && d == m);
        if (lane == 0) {
            p.end[blockIdx.x] = __ffsll((long long)at) - 1;    // the lowest state that attains the maximum
            if (p.clip_score) p.clip_score[q.clip] = start + acc + m;
        }
    }
}

// the back-pointers of a piece into LDS, 16 bytes per thread and pass where the source allows: the image starts at the
// source's own offset within 16 bytes.  Returns the image; lds holds vt_stage_bytes(C) bytes.
__device__ __forceinline__ uint8_t* vt_stage(uint8_t* lds, const uint8_t* __restrict__ src, int nbytes) {
    const int mis = (int)((uintptr_t)src & 15);
    uint8_t* dst = lds + mis;
    const int head = mis ? (16 - mis < nbytes ? 16 - mis : nbytes) : 0;
    for (int i = threadIdx.x; i < head; i += VT_BLOCK) dst[i] = src[i];
    const int body = (nbytes - head) / 16;
    const uint4* s4 = reinterpret_cast<const uint4*>(src + head);
    uint4* d4 = reinterpret_cast<uint4*>(dst + head);
    for (int i = threadIdx.x; i < body; i += VT_BLOCK) d4[i] = s4[i];
    for (int i = head + body * 16 + threadIdx.x; i < nbytes; i += VT_BLOCK) dst[i] = src[i];
    return dst;
}

// a piece's back-pointers and the at most 15 bytes before its image; for C = 64 every piece starts on a multiple of 64 bytes
// and the image needs none, so 64 KB are never exceeded
constexpr unsigned vt_stage_bytes(int C) { return C == VT_MAXC ? VT_CHUNK * VT_MAXC : VT_CHUNK * C + 16; }
extern __shared__ __attribute__((aligned(16))) uint8_t vt_lds[];

__global__ void __launch_bounds__(VT_BLOCK) vt_backmap_kernel(VtArgs p) {
    uint8_t* lds = vt_lds;
    const int C = p.C;
    VtPiece q;
    if (!vt_piece(p, p.offsets, blockIdx.x, &q)) return;
    if (q.k == 0) return;                                      // no piece lies before the first
    const uint8_t* stage = vt_stage(lds, p.bp + q.t0 * C, q.len * C);
    __syncthreads();
    if ((int)threadIdx.x < C) {
        int cur = threadIdx.x;
        for (int t = q.len - 1; t >= 1; --t) cur = stage[t * C + cur];
        p.map[(int64_t)blockIdx.x * C + threadIdx.x] = stage[cur];          // row 0: the state at the last frame of piece k - 1
    }
}

__global__ void __launch_bounds__(VT_SEGS * 64) vt_compose_kernel(VtArgs p) {
    __shared__ uint8_t seg[VT_SEGS][VT_MAXC];
    __shared__ int seg_end[VT_SEGS];
    const int C = p.C, c = blockIdx.x, sg = threadIdx.x >> 6, s = threadIdx.x & 63;
    int64_t base = 0;
    const int64_t n = vt_clip(p.table, c, p.n_total, &base);
    if (n <= VT_CHUNK) return;
    const int pieces = (int)((n + VT_CHUNK - 1) / VT_CHUNK);
    const int64_t g0 = p.offsets[c];
    // pieces pieces - 1 .. 1 carry a map; segment sg holds those from hi down to lo
    const int L = (pieces - 1 + VT_SEGS - 1) / VT_SEGS;
    const int hi = pieces - 1 - sg * L, lo = hi - L + 1 > 1 ? hi - L + 1 : 1;
    if (s < C) {
        int cur = s;
        for (int k = hi; k >= lo; --k) cur = p.map[(g0 + k) * C + cur];
        seg[sg][s] = (uint8_t)cur;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int e = p.end[g0 + pieces - 1];
        e = e < 0 || e >= C ? 0 : e;
        for (int g = 0; g < VT_SEGS; ++g) {
            seg_end[g] = e;
            if (pieces - 1 - g * L >= 1) e = seg[g][e];
        }
    }
    __syncthreads();
    if (s == 0) {
        int e = seg_end[sg];
        for (int k = hi; k >= lo; --k) {
            e = p.map[(g0 + k) * C + e];
            p.end[g0 + k - 1] = e;
        }
    }
}

__global__ void __launch_bounds__(VT_BLOCK) vt_emit_kernel(VtArgs p) {
    uint8_t* lds = vt_lds;
    const int C = p.C;
    VtPiece q;
    if (!vt_piece(p, p.offsets, blockIdx.x, &q)) return;
    uint8_t* stage = vt_stage(lds, p.bp + q.t0 * C, q.len * C);
    __syncthreads();
    if (threadIdx.x == 0) {
        int cur = p.end[blockIdx.x];
        cur = cur < 0 || cur >= C ? 0 : cur;
        for (int t = q.len - 1; t >= 0; --t) {
            const int prev = t > 0 ? stage[t * C + cur] : 0;  // row 0 belongs to the piece before (vt_backmap_kernel)
            stage[t * C] = (uint8_t)cur;                       // the path takes the place of column 0 of the rows already read
            cur = prev;
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < q.len; t += VT_BLOCK) p.labels[q.t0 + t] = stage[t * C];
}

template <int CP>
int vt_launch_cp(const VtArgs& a, long long pieces, long long long_pieces, hipStream_t st) {
    if (long_pieces > 0) {
        hipLaunchKernelGGL(vt_transfer_kernel<CP>, dim3((unsigned)long_pieces, (unsigned)a.C), dim3(64), 0, st, a);
        if (CHECK_LAUNCH()) return -2;
        hipLaunchKernelGGL(vt_scan_kernel, dim3((unsigned)a.n_clips), dim3(64), 0, st, a);
        if (CHECK_LAUNCH()) return -2;
    }
    hipLaunchKernelGGL(vt_forward_kernel<CP>, dim3((unsigned)pieces), dim3(64), 0, st, a);
    if (CHECK_LAUNCH()) return -2;
    if (long_pieces > 0) {
        hipLaunchKernelGGL(vt_backmap_kernel, dim3((unsigned)pieces), dim3(VT_BLOCK), vt_stage_bytes(a.C), st, a);
        if (CHECK_LAUNCH()) return -2;
        hipLaunchKernelGGL(vt_compose_kernel, dim3((unsigned)a.n_clips), dim3(VT_SEGS * 64), 0, st, a);
        if (CHECK_LAUNCH()) return -2;
    }
    hipLaunchKernelGGL(vt_emit_kernel, dim3((unsigned)pieces), dim3(VT_BLOCK), vt_stage_bytes(a.C), st, a);
    return CHECK_LAUNCH();
}

int vt_launch(const VtArgs& a, long long pieces, long long long_pieces, hipStream_t st) {
    const int C = a.C;
    if (C <= 2) return vt_launch_cp<2>(a, pieces, long_pieces, st);
    if (C <= 4) return vt_launch_cp<4>(a, pieces, long_pieces, st);
    if (C <= 8) return vt_launch_cp<8>(a, pieces, long_pieces, st);
    if (C <= 16) return vt_launch_cp<16>(a, pieces, long_pieces, st);
    if (C <= 32) return vt_launch_cp<32>(a, pieces, long_pieces, st);
    return vt_launch_cp<64>(a, pieces, long_pieces, st);
}

unsigned vt_stream_blocks(int64_t items) {
    int64_t blocks = (items + VT_BLOCK - 1) / VT_BLOCK;
    return (unsigned)(blocks < 1 ? 1 : blocks > VT_MAX_STREAM_BLOCKS ? VT_MAX_STREAM_BLOCKS : blocks);
}

}  // namespace

extern "C" int cbasx_viterbi_scores(const float* probs_dev, int64_t n_total, int32_t C, int32_t* scores_dev, uint32_t* flags_dev,
                                    void* stream) {
    if (!probs_dev || !scores_dev || !flags_dev) return cbas_fail(CBAS_EINVAL, "cbasx_viterbi_scores: probs_dev / scores_dev / flags_dev NULL");
    if (n_total < 0 || n_total > VT_MAX_FRAMES || C < 1 || C > VT_MAXC)
        return cbas_fail(CBAS_EINVAL, "cbasx_viterbi_scores: n_total=%lld, C=%d: 0 <= n_total <= 2^40 and 1 <= C <= %d", (long long)n_total, C, VT_MAXC);
    if (((uintptr_t)probs_dev | (uintptr_t)scores_dev | (uintptr_t)flags_dev) % 4)
        return cbas_fail(CBAS_EINVAL, "cbasx_viterbi_scores: probs_dev, scores_dev and flags_dev must be 4-byte aligned");
    if (n_total == 0) return CBAS_OK;
    hipLaunchKernelGGL(vt_scores_kernel, dim3(vt_stream_blocks(n_total * C)), dim3(VT_BLOCK), 0, (hipStream_t)stream, probs_dev, n_total * C,
                       scores_dev, flags_dev);
    LAUNCH_TRY(CHECK_LAUNCH());
    return CBAS_OK;
}

extern "C" int64_t cbasx_viterbi_workspace_bytes(int64_t n_total, int32_t n_clips, int32_t C) {
    VtLayout L;
    if (!vt_layout(n_total, n_clips, C, &L)) {
        cbas_fail(CBAS_EINVAL, "cbasx_viterbi_workspace_bytes: n_total=%lld, n_clips=%d, C=%d: 0 <= n_total <= 2^40, n_clips >= 1, 1 <= C <= %d "
                  "and at most 2^31 - 1 pieces", (long long)n_total, n_clips, C, VT_MAXC);
        return -1;
    }
    return (int64_t)L.total;
}

extern "C" int cbasx_viterbi_decode(const int32_t* scores_dev, int64_t n_total, const int64_t* clip_table_dev, int32_t n_clips, int32_t C,
                                    const int32_t* log_trans_dev, const int32_t* log_prior_dev, int32_t* labels_dev,
                                    int64_t* clip_score_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (!scores_dev || !clip_table_dev || !log_trans_dev || !labels_dev || !workspace_dev)
        return cbas_fail(CBAS_EINVAL, "cbasx_viterbi_decode: a NULL pointer among scores / clip_table / log_trans / labels / workspace");
    VtLayout L;
    if (!vt_layout(n_total, n_clips, C, &L))
        return cbas_fail(CBAS_EINVAL, "cbasx_viterbi_decode: n_total=%lld, n_clips=%d, C=%d: 0 <= n_total <= 2^40, n_clips >= 1, 1 <= C <= %d "
                         "and at most 2^31 - 1 pieces", (long long)n_total, n_clips, C, VT_MAXC);
    if (workspace_bytes < (int64_t)L.total)
        return cbas_fail(CBAS_EINVAL, "cbasx_viterbi_decode: the workspace holds %lld bytes, %lld are needed (cbasx_viterbi_workspace_bytes)",
                         (long long)workspace_bytes, (long long)L.total);
    if ((uintptr_t)workspace_dev % 256) return cbas_fail(CBAS_EINVAL, "cbasx_viterbi_decode: the workspace must be 256-byte aligned");
    if (((uintptr_t)scores_dev | (uintptr_t)log_trans_dev | (uintptr_t)log_prior_dev | (uintptr_t)labels_dev) % 4 ||
        ((uintptr_t)clip_table_dev | (uintptr_t)clip_score_dev) % 8)
        return cbas_fail(CBAS_EINVAL, "cbasx_viterbi_decode: scores, log_trans, log_prior and labels must be 4-byte aligned, clip_table and "
                         "clip_score 8-byte aligned");
    if (cbas_use_device_of(scores_dev) != CBAS_OK) return CBAS_EHIP;
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace_dev);
    unsigned* flags = reinterpret_cast<unsigned*>(ws + L.flags);
    int* counts = reinterpret_cast<int*>(ws + L.counts);
    int* lcounts = reinterpret_cast<int*>(ws + L.lcounts);
    long long* offsets = reinterpret_cast<long long*>(ws + L.offsets);
    long long* loffsets = reinterpret_cast<long long*>(ws + L.loffsets);

    // the checking pass: writes into the workspace only
    HIP_TRY(hipMemsetAsync(flags, 0, 256, st));
    const int64_t items = n_total * C > n_clips ? n_total * C : n_clips;
    hipLaunchKernelGGL(vt_check_kernel, dim3(vt_stream_blocks(items)), dim3(VT_BLOCK), 0, st, scores_dev, n_total, clip_table_dev, n_clips, C,
                       log_trans_dev, log_prior_dev, counts, lcounts, flags);
    LAUNCH_TRY(CHECK_LAUNCH());
    LAUNCH_TRY(launch_runs_scan(counts, n_clips, offsets, st));
    LAUNCH_TRY(launch_runs_scan(lcounts, n_clips, loffsets, st));
    unsigned bad = 0;
    long long pieces = 0, long_pieces = 0;
    HIP_TRY(hipMemcpyAsync(&bad, flags, sizeof(bad), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&pieces, offsets + n_clips, sizeof(pieces), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&long_pieces, loffsets + n_clips, sizeof(long_pieces), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad & VT_FLAG_TABLE)
        return cbas_fail(CBAS_EINVAL, "cbasx_viterbi_decode: a clip table entry reaches outside the %lld frames of scores", (long long)n_total);
    if (bad & VT_FLAG_TRANS) return cbas_fail(CBAS_EINVAL, "cbasx_viterbi_decode: a transition lies outside [-2^20, 2^20]");
    if (bad & VT_FLAG_PRIOR) return cbas_fail(CBAS_EINVAL, "cbasx_viterbi_decode: a prior lies outside [-2^20, 2^20]");
    if (bad & VT_FLAG_SCORE) return cbas_fail(CBAS_EINVAL, "cbasx_viterbi_decode: a score lies outside [%d, 0]", VT_EMIN);
    if (pieces > L.pieces || long_pieces > L.long_pieces)
        return cbas_fail(CBAS_EINVAL, "cbasx_viterbi_decode: the clips hold more frames than the %lld of scores: clips must not overlap",
                         (long long)n_total);

    if (n_total > 0) HIP_TRY(hipMemsetAsync(labels_dev, 0xff, (size_t)n_total * sizeof(int32_t), st));      // -1: owned by no clip
    if (clip_score_dev) HIP_TRY(hipMemsetAsync(clip_score_dev, 0, (size_t)n_clips * sizeof(int64_t), st));
    if (pieces == 0) return CBAS_OK;
    const VtArgs a{scores_dev, n_total, clip_table_dev, n_clips, C, log_trans_dev, log_prior_dev, labels_dev,
                   reinterpret_cast<long long*>(clip_score_dev), counts, lcounts, offsets, loffsets, reinterpret_cast<int*>(ws + L.end),
                   reinterpret_cast<uint8_t*>(ws + L.map), reinterpret_cast<int*>(ws + L.t_rel), reinterpret_cast<long long*>(ws + L.t_off),
                   reinterpret_cast<int*>(ws + L.vstart), reinterpret_cast<long long*>(ws + L.vbase), reinterpret_cast<uint8_t*>(ws + L.bp)};
    LAUNCH_TRY(vt_launch(a, pieces, long_pieces, st));
    return CBAS_OK;
}
