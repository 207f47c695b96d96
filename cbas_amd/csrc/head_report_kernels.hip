// The kernels behind the disagreement report of a training job (backend/workthreads.py:760-803): what the reference does with
// pandas on the `_outputs.csv` of every training clip, on probabilities that are already on the device.
//
//   probs_top1_kernel   probs (n, C) -> index of the first row maximum (pandas idxmax / torch.argmax) and that maximum
//                       (:762-763).
//   the run scan        per labelled instance, the maximal runs of consecutive frames whose prediction differs from the human
//                       label, each with its most frequent prediction and its mean confidence (:777-803).
//
// The scan writes records whose number is not known in advance, in an order that must not depend on the order of execution, so
// nothing is appended with an atomic.  Four launches:
//   runs_count_kernel   one workgroup per instance walks its frames 256 at a time and counts the run starts (an error frame
//                       whose predecessor inside the instance is no error frame); it also validates the instance and every
//                       table entry and prediction it reads, BEFORE anything is indexed with them.
//   runs_scan_kernel    exclusive scan of the counts by one workgroup: record offsets per instance and the total.
//   runs_mark_kernel    the same walk again: the k-th run start and the k-th run end of an instance (both found by ballots and
//                       a running count, in ascending frame order) are written to record offset + k.
//   runs_reduce_kernel  one wave per record: lane l adds the confidences of frames start + l, start + l + 64, ... in ascending
//                       order in float64, a fixed butterfly combines the 64 partial sums; the predictions are counted into a
//                       per-wave histogram in LDS with integer atomics (order-free) and the winner is the largest count, ties
//                       going to the smallest name rank (pandas mode() returns sorted values, the reference takes [0]).
// A record is a function of its run alone: the same run reported by two overlapping instances has the same bits.  For top-1
// probabilities (>= 1 / C >= 2^-6, <= 1) every partial sum of up to 2^22 float32 confidences is exact in float64, so the sum equals
// the one taken in ascending frame order bit for bit; for other values it is a float64 sum in the fixed order above.
#include "kernels.h"
#include "run_sum.h"

namespace {

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -2)

constexpr int TOP1_BLOCK = 256;
constexpr int RUNS_BLOCK = 256;
constexpr int RUNS_WAVES = RUNS_BLOCK / 64;

__global__ void __launch_bounds__(TOP1_BLOCK)
probs_top1_kernel(const float* __restrict__ probs, int64_t n, int C, int* __restrict__ pred, float* __restrict__ conf,
                  unsigned* flags) {
    const int64_t r = (int64_t)blockIdx.x * TOP1_BLOCK + threadIdx.x;
    if (r >= n) return;
    const float* p = probs + r * C;
    float best = p[0];
    int arg = 0;
    bool nan = best != best;
    for (int c = 1; c < C; ++c) {
        const float v = p[c];
        nan |= v != v;
        if (v > best) { best = v; arg = c; }                   // strict: the first of equal maxima stays
    }
    if (nan) atomicOr(flags, HEAD_SCORE_FLAG_NAN);
    pred[r] = nan ? -1 : arg;
    conf[r] = nan ? __builtin_nanf("") : best;
}

// What one workgroup knows about its instance after validation.  `hi < lo`: no frame (also for a refused instance).
struct InstanceRange {
    int64_t base;      // first frame of the clip in pred / conf
    int lo, hi;        // frames [lo, hi] of the clip
    int label;
};

__device__ __forceinline__ InstanceRange instance_range(const RunsParams& p, int i, unsigned* flags) {
    InstanceRange r{0, 0, -1, -1};
    const int c = p.inst_clip[i], start = p.inst_start[i], end = p.inst_end[i], label = p.inst_label[i];
    unsigned bad = 0;
    if (c < 0 || c >= p.n_clips) bad |= RUNS_FLAG_CLIP;
    if (label < -1 || label >= p.n_classes) bad |= RUNS_FLAG_LABEL;
    if (start < 0 || end < start) bad |= RUNS_FLAG_RANGE;
    if (!(bad & RUNS_FLAG_CLIP)) {
        const int64_t base = p.clip_table[2 * (int64_t)c], n = p.clip_table[2 * (int64_t)c + 1];
        if (base < 0 || n < 0 || n > 0x7fffffff || base > p.n_frames_total || n > p.n_frames_total - base) bad |= RUNS_FLAG_TABLE;
        else if (!bad) {
            r.base = base;
            r.lo = start;
            r.hi = (int)((int64_t)end < n - 1 ? (int64_t)end : n - 1);
            r.label = label;
        }
    }
    if (bad && threadIdx.x == 0) atomicOr(flags, bad);
    return r;
}

// error frame: the prediction differs from the label; with label -1 (a label that is no behaviour) every frame is one
__device__ __forceinline__ bool is_error(int pred, int label) { return label < 0 || pred != label; }

// The walk both passes share.  For tile k the thread looks at frame f = lo + 256 k + threadIdx.x and finds out whether a run
// starts and whether one ends there, and their ranks among the instance's runs.  MARK writes them to out[rank] while rank < room (the count pass sized `room`; predictions that changed since then must not write past it).
// Returns the number of runs.
template <bool MARK>
__device__ __forceinline__ int walk_instance(const RunsParams& p, const InstanceRange& r, unsigned* flags, RunRecord* out,
                                             long long room, int inst) {
    __shared__ int wave_starts[RUNS_WAVES], wave_ends[RUNS_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int done_starts = 0, done_ends = 0;                        // runs begun / ended in the tiles before this one (uniform)
    for (int64_t t0 = r.lo; t0 <= r.hi; t0 += RUNS_BLOCK) {
        const int64_t f = t0 + threadIdx.x;
        bool s = false, e = false;
        if (f <= r.hi) {
            const int* q = p.pred + r.base + f;
            const int here = q[0];
            const int before = f > r.lo ? q[-1] : here, after = f < r.hi ? q[1] : here;
            if (here < -1 || here >= p.n_classes) atomicOr(flags, RUNS_FLAG_PRED);
            const bool err = is_error(here, r.label);
            s = err && !(f > r.lo && is_error(before, r.label));
            e = err && !(f < r.hi && is_error(after, r.label));
        }
        const unsigned long long ms = __ballot(s), me = __ballot(e);
        if (lane == 0) {
            wave_starts[wave] = __popcll(ms);
            wave_ends[wave] = __popcll(me);
        }
        __syncthreads();
        int before_s = done_starts, before_e = done_ends, all_s = 0, all_e = 0;
        for (int w = 0; w < RUNS_WAVES; ++w) {
            if (w < wave) { before_s += wave_starts[w]; before_e += wave_ends[w]; }
            all_s += wave_starts[w];
            all_e += wave_ends[w];
        }
        if (MARK) {
            const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
            const long long ks = before_s + __popcll(ms & below), ke = before_e + __popcll(me & below);
            if (s && ks < room) {
                out[ks].instance = inst;
                out[ks].start_frame = (int)f;
            }
            if (e && ke < room) out[ke].end_frame = (int)f;
        }
        done_starts += all_s;
        done_ends += all_e;
        __syncthreads();                                       // wave_starts / wave_ends are rewritten by the next tile
    }
    return done_starts;
}

__global__ void __launch_bounds__(RUNS_BLOCK) runs_count_kernel(RunsParams p, int* __restrict__ counts, unsigned* flags) {
    const int i = blockIdx.x;
    const InstanceRange r = instance_range(p, i, flags);
    const int n = walk_instance<false>(p, r, flags, nullptr, 0, i);
    if (threadIdx.x == 0) counts[i] = n;
}

// offsets[i] = counts[0] + ... + counts[i - 1]; offsets[n] = the total.  One workgroup, 256 counts per step.
__global__ void __launch_bounds__(RUNS_BLOCK) runs_scan_kernel(const int* __restrict__ counts, int n, long long* __restrict__ offsets) {
    __shared__ long long wave_sum[RUNS_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (int i0 = 0; i0 < n; i0 += RUNS_BLOCK) {
        const int i = i0 + threadIdx.x;
        const long long v = i < n ? counts[i] : 0;
        long long x = v;                                       // inclusive scan inside the wave
        for (int d = 1; d < 64; d <<= 1) {
            const long long y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wave_sum[wave] = x;
        __syncthreads();
        long long before = carry, all = 0;
        for (int w = 0; w < RUNS_WAVES; ++w) {
            if (w < wave) before += wave_sum[w];
            all += wave_sum[w];
        }
        if (i < n) offsets[i] = before + x - v;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[n] = carry;
}

__global__ void __launch_bounds__(RUNS_BLOCK) runs_mark_kernel(RunsParams p, const long long* __restrict__ offsets, RunRecord* records,
                                                               unsigned* flags) {
    const int i = blockIdx.x;
    if (offsets[i + 1] == offsets[i]) return;                  // uniform: no run in this instance
    const InstanceRange r = instance_range(p, i, flags);
    walk_instance<true>(p, r, flags, records + offsets[i], offsets[i + 1] - offsets[i], i);
}

__global__ void __launch_bounds__(RUNS_BLOCK) runs_reduce_kernel(RunsParams p, RunRecord* records, long long n_records) {
    __shared__ int hist[RUNS_WAVES][HEAD_SCORE_MAX_CLASSES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long k = (long long)blockIdx.x * RUNS_WAVES + wave;
    const bool live = k < n_records;
    hist[wave][lane] = 0;
    __syncthreads();
    int first = 0, last = -1;
    int64_t run_base = 0;
    if (live) {
        const RunRecord rec = records[k];
        // the launcher filled the records with -1 before the mark pass: a record that pass did not complete (the predictions
        // changed under the call) keeps a negative field and is left as it is; nothing is indexed with an unchecked value
        if (rec.instance >= 0 && rec.instance < p.n_instances && rec.start_frame >= 0 && rec.end_frame >= rec.start_frame) {
            const int c = p.inst_clip[rec.instance];
            if (c >= 0 && c < p.n_clips) {
                const int64_t base = p.clip_table[2 * (int64_t)c], n = p.clip_table[2 * (int64_t)c + 1];
                if (base >= 0 && n >= 0 && base <= p.n_frames_total && n <= p.n_frames_total - base && rec.end_frame < n) {
                    first = rec.start_frame;
                    last = rec.end_frame;
                    run_base = base;
                    for (int64_t f = (int64_t)first + lane; f <= last; f += 64) {
                        const int cls = p.pred[base + f];
                        if (cls >= 0 && cls < p.n_classes) atomicAdd(&hist[wave][cls], 1);
                    }
                }
            }
        }
    }
    const double sum = run_conf_sum(p.conf + run_base, first, last, lane);      // run_sum.h: shared with cbas_label_runs
    __syncthreads();
    // lane c speaks for class c: the largest count wins, then the smallest name rank; a run without a countable prediction
    // (every frame's row held a NaN) reports -1
    const int count = lane < p.n_classes ? hist[wave][lane] : 0;
    long long key = -1;
    if (count > 0) key = ((long long)count << 16) | (long long)((255 - (p.name_rank[lane] & 255)) << 8) | lane;
    for (int d = 32; d > 0; d >>= 1) {
        const long long other = __shfl_xor(key, d);
        key = other > key ? other : key;
    }
    if (live && last >= first && lane == 0) {
        records[k].model_prediction = key < 0 ? -1 : (int)(key & 255);
        records[k].model_confidence = sum / (double)((int64_t)last - first + 1);
    }
}

}  // namespace

int launch_probs_top1(const float* probs, int64_t n, int C, int* pred, float* conf, unsigned* flags, hipStream_t st) {
    if (!probs || !pred || !conf || !flags || n < 1 || C < 1 || C > HEAD_SCORE_MAX_CLASSES) return -1;
    const int64_t blocks = (n + TOP1_BLOCK - 1) / TOP1_BLOCK;
    if (blocks > 0x7fffffff) return -1;
    hipLaunchKernelGGL(probs_top1_kernel, dim3((unsigned)blocks), dim3(TOP1_BLOCK), 0, st, probs, n, C, pred, conf, flags);
    return CHECK_LAUNCH();
}

static bool runs_params_ok(const RunsParams& p) {
    return p.pred && p.conf && p.clip_table && p.inst_clip && p.inst_start && p.inst_end && p.inst_label && p.name_rank &&
           p.n_frames_total >= 0 && p.n_clips >= 1 && p.n_instances >= 1 && p.n_classes >= 1 && p.n_classes <= HEAD_SCORE_MAX_CLASSES;
}

int launch_runs_scan(const int* counts, int n, long long* offsets, hipStream_t st) {
    if (!counts || !offsets || n < 1) return -1;
    hipLaunchKernelGGL(runs_scan_kernel, dim3(1), dim3(RUNS_BLOCK), 0, st, counts, n, offsets);
    return CHECK_LAUNCH();
}

int launch_runs_count(const RunsParams& p, int* counts, long long* offsets, unsigned* flags, hipStream_t st) {
    if (!runs_params_ok(p) || !counts || !offsets || !flags) return -1;
    hipLaunchKernelGGL(runs_count_kernel, dim3((unsigned)p.n_instances), dim3(RUNS_BLOCK), 0, st, p, counts, flags);
    if (CHECK_LAUNCH()) return -2;
    return launch_runs_scan(counts, p.n_instances, offsets, st);
}

int launch_runs_emit(const RunsParams& p, const long long* offsets, RunRecord* records, long long n_records, unsigned* flags,
                     hipStream_t st) {
    if (!runs_params_ok(p) || !offsets || !records || !flags || n_records < 1) return -1;
    const long long blocks = (n_records + RUNS_WAVES - 1) / RUNS_WAVES;
    if (blocks > 0x7fffffff) return -1;
    if (hipMemsetAsync(records, 0xff, (size_t)n_records * sizeof(RunRecord), st) != hipSuccess) return -2;
    hipLaunchKernelGGL(runs_mark_kernel, dim3((unsigned)p.n_instances), dim3(RUNS_BLOCK), 0, st, p, offsets, records, flags);
    if (CHECK_LAUNCH()) return -2;
    hipLaunchKernelGGL(runs_reduce_kernel, dim3((unsigned)blocks), dim3(RUNS_BLOCK), 0, st, p, records, n_records);
    return CHECK_LAUNCH();
}
