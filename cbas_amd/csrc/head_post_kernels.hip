// The kernels behind what CBAS does with a clip's probabilities after inference (backend/cbas.py:903-1000), on per-frame
// predictions and probabilities that are already on the device.  All clips lie back to back; clip_table (n_clips, 2) holds
// each clip's (first frame, frames).
//
//   labels_median_kernel   scipy.signal.medfilt(predicted_index, kernel_size) per clip (:939): every clip is padded with
//                          kernel_size // 2 zeros at both ends, windows never cross clips.  The values are the at most 65
//                          integers -1 .. C - 1, so the median is a counting problem: the smallest value whose cumulative
//                          count in the window, the padding zeros added to value 0, reaches (kernel_size + 1) / 2.  A thread
//                          owns MED_SEG consecutive frames and one column of a histogram in LDS (hist[value][thread]: the
//                          threads of a wave hit 64 different banks): it counts the window of its first frame once, then
//                          slides - one value leaves, one enters - and reads the median off the cumulative counts.  Exact for
//                          any odd kernel size, also one larger than the clip; no thread reads another's column, so the
//                          kernel has no barrier and no atomic but the error flag.
//   the label run scan     one record per maximal run of consecutive frames of a clip with the same key != -1 (:910-925 with
//                          the threshold, :944-955 without).  The count -> exclusive scan -> emit scheme of
//                          head_report_kernels.hip with one workgroup per clip: label_runs_count_kernel, launch_runs_scan,
//                          label_runs_mark_kernel, label_runs_reduce_kernel (one wave per record; the mean confidence through
//                          run_conf_sum of run_sum.h, the summation cbas_disagreement_runs uses).  Nothing is appended with
//                          an atomic: the records are ordered by (clip, start) whatever the order of execution.
//   activity_bins_kernel   the actogram's per-frame activity (p_b * [max of the others < p_b]) >= threshold (:977-979), summed
//                          in bins of bin_frames frames (:999) with 64-bit integer atomics: one per wave where the wave lies
//                          in one bin, else one per active frame.
// Every table entry and label is validated before anything is indexed with it; a refusal sets a POST_FLAG_* bit.
#include "kernels.h"
#include "run_sum.h"

namespace {

#define CHECK_LAUNCH() (hipGetLastError() == hipSuccess ? 0 : -2)

constexpr int MED_BLOCK = 128;                         // threads = histogram columns
constexpr int MED_SEG = 8;                             // consecutive frames per thread
constexpr int64_t MED_TILE = (int64_t)MED_BLOCK * MED_SEG;
constexpr int MED_SLOTS = HEAD_SCORE_MAX_CLASSES + 1;  // values -1 .. 63
constexpr int MED_MAX_TILE_BLOCKS = 64;                // workgroups that share the tiles of one clip
constexpr int RUNS_BLOCK = 256;
constexpr int RUNS_WAVES = RUNS_BLOCK / 64;
constexpr int REDUCE_MAX_BLOCKS = 4096;
constexpr int BINS_BLOCK = 256;

// frames of clip c, or -1 for an entry that reaches outside [0, n_frames_total) (flagged); *base = its first frame
__device__ __forceinline__ int64_t clip_frames(const int64_t* __restrict__ table, int c, int64_t n_frames_total, unsigned* flags,
                                               int64_t* base) {
    const int64_t b = table[2 * (int64_t)c], n = table[2 * (int64_t)c + 1];
    if (b < 0 || n < 0 || n > 0x7fffffff || b > n_frames_total || n > n_frames_total - b) {
        if (threadIdx.x == 0) atomicOr(flags, POST_FLAG_TABLE);
        return -1;
    }
    *base = b;
    return n;
}

__global__ void __launch_bounds__(MED_BLOCK)
labels_median_kernel(const int* __restrict__ pred, int64_t n_frames_total, const int64_t* __restrict__ table, int C, int ksize,
                     int* __restrict__ out, unsigned* flags) {
    __shared__ int hist[MED_SLOTS][MED_BLOCK];
    const int tid = threadIdx.x;
    int64_t base = 0;
    const int64_t n = clip_frames(table, blockIdx.x, n_frames_total, flags, &base);
    const int64_t half = ksize / 2, rank = half + 1;
    const int* x = pred + base;
    for (int64_t tile = blockIdx.y; tile * MED_TILE < n; tile += gridDim.y) {
        const int64_t f0 = tile * MED_TILE + (int64_t)tid * MED_SEG;
        if (f0 >= n) continue;
        const int64_t f1 = f0 + MED_SEG < n ? f0 + MED_SEG : n;
        for (int s = 0; s <= C; ++s) hist[s][tid] = 0;
        int64_t lo = f0 - half > 0 ? f0 - half : 0, hi = f0 + half < n - 1 ? f0 + half : n - 1;
        for (int64_t j = lo; j <= hi; ++j) {
            const int v = x[j];
            if (v < -1 || v >= C) atomicOr(flags, POST_FLAG_VALUE);
            else hist[v + 1][tid] += 1;
        }
        for (int64_t f = f0; f < f1; ++f) {
            const int64_t pad = (int64_t)ksize - (hi - lo + 1);        // zeros of the padding inside this window
            int64_t cum = 0;
            int med = C - 1;
            for (int s = 0; s <= C; ++s) {
                cum += hist[s][tid] + (s == 1 ? pad : 0);
                if (cum >= rank) { med = s - 1; break; }
            }
            out[base + f] = med;
            if (f + 1 < f1) {                                          // the window of frame f + 1
                const int64_t nlo = f + 1 - half > 0 ? f + 1 - half : 0, nhi = f + 1 + half < n - 1 ? f + 1 + half : n - 1;
                if (nlo > lo) {
                    const int v = x[lo];
                    if (v >= -1 && v < C) hist[v + 1][tid] -= 1;
                }
                if (nhi > hi) {
                    const int v = x[nhi];
                    if (v < -1 || v >= C) atomicOr(flags, POST_FLAG_VALUE);
                    else hist[v + 1][tid] += 1;
                }
                lo = nlo;
                hi = nhi;
            }
        }
    }
}

// the key a frame counts with: -1 for no label, for a label outside [0, C) (one below -1 or above C - 1 is flagged) and, with
// the threshold, for a probability that is not >= threshold in float64 (`row['max_prob'] >= threshold`, :912; a NaN is not)
__device__ __forceinline__ int run_key(const LabelRunsParams& p, int64_t idx, unsigned* flags) {
    const int k = p.key[idx];
    if (k < -1 || k >= p.n_classes) {
        atomicOr(flags, POST_FLAG_VALUE);
        return -1;
    }
    if (k < 0) return -1;
    if (p.use_threshold && !((double)p.conf[idx] >= p.threshold)) return -1;
    return k;
}

// The walk the count and the mark pass share, as walk_instance of head_report_kernels.hip: for tile t the thread looks at
// frame f = 256 t + threadIdx.x of the clip and finds out whether a run starts and whether one ends there, and their ranks
// among the clip's runs.  MARK writes them to out[rank] while rank < room.  Returns the number of runs.
template <bool MARK>
__device__ __forceinline__ int walk_clip(const LabelRunsParams& p, int64_t base, int64_t n, unsigned* flags, LabelRunRecord* out,
                                         long long room, int clip) {
    __shared__ int wave_starts[RUNS_WAVES], wave_ends[RUNS_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int done_starts = 0, done_ends = 0;                        // runs begun / ended in the tiles before this one (uniform)
    for (int64_t t0 = 0; t0 < n; t0 += RUNS_BLOCK) {
        const int64_t f = t0 + threadIdx.x;
        bool s = false, e = false;
        int here = -1;
        if (f < n) {
            here = run_key(p, base + f, flags);
            if (here >= 0) {
                s = f == 0 || run_key(p, base + f - 1, flags) != here;
                e = f == n - 1 || run_key(p, base + f + 1, flags) != here;
            }
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
                out[ks].clip = clip;
                out[ks].start_frame = (int)f;
                out[ks].label = here;
            }
            if (e && ke < room) out[ke].end_frame = (int)f;
        }
        done_starts += all_s;
        done_ends += all_e;
        __syncthreads();                                       // wave_starts / wave_ends are rewritten by the next tile
    }
    return done_starts;
}

__global__ void __launch_bounds__(RUNS_BLOCK) label_runs_count_kernel(LabelRunsParams p, int* __restrict__ counts, unsigned* flags) {
    const int c = blockIdx.x;
    int64_t base = 0;
    const int64_t n = clip_frames(p.clip_table, c, p.n_frames_total, flags, &base);       // -1: refused, no frame is walked
    const int runs = walk_clip<false>(p, base, n, flags, nullptr, 0, c);
    if (threadIdx.x == 0) counts[c] = runs;
}

__global__ void __launch_bounds__(RUNS_BLOCK) label_runs_mark_kernel(LabelRunsParams p, const long long* __restrict__ offsets,
                                                                     LabelRunRecord* records, long long capacity, unsigned* flags) {
    const int c = blockIdx.x;
    const long long first = offsets[c], end = offsets[c + 1] < capacity ? offsets[c + 1] : capacity;
    if (end <= first) return;                                  // uniform: no run of this clip has room
    int64_t base = 0;
    const int64_t n = clip_frames(p.clip_table, c, p.n_frames_total, flags, &base);
    walk_clip<true>(p, base, n, flags, records + first, end - first, c);
}

__global__ void __launch_bounds__(RUNS_BLOCK) label_runs_reduce_kernel(LabelRunsParams p, const long long* __restrict__ offsets,
                                                                       LabelRunRecord* records, long long capacity) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long total = offsets[p.n_clips], n_records = total < capacity ? total : capacity;
    for (long long k = (long long)blockIdx.x * RUNS_WAVES + wave; k < n_records; k += (long long)gridDim.x * RUNS_WAVES) {
        const LabelRunRecord rec = records[k];
        // the launcher filled the records with -1 before the mark pass: a record that pass did not complete (the keys changed
        // under the call) keeps a negative field and is left as it is; nothing is indexed with an unchecked value
        if (rec.clip < 0 || rec.clip >= p.n_clips || rec.start_frame < 0 || rec.end_frame < rec.start_frame) continue;
        const int64_t base = p.clip_table[2 * (int64_t)rec.clip], n = p.clip_table[2 * (int64_t)rec.clip + 1];
        if (base < 0 || n < 0 || base > p.n_frames_total || n > p.n_frames_total - base || rec.end_frame >= n) continue;
        const double sum = run_conf_sum(p.conf + base, rec.start_frame, rec.end_frame, lane);
        if (lane == 0) records[k].confidence = sum / (double)((int64_t)rec.end_frame - rec.start_frame + 1);
    }
}

__global__ void __launch_bounds__(BINS_BLOCK)
activity_bins_kernel(const float* __restrict__ probs, int64_t n, int C, int b, double threshold, int64_t bin_frames,
                     unsigned long long* __restrict__ bins) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * BINS_BLOCK + threadIdx.x;
    bool active = false;
    if (r < n) {
        const float* row = probs + r * C;
        const float pb = row[b];
        float m = 0.f;
        bool any = false;                                      // pandas' max(axis=1) skips NaN; over no value it is NaN: not < p_b
        for (int c = 0; c < C; ++c) {
            const float v = row[c];
            if (c != b && v == v) {
                m = any && m > v ? m : v;
                any = true;
            }
        }
        const bool is_max = any && m < pb;                     // strict: a tie is no maximum (:978)
        active = (double)pb * (is_max ? 1.0 : 0.0) >= threshold;      // `probs * is_max >= threshold` (:979); a NaN p_b counts nothing
    }
    const unsigned long long mask = __ballot(active);
    if (!mask) return;
    const int64_t r0 = r - lane, r1 = r0 + 63 < n - 1 ? r0 + 63 : n - 1;
    if (r0 / bin_frames == r1 / bin_frames) {
        if (lane == 0) atomicAdd(&bins[r0 / bin_frames], (unsigned long long)__popcll(mask));
    } else if (active) {
        atomicAdd(&bins[r / bin_frames], 1ull);
    }
}

}  // namespace

int launch_labels_median(const int* pred, int64_t n_frames_total, const int64_t* clip_table, int n_clips, int C, int kernel_size,
                         int* out, unsigned* flags, hipStream_t st) {
    if (!pred || !clip_table || !out || !flags || n_frames_total < 0 || n_clips < 1 || C < 1 || C > HEAD_SCORE_MAX_CLASSES ||
        kernel_size < 1 || !(kernel_size & 1))
        return -1;
    int64_t tiles = (n_frames_total + MED_TILE - 1) / MED_TILE;
    tiles = tiles < 1 ? 1 : tiles > MED_MAX_TILE_BLOCKS ? MED_MAX_TILE_BLOCKS : tiles;
    hipLaunchKernelGGL(labels_median_kernel, dim3((unsigned)n_clips, (unsigned)tiles), dim3(MED_BLOCK), 0, st, pred, n_frames_total,
                       clip_table, C, kernel_size, out, flags);
    return CHECK_LAUNCH();
}

static bool label_runs_params_ok(const LabelRunsParams& p) {
    return p.key && p.conf && p.clip_table && p.n_frames_total >= 0 && p.n_clips >= 1 && p.n_classes >= 1 &&
           p.n_classes <= HEAD_SCORE_MAX_CLASSES && !(p.use_threshold && p.threshold != p.threshold);
}

int launch_label_runs_count(const LabelRunsParams& p, int* counts, long long* offsets, unsigned* flags, hipStream_t st) {
    if (!label_runs_params_ok(p) || !counts || !offsets || !flags) return -1;
    hipLaunchKernelGGL(label_runs_count_kernel, dim3((unsigned)p.n_clips), dim3(RUNS_BLOCK), 0, st, p, counts, flags);
    if (CHECK_LAUNCH()) return -2;
    return launch_runs_scan(counts, p.n_clips, offsets, st);
}

int launch_label_runs_emit(const LabelRunsParams& p, const long long* offsets, LabelRunRecord* records, long long capacity,
                           unsigned* flags, hipStream_t st) {
    if (!label_runs_params_ok(p) || !offsets || !records || !flags || capacity < 1) return -1;
    long long blocks = (capacity + RUNS_WAVES - 1) / RUNS_WAVES;
    blocks = blocks > REDUCE_MAX_BLOCKS ? REDUCE_MAX_BLOCKS : blocks;
    if (hipMemsetAsync(records, 0xff, (size_t)capacity * sizeof(LabelRunRecord), st) != hipSuccess) return -2;
    hipLaunchKernelGGL(label_runs_mark_kernel, dim3((unsigned)p.n_clips), dim3(RUNS_BLOCK), 0, st, p, offsets, records, capacity, flags);
    if (CHECK_LAUNCH()) return -2;
    hipLaunchKernelGGL(label_runs_reduce_kernel, dim3((unsigned)blocks), dim3(RUNS_BLOCK), 0, st, p, offsets, records, capacity);
    return CHECK_LAUNCH();
}

int launch_activity_bins(const float* probs, int64_t n, int C, int behavior, double threshold, int64_t bin_frames,
                         unsigned long long* bins, int64_t n_bins, hipStream_t st) {
    if (!probs || !bins || n < 1 || C < 1 || C > HEAD_SCORE_MAX_CLASSES || behavior < 0 || behavior >= C || bin_frames < 1 ||
        n_bins != (n - 1) / bin_frames + 1)
        return -1;
    const int64_t blocks = (n + BINS_BLOCK - 1) / BINS_BLOCK;
    if (blocks > 0x7fffffff) return -1;
    hipLaunchKernelGGL(activity_bins_kernel, dim3((unsigned)blocks), dim3(BINS_BLOCK), 0, st, probs, n, C, behavior, threshold,
                       bin_frames, bins);
    return CHECK_LAUNCH();
}
