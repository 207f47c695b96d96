"""Deterministic inputs for the run-scan, median, winner, bin and top-1 kernels (csrc/head_post_kernels.hip,
csrc/head_report_kernels.hip) that sit on their wave (64), tile (256 / 1024) and grid seams, each with the result it must give.

The expectations are written from the construction - a run is where the builder put it, a record's offset is the prefix sum of
the counts the builder chose - and never computed by ``cbas_amd.postprocess`` or ``cbas_amd.train``;
tests/test_scan_seams_host.py pins them to the package's numpy routines (and scipy) without a GPU, tests/test_gpu_scan_seams.py
holds the kernels to them.  No GPU, no torch: numpy only.

Confidences are float32 values in [1/64, 1] (what a top-1 probability of at most 64 classes can be): every partial sum of up to
2^22 of them is exact in float64, so a run's mean is the plain ascending float64 sum divided by its length, in any order of
summation, bit for bit.
"""
from collections import namedtuple

import numpy as np

LABEL_RUN_DTYPE = np.dtype([("clip", "<i4"), ("start_frame", "<i4"), ("end_frame", "<i4"), ("label", "<i4"), ("confidence", "<f8")])
RUN_DTYPE = np.dtype([("instance", "<i4"), ("start_frame", "<i4"), ("end_frame", "<i4"), ("model_prediction", "<i4"),
                      ("model_confidence", "<f8")])

# key / conf: all clips back to back; table (n_clips, 2) = (first frame, frames); records: LABEL_RUN_DTYPE, ordered by (clip, start);
# counts[c] = records of clip c (their offsets are its prefix sums)
LabelCase = namedtuple("LabelCase", "name key conf table n_classes threshold records counts")
# inst: (n, 4) = (clip, start, end, label); rank: the name ranks; records: RUN_DTYPE, ordered by (instance, start)
RunsCase = namedtuple("RunsCase", "name pred conf table inst rank n_classes records counts")


def confidences(n, seed=0, lo=1.0 / 64, hi=1.0):
    """n float32 values in [lo, hi], a fixed scramble of the frame number."""
    f = np.arange(n, dtype=np.uint64) + np.uint64(seed)
    h = (f * np.uint64(2654435761)) % np.uint64(1 << 20)
    c = (lo + h.astype(np.float64) / float(1 << 20) * (hi - lo)).astype(np.float32)
    return np.clip(c, np.float32(lo), np.float32(hi))


def mean64(conf, a, b):
    """The float64 mean of conf[a .. b], added one after the other in ascending order."""
    return float(np.cumsum(conf[a:b + 1].astype(np.float64))[-1] / (b - a + 1))


def winner_of(counts, rank):
    """The smallest name rank among the largest counts; -1 when nothing was counted.  counts: {class: frames}."""
    counts = {c: k for c, k in counts.items() if c >= 0 and k > 0}
    if not counts:
        return -1
    top = max(counts.values())
    return min((c for c, k in counts.items() if k == top), key=lambda c: rank[c])


# ---------------------------------------------------------------------------------------------------------------
# segments: a clip as [(frames, label)], label -1 for frames without a key; neighbours differ, so every segment with a label
# is one run of cbas_label_runs
# ---------------------------------------------------------------------------------------------------------------
def segment_keys(segments):
    assert all(n >= 1 and k >= -1 for n, k in segments)
    assert all(a[1] != b[1] for a, b in zip(segments, segments[1:])), "neighbouring segments must differ"
    return np.concatenate([np.full(n, k, np.int32) for n, k in segments])


def segment_runs(segments):
    """[(start, end, label)] of the segments that carry a label."""
    runs, f = [], 0
    for n, k in segments:
        if k >= 0:
            runs.append((f, f + n - 1, k))
        f += n
    return runs


COMB_FRAMES = 4 * 67 * 68 // 2 + 300
COMB_SHIFTS = (1, 2, 3, 4)


def comb_segments(n_frames=COMB_FRAMES, n_classes=9):
    """Runs of lengths 1 .. 67, 1 .. 67, ..., separated alternately by nothing (the label changes) and by one frame without a
    key, cut at n_frames: the starts and the ends walk through the lanes of a wave and the waves of a tile (COMB_SHIFTS fills
    the phases the comb alone leaves out)."""
    segs, total, j = [], 0, 0
    while total < n_frames:
        length = min(j % 67 + 1, n_frames - total)
        segs.append((length, j % n_classes))
        total += length
        if j % 2 == 1 and total < n_frames:
            segs.append((1, -1))
            total += 1
        j += 1
    return segs


# every variant is one clip
SEAM_SEGMENTS = {
    # the label changes on 63|64 and on 255|256; a run starts on frame 0 and one ends on the last frame
    "change_on_seams": [(64, 1), (192, 2), (300, 3)],
    # a run ends on 62 / 254 and the next starts on 64 / 256 behind one frame without a key; the first and the last frame have none
    "gap_on_63_and_255": [(1, -1), (62, 1), (1, -1), (191, 2), (1, -1), (100, 3), (1, -1)],
    # a run ends on 63 / 255, the frame without a key is 64 / 256
    "gap_on_64_and_256": [(64, 1), (1, -1), (191, 2), (1, -1), (50, 3)],
    # runs of one frame on 63, 64, 255 and 256, nothing else in the clip; and on frame 0 and the last frame
    "single_frames_on_seams": [(1, 4), (62, -1), (1, 1), (1, 2), (190, -1), (1, 1), (1, 2), (9, -1), (1, 5)],
    # wave 1 (frames 64 .. 127) lies inside the run 60 .. 139, between waves that have boundaries; the run 151 .. 850 holds the
    # whole tile 256 .. 511 and all of waves 3 and 8 .. 12: zero boundaries there
    "no_boundary_in_a_wave_or_tile": [(40, 1), (20, 2), (80, 3), (10, 1), (1, -1), (700, 2), (1, -1), (30, 3)],
    # one run is the whole clip of three tiles and a bit
    "one_run": [(777, 6)],
    # exactly one tile, exactly one wave, one frame
    "one_tile": [(256, 7)],
    "one_wave": [(64, 8)],
    "one_frame": [(1, 0)],
}


def label_case(name, clips, n_classes, threshold=None, runs=None, conf=None, seed=0):
    """clips: one segment list per clip (an empty list: a clip without frames).  runs: per clip [(start, end, label)] when they
    are not the segments'."""
    keys = [segment_keys(s) if s else np.empty(0, np.int32) for s in clips]
    sizes = [k.size for k in keys]
    table = np.array([[sum(sizes[:i]), n] for i, n in enumerate(sizes)], np.int64).reshape(-1, 2)
    key = np.concatenate(keys) if keys else np.empty(0, np.int32)
    conf = confidences(key.size, seed) if conf is None else conf
    runs = [segment_runs(s) for s in clips] if runs is None else runs
    rows = [(c, a, b, k, mean64(conf, int(table[c, 0]) + a, int(table[c, 0]) + b)) for c, rr in enumerate(runs) for a, b, k in rr]
    return LabelCase(name, key, conf, table, n_classes, threshold, np.array(rows, LABEL_RUN_DTYPE).reshape(-1),
                     np.array([len(rr) for rr in runs], np.int64))


def comb_cases():
    """The comb alone (with no threshold, with one every confidence passes and with one none does), the comb behind 1 .. 4 frames
    without a key as four clips of one table - the comb alone leaves 5 of the 64 lanes without a start; with the shifted ones
    a start and an end fall on each of the 256 frames of a tile - and every seam variant as the clips of one table."""
    segs = comb_segments()
    out = [label_case("comb", [segs], 9), label_case("comb_threshold_all_pass", [segs], 9, threshold=1.0 / 64),
           label_case("comb_threshold_none_pass", [segs], 9, threshold=2.0, runs=[[]]),
           label_case("comb_shifted", [[(p, -1)] + segs for p in COMB_SHIFTS], 9, seed=2)]
    names = list(SEAM_SEGMENTS)
    out.append(label_case("seams[" + ",".join(names) + "]", [SEAM_SEGMENTS[n] for n in names], 9, seed=5))
    out.append(label_case("seams_threshold_all_pass", [SEAM_SEGMENTS[n] for n in names], 9, threshold=0.0, seed=5))
    return out


DIP_FRAMES = {"dips_63_64_255_256": (63, 64, 255, 256), "dips_63_256": (63, 256), "dips_64_255": (64, 255),
              "dips_0_and_last": (0, 699), "dips_127_128_511_512": (127, 128, 511, 512)}


def dip_cases():
    """One run of 700 frames - whole waves and the tile 256 .. 511 lie inside it - whose confidence dips under the threshold on
    the named frames: with the threshold the dips split it, without it is one run."""
    n, label, clips, runs, conf = 700, 3, [], [], []
    for name, dips in DIP_FRAMES.items():
        c = confidences(n, seed=len(clips), lo=0.625, hi=1.0)
        c[list(dips)] = np.float32(0.25)
        conf.append(c)
        clips.append([(n, label)])
        edges = [-1] + sorted(dips) + [n]
        runs.append([(a + 1, b - 1, label) for a, b in zip(edges, edges[1:]) if b - 1 >= a + 1])
    conf = np.concatenate(conf)
    return [label_case("dips_threshold", clips, 9, threshold=0.5, runs=runs, conf=conf),
            label_case("dips_no_threshold", clips, 9, conf=conf)]


# ---------------------------------------------------------------------------------------------------------------
# many clips / many instances: entry i has (i * 7) % 5 records, so the offsets are a known prefix sum with zeros everywhere
# ---------------------------------------------------------------------------------------------------------------
MANY_N = (63, 64, 65, 128, 255, 256, 257, 511, 513, 1000)


def many_clips_case(n, n_classes=9):
    clips = []
    for i in range(n):
        r = (i * 7) % 5
        segs = []
        if r == 0:
            length = 0 if i % 10 == 0 else i % 7                 # a clip without frames, or one without a key
            if length:
                segs.append((length, -1))
        else:
            if i % 3:
                segs.append((i % 3, -1))
            for j in range(r):
                segs.append((1 + (i + j) % 4, (i + j) % n_classes))
                if j % 2 == 1 and j < r - 1:
                    segs.append((1, -1))
            if i % 11 == 3:                                       # the last run reaches the last of 40 frames
                segs[-1] = (segs[-1][0] + 40 - sum(s[0] for s in segs), segs[-1][1])
            elif i % 4 == 1:
                segs.append((2, -1))
        assert sum(s[0] for s in segs) <= 40
        clips.append(segs)
    case = label_case(f"many_clips_{n}", clips, n_classes, seed=n)
    assert np.array_equal(case.counts, (np.arange(n) * 7) % 5)
    return case


INSTANCE_CLIPS = (300, 41, 1000, 520)
INSTANCE_LABEL = 1


def many_instances_case(n, n_classes=9):
    """Four clips shared by all instances.  In every clip the frames f with f % 8 in {0, 1, 2} are predicted as class
    2 + (f // 8 + clip) % 7, all others as class 1, the label of the instances: an error run every 8 frames.  Instance i looks at
    (i * 7) % 5 of them - whole, or cut at its first or its last frame; with none it lies between two runs, on one right frame
    or past its clip."""
    label = INSTANCE_LABEL
    preds, table, base = [], [], 0
    for c, ln in enumerate(INSTANCE_CLIPS):
        f = np.arange(ln)
        preds.append(np.where(f % 8 < 3, 2 + (f // 8 + c) % 7, label).astype(np.int32))
        table.append((base, ln))
        base += ln
    pred = np.concatenate(preds)
    conf = confidences(pred.size, seed=n)
    rank = np.arange(n_classes - 1, -1, -1).astype(np.int32)
    inst, rows, counts = [], [], []
    for i in range(n):
        r, c = (i * 7) % 5, i % 4
        ln, b0 = INSTANCE_CLIPS[c], table[c][0]
        a = (i * 13) % ((ln - 33) // 8 + 1)
        lab, runs = label, []
        if r == 0:
            m = (i // 5) % 3
            s, e = ((ln + 3, ln + 10), (8 * a + 3, 8 * a + 7), (8 * a + 5, 8 * a + 5))[m]
        elif r == 1 and c == 1 and i % 3 == 0:                   # the end lies past the clip: its last frame, 40, is the run
            s, e = 35, 60
            runs = [(40, 40, 2 + (5 + c) % 7)]
        elif r == 1 and c == 2 and i % 3 == 1:                   # a label that is no behaviour: five right frames are one run
            s, e, lab = 8 * a + 3, 8 * a + 7, -1
            runs = [(s, e, label)]
        else:
            phase = i % 3
            s = 8 * a + (1 if phase == 1 else 0)
            e = 8 * (a + r - 1) + (1 if phase == 2 else 2 + (i // 3) % 5)
            runs = [(max(s, 8 * (a + j)), min(e, 8 * (a + j) + 2), 2 + (a + j + c) % 7) for j in range(r)]
        inst.append((c, s, e, lab))
        counts.append(len(runs))
        rows += [(i, rs, re, w, mean64(conf, b0 + rs, b0 + re)) for rs, re, w in runs]
    assert counts == [(i * 7) % 5 for i in range(n)]
    return RunsCase(f"many_instances_{n}", pred, conf, np.array(table, np.int64), np.array(inst, np.int64), rank, n_classes,
                    np.array(rows, RUN_DTYPE).reshape(-1), np.array(counts, np.int64))


# ---------------------------------------------------------------------------------------------------------------
# many records: more than 2 * 4096 * 4 = 32 768, what one sweep of label_runs_reduce_kernel's grid covers twice
# ---------------------------------------------------------------------------------------------------------------
MANY_RECORD_FRAMES = 40000


def _single_frame_case(name, key, conf, table, threshold, keep):
    rows = [(c, f, f, int(key[b + f]), float(np.float64(conf[b + f]))) for c, (b, n) in enumerate(table.tolist())
            for f in range(n) if keep[b + f]]
    counts = [int(keep[b:b + n].sum()) for b, n in table.tolist()]
    return LabelCase(name, key, conf, table, 2, threshold, np.array(rows, LABEL_RUN_DTYPE).reshape(-1), np.array(counts, np.int64))


def many_records_cases():
    n = MANY_RECORD_FRAMES
    f = np.arange(n)
    key = (f % 2).astype(np.int32)
    conf = confidences(n, seed=3)
    out = [_single_frame_case("many_records", key, conf, np.array([[0, n]], np.int64), None, np.ones(n, bool))]
    # every third frame dips under the threshold; the two frames between two dips differ in their key: still one frame per record
    dipped = confidences(n, seed=4, lo=0.625, hi=1.0)
    dipped[f % 3 == 0] = np.float32(0.25)
    out.append(_single_frame_case("many_records_threshold", key, dipped, np.array([[0, n]], np.int64), 0.5, f % 3 != 0))
    # the same frames as three clips of uneven length between two clips of 10 frames
    m = n + 20
    g = np.arange(m)
    key5 = (g % 2).astype(np.int32)
    table = np.array([[0, 10], [10, 7001], [7011, 20000], [27011, 12999], [40010, 10]], np.int64)
    assert table[-1].sum() == m
    out.append(_single_frame_case("many_records_five_clips", key5, confidences(m, seed=6), table, None, np.ones(m, bool)))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the walks of cbas_disagreement_runs on the same segments: neighbouring segments with a label merge into one error run
# ---------------------------------------------------------------------------------------------------------------
def error_runs(segments, lo, hi, rank):
    """[(start, end, winner)] of the error runs inside frames [lo, hi] when a frame without a key is predicted right and every
    other frame is predicted as its key: the counts of a run are the lengths of its segments inside the window."""
    out, cur, f = [], None, 0
    for n, k in list(segments) + [(1, -1)]:
        a, b = max(f, lo), min(f + n - 1, hi)
        if k < 0:
            if cur is not None:
                out.append((cur[0], cur[1], winner_of(cur[2], rank)))
            cur = None
        elif a <= b:
            if cur is None:
                cur = [a, b, {}]
            cur[1] = b
            cur[2][k] = cur[2].get(k, 0) + b - a + 1
        f += n
    return out


def walk_instances_case():
    """The comb and the seam variants as clips; the label of every instance is class 9, which no key is, and a frame without a
    key is predicted as 9.  Windows: the whole clip, one that starts and ends inside runs, and one shifted so that the tiles of
    the walk (256 frames from the instance's start) begin on another phase."""
    n_classes, label = 10, 9
    rank = np.array([3, 9, 0, 7, 5, 1, 8, 2, 6, 4], np.int32)
    clips = [comb_segments()] + [SEAM_SEGMENTS[k] for k in SEAM_SEGMENTS]
    keys = [segment_keys(s) for s in clips]
    sizes = [k.size for k in keys]
    table = np.array([[sum(sizes[:i]), n] for i, n in enumerate(sizes)], np.int64)
    pred = np.concatenate(keys)
    pred = np.where(pred < 0, label, pred).astype(np.int32)
    conf = confidences(pred.size, seed=8)
    inst, rows, counts = [], [], []
    for c, (segs, n) in enumerate(zip(clips, sizes)):
        windows = [(0, n - 1)]
        if n > 300:
            windows += [(37, n - 6), (64, n - 1), (1, 256), (63, 63 + 255), (200, n + 50)]
        for lo, hi in windows:
            runs = error_runs(segs, lo, min(hi, n - 1), rank)
            i = len(inst)
            inst.append((c, lo, hi, label))
            counts.append(len(runs))
            rows += [(i, a, b, w, mean64(conf, int(table[c, 0]) + a, int(table[c, 0]) + b)) for a, b, w in runs]
    return RunsCase("walk_instances", pred, conf, table, np.array(inst, np.int64), rank, n_classes,
                    np.array(rows, RUN_DTYPE).reshape(-1), np.array(counts, np.int64))


# ---------------------------------------------------------------------------------------------------------------
# the winner of a run over 64 classes
# ---------------------------------------------------------------------------------------------------------------
def winner_ranks():
    """A permutation of 0 .. 63 that reverses and interleaves: the even classes get ranks 31 .. 0, the odd ones 63 .. 32."""
    c = np.arange(64)
    return np.where(c % 2 == 0, 31 - c // 2, 63 - (c - 1) // 2).astype(np.int32)


def _scrambled(values):
    v = np.array(values, np.int32)
    step = next(s for s in (7, 11, 13, 3, 5, 1) if np.gcd(s, v.size) == 1)
    return v[(np.arange(v.size) * step) % v.size]


# (name, {class: frames}, frames without a prediction, winner): the winner is stated here, by hand, from the ranks above
WINNER_RUNS = [
    ("tie_5_40_63", {5: 4, 40: 4, 63: 4, 7: 2, 8: 1, 62: 3}, 0, 40),        # ranks 61, 11, 32; class 62 (rank 0) has fewer frames
    ("tie_62_63", {62: 3, 63: 3, 0: 1}, 1, 62),                              # ranks 0, 32
    ("tie_of_all_64", {c: 1 for c in range(64)}, 0, 62),                     # rank 0
    ("worst_rank_wins_by_count", {1: 5, 62: 4, 40: 4}, 0, 1),                # class 1 has rank 63
    ("no_prediction", {}, 9, -1),
    ("one_frame", {33: 1}, 0, 33),
    ("long_tie_17_18", {17: 70, 18: 70, 19: 69, 62: 30}, 5, 18),             # ranks 55, 22: more than 64 frames, the lanes stride
    ("tie_high_lanes", {9: 2, 10: 2, 11: 2, 63: 2, 61: 2}, 0, 10),           # ranks 59, 26, 58, 32, 33
]


def winner_case():
    rank = winner_ranks()
    assert sorted(rank.tolist()) == list(range(64))
    preds, inst, rows = [], [], []
    f = 0
    for i, (name, counts, none, winner) in enumerate(WINNER_RUNS):
        assert winner == winner_of(counts, rank), name
        p = _scrambled([c for c, k in counts.items() for _ in range(k)] + [-1] * none)
        preds.append(p)
        # a label that is no behaviour makes every frame an error frame; so does a class the run does not hold
        inst.append((0, f, f + p.size - 1, -1 if i % 2 == 0 or 0 in counts else 0))
        rows.append((i, f, f + p.size - 1, winner))
        f += p.size
    pred = np.concatenate(preds)
    conf = confidences(pred.size, seed=11)
    records = np.array([(i, a, b, w, mean64(conf, a, b)) for i, a, b, w in rows], RUN_DTYPE)
    return RunsCase("winner", pred, conf, np.array([[0, pred.size]], np.int64), np.array(inst, np.int64), rank, 64, records,
                    np.ones(len(rows), np.int64))


# ---------------------------------------------------------------------------------------------------------------
# the median
# ---------------------------------------------------------------------------------------------------------------
MEDIAN_BLOCK = 512                     # >= every kernel size but 2001; 65 536 and 66 560 are multiples
MEDIAN_LONG = 65536 + 1024 + 5
MEDIAN_CLIPS = (7, 8, 9, 1023, 1024, 1025, 2 * 1024 + 8, 3, MEDIAN_LONG)
MEDIAN_GAP_AFTER = 5                   # 10 frames that belong to no clip lie behind the clip of 1025 frames
MEDIAN_GAP = 10
MEDIAN_KSIZES = (1, 3, 31, 301)
MEDIAN_WIDE = (1025, 2001)             # the kernel size wider than a tile runs on this clip alone
OUTLIER_EVERY, OUTLIER_PHASE = 37, 11


def median_clip(n, n_classes, clip=0):
    """(x, block): the step pattern of one clip.  Block j (frames 512 j .. 512 j + 511) has the value
    ((j + clip) * 5 + 3) % (C + 1) - 1, so neighbours differ and -1 occurs; every frame f with f % 37 == 11 is an outlier with
    another value.  The block edges of the long clip lie on 65 535|65 536 and 66 559|66 560, where the workgroups that stride
    begin their second tile."""
    f = np.arange(n)
    block = ((f // MEDIAN_BLOCK + clip) * 5 + 3) % (n_classes + 1)
    x = np.where(f % OUTLIER_EVERY == OUTLIER_PHASE, (block + 1 + (f // OUTLIER_EVERY) % n_classes) % (n_classes + 1), block)
    return (x - 1).astype(np.int32), (block - 1).astype(np.int32)


def median_expected(x, ksize, n_classes):
    """medfilt of one clip by counting: the window of frame f is the frames [f - k // 2, f + k // 2] inside the clip and one zero
    for every frame outside; its median is the smallest value v whose count of values <= v reaches k // 2 + 1.  The counts come
    from prefix sums over the frames, value by value: no sort and no window is materialised."""
    n, half = x.size, ksize // 2
    f = np.arange(n)
    lo, hi = np.maximum(f - half, 0), np.minimum(f + half, n - 1)
    pad = ksize - (hi - lo + 1)
    out = np.full(n, n_classes - 1, np.int32)
    found = np.zeros(n, bool)
    cum = np.zeros(n, np.int64)
    for v in range(-1, n_classes):
        prefix = np.concatenate([[0], np.cumsum(x == v)])
        cum += prefix[hi + 1] - prefix[lo] + (pad if v == 0 else 0)
        hit = ~found & (cum >= half + 1)
        out[hit] = v
        found |= hit
    assert found.all()
    return out


def median_interior(n, ksize):
    """The frames whose window lies inside the clip and inside one block: there the window holds at most ceil(k / 37) < k // 2 + 1
    outliers (k = 1 keeps an outlier), so the median IS the block's value - the closed form of the pattern."""
    f = np.arange(n)
    half = ksize // 2
    inside = (f - half >= 0) & (f + half <= n - 1) & ((f - half) // MEDIAN_BLOCK == (f + half) // MEDIAN_BLOCK)
    return inside & (ksize > 1)


def median_table_case(n_classes):
    """(flat values, table, [(x, block)] per clip): all clips back to back, a gap of 10 frames behind clip MEDIAN_GAP_AFTER; the
    clip of 3 frames stands before the long one."""
    parts, table, flat, base = [], [], [], 0
    for c, n in enumerate(MEDIAN_CLIPS):
        x, block = median_clip(n, n_classes, c)
        parts.append((x, block))
        table.append((base, n))
        flat.append(x)
        base += n
        if c == MEDIAN_GAP_AFTER:
            flat.append(np.full(MEDIAN_GAP, n_classes - 1, np.int32))
            base += MEDIAN_GAP
    return np.concatenate(flat), np.array(table, np.int64), parts


# ---------------------------------------------------------------------------------------------------------------
# the bins and the top-1
# ---------------------------------------------------------------------------------------------------------------
BIN_N = (1, 63, 64, 65, 257)
BIN_TIE_FRAMES, BIN_NAN_FRAMES = (60, 255), (63, 192)          # multiples of 3: they would be active
BIN_CLASSES, BIN_BEHAVIOR, BIN_THRESHOLD = 5, 2, 0.5


def bin_frames_of(n):
    return sorted({1, 63, 64, 65, n})


def bins_rows(n):
    """(n, 5) float32: column 2 holds 0.9 on the frames f % 3 == 0 and 0.1 elsewhere, the other columns 0.025 and 0.225: frame f
    is active iff f % 3 == 0 - but not the tie rows (every column 0.9) and the NaN rows."""
    f = np.arange(n)
    p = np.empty((n, BIN_CLASSES), np.float32)
    p[:] = np.where(f % 3 == 0, np.float32(0.025), np.float32(0.225))[:, None]
    p[:, BIN_BEHAVIOR] = np.where(f % 3 == 0, np.float32(0.9), np.float32(0.1))
    for t in BIN_TIE_FRAMES:
        if t < n:
            p[t] = np.float32(0.9)
    for t in BIN_NAN_FRAMES:
        if t < n:
            p[t] = np.nan
    return p


def bins_expected(n, bin_frames):
    bins = np.zeros(-(-n // bin_frames), np.int64)
    for f in range(0, n, 3):
        if f not in BIN_TIE_FRAMES and f not in BIN_NAN_FRAMES:
            bins[f // bin_frames] += 1
    return bins


TOP1_N = (255, 256, 257)
TOP1_NAN_ROWS = (0, 255, 256)


def top1_rows(n, n_classes=64):
    """(probs, pred, conf): row r has its maximum 0.75 + r / 2048 on column (r * 37) % 64 (neighbouring rows differ), everything
    else below 0.5; the rows 0, 255 and 256 that exist hold a NaN and get -1 / NaN."""
    r = np.arange(n)
    col = (r * 37) % n_classes
    h = (np.arange(n * n_classes, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 16)
    p = (h.astype(np.float64) / float(1 << 17)).astype(np.float32).reshape(n, n_classes)
    best = (0.75 + r / 2048.0).astype(np.float32)
    p[r, col] = best
    pred, conf = col.astype(np.int32), best.copy()
    for k, t in enumerate(TOP1_NAN_ROWS):
        if t < n:
            p[t, (t + 5 * k) % n_classes] = np.nan
            pred[t] = -1
            conf[t] = np.nan
    return p, pred, conf
