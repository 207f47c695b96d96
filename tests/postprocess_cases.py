"""Seeded inputs shared by the post-processing tests and tests/golden/make_goldens_postprocess.py: probability rows whose
top-1 label runs in blocks of random length with flicker (single-frame switches inside a block), so that the median filter
has something to change, inside the clip and at its zero-padded ends; the cases the reference was run on; and the input
condition of DESIGN.md "Events, pre-labels and actogram bins": no probability within 2^-24 relative of a threshold."""
import numpy as np

MODEL = "m"
# predictions_to_instances: (seed, frames, classes, threshold)
EVENT_CASES = [(1, 400, 9, 0.7), (2, 257, 5, 0.5), (3, 64, 2, 0.9), (4, 1, 3, 0.3), (5, 300, 9, 0.0), (6, 130, 1, 0.5)]
# predictions_to_instances_with_confidence: (seed, frames, classes, smoothing_window)
BLOCK_CASES = [(11, 400, 9, 1), (12, 400, 9, 5), (13, 300, 5, 31), (14, 90, 9, 4), (15, 7, 3, 15), (16, 130, 1, 3), (17, 2, 4, 3)]
# Actogram(preloaded_df=...): (seed, frames, classes, behaviour index, threshold, framerate, binsize_minutes)
ACTO_DF_CASES = [(21, 500, 9, 2, 0.5, 0.1, 1), (22, 333, 5, 0, 0.0, 0.05, 2), (23, 100, 1, 0, 0.5, 0.1, 1), (24, 64, 3, 1, 0.9, 10.0, 1),
                 (25, 200, 4, 3, -1.0, 0.1, 1)]
# Actogram(directory=..., model=...): files whose names need the numeric sort, with their seeds and frames
ACTO_DIR_FILES = [("rec_10_m_outputs.csv", 31, 70), ("rec_2_m_outputs.csv", 32, 45), ("rec_1_m_outputs.csv", 33, 58)]
ACTO_DIR_CASES = [(9, 4, 0.5, 0.1, 1), (9, 0, 0.35, 0.2, 1)]          # (classes, behaviour index, threshold, framerate, minutes)


def names(n_classes: int) -> list:
    return [f"beh{c}" for c in range(n_classes)]


def probabilities(seed: int, n: int, n_classes: int) -> np.ndarray:
    """float32 rows (n, C): softmax of noise plus a boost on the block's label; blocks of 3 - 40 frames, 8 % of the frames
    flicker to another label, the boost varies so that the top-1 probability crosses the usual thresholds, and every 13th row
    has an exact tie between its two largest entries."""
    rng = np.random.default_rng(seed)
    label = np.empty(n, np.int64)
    a = 0
    while a < n:
        b = min(n, a + int(rng.integers(3, 41)))
        label[a:b] = rng.integers(0, n_classes)
        a = b
    flicker = rng.random(n) < 0.08
    label = np.where(flicker, rng.integers(0, n_classes, n), label)
    z = rng.standard_normal((n, n_classes)) * 0.5
    z[np.arange(n), label] += rng.uniform(0.5, 4.0, n)
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
    if n_classes > 1:
        for r in range(5, n, 13):
            order = np.argsort(p[r])
            p[r, order[-2]] = p[r, order[-1]]
    return p


def clear_of(p: np.ndarray, threshold: float) -> bool:
    """The input condition: no value within 2^-23 relative of the threshold (twice the CSV's 2^-24)."""
    return not bool((np.abs(p.astype(np.float64) - threshold) <= abs(threshold) * 2.0 ** -23).any())
