"""Decode bouts from per-frame probabilities: the Viterbi path of every clip under a sticky transition model, on the device.

    python -m cbas_amd.bouts --dir RECORDINGS --model NAME [--stay P | --mean-duration F | --instances labels.csv |
                             --fit-transitions ITERS] --out bouts.csv [--write-outputs NAME_viterbi] [--posteriors NAME_hmm]
                             [--save-transitions FILE.npy]

Every route from CLS rows to behaviour ends in an ``(N, C)`` probability matrix (the trained head, ``knn_labels``,
``probe_labels``, one-hot motifs).  ``viterbi_labels`` treats its rows as emissions of a hidden Markov model whose transition
matrix says how long a bout lasts and which behaviour follows which, and returns the most likely label sequence per clip
(``cbasx_viterbi_scores`` -> ``cbasx_viterbi_decode``, csrc/seq_viterbi.hip); ``decode_bouts`` hands it to
``postprocess.label_runs``.  Scores are integers, 256 per factor of two (``rint(256 * log2 p)``), so the device's piecewise
decode of a long clip is the serial definition bit for bit; ``viterbi_host`` states that definition in numpy and is what a CPU
tensor goes through.  The reference's only temporal model is the median filter (``postprocess.labels_median``).
DESIGN.md section 24.

The same model's forward-backward pass (``cbasx_hmm_posteriors``, csrc/seq_hmm.hip) gives what the hard path
cannot: ``posteriors`` returns the smoothed probabilities ``P(state_t | the whole clip)``, graded like a head's output and so fit
for the thresholds of ``predictions_to_instances`` and ``activity_bins``, and ``fit_transitions`` learns the transition matrix from
unlabelled recordings by a few rounds of expectation-maximisation over the expected transition counts.
"""
from __future__ import annotations

import argparse
import csv
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

UNIT, SCORE_MIN, TRANS_LIMIT, MAX_CLASSES, CHUNK = 256, -8192, 1 << 20, 64, 1024      # CBASX_VITERBI_* of include/cbas_mi355x_ext.h
FLAG_NAN = 1
CSV_COLUMNS = ["file", "start_frame", "end_frame", "label", "confidence"]


# ---- transition builders (host, float64) ----------------------------------------------------------------------------------------
def log_scores(p) -> np.ndarray:
    """``rint(256 * log2 p)`` as int32, held to [-2^20, 2^20]: a probability of 0 is the strongest "never"."""
    p = np.asarray(p, np.float64)
    if p.size and (np.isnan(p).any() or (p < 0).any()):
        raise ValueError("a probability is negative or not a number")
    with np.errstate(divide="ignore"):
        s = UNIT * np.log2(p)
    return np.clip(np.rint(np.clip(s, -TRANS_LIMIT, TRANS_LIMIT)), -TRANS_LIMIT, TRANS_LIMIT).astype(np.int32)


def _classes(n_classes: int) -> int:
    c = int(n_classes)
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError(f"{n_classes} classes: cbasx_viterbi_decode takes 1 .. {MAX_CLASSES}")
    return c


def _sticky(stay: np.ndarray, off: np.ndarray) -> np.ndarray:
    """Rows ``stay[a]`` on the diagonal and ``(1 - stay[a]) * off[a]`` beside it (``off`` rows sum to 1 off the diagonal)."""
    P = (1.0 - stay)[:, None] * off
    P[np.diag_indices(stay.size)] = stay
    return P


def sticky_transitions(n_classes: int, stay: Optional[float] = None, mean_duration: Optional[float] = None, as_probs: bool = False) -> np.ndarray:
    """``(C, C)`` int32: ``stay`` on the diagonal, the rest of each row spread evenly.  Give ``stay`` (default 0.98) or
    ``mean_duration`` in frames (``stay = 1 - 1 / mean_duration``: a bout of a geometric length with that mean), not both.
    With ``as_probs`` the same matrix as float32 probabilities, which is what ``posteriors`` and ``fit_transitions`` take."""
    c = _classes(n_classes)
    if stay is not None and mean_duration is not None:
        raise ValueError("give stay or mean_duration, not both")
    if mean_duration is not None:
        if not float(mean_duration) > 1.0:
            raise ValueError(f"mean_duration = {mean_duration}: more than 1 frame")
        stay = 1.0 - 1.0 / float(mean_duration)
    stay = 0.98 if stay is None else float(stay)
    if not 0.0 < stay < 1.0:
        raise ValueError(f"stay = {stay}: a probability strictly between 0 and 1")
    if c == 1:
        return np.ones((1, 1), np.float32) if as_probs else np.zeros((1, 1), np.int32)
    off = np.full((c, c), 1.0 / (c - 1))
    P = _sticky(np.full(c, stay), off)
    return P.astype(np.float32) if as_probs else log_scores(P)


def transitions_from_instances(instances, behaviors: Sequence[str], smoothing: float = 1.0) -> np.ndarray:
    """``(C, C)`` int32 from labelled bouts ``(cls_path, start, end, label)`` (``end`` inclusive; what
    ``knn.LabelBank.from_instances`` takes).  A class stays with ``1 - 1 / (the mean length of its bouts)``; a class without a
    bout takes the mean length of all bouts.  What leaves class a goes to b != a in proportion to ``smoothing`` + the number of
    times a bout of b is the next bout after one of a in the same file (by start frame).  Skipped: labels not in
    ``behaviors``, a start or end of -1."""
    behaviors = [str(b) for b in behaviors]
    c = _classes(len(behaviors))
    smoothing = float(smoothing)
    if not smoothing >= 0.0:
        raise ValueError(f"smoothing = {smoothing}: at least 0")
    lengths: List[List[int]] = [[] for _ in range(c)]
    by_file = {}
    for path, start, end, name in instances:
        name = str(name).strip()
        start, end = int(start), int(end)
        if name not in behaviors or start == -1 or end == -1:
            continue
        if end < start:
            raise ValueError(f"an instance of {name} ends at {end}, before its start {start}")
        k = behaviors.index(name)
        lengths[k].append(end - start + 1)
        by_file.setdefault(os.fspath(path) if path else "", []).append((start, k))
    every = [n for per in lengths for n in per]
    if not every:
        raise ValueError("no instance carries one of the behaviours")
    if c == 1:
        return np.zeros((1, 1), np.int32)
    mean = np.array([np.mean(per) if per else np.mean(every) for per in lengths], np.float64)
    stay = 1.0 - 1.0 / np.maximum(mean, 1.0)
    counts = np.full((c, c), smoothing)
    for bouts in by_file.values():
        bouts.sort()
        for (_, a), (_, b) in zip(bouts[:-1], bouts[1:]):
            if a != b:
                counts[a, b] += 1.0
    counts[np.diag_indices(c)] = 0.0
    rows = counts.sum(axis=1, keepdims=True)
    off = np.where(rows > 0, counts / np.where(rows > 0, rows, 1.0), (1.0 - np.eye(c)) / (c - 1))      # no evidence, no smoothing: evenly
    return log_scores(_sticky(stay, off))


def transitions_from_counts(counts, smoothing: float = 1.0) -> np.ndarray:
    """``(C, C)`` int32 from frame-to-frame counts (``motifs.transition_counts``: the diagonal counts a frame followed by its own
    class): every row of ``counts + smoothing``, normalised."""
    n = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    n = n.astype(np.float64)
    if n.ndim != 2 or n.shape[0] != n.shape[1]:
        raise ValueError(f"counts of shape {n.shape}: (C, C)")
    _classes(n.shape[0])
    if not np.isfinite(n).all() or (n < 0).any() or not float(smoothing) >= 0.0:
        raise ValueError("counts and smoothing must be finite and at least 0")
    n = n + float(smoothing)
    rows = n.sum(axis=1, keepdims=True)
    if (rows <= 0).any():
        raise ValueError("a class has no count and there is no smoothing")
    return log_scores(n / rows)


# ---- the numpy statement of the definition ------------------------------------------------------------------------------------------
def scores_host(probs) -> np.ndarray:
    """``cbasx_viterbi_scores`` in float64: ``clamp(rint(256 * log2(max(p, 2^-32))), -8192, 0)``; a NaN and a negative are -8192."""
    p = np.asarray(probs, np.float64)
    p = np.where(np.isnan(p) | (p < 2.0 ** -32), 2.0 ** -32, p)
    return np.clip(np.rint(UNIT * np.log2(p)), SCORE_MIN, 0).astype(np.int32)


def viterbi_host(scores, clip_table, transitions, prior=None) -> Tuple[np.ndarray, np.ndarray]:
    """``cbasx_viterbi_decode`` on the host: ``(labels (N,) int32, clip_score (n_clips,) int64)``; the lowest state wins a tie, at
    the end and at every back-pointer."""
    e = np.asarray(scores, np.int64)
    A = np.asarray(transitions, np.int64)
    table = np.asarray(clip_table, np.int64).reshape(-1, 2)
    N, C = e.shape
    pri = np.zeros(C, np.int64) if prior is None else np.asarray(prior, np.int64)
    labels = np.full(N, -1, np.int32)
    clip_score = np.zeros(table.shape[0], np.int64)
    for c, (first, n) in enumerate(table):
        if first < 0 or n < 0 or first + n > N:
            raise ValueError(f"clip {c} = ({first}, {n}) reaches outside the {N} frames")
        if n == 0:
            continue
        x = e[first:first + n]
        bp = np.zeros((n, C), np.int64)
        d = pri + x[0]
        for t in range(1, n):
            cand = d[:, None] + A                              # [i][j]
            bp[t] = cand.argmax(axis=0)                        # the first maximum: the lowest i
            d = cand.max(axis=0) + x[t]
        state = int(d.argmax())
        clip_score[c] = d[state]
        for t in range(n - 1, -1, -1):
            labels[first + t] = state
            state = int(bp[t, state])
    return labels, clip_score


# ---- the device calls ---------------------------------------------------------------------------------------------------------------
def _transitions(transitions, prior, C: int) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    A = transitions.detach().cpu().numpy() if torch.is_tensor(transitions) else np.asarray(transitions)
    if A.shape != (C, C) or not np.issubdtype(A.dtype, np.integer):
        raise ValueError(f"transitions of shape {A.shape} and type {A.dtype}: integer scores ({C}, {C}) (sticky_transitions, ...)")
    if prior is not None:
        prior = prior.detach().cpu().numpy() if torch.is_tensor(prior) else np.asarray(prior)
        if prior.shape != (C,) or not np.issubdtype(prior.dtype, np.integer):
            raise ValueError(f"prior of shape {prior.shape} and type {prior.dtype}: integer scores ({C},)")
        if np.abs(prior.astype(np.int64)).max() > TRANS_LIMIT:
            raise ValueError("a prior lies outside [-2^20, 2^20]")
        prior = np.ascontiguousarray(prior, np.int32)
    if np.abs(A.astype(np.int64)).max() > TRANS_LIMIT:
        raise ValueError("a transition lies outside [-2^20, 2^20]")
    return np.ascontiguousarray(A, np.int32), prior


def _host_table(clip_table) -> np.ndarray:
    t = clip_table.detach().cpu().numpy() if torch.is_tensor(clip_table) else np.asarray(clip_table)
    t = np.ascontiguousarray(t.astype(np.int64).reshape(-1, 2))
    if t.shape[0] < 1:
        raise ValueError("the clip table must hold at least one (first frame, frames) row")
    return t


def one_hot_scores(labels, C: int):
    """Scores of hard labels: 0 for the frame's label, -8192 for every other class; a label of -1 says nothing (all 0)."""
    if torch.is_tensor(labels):
        lab = labels.to(torch.int64)
        if lab.numel() and (int(lab.min()) < -1 or int(lab.max()) >= C):
            raise ValueError(f"a label outside [-1, {C})")
        cls = torch.arange(C, device=lab.device)
        return torch.where((lab[:, None] == cls[None, :]) | (lab[:, None] < 0), 0, SCORE_MIN).to(torch.int32).contiguous()
    lab = np.asarray(labels, np.int64)
    if lab.size and (lab.min() < -1 or lab.max() >= C):
        raise ValueError(f"a label outside [-1, {C})")
    return np.where((lab[:, None] == np.arange(C)[None, :]) | (lab[:, None] < 0), 0, SCORE_MIN).astype(np.int32)


def device_scores(probs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``cbasx_viterbi_scores``: ``(scores (N, C) int32, flags (1,) int32)`` of device probabilities; asynchronous."""
    if probs.dim() != 2 or probs.dtype != torch.float32 or not probs.is_cuda or not probs.is_contiguous():
        raise ValueError(f"probs must be a contiguous float32 (N, C) tensor on a GPU, got {probs.dtype} {tuple(probs.shape)}")
    dev = probs.device
    with torch.cuda.device(dev):
        scores = torch.empty(probs.shape, dtype=torch.int32, device=dev)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().cbasx_viterbi_scores(probs.data_ptr(), int(probs.shape[0]), int(probs.shape[1]), scores.data_ptr(),
                                                    flags.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "cbasx_viterbi_scores")
    return scores, flags


def device_decode(scores: torch.Tensor, table: np.ndarray, A: np.ndarray, prior: Optional[np.ndarray]) -> Tuple[torch.Tensor, torch.Tensor]:
    """``cbasx_viterbi_decode``: ``(labels (N,) int32, clip_score (n_clips,) int64)`` on the device of ``scores`` (N, C) int32."""
    if scores.dim() != 2 or scores.dtype != torch.int32 or not scores.is_cuda or not scores.is_contiguous():
        raise ValueError(f"scores must be a contiguous int32 (N, C) tensor on a GPU, got {scores.dtype} {tuple(scores.shape)}")
    dev = scores.device
    N, C = int(scores.shape[0]), int(scores.shape[1])
    lib = _lib.load()
    with torch.cuda.device(dev):
        table_dev = torch.from_numpy(table).to(dev)
        A_dev = torch.from_numpy(A).to(dev)
        prior_dev = None if prior is None else torch.from_numpy(prior).to(dev)
        labels = torch.empty(N, dtype=torch.int32, device=dev)
        clip_score = torch.empty(table.shape[0], dtype=torch.int64, device=dev)
        ws, need = _lib.workspace("cbasx_viterbi_workspace_bytes", dev, N, int(table.shape[0]), C)
        _lib.check(lib.cbasx_viterbi_decode(scores.data_ptr(), N, table_dev.data_ptr(), int(table.shape[0]), C, A_dev.data_ptr(),
                                            None if prior_dev is None else prior_dev.data_ptr(), labels.data_ptr(), clip_score.data_ptr(),
                                            ws.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream), "cbasx_viterbi_decode")
    return labels, clip_score


def viterbi_labels(probs, clip_table, transitions, prior=None, return_scores: bool = False):
    """The Viterbi labels ``(N,)`` int32 of every clip of ``clip_table`` (``(first frame, frames)`` rows; frames outside every
    clip get -1).  ``probs``: ``(N, C)`` float32 probabilities - a NaN counts as probability 0 - or ``(N,)`` integer labels, read
    as one-hot.  ``transitions`` ``(C, C)`` and ``prior`` ``(C,)`` are integer scores (``sticky_transitions``, ...).  A tensor on
    a GPU is decoded there and the labels stay there; a CPU tensor or an array goes through ``viterbi_host`` and comes back as
    a CPU tensor.  With ``return_scores`` also ``clip_score`` ``(n_clips,)`` int64, the score of every clip's path."""
    hard = (probs.dim() if torch.is_tensor(probs) else np.asarray(probs).ndim) == 1
    C = int(np.shape(transitions)[0]) if hard else int(probs.shape[1])
    _classes(C)
    A, pri = _transitions(transitions, prior, C)
    table = _host_table(clip_table)
    if torch.is_tensor(probs) and probs.is_cuda:
        scores = one_hot_scores(probs, C) if hard else device_scores(probs.to(torch.float32).contiguous())[0]
        labels, clip_score = device_decode(scores, table, A, pri)
    else:
        host = probs.detach().numpy() if torch.is_tensor(probs) else np.asarray(probs)
        scores = one_hot_scores(host, C) if hard else scores_host(host)
        labels, clip_score = (torch.from_numpy(x) for x in viterbi_host(scores, table, A, pri))
    return (labels, clip_score) if return_scores else labels


def decode_bouts(probs, clip_table, transitions, prior=None, min_frames: int = 1) -> np.ndarray:
    """``viterbi_labels`` then ``postprocess.label_runs``: the bouts as ``postprocess.LABEL_RUN_DTYPE`` records ordered by clip
    and start, ``confidence`` the mean over the bout of each frame's probability of its decoded label (1 for hard labels).
    Bouts of fewer than ``min_frames`` frames are dropped."""
    from . import postprocess as _post
    labels = viterbi_labels(probs, clip_table, transitions, prior)
    table = _host_table(clip_table)
    hard = probs.dim() == 1 if torch.is_tensor(probs) else np.asarray(probs).ndim == 1
    C = int(np.shape(transitions)[0])
    if labels.is_cuda:
        if hard:
            conf = torch.ones(labels.shape[0], dtype=torch.float32, device=labels.device)
        else:
            conf = probs.to(torch.float32).gather(1, labels.clamp(min=0).to(torch.int64)[:, None])[:, 0].contiguous()
        records = _post.label_runs(labels, conf, table, C)
    else:
        lab = labels.numpy()
        p = None if hard else (probs.detach().numpy() if torch.is_tensor(probs) else np.asarray(probs)).astype(np.float32)
        conf = np.ones(lab.size, np.float32) if hard else p[np.arange(lab.size), np.maximum(lab, 0)]
        rows = [(c, a, b, k, m) for c, (first, n) in enumerate(table)
                for a, b, k, m in _post.label_runs_host(lab[first:first + n], conf[first:first + n])]
        records = np.array(rows, dtype=_post.LABEL_RUN_DTYPE) if rows else np.empty(0, _post.LABEL_RUN_DTYPE)
    keep = records["end_frame"] - records["start_frame"] + 1 >= int(min_frames)
    return records[keep]


def index_bouts(index, probs, transitions, prior=None, min_frames: int = 1) -> np.ndarray:
    """``decode_bouts`` over a ``search.FrameIndex``: one clip per file, so ``clip`` of a record is the file's number."""
    n = int(probs.shape[0])
    if n != index.n_rows:
        raise ValueError(f"{n} rows of probabilities for the {index.n_rows} rows of the index")
    return decode_bouts(probs, index._table, transitions, prior, min_frames)


def write_outputs(index, labels, behaviors: Sequence[str], model_name: str) -> List[str]:
    """One-hot ``(N, C)`` probabilities of decoded labels as ``<stem>_<model_name>_outputs.csv`` beside every file of the index
    (``knn.write_outputs``, the writer ``motifs.write_outputs`` uses): ``activity_bins`` and the actogram take them unchanged.
    A frame without a label (-1) is a row of zeros."""
    from . import knn as _knn
    t = labels if torch.is_tensor(labels) else torch.from_numpy(np.asarray(labels))
    t = t.to(torch.int64)
    C = len(behaviors)
    if t.dim() != 1 or int(t.shape[0]) != index.n_rows or (t.numel() and (int(t.min()) < -1 or int(t.max()) >= C)):
        raise ValueError(f"labels of shape {tuple(t.shape)}: ({index.n_rows},) with values in [-1, {C})")
    probs = torch.nn.functional.one_hot(t + 1, C + 1)[:, 1:].to(torch.float32)
    return _knn.write_outputs(index, probs, list(behaviors), model_name)


# ---- forward-backward: smoothed probabilities and learned transitions --------------------------------------
HMM_CHUNK, HMM_FLOOR, HMM_ROW_TOL = 1024, 2.0 ** -32, 1e-4      # CBASX_HMM_* of include/cbas_mi355x_ext.h
FLAG_EMISSION, FLAG_POSTERIOR = 1, 2


def _stochastic(M, what: str, shape) -> np.ndarray:
    """``M`` as float64 of ``shape`` with every entry finite and at least 0 and every row summing to 1 within 1e-4, or ValueError."""
    M = M.detach().cpu().numpy() if torch.is_tensor(M) else np.asarray(M)
    if M.shape != tuple(shape) or np.issubdtype(M.dtype, np.integer) or M.dtype == bool:
        raise ValueError(f"{what} of shape {M.shape} and type {M.dtype}: float probabilities {tuple(shape)} (transition_probs turns scores into them)")
    M = M.astype(np.float64)
    if not np.isfinite(M).all() or (M < 0).any():
        raise ValueError(f"{what}: an entry is negative or not finite")
    if (np.abs(M.sum(axis=-1) - 1.0) > HMM_ROW_TOL).any():
        raise ValueError(f"{what}: a row does not sum to 1 within {HMM_ROW_TOL}")
    return M


def transition_probs(scores_or_probs) -> np.ndarray:
    """Float32 probabilities ``(C, C)`` or ``(C,)`` for ``posteriors``: integer scores (``sticky_transitions``, ``log_scores``,
    ...) become ``2^(s / 256)`` with every row renormalised, since rounded scores do not sum to exactly 1; float probabilities are
    checked and passed on.  ``log_scores`` is the way back."""
    M = scores_or_probs.detach().cpu().numpy() if torch.is_tensor(scores_or_probs) else np.asarray(scores_or_probs)
    if M.ndim not in (1, 2) or (M.ndim == 2 and M.shape[0] != M.shape[1]):
        raise ValueError(f"shape {M.shape}: (C, C) transitions or a (C,) prior")
    _classes(M.shape[-1])
    if np.issubdtype(M.dtype, np.integer):
        P = np.exp2(np.clip(M.astype(np.float64), -TRANS_LIMIT, TRANS_LIMIT) / UNIT)
        rows = P.sum(axis=-1, keepdims=True)
        if (rows <= 0).any():
            raise ValueError("a row of scores leaves no transition with a positive probability")
        return (P / rows).astype(np.float32)
    return _stochastic(M, "probabilities", M.shape).astype(np.float32)


@np.errstate(all="ignore")                                 # a clip without a posterior is reported by its flag and its NaN rows
def posteriors_host(probs, clip_table, transitions, prior=None, dtype=np.float64):
    """The serial definition of ``cbasx_hmm_posteriors`` in numpy: ``(gamma (N, C) dtype, Xi (C, C) float64, Pi (C,) float64,
    loglik (n_clips,) float64 in bits, flags)``.  Per clip: ``b_t = max(p_t, 2^-32)``; ``a_0 = prior * b_0``, ``a_t = (alpha_{t-1}
    A) * b_t``, ``alpha_t = a_t / sum(a_t)``, ``loglik = sum_t log2 sum(a_t)``; ``beta_{T-1} = 1``, ``beta_t = A (b_{t+1} *
    beta_{t+1})`` over the power of two of its largest entry; ``gamma_t = alpha_t * beta_t`` over its sum; ``xi_t[i][j] =
    alpha_t[i] A[i][j] b_{t+1}[j] beta_{t+1}[j]`` over its sum.  All of it in ``dtype`` except the sums over frames and clips
    (``Xi``, ``Pi``, ``loglik``), which are float64: ``dtype=np.float32`` is the restatement the device's tolerances are measured
    with.  What CPU tensors and arrays go through."""
    dt = np.dtype(dtype)
    p = np.asarray(probs)
    if p.ndim != 2:
        raise ValueError(f"probs of shape {p.shape}: (N, C)")
    N, C = p.shape
    _classes(C)
    A = _stochastic(transitions, "transitions", (C, C)).astype(dt)
    pri = (np.full(C, 1.0 / C) if prior is None else _stochastic(prior, "prior", (C,))).astype(dt)
    table = _host_table(clip_table)
    wrong = np.isnan(p) | (p < 0)
    b_all = np.where(wrong | (p < HMM_FLOOR), HMM_FLOOR, p).astype(dt)
    gamma = np.zeros((N, C), dt)
    Xi, Pi, loglik, flags = np.zeros((C, C)), np.zeros(C), np.zeros(table.shape[0]), 0
    for c, (first, n) in enumerate(table):
        if first < 0 or n < 0 or first + n > N:
            raise ValueError(f"clip {c} = ({first}, {n}) reaches outside the {N} frames")
        if n == 0:
            continue
        if wrong[first:first + n].any():
            flags |= FLAG_EMISSION
        b = b_all[first:first + n]
        alpha = np.empty((n, C), dt)
        sums = np.empty(n, dt)
        a = pri * b[0]
        for t in range(n):
            if t:
                a = (a @ A) * b[t]
            sums[t] = a.sum()
            a = a / sums[t]
            alpha[t] = a
        loglik[c] = np.log2(sums.astype(np.float64)).sum()
        W = np.empty((n, C), dt)                               # W[t] = b_t * beta_t, beta_t up to a power of two
        raw = np.empty((n, C), dt)                             # raw[t] = A W[t + 1]: beta_t in the scale of W[t + 1]
        beta = np.ones(C, dt)
        raw[n - 1] = beta
        for t in range(n - 1, 0, -1):
            W[t] = b[t] * beta
            raw[t - 1] = A @ W[t]
            top = raw[t - 1].max()
            beta = np.ldexp(raw[t - 1], -int(np.frexp(top)[1])) if np.isfinite(top) and top > 0 else raw[t - 1]
        g = alpha * raw
        Z = g.sum(axis=1)
        bad = ~(np.isfinite(Z) & (Z > 0))
        with np.errstate(divide="ignore", invalid="ignore"):
            gamma[first:first + n] = np.where(bad[:, None], np.nan, g / Z[:, None])
            coef = np.where(bad[:-1, None], 0, alpha[:-1] / Z[:-1, None])          # a step without a posterior counts nothing
        if bad.any():
            flags |= FLAG_POSTERIOR
        if n > 1:
            # sum_t xi_t = A * sum_t (alpha_t / Z_t) (x) W[t + 1], and Z_t = sum_ij alpha_t[i] A[i][j] W[t + 1][j] is the sum of xi_t
            # (a coefficient of 0 does not silence a W that is not finite: 0 * inf is a NaN, so such a step's W goes too)
            Xi += A.astype(np.float64) * (coef.astype(np.float64).T @ np.where(bad[:-1, None], 0, W[1:]).astype(np.float64))
        Pi += gamma[first].astype(np.float64)
    return gamma, Xi, Pi, loglik, flags


def _device_table(clip_table, dev) -> torch.Tensor:
    if torch.is_tensor(clip_table) and clip_table.is_cuda:
        t = clip_table.to(dev, torch.int64).reshape(-1, 2).contiguous()
        if t.shape[0] < 1:
            raise ValueError("the clip table must hold at least one (first frame, frames) row")
        return t
    return torch.from_numpy(_host_table(clip_table)).to(dev)


def _device_probs(M, what: str, shape, dev) -> torch.Tensor:
    """Transitions or a prior for the device call.  What is on a GPU already stays there and is checked by the call's own
    checking pass, so nothing is read back; everything else is checked here."""
    if torch.is_tensor(M) and M.is_cuda:
        if tuple(M.shape) != tuple(shape) or not M.dtype.is_floating_point:
            raise ValueError(f"{what} of shape {tuple(M.shape)} and type {M.dtype}: float probabilities {tuple(shape)}")
        return M.to(dev, torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(_stochastic(M, what, shape), np.float32)).to(dev)


def device_posteriors(probs: torch.Tensor, table_dev: torch.Tensor, A_dev: torch.Tensor, prior_dev: Optional[torch.Tensor] = None,
                      counts: bool = True):
    """``cbasx_hmm_posteriors`` on device tensors: ``(gamma (N, C) float32, Xi (C, C), Pi (C,), loglik (n_clips,) float64 - or
    None each without ``counts`` - and flags (1,) int32)``.  The call synchronises the stream once, for its checking pass."""
    if probs.dim() != 2 or probs.dtype != torch.float32 or not probs.is_cuda or not probs.is_contiguous():
        raise ValueError(f"probs must be a contiguous float32 (N, C) tensor on a GPU, got {probs.dtype} {tuple(probs.shape)}")
    dev = probs.device
    N, C, n_clips = int(probs.shape[0]), int(probs.shape[1]), int(table_dev.shape[0])
    lib = _lib.load()
    with torch.cuda.device(dev):
        store = torch.empty((max(N, 1), C), dtype=torch.float32, device=dev)          # never a null pointer
        gamma = store[:N]
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        xi = torch.empty((C, C), dtype=torch.float64, device=dev) if counts else None
        pi = torch.empty(C, dtype=torch.float64, device=dev) if counts else None
        loglik = torch.empty(n_clips, dtype=torch.float64, device=dev) if counts else None
        ws, need = _lib.workspace("cbasx_hmm_workspace_bytes", dev, N, n_clips, C)
        src = probs if N else torch.empty((1, C), dtype=torch.float32, device=dev)
        _lib.check(lib.cbasx_hmm_posteriors(src.data_ptr(), N, table_dev.data_ptr(), n_clips, C, A_dev.data_ptr(),
                                            None if prior_dev is None else prior_dev.data_ptr(), store.data_ptr(),
                                            None if xi is None else xi.data_ptr(), None if pi is None else pi.data_ptr(),
                                            None if loglik is None else loglik.data_ptr(), flags.data_ptr(), ws.data_ptr(), need,
                                            torch.cuda.current_stream(dev).cuda_stream), "cbasx_hmm_posteriors")
    return gamma, xi, pi, loglik, flags


def posteriors(probs, clip_table, transitions, prior=None, return_counts: bool = False, emission_prior=None):
    """The smoothed probabilities ``gamma`` ``(N, C)`` float32, ``gamma[t, c] = P(state_t = c | the whole clip)``, of every clip of
    ``clip_table`` (``(first frame, frames)`` rows; frames outside every clip get a row of zeros) by the forward-backward pass.
    ``transitions`` ``(C, C)`` and ``prior`` ``(C,)`` (None: uniform) are float PROBABILITIES (``transition_probs``,
    ``sticky_transitions(..., as_probs=True)``, ``fit_transitions``).  A NaN or negative probability counts as 2^-32.  A tensor
    on a GPU is smoothed there (``cbasx_hmm_posteriors``) and the result stays there; a CPU tensor or an array goes through
    ``posteriors_host`` and comes back as CPU tensors.  With ``return_counts`` also ``(Xi, Pi, loglik)`` in float64: the expected
    transition counts ``(C, C)``, the expected first states ``(C,)`` and every clip's log-likelihood in bits.  ``emission_prior``
    ``(C,)`` divides every row by these class frequencies and renormalises it first - the scaled-likelihood correction for a
    classifier's outputs."""
    C = int(probs.shape[1])
    _classes(C)
    if torch.is_tensor(probs) and probs.is_cuda:
        dev = probs.device
        p = probs.to(torch.float32)
        if emission_prior is not None:
            p = p / torch.as_tensor(emission_prior, dtype=torch.float32, device=dev).reshape(1, C)
            p = p / p.sum(dim=1, keepdim=True)
        gamma, Xi, Pi, loglik, _ = device_posteriors(p.contiguous(), _device_table(clip_table, dev), _device_probs(transitions, "transitions", (C, C), dev),
                                                     None if prior is None else _device_probs(prior, "prior", (C,), dev), counts=return_counts)
    else:
        p = (probs.detach().numpy() if torch.is_tensor(probs) else np.asarray(probs)).astype(np.float32)
        if emission_prior is not None:
            p = p / np.asarray(emission_prior, np.float32).reshape(1, C)
            p = p / p.sum(axis=1, keepdims=True)
        gamma, Xi, Pi, loglik, _ = posteriors_host(p, clip_table, transitions, prior)
        gamma, Xi, Pi, loglik = torch.from_numpy(gamma.astype(np.float32)), torch.from_numpy(Xi), torch.from_numpy(Pi), torch.from_numpy(loglik)
    return (gamma, Xi, Pi, loglik) if return_counts else gamma


def fit_transitions(probs, clip_table, init=None, iters: int = 10, smoothing: float = 1.0, fit_prior: bool = False):
    """Learn the transitions from the recordings themselves: exactly ``iters`` rounds of ``posteriors`` -> ``A = rows of (Xi +
    smoothing), normalised`` (Baum-Welch with the emissions held fixed) and, with ``fit_prior``, ``prior = (Pi + smoothing),
    normalised``.  ``init`` ``(C, C)`` probabilities default to ``sticky_transitions(C, as_probs=True)``.  Returns ``(A (C, C)
    float32, prior (C,) float32, loglik (iters,) float64)`` as arrays: ``loglik[r]`` is the total log-likelihood in bits under the
    transitions round ``r`` STARTED from, so it does not decrease from round to round.  On a GPU the small update is torch on the
    device; nothing is read back before the last round.  ``log_scores(A)`` is what ``viterbi_labels`` takes.  With ``smoothing`` 0
    a state no frame ever visits leaves an empty row, which the next round refuses."""
    C = int(probs.shape[1])
    _classes(C)
    iters, smoothing = int(iters), float(smoothing)
    if iters < 1 or not smoothing >= 0.0:
        raise ValueError(f"iters = {iters}, smoothing = {smoothing}: at least one round and a smoothing of at least 0")
    on_gpu = torch.is_tensor(probs) and probs.is_cuda
    dev = probs.device if on_gpu else torch.device("cpu")
    A = torch.from_numpy(_stochastic(sticky_transitions(C, as_probs=True) if init is None else init, "init", (C, C))).to(dev)
    pri = torch.full((C,), 1.0 / C, dtype=torch.float64, device=dev)
    table = _device_table(clip_table, dev) if on_gpu else _host_table(clip_table)
    p = probs.to(torch.float32).contiguous() if on_gpu else probs
    rounds = []
    for _ in range(iters):
        _, Xi, Pi, loglik = posteriors(p, table, A, pri if fit_prior else None, return_counts=True)
        rounds.append(loglik.sum())
        A = Xi + smoothing
        A = A / A.sum(dim=1, keepdim=True)
        if fit_prior:
            pri = (Pi + smoothing) / (Pi + smoothing).sum()
    return A.cpu().numpy().astype(np.float32), pri.cpu().numpy().astype(np.float32), torch.stack(rounds).cpu().numpy()


def index_posteriors(index, probs, transitions, prior=None, return_counts: bool = False, emission_prior=None):
    """``posteriors`` over a ``search.FrameIndex``: one clip per file."""
    n = int(probs.shape[0])
    if n != index.n_rows:
        raise ValueError(f"{n} rows of probabilities for the {index.n_rows} rows of the index")
    return posteriors(probs, index._table, transitions, prior, return_counts=return_counts, emission_prior=emission_prior)


# ---- command line -------------------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m cbas_amd.bouts", description=__doc__.split("\n\n")[0])
    ap.add_argument("--dir", required=True, help="a recording directory with *_NAME_outputs.csv files")
    ap.add_argument("--model", required=True, metavar="NAME", help="the model whose _outputs.csv files are decoded")
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--stay", type=float, default=None, metavar="P", help="probability that a frame keeps the label of the one before (default 0.98)")
    how.add_argument("--mean-duration", type=float, default=None, metavar="F", help="mean bout length in frames: stay = 1 - 1 / F")
    how.add_argument("--instances", default=None, metavar="labels.csv", help="file,start,end,label lines: stay and order from labelled bouts")
    how.add_argument("--fit-transitions", type=int, default=None, metavar="ITERS",
                     help="learn the transitions from the files read, in ITERS rounds of forward-backward, before decoding or smoothing")
    ap.add_argument("--min-frames", type=int, default=1, help="shortest bout written")
    ap.add_argument("--out", required=True, help="the CSV to write: " + ",".join(CSV_COLUMNS))
    ap.add_argument("--write-outputs", default=None, metavar="NAME_viterbi", help="write one-hot *_NAME_viterbi_outputs.csv beside every file")
    ap.add_argument("--posteriors", default=None, metavar="NAME_hmm", help="write the smoothed probabilities as *_NAME_hmm_outputs.csv beside every file")
    ap.add_argument("--save-transitions", default=None, metavar="FILE.npy", help="write the transition probabilities that were used, (C, C) float32")
    ap.add_argument("--device", default=None, help="cuda:0, cpu, ... (default: a GPU when there is one)")
    return ap


def parse_cli(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.stay is not None and not 0.0 < a.stay < 1.0:
        ap.error(f"--stay {a.stay}: strictly between 0 and 1")
    if a.mean_duration is not None and not a.mean_duration > 1.0:
        ap.error(f"--mean-duration {a.mean_duration}: more than 1 frame")
    if a.min_frames < 1:
        ap.error(f"--min-frames {a.min_frames}: at least 1")
    if a.write_outputs is not None and a.write_outputs == a.model:
        ap.error("--write-outputs must not name the model that is read")
    if a.fit_transitions is not None and a.fit_transitions < 1:
        ap.error(f"--fit-transitions {a.fit_transitions}: at least 1 round")
    if a.posteriors is not None and a.posteriors in (a.model, a.write_outputs):
        ap.error("--posteriors must name neither the model that is read nor the --write-outputs files")
    if a.save_transitions is not None and not a.save_transitions.endswith(".npy"):
        ap.error(f"--save-transitions {a.save_transitions}: a .npy file")
    return ap, a


def write_csv(path: str, files: Sequence[str], records: np.ndarray, behaviors: Sequence[str]) -> None:
    """One line per bout: the file, its first and last frame within the file, the behaviour's name, the mean confidence."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(CSV_COLUMNS)
        for r in records:
            w.writerow([files[int(r["clip"])], int(r["start_frame"]), int(r["end_frame"]), behaviors[int(r["label"])],
                        f"{float(r['confidence']):.6f}"])


def main(argv=None) -> int:
    from . import knn as _knn, pipeline as _pipeline, postprocess as _post
    ap, a = parse_cli(argv)
    files = _post.outputs_files(a.dir, a.model) if os.path.isdir(a.dir) else []
    if not files:
        ap.error(f"no *_{a.model}_outputs.csv file in {a.dir}")
    behaviors, parts = None, []
    for path in files:
        header, values, _exact = _pipeline.read_outputs_csv(path)
        if behaviors is None:
            behaviors = header
        if header != behaviors:
            ap.error(f"{path} has the columns {header}, {files[0]} has {behaviors}")
        parts.append(values.astype(np.float32))
    lengths = np.array([p.shape[0] for p in parts], np.int64)
    table = np.stack([np.concatenate([[0], np.cumsum(lengths)[:-1]]), lengths], axis=1)
    probs = torch.from_numpy(np.concatenate(parts) if parts else np.empty((0, len(behaviors)), np.float32))
    device = torch.device(a.device) if a.device else torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    if device.type == "cuda":
        probs = probs.to(device)
    fitted = None
    try:
        if a.fit_transitions is not None:
            fitted, _, rounds = fit_transitions(probs, table, iters=a.fit_transitions)
            transitions = log_scores(fitted)
            print(f"transitions after {a.fit_transitions} rounds (log-likelihood {rounds[0]:.1f} -> {rounds[-1]:.1f} bits), rows from, columns to: "
                  + " ".join(behaviors))
            print(np.array2string(fitted, precision=4, suppress_small=True, max_line_width=200))
        elif a.instances:
            transitions = transitions_from_instances(_knn.read_instances_csv(a.instances)[0], behaviors)
        else:
            transitions = sticky_transitions(len(behaviors), stay=a.stay, mean_duration=a.mean_duration)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    used = transition_probs(transitions) if fitted is None else fitted
    if a.save_transitions:
        np.save(a.save_transitions, used)
        print(f"transitions -> {a.save_transitions}")
    records = decode_bouts(probs, table, transitions, min_frames=a.min_frames)
    write_csv(a.out, files, records, behaviors)
    print(f"{len(records)} bouts over {int(lengths.sum())} frames of {len(files)} files -> {a.out}")
    if a.write_outputs:
        labels = viterbi_labels(probs, table, transitions).cpu().numpy().astype(np.int64)
        one_hot = (labels[:, None] == np.arange(len(behaviors))[None, :]).astype(np.float32)
        suffix = f"_{a.model}_outputs.csv"
        for path, (first, n) in zip(files, table):
            _pipeline.write_probs_csv(path[:-len(suffix)] + f"_{a.write_outputs}_outputs.csv", one_hot[first:first + n], list(behaviors))
        print(f"{len(files)} files like {files[0][:-len(suffix)]}_{a.write_outputs}_outputs.csv")
    if a.posteriors:
        gamma = posteriors(probs, table, used).cpu().numpy()
        suffix = f"_{a.model}_outputs.csv"
        for path, (first, n) in zip(files, table):
            _pipeline.write_probs_csv(path[:-len(suffix)] + f"_{a.posteriors}_outputs.csv", gamma[first:first + n], list(behaviors))
        print(f"{len(files)} files like {files[0][:-len(suffix)]}_{a.posteriors}_outputs.csv")
    return 0


if __name__ == "__main__":
    sys.exit(main())
