"""Fit a motif HMM on the resident rows: motifs whose emission model is learned from the features together with the transitions.

``motifs.cluster_frames`` finds motifs one frame at a time and ``bouts.posteriors`` smooths probabilities somebody else made; this
module closes the loop.  States c = 0 .. C-1 have unit mean directions ``mu_c`` over the working rows ``u_t`` (a row over its norm,
as ``cbas_rows_kmeans_*`` defines it) and ONE shared concentration ``kappa = 1 / temperature`` that is held fixed:

    b_t[c] = softmax_c(kappa * (u_t . mu_c))                 von Mises-Fisher emissions of equal kappa

  E step   ``cbasx_rows_emissions`` (csrc/rows_hmm.hip) -> ``cbasx_hmm_posteriors`` (csrc/seq_hmm.hip), unchanged
  M step   ``cbasx_rows_weighted_sums``: S_c = sum_t gamma[t, c] u_t, then mu_c = S_c / |S_c|; A and the prior from the expected
           counts exactly as ``bouts.fit_transitions`` forms them

With kappa fixed and shared this is exact EM: the density's normaliser does not depend on c and cancels.  kappa is a parameter on
purpose - its maximum-likelihood value for 768-dimensional rows is in the thousands, which makes every posterior one-hot and the
transitions irrelevant; the temperature says how much one frame counts against its neighbours.  DESIGN.md section 26.

A ``search.FrameIndex`` on a GPU is fitted there and nothing but the model leaves the device.  An index built on "cpu" goes through
the float64 numpy statement of the same rounds (``emissions_host``, ``weighted_sums_host``, ``bouts.posteriors_host``): the
definition, at the speed of the definition - for tests and small files, not for recordings.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, bouts as _bouts

MAX_STATES, MAX_DIM = 64, 1536                        # CBASX_ROWS_HMM_MAX_STATES / _MAX_DIM of include/cbas_mi355x_ext.h
MAX_PARTS, PART_ROWS = 256, 64                        # CBASX_ROWS_HMM_MAX_PARTS / _PART_ROWS
MASS_MIN = 1e-6                                       # a state of less expected mass keeps its mean
LN9 = math.log(9.0)


# ---- the two device passes --------------------------------------------------------------------------------------------------------
def _rows_ok(rows: torch.Tensor) -> Tuple[int, int, int]:
    if rows.dim() != 2 or rows.dtype != torch.float16 or not rows.is_cuda or rows.stride(1) != 1:
        raise ValueError(f"rows must be a float16 (N, D) tensor on a GPU with unit column stride, got {rows.dtype} {tuple(rows.shape)}")
    return int(rows.shape[0]), int(rows.shape[1]), int(rows.stride(0)) if rows.shape[0] > 1 else int(rows.shape[1])


def device_emissions(rows: torch.Tensor, means: torch.Tensor, kappa: float, log_weights: Optional[torch.Tensor] = None,
                     normalize: bool = True, want_lognorm: bool = True):
    """``cbasx_rows_emissions``: ``(probs (N, C) float32, lognorm (N,) float32 in bits or None)`` on the device of ``rows``
    ((N, D) fp16) for ``means`` (C, D) float32 there; asynchronous."""
    N, D, ld = _rows_ok(rows)
    dev = rows.device
    if means.dim() != 2 or int(means.shape[1]) != D or means.dtype != torch.float32 or means.device != dev or not means.is_contiguous():
        raise ValueError(f"means must be a contiguous float32 (C, {D}) tensor on {dev}, got {means.dtype} {tuple(means.shape)}")
    C = int(means.shape[0])
    with torch.cuda.device(dev):
        probs = torch.empty((max(N, 1), C), dtype=torch.float32, device=dev)[:N]
        lognorm = torch.empty(max(N, 1), dtype=torch.float32, device=dev)[:N] if want_lognorm else None
        _lib.check(_lib.load().cbasx_rows_emissions(rows.data_ptr(), N, D, ld, C, int(bool(normalize)), means.data_ptr(), float(kappa),
                                                    None if log_weights is None else log_weights.data_ptr(), probs.data_ptr(),
                                                    None if lognorm is None else lognorm.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "cbasx_rows_emissions")
    return probs, lognorm


def device_weighted_sums(rows: torch.Tensor, weights: torch.Tensor, normalize: bool = True, workspace: Optional[torch.Tensor] = None):
    """``cbasx_rows_weighted_sums``: ``(sums (C, D) float64, mass (C,) float64)`` on the device of ``rows`` for ``weights`` (N, C)
    float32 there; asynchronous."""
    N, D, ld = _rows_ok(rows)
    dev = rows.device
    if weights.dim() != 2 or int(weights.shape[0]) != N or weights.dtype != torch.float32 or weights.device != dev or not weights.is_contiguous():
        raise ValueError(f"weights must be a contiguous float32 ({N}, C) tensor on {dev}, got {weights.dtype} {tuple(weights.shape)}")
    C = int(weights.shape[1])
    with torch.cuda.device(dev):
        sums = torch.empty((C, D), dtype=torch.float64, device=dev)
        mass = torch.empty(C, dtype=torch.float64, device=dev)
        need = _lib.workspace_bytes("cbasx_rows_weighted_sums_workspace_bytes", N, D, C)
        ws = workspace if workspace is not None and workspace.numel() >= need else torch.empty(need, dtype=torch.uint8, device=dev)
        src = weights if N else torch.empty((1, C), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().cbasx_rows_weighted_sums(rows.data_ptr(), N, D, ld, C, int(bool(normalize)), src.data_ptr(), sums.data_ptr(),
                                                        mass.data_ptr(), ws.data_ptr(), int(ws.numel()), torch.cuda.current_stream(dev).cuda_stream),
                   "cbasx_rows_weighted_sums")
    return sums, mass


# ---- the same two passes in float64 numpy: what an index on "cpu" goes through ----------------------------------------------------
def _working_rows(x, normalize: bool) -> np.ndarray:
    x = np.asarray(x, np.float64)
    if not normalize:
        return x
    norm = np.sqrt((x * x).sum(axis=1, keepdims=True))
    return np.divide(x, norm, out=np.zeros_like(x), where=norm > 0)


def emissions_host(x, means, kappa: float, log_weights=None, normalize: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """``cbasx_rows_emissions`` in float64: ``(probs (N, C), lognorm (N,) in bits)``."""
    z = float(kappa) * (_working_rows(x, normalize) @ np.asarray(means, np.float64).T)
    if log_weights is not None:
        z = z + np.asarray(log_weights, np.float64)[None, :]
    m = z.max(axis=1, keepdims=True)
    ex = np.exp(z - m)
    s = ex.sum(axis=1, keepdims=True)
    return ex / s, ((m + np.log(s)) / math.log(2.0))[:, 0]


def weighted_sums_host(x, weights, normalize: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """``cbasx_rows_weighted_sums`` in float64: ``(sums (C, D), mass (C,))``."""
    w = np.asarray(weights, np.float64)
    return w.T @ _working_rows(x, normalize), w.sum(axis=0)


def _kmeans_host(u: np.ndarray, k: int, iters: int) -> np.ndarray:
    """Farthest-point seeds and ``iters`` Lloyd rounds over working rows in float64 (the rule of ``cbas_rows_kmeans_fit``): the
    starting means of a fit on a "cpu" index."""
    d = ((u - u.mean(axis=0)) ** 2).sum(axis=1)
    picks, mind = [int(d.argmax())], None
    for _ in range(1, k):
        d = ((u - u[picks[-1]]) ** 2).sum(axis=1)
        mind = d if mind is None else np.minimum(mind, d)
        picks.append(int(mind.argmax()))
    cent = u[picks].copy()
    for _ in range(iters):
        lab = (u @ cent.T - 0.5 * (cent * cent).sum(axis=1)[None, :]).argmax(axis=1)
        for j in range(k):
            if (lab == j).any():
                cent[j] = u[lab == j].mean(axis=0)
    return cent


# ---- the M step ---------------------------------------------------------------------------------------------------------------------
def em_update(means: torch.Tensor, sums: torch.Tensor, mass: torch.Tensor, Xi: torch.Tensor, Pi: torch.Tensor, prior: torch.Tensor,
              smoothing: float, fit_prior: bool):
    """``(means (C, D) float32, A (C, C) float64, prior (C,) float64)`` from a round's sums: ``mu = S / |S|`` - a state of mass
    below 1e-6 (or with S = 0) keeps its mean -, ``A`` = the rows of ``Xi + smoothing`` normalised and, with ``fit_prior``, the prior
    = ``Pi + smoothing`` normalised, as ``bouts.fit_transitions`` forms them.  Plain torch on whatever device the tensors are on."""
    norm = sums.norm(dim=1, keepdim=True)
    keep = (mass < MASS_MIN)[:, None] | ~(norm > 0)
    new = torch.where(keep, means.to(torch.float64), sums / torch.where(norm > 0, norm, torch.ones_like(norm))).to(torch.float32)
    A = Xi + smoothing
    A = A / A.sum(dim=1, keepdim=True)
    if fit_prior:
        prior = (Pi + smoothing) / (Pi + smoothing).sum()
    return new, A, prior


def calibrate_temperature(probs_at_kappa_1: torch.Tensor, owned: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The self-calibrated temperature from one emissions pass at kappa = 1: ``log(p1 / p2)`` of a frame's two best states is its
    top-2 cosine gap; the temperature is the median gap over ``ln 9``, so that a typical frame alone gives its own motif 9 : 1.  A
    0-dim float64 tensor on the device of the probabilities (1.0 for a single state, at least 1e-6)."""
    p = probs_at_kappa_1 if owned is None else probs_at_kappa_1[owned]
    if p.shape[1] < 2 or p.shape[0] < 1:
        return torch.ones((), dtype=torch.float64, device=p.device)
    top = p.to(torch.float64).topk(2, dim=1).values
    gap = (top[:, 0].log() - top[:, 1].log()).median()
    return (gap / LN9).clamp_min(1e-6)


# ---- the model --------------------------------------------------------------------------------------------------------------------
class MotifHMM:
    """A fitted motif HMM: ``means`` (C, D) float32 unit directions by descending ``occupancy`` (C) float64 (the expected frames
    per state), ``transitions`` (C, C) and ``prior`` (C) float32 probabilities, ``temperature`` (1 / kappa), ``loglik`` (iters)
    float64 - round r's total log-likelihood in bits under the parameters the round STARTED from -, ``dim``, ``normalize``."""

    def __init__(self, means, transitions, prior, temperature: float, occupancy, loglik, dim: int, normalize: bool):
        self.means = np.ascontiguousarray(means, np.float32)
        self.transitions = np.ascontiguousarray(transitions, np.float32)
        self.prior = np.ascontiguousarray(prior, np.float32)
        self.temperature = float(temperature)
        self.occupancy = np.asarray(occupancy, np.float64)
        self.loglik = np.asarray(loglik, np.float64)
        self.dim, self.normalize = int(dim), bool(normalize)
        C = self.means.shape[0] if self.means.ndim == 2 else -1
        if self.means.ndim != 2 or self.means.shape[1] != self.dim or self.transitions.shape != (C, C) or self.prior.shape != (C,) \
                or self.occupancy.shape != (C,):
            raise ValueError(f"means of shape {self.means.shape}, transitions {self.transitions.shape}, prior {self.prior.shape} and occupancy "
                             f"{self.occupancy.shape} for rows of width {self.dim}")
        if not self.temperature > 0.0 or not math.isfinite(self.temperature):
            raise ValueError(f"temperature = {temperature}: positive and finite")

    @property
    def n_states(self) -> int:
        return int(self.means.shape[0])

    n_clusters = n_states                                         # what motifs.motif_runs and motifs.exemplars ask a clustering for

    @property
    def centroids(self) -> np.ndarray:
        return self.means

    @property
    def kappa(self) -> float:
        return 1.0 / self.temperature

    def save(self, path: str) -> None:
        np.savez(path, means=self.means, transitions=self.transitions, prior=self.prior, temperature=np.float64(self.temperature),
                 occupancy=self.occupancy, loglik=self.loglik, dim=np.int64(self.dim), normalize=np.int64(self.normalize))

    @classmethod
    def load(cls, path: str) -> "MotifHMM":
        with np.load(path, allow_pickle=False) as z:
            return cls(z["means"], z["transitions"], z["prior"], float(z["temperature"]), z["occupancy"], z["loglik"], int(z["dim"]),
                       bool(int(z["normalize"])))

    def _check(self, index) -> None:
        if index.dim != self.dim:
            raise ValueError(f"the model was fitted on rows of width {self.dim}; this index holds rows of width {index.dim}")

    def emissions(self, index) -> torch.Tensor:
        """``probs`` (N, C) float32 on the index's device: every frame's emission probabilities."""
        self._check(index)
        if index.device.type == "cuda":
            return device_emissions(index.rows, torch.from_numpy(self.means).to(index.device), self.kappa, None, self.normalize, False)[0]
        return torch.from_numpy(emissions_host(index.rows.numpy(), self.means, self.kappa, None, self.normalize)[0].astype(np.float32))

    def posteriors(self, index) -> torch.Tensor:
        """``gamma`` (N, C) float32 on the index's device: P(state | the whole file) of every frame, one clip per file."""
        return _bouts.posteriors(self.emissions(index), index._table, self.transitions, self.prior)

    def labels(self, index) -> torch.Tensor:
        """The Viterbi motif (N,) int32 of every frame under ``log_scores(transitions)`` and ``log_scores(prior)``."""
        return _bouts.viterbi_labels(self.emissions(index), index._table, _bouts.log_scores(self.transitions), _bouts.log_scores(self.prior))


def _initial_means(index, init, C: int, normalize: bool) -> np.ndarray:
    """(C, D) float64 unit directions from a ``motifs.FrameClusters``, an array, or - None - a short k-means."""
    from . import motifs as _motifs
    if init is None:
        if C < 2:
            u = _working_rows(index.rows[: 1 << 16].cpu().numpy(), normalize)
            m = u.mean(axis=0, keepdims=True)
        elif index.device.type == "cuda":
            m = _motifs.cluster_frames(index, n_clusters=C, iters=5, normalize=normalize)[2].centroids
        else:
            m = _kmeans_host(_working_rows(index.rows.numpy(), normalize), C, 5)
    elif isinstance(init, _motifs.FrameClusters):
        if init.dim != index.dim:
            raise ValueError(f"the clusters were fitted on rows of width {init.dim}; this index holds rows of width {index.dim}")
        m = init.centroids
    else:
        m = init.detach().cpu().numpy() if torch.is_tensor(init) else np.asarray(init)
    m = np.asarray(m, np.float64)
    if m.shape != (C, index.dim) or not np.isfinite(m).all():
        raise ValueError(f"initial means of shape {m.shape}: finite, ({C}, {index.dim})")
    norm = np.sqrt((m * m).sum(axis=1, keepdims=True))
    if (norm <= 0).any():
        raise ValueError("an initial mean is zero: it has no direction")
    return m / norm


def fit(index, n_states: int = 16, iters: int = 20, temperature: Optional[float] = None, init=None, transitions=None, smoothing: float = 1.0,
        fit_prior: bool = False, normalize: bool = True):
    """``(gamma, model)``: ``gamma`` (N, C) float32 on the index's device, the posterior of every frame, and the ``MotifHMM``.

    ``iters`` rounds of EM - emissions, ``bouts.device_posteriors``, weighted sums, ``em_update`` - and one closing E step under the
    final parameters.  ``init``: a ``motifs.FrameClusters``, a (C, D) array of means, or None for ``index.cluster(n_states,
    iters=5)``.  ``transitions`` (C, C) probabilities default to ``bouts.sticky_transitions(C, mean_duration=40, as_probs=True)``.
    ``temperature`` None is calibrated before the first round (``calibrate_temperature`` on the initial means) and returned in the
    model.  On a GPU nothing is read back before the last round apart from the one synchronisation ``cbasx_hmm_posteriors`` makes.
    The states come back by descending expected occupancy, means, transitions, prior and the columns of gamma permuted together."""
    C, iters, smoothing = int(n_states), int(iters), float(smoothing)
    if isinstance(init, np.ndarray) or torch.is_tensor(init):
        C = int(init.shape[0])
    elif init is not None and hasattr(init, "n_clusters"):
        C = int(init.n_clusters)
    if not 1 <= C <= MAX_STATES:
        raise ValueError(f"{C} states: 1 .. {MAX_STATES}")
    if iters < 0 or not smoothing >= 0.0:
        raise ValueError(f"iters = {iters}, smoothing = {smoothing}: at least 0 each")
    if temperature is not None and not (float(temperature) > 0.0 and math.isfinite(float(temperature))):
        raise ValueError(f"temperature = {temperature}: positive and finite")
    A0 = _bouts._stochastic(_bouts.sticky_transitions(C, mean_duration=40, as_probs=True) if transitions is None else transitions, "transitions", (C, C))
    mu0 = _initial_means(index, init, C, bool(normalize)).astype(np.float32)
    on_gpu = index.device.type == "cuda"
    dev = index.device
    N, D = index.n_rows, index.dim
    means = torch.from_numpy(mu0).to(dev)
    A = torch.from_numpy(A0).to(dev)
    prior = torch.full((C,), 1.0 / C, dtype=torch.float64, device=dev)
    owned = torch.zeros(N, dtype=torch.bool)
    for first, n in index._table:
        owned[int(first):int(first) + int(n)] = True
    owned = owned.to(dev)
    x_host = None if on_gpu else index.rows.numpy()
    table = index.clip_table if on_gpu else index._table
    ws = None
    if on_gpu:
        ws = torch.empty(_lib.workspace_bytes("cbasx_rows_weighted_sums_workspace_bytes", N, D, C), dtype=torch.uint8, device=dev)

    def e_pass(kappa: float, want_lognorm: bool = True):
        if on_gpu:
            return device_emissions(index.rows, means.contiguous(), kappa, None, normalize, want_lognorm)
        p, ln = emissions_host(x_host, means.numpy(), kappa, None, normalize)
        return torch.from_numpy(p.astype(np.float32)), torch.from_numpy(ln)

    def smooth(probs):
        if on_gpu:
            return _bouts.device_posteriors(probs, table, A.to(torch.float32).contiguous(), prior.to(torch.float32).contiguous() if fit_prior else None)[:4]
        g, Xi, Pi, ll, _ = _bouts.posteriors_host(probs.numpy(), table, A.numpy(), prior.numpy() if fit_prior else None)
        return torch.from_numpy(g.astype(np.float32)), torch.from_numpy(Xi), torch.from_numpy(Pi), torch.from_numpy(ll)

    if temperature is None:
        temperature = float(calibrate_temperature(e_pass(1.0, False)[0], owned))       # the one read-back before the rounds
    kappa = 1.0 / float(temperature)
    history = []
    for _ in range(iters):
        probs, lognorm = e_pass(kappa)
        gamma, Xi, Pi, loglik = smooth(probs)
        history.append(loglik.sum() + torch.where(owned, lognorm.to(torch.float64), 0.0).sum())      # no index by a mask: that would synchronise
        if on_gpu:
            sums, mass = device_weighted_sums(index.rows, gamma.contiguous(), normalize, ws)
        else:
            sums, mass = (torch.from_numpy(v) for v in weighted_sums_host(x_host, gamma.numpy(), normalize))
        means, A, prior = em_update(means, sums, mass, Xi, Pi, prior, smoothing, fit_prior)
    # the closing E step runs twice: once for the occupancies that order the states, once more through the renumbered model itself,
    # so that what is returned is bit for bit what the saved model gives on the same rows (a sum over states depends on their order)
    occupancy = smooth(e_pass(kappa, False)[0])[0].to(torch.float64).sum(dim=0)
    order = torch.argsort(-occupancy, stable=True)
    model = MotifHMM(means[order].cpu().numpy(), A[order][:, order].cpu().numpy().astype(np.float32),
                     prior[order].cpu().numpy().astype(np.float32), float(temperature), occupancy[order].cpu().numpy(),
                     torch.stack(history).cpu().numpy() if history else np.zeros(0), D, bool(normalize))
    return model.posteriors(index), model
