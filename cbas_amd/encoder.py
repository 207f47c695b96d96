"""``DinoEncoder`` — drop-in for the reference's encoder object (backend/cbas.py:650-677).

Same constructor (``DinoEncoder(model_identifier: str, device="cuda")``), same ``.device``
attribute, same call contract (``encoder(x)`` with ``x`` float32 ``(B, S, H, W)`` in [0, 1] ->
``(B, S, D)``), but the forward pass runs in the hand-written HIP kernels of libcbas_mi355x.so
through the C ABI (``cbas_enc_*``).  torch tensors are only containers for device memory.

Extras beyond the reference interface (used by ``encode_file`` and the benchmarks):
``encode_u8`` takes uint8 frames already in HBM, ``submit_host``/``wait`` stream host chunks
through pinned staging with copy/compute overlap.  ``cls_attention``, ``hidden_state`` / ``patch_tokens`` /
``similarity_map`` and ``patch_pca`` are the three ways to look at what the encoder sees; ``hidden_states``, ``cls_attention(layer=)``
and ``attention_rollout`` look below the last layer.
"""
from __future__ import annotations

import os

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .config import ViTConfig, find_checkpoint_dir, is_convnext, parse_fp8_plan, fp8_plan_name, FP8_PLAN_DEFAULT
from .weights import load_encoder_checkpoint, convnext_param_shapes


def pack_encoder_weights(cfg: ViTConfig, w: Dict[str, np.ndarray]) -> np.ndarray:
    """Flatten an HF state dict into the blob order documented in include/cbas_mi355x.h."""
    if is_convnext(cfg):
        # the ConvNeXt blob is the state dict in convnext_param_shapes' order, every tensor as stored
        return np.ascontiguousarray(np.concatenate([np.asarray(w[k], np.float32).reshape(-1)
                                                    for k in convnext_param_shapes(cfg)]))
    from .weights import canonical_encoder_weights
    w = dict(canonical_encoder_weights(cfg, w))    # DINOv2-with-registers keys -> the DINOv3 names used below
    D = cfg.hidden_size
    parts = [w["embeddings.cls_token"].reshape(-1)]
    if cfg.num_register_tokens > 0:                # plain DINOv2 (R = 0) has no such tensor: an empty register block
        parts.append(w["embeddings.register_tokens"].reshape(-1))
    if cfg.pos_embed_grid > 0:
        parts.append(w["embeddings.position_embeddings"].reshape(-1))
    parts += [w["embeddings.patch_embeddings.weight"].reshape(-1), w["embeddings.patch_embeddings.bias"].reshape(-1)]
    zero_kb = np.zeros(D, np.float32)
    gate = ("mlp.gate_proj.weight", "mlp.gate_proj.bias") if cfg.use_gated_mlp else ()     # immediately before up_proj
    for i in range(cfg.num_hidden_layers):
        p = f"model.layer.{i}."
        w.setdefault(p + "attention.k_proj.bias", zero_kb)       # DINOv3 has no key bias ([tf] key_bias=False)
        for k in ("norm1.weight", "norm1.bias", "attention.q_proj.weight", "attention.q_proj.bias",
                  "attention.k_proj.weight", "attention.k_proj.bias", "attention.v_proj.weight", "attention.v_proj.bias",
                  "attention.o_proj.weight", "attention.o_proj.bias", "layer_scale1.lambda1",
                  "norm2.weight", "norm2.bias", *gate, "mlp.up_proj.weight", "mlp.up_proj.bias",
                  "mlp.down_proj.weight", "mlp.down_proj.bias", "layer_scale2.lambda1"):
            parts.append(np.asarray(w[p + k], np.float32).reshape(-1))
    parts += [w["norm.weight"].reshape(-1), w["norm.bias"].reshape(-1)]
    blob = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32) for p in parts]))
    assert blob.shape[0] > D
    return blob


def _device_index(device: torch.device) -> int:
    if device.type != "cuda":
        raise RuntimeError(
            f"cbas_amd runs only on an AMD GPU exposed as torch device 'cuda' (got {device}); there is no CPU path")
    return device.index if device.index is not None else torch.cuda.current_device()


def _frame_args(frames: torch.Tensor, channel: int, what: str):
    """The two frame forms of the synchronous forwards: uint8 (n,H,W,3) / (n,H,W), or float32 (B,1,H,W).  Returns the contiguous
    tensor, n, H, W, the uint8 byte strides (None for float32) and the byte offset of ``channel``."""
    assert frames.is_cuda
    if frames.dtype == torch.uint8:
        frames = frames.contiguous()
        if frames.dim() == 4:
            n, H, W, Cn = frames.shape
            return frames, n, H, W, (H * W * Cn, W * Cn, Cn), channel
        n, H, W = frames.shape
        return frames, n, H, W, (H * W, W, 1), 0
    if frames.dtype != torch.float32 or frames.dim() != 4 or frames.shape[1] != 1:
        raise ValueError(f"{what} takes uint8 (n,H,W,3) / (n,H,W) frames or a float32 (B,1,H,W) tensor")
    frames = frames.contiguous()
    n, _, H, W = frames.shape
    return frames, n, H, W, None, 0


def token_grid(cfg, H: int, W: int):
    """(nh, nw, P0) of ``hidden_state``'s rows for an H x W frame: the patch grid and the rows in front of it (ViT: CLS and
    registers; ConvNeXt: the pooled row, over the last stage's grid of 32 x 32 pixel cells)."""
    if is_convnext(cfg):
        nh, nw = cfg.stage_grids(H, W)[-1]
        return nh, nw, 1
    return H // cfg.patch_size, W // cfg.patch_size, cfg.num_prefix_tokens


def query_token_index(cfg, H: int, W: int, query) -> int:
    """The row of ``hidden_state`` under pixel ``query = (y, x)`` of an H x W frame (None: 0, the CLS / pooled row).  Pixels of
    the margin a grid of whole patches leaves uncovered have no patch: ``ValueError``."""
    if query is None:
        return 0
    nh, nw, P0 = token_grid(cfg, H, W)
    cell = 32 if is_convnext(cfg) else cfg.patch_size
    y, x = int(query[0]), int(query[1])
    if not (0 <= y < nh * cell and 0 <= x < nw * cell):
        raise ValueError(f"query pixel ({y}, {x}) is outside the {nh * cell} x {nw * cell} pixels the {nh} x {nw} patch grid covers")
    return P0 + (y // cell) * nw + x // cell


def normalize_layers(layers, L: int, lo: int = 0, what: str = "hidden-state"):
    """A list of layer indices in [lo, L] from ``None`` / ``"all"`` (every one), an int or a sequence; negative values count from
    the end (-1 = L).  Out of range: ``ValueError``."""
    if layers is None or (isinstance(layers, str) and layers == "all"):
        return list(range(lo, L + 1))
    if isinstance(layers, str):
        raise ValueError(f"{what} layers {layers!r}: a list of indices, or 'all'")
    seq = [layers] if isinstance(layers, (int, np.integer)) else list(layers)
    if not seq:
        raise ValueError(f"an empty list of {what} layers")
    out = []
    for v in seq:
        i = int(v)
        i = i + L + 1 if i < 0 else i
        if not lo <= i <= L:
            raise ValueError(f"{what} layer {int(v)} is outside {lo} .. {L} (negative values count from the end)")
        out.append(i)
    return out


PCA_DEFAULT_ITERS = 64      # rounds of subspace iteration in ``patch_pca``: chosen on the host by tests/test_patch_pca_host.py


class PatchPCABasis:
    """What ``DinoEncoder.patch_pca`` fitted: ``mean`` (b, D), ``components`` (b, k, D) with unit rows ordered by ``eigenvalues``
    (b, k) descending, ``total_variance`` (b,) - float32 tensors, b = 1 for scope "batch" and one per frame for scope "frame" - and
    ``stamp``, the fitting encoder's (``DinoEncoder.stamp``).  A basis colours only rows of the encoder it was fitted on: ``check``
    refuses another width or stamp.  The stamp is a name, not a digest of the weights: it catches another checkpoint or
    precision, not two sets of weights loaded under one name (``from_weights`` encoders all share ``<in-memory>``)."""

    def __init__(self, mean, components, eigenvalues, total_variance, scope: str, stamp: str):
        if scope not in ("frame", "batch"):
            raise ValueError(f"scope {scope!r}: 'frame' or 'batch'")
        if components.dim() != 3 or mean.dim() != 2 or tuple(mean.shape) != (components.shape[0], components.shape[2]) \
                or tuple(eigenvalues.shape) != tuple(components.shape[:2]) or tuple(total_variance.shape) != (components.shape[0],):
            raise ValueError("a basis is mean (b, D), components (b, k, D), eigenvalues (b, k), total_variance (b,)")
        if scope == "batch" and components.shape[0] != 1:
            raise ValueError("a batch-scope basis is one basis")
        self.mean, self.components, self.eigenvalues, self.total_variance = mean, components, eigenvalues, total_variance
        self.scope, self.stamp = scope, str(stamp)

    @property
    def n_bases(self) -> int:
        return int(self.components.shape[0])

    @property
    def n_components(self) -> int:
        return int(self.components.shape[1])

    @property
    def dim(self) -> int:
        return int(self.components.shape[2])

    @property
    def explained_variance_ratio(self):
        """eigenvalues / total_variance, (b, k): the share of the patch rows' variance each component carries."""
        return self.eigenvalues / self.total_variance[:, None]

    def check(self, dim: int, stamp: str) -> None:
        if self.dim != int(dim):
            raise ValueError(f"this basis was fitted on rows of width {self.dim}; the encoder's rows are {int(dim)} wide")
        if self.stamp != str(stamp):
            raise ValueError(f"this basis was fitted on encoder {self.stamp!r}, not on {str(stamp)!r}: its directions mean nothing here")


KMEANS_DEFAULT_ITERS = 16   # Lloyd rounds in ``patch_clusters``: chosen on the host by tests/test_patch_kmeans_host.py


class PatchClusters:
    """What ``DinoEncoder.patch_clusters`` fitted: ``centroids`` (b, k, D) float32 ordered by ``counts`` (b, k) int32 descending,
    ``inertia`` (b, iters + 1) float32 - the sum of squared distances after 0 .. iters updates - and ``init_index`` (b, k) int32, the
    seed rows in seeding order; b = 1 for scope "batch" and one per frame for scope "frame".  ``normalize``: whether rows are scaled
    to unit length before they are compared; ``stamp``: the fitting encoder's (``DinoEncoder.stamp``).  A set labels only rows of
    the encoder it was fitted on: ``check`` refuses another width or stamp, as ``PatchPCABasis.check`` does."""

    def __init__(self, centroids, counts, inertia, init_index, scope: str, normalize: bool, stamp: str):
        if scope not in ("frame", "batch"):
            raise ValueError(f"scope {scope!r}: 'frame' or 'batch'")
        if centroids.dim() != 3 or tuple(counts.shape) != tuple(centroids.shape[:2]) or tuple(init_index.shape) != tuple(centroids.shape[:2]) \
                or inertia.dim() != 2 or inertia.shape[0] != centroids.shape[0]:
            raise ValueError("a cluster set is centroids (b, k, D), counts (b, k), inertia (b, iters + 1), init_index (b, k)")
        if scope == "batch" and centroids.shape[0] != 1:
            raise ValueError("a batch-scope cluster set is one set")
        self.centroids, self.counts, self.inertia, self.init_index = centroids, counts, inertia, init_index
        self.scope, self.normalize, self.stamp = scope, bool(normalize), str(stamp)

    @property
    def n_sets(self) -> int:
        return int(self.centroids.shape[0])

    @property
    def n_clusters(self) -> int:
        return int(self.centroids.shape[1])

    @property
    def dim(self) -> int:
        return int(self.centroids.shape[2])

    def check(self, dim: int, stamp: str) -> None:
        if self.dim != int(dim):
            raise ValueError(f"these clusters were fitted on rows of width {self.dim}; the encoder's rows are {int(dim)} wide")
        if self.stamp != str(stamp):
            raise ValueError(f"these clusters were fitted on encoder {self.stamp!r}, not on {str(stamp)!r}: their centroids mean nothing here")


# What an encoder built the reference's way - DinoEncoder(model_identifier, device), integration.install(),
# `python -m cbas_amd.encode_files` - computes in: 4 = fp32 storage / attention / LayerNorm with the GEMM products as three-term
# fp16 splits: the mode that meets BOTH halves of the path's contract (CLS within 1e-3 - by three orders of magnitude - and
# argmax labels identical to the reference CPU path).  The fp16-operand mode (0) is the explicit fast mode.
DEFAULT_PRECISION = 4


class DinoEncoder:
    """MI355X encoder (DINOv3 ViT / ConvNeXt, DINOv2 with or without registers) behind the reference's ``DinoEncoder`` interface."""

    def __init__(self, model_identifier: str, device="cuda", max_batch: int = 128,
                 max_frame: Tuple[int, int] = (256, 256), precision: Optional[int] = None, fp8_plan=None):
        # max_batch: frames per encoder launch sequence.  A frame's row does not depend on its batch (bit-exact:
        # tests/test_gpu_parity.py::test_vitb_full_batch_invariance), so this is scheduling only: 128 runs the file path
        # ~3 % faster than 64 (fewer partly-filled tile rounds per frame; 256 adds nothing) for ~1 GB more workspace.
        print(f"Loading DINO encoder model: {model_identifier}")          # the reference's line (backend/cbas.py:654)
        ckpt = find_checkpoint_dir(model_identifier)
        cfg, weights = load_encoder_checkpoint(ckpt)
        if precision is None:
            # CBAS constructs the encoder as DinoEncoder(model_identifier=..., device=...) (startup_page.py:66-69): an
            # unmodified checkout gets DEFAULT_PRECISION = 4, the contract-complete mode - CLS rows ~1e-6 from the reference's
            # fp32 CPU path and EVERY argmax label the reference's (tests/test_gpu_fp32.py strict gates; 10.5k frames/s for
            # ViT-B/16 on one MI355X).  CBAS_PRECISION=0 opts into the reference's own GPU behaviour - fp16 operands, as under
            # its torch.autocast (cbas.py:433-434) - 2.2x faster, rows within 1e-3, <= 1 % of near-tie labels differ from the
            # CPU path.  MX-fp8 (2) is refused here: its rows need their own heads.
            precision = int(os.environ.get("CBAS_PRECISION", str(DEFAULT_PRECISION)))
            if precision == 2:
                raise ValueError("CBAS_PRECISION=2 (MX-fp8) is not selectable through the environment: its rows are not "
                                 "interchangeable with the other modes' (pass precision=2 explicitly)")
        if fp8_plan is None and int(precision) == 2:
            # precision 2 is only ever asked for explicitly; WHICH of its GEMMs are MX-fp8 may come from the environment
            # (name or mask: config.parse_fp8_plan) - the files are stamped with the plan either way (pipeline.file_attrs)
            fp8_plan = os.environ.get("CBAS_FP8_PLAN") or None
        self._init(cfg, weights, device, max_batch, max_frame, precision, **({} if fp8_plan is None else {"fp8_plan": fp8_plan}))
        self.model_identifier = model_identifier
        mode = {0: "fp16 operands - the reference's own GPU behaviour under autocast (fast mode)", 1: "fp16 activations, hi + lo split weights",
                2: "MX-fp8 operands", 3: "fp32 end to end (label-exact)",
                4: "fp32 with split-fp16 GEMM products (label-exact; CBAS_PRECISION=0 selects the fast mode)"}.get(int(precision), "?")
        if int(precision) == 2 and self.fp8_plan != FP8_PLAN_DEFAULT:
            mode += f", plan {fp8_plan_name(self.fp8_plan)!r} (mask {self.fp8_plan}: the other GEMMs run on fp16 operands)"
        print(f"cbas_amd: MI355X encoder on {getattr(self, 'device', device)}, precision {int(precision)}: {mode}")

    @classmethod
    def from_weights(cls, cfg: ViTConfig, weights: Dict[str, np.ndarray], device="cuda", max_batch: int = 64,
                     max_frame: Tuple[int, int] = (256, 256), precision: int = 0, fp8_plan=None) -> "DinoEncoder":
        """``fp8_plan`` (precision 2 only): which GEMMs take MX-fp8 operands - "all" (the default), "mlp", "mlp_qkv", "up",
        "down", GEMM names joined by '+', or a mask (config.parse_fp8_plan)."""
        self = cls.__new__(cls)
        self._init(cfg, weights, device, max_batch, max_frame, precision, fp8_plan)
        self.model_identifier = "<in-memory>"
        return self

    def _init(self, cfg: ViTConfig, weights, device, max_batch, max_frame, precision, fp8_plan=None):
        cfg.validate()
        convnext = is_convnext(cfg)
        if fp8_plan is not None and int(precision) != 2:
            raise ValueError(f"fp8_plan={fp8_plan!r} needs precision=2 (MX-fp8); precision {int(precision)} has no fp8 GEMMs")
        self._fp8_plan = parse_fp8_plan(fp8_plan)
        if convnext and int(precision) not in (3, 4):
            raise ValueError(f"precision {int(precision)}: DINOv3 ConvNeXt encoders run in precision 3 (fp32) or 4 (the default: "
                             "fp32 with split-fp16 GEMM products) only")
        # the MLP kind travels beside the config struct (cbas_enc_create_mlp): every handle of this encoder - the one rebuilt
        # for larger frames and the precision-3 range-fallback twin included - is created through _create with it
        self._mlp = _lib.MLP_SWIGLU if getattr(cfg, "use_gated_mlp", False) else _lib.MLP_GELU
        if self._mlp == _lib.MLP_SWIGLU and int(precision) not in (0, 3, 4):
            raise ValueError(f"precision {int(precision)}: a gated-MLP encoder (DINOv3 ViT-S+ / H+) runs in precision 0, 3 or 4 "
                             "(there is no MX-fp8 and no hi+lo form of the gated GEMM)")
        self.config = cfg
        self.device = torch.device(device)
        self._dev = _device_index(self.device)
        self.max_batch = int(max_batch)
        self.max_frame = (int(max_frame[0]), int(max_frame[1]))
        self._lib = _lib.load()
        if convnext:
            self._cfg_c = _lib.EncConfig(hidden_size=cfg.hidden_size, layer_norm_eps=cfg.layer_norm_eps, max_batch=self.max_batch,
                                         max_height=self.max_frame[0], max_width=self.max_frame[1], precision=int(precision),
                                         family=1, stage_widths=(C.c_int32 * 4)(*cfg.hidden_sizes),
                                         stage_depths=(C.c_int32 * 4)(*cfg.depths))
        else:
            self._cfg_c = _lib.EncConfig(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers,
                                         cfg.num_attention_heads, cfg.num_register_tokens, cfg.patch_size,
                                         cfg.layer_norm_eps, cfg.rope_theta, self.max_batch, self.max_frame[0],
                                         self.max_frame[1], int(precision), int(cfg.use_rope), int(cfg.pos_embed_grid))
        blob = pack_encoder_weights(cfg, weights)
        need = self._lib.cbas_enc_weights_count_mlp(C.byref(self._cfg_c), self._mlp)
        if need != blob.shape[0]:
            raise RuntimeError(f"weight blob has {blob.shape[0]} floats, library expects {need}")
        self._blob = blob                 # kept so that the handle can be rebuilt for larger frames
        self._h = None
        self._create()

    def _create(self) -> None:
        h = C.c_void_p()
        _lib.check(self._lib.cbas_enc_create_mlp(C.byref(self._cfg_c), self._mlp, self._blob.ctypes.data, self._blob.shape[0],
                                                 self._dev, C.byref(h)), "cbas_enc_create_mlp")
        self._h = h
        if getattr(self.config, "model_type", None) == "dinov2":
            # plain DINOv2 resamples its position table without antialiasing (HF modeling_dinov2.py:86-91).  Set on EVERY handle
            # built from this config - the rebuild for larger frames and the precision-3 range-fallback twin come through here
            _lib.check(self._lib.cbas_enc_set_pos_interp(h, _lib.POS_INTERP_BICUBIC), "cbas_enc_set_pos_interp")
        if self.precision == 2 and self._fp8_plan != FP8_PLAN_DEFAULT:
            # like the position filter: on every handle of this encoder, the one rebuilt for larger frames included
            _lib.check(self._lib.cbas_enc_set_fp8_plan(h, self._fp8_plan), "cbas_enc_set_fp8_plan")

    def _fit_frame(self, H: int, W: int) -> None:
        """The reference takes any frame size; the workspace here is sized at create.  Frames larger than
        ``max_frame`` rebuild the handle once with a workspace that fits them (weights are re-uploaded)."""
        if H <= self.max_frame[0] and W <= self.max_frame[1]:
            return
        if getattr(self, "_slot_n", None):
            raise RuntimeError("frame size grew while batches are in flight; wait for them first")
        new = (max(H, self.max_frame[0]), max(W, self.max_frame[1]))
        print(f"cbas_amd: frames of {H}x{W} exceed the encoder workspace ({self.max_frame[0]}x{self.max_frame[1]}); "
              f"rebuilding it for {new[0]}x{new[1]}")
        torch.cuda.synchronize(self.device)
        self.close()
        self.max_frame = new
        self._cfg_c.max_height, self._cfg_c.max_width = new
        self._create()

    @property
    def precision(self) -> int:
        """0 fp16 operands (the explicit fast mode; `from_weights`' default), 1 fp16 hi+lo weights, 2 MX-fp8 throughput mode,
        3 fp32 end to end - the reference's CPU arithmetic, 4 the same with the GEMM products as three-term fp16 splits (as
        exact, three times as fast: the DEFAULT of an encoder built the reference's way) (include/cbas_mi355x.h)."""
        return int(self._cfg_c.precision)

    @property
    def fp8_plan(self) -> int:
        """Precision 2: the mask of GEMMs that take MX-fp8 operands (1 qkv, 2 proj, 4 up, 8 down; 15 = "all", the default);
        0 in every other precision.  ``config.fp8_plan_name`` gives its name."""
        return int(getattr(self, "_fp8_plan", 0)) if self.precision == 2 else 0

    # -- nn.Module-like surface used by the reference ------------------------------------------
    def eval(self):
        return self

    def to(self, device):
        if torch.device(device) != self.device and torch.device(device).type != self.device.type:
            raise RuntimeError("the MI355X encoder cannot be moved off its device")
        return self

    def parameters(self):
        return iter(())

    def _register_session(self, session) -> None:
        import weakref
        if getattr(self, "_sessions", None) is None:
            self._sessions = weakref.WeakSet()
        self._sessions.add(session)

    def range_fallback(self) -> "DinoEncoder":
        """The same model in precision 3 (fp32 end to end: no operand range limit), built on first use from this encoder's own
        weight blob and closed with it.  The file paths re-encode a video here when its activations left this encoder's
        range (CBAS_ERANGE: fp16 storage in precision 0, the scaled fp16 halves of precision 4) - the reference's fp32
        arithmetic has no such limit, so a drop-in must not fail where the reference would have produced rows."""
        twin = getattr(self, "_range_twin", None)
        if twin is None:
            twin = DinoEncoder.__new__(DinoEncoder)
            twin.config, twin.device, twin._dev = self.config, self.device, self._dev
            twin.max_batch, twin.max_frame = self.max_batch, self.max_frame
            twin._lib, twin._blob = self._lib, self._blob
            twin._cfg_c = _lib.EncConfig.from_buffer_copy(self._cfg_c)       # every field, the family's included
            twin._cfg_c.precision = 3
            twin._mlp = self._mlp                # a gated encoder's twin is gated
            twin._fp8_plan = self._fp8_plan      # carried, not applied: the fp32 twin has no fp8 GEMM (its fp8_plan reads 0)
            twin._h = None
            twin.model_identifier = getattr(self, "model_identifier", "<in-memory>")
            twin._create()
            self._range_twin = twin
        return twin

    def close(self):
        twin = getattr(self, "_range_twin", None)
        if twin is not None:
            self._range_twin = None
            twin.close()
        # fused sessions drain through this handle when they are destroyed: close them while it still exists
        for s in list(getattr(self, "_sessions", None) or ()):
            try:
                s.close()
            except Exception:  # noqa: BLE001
                pass
        if getattr(self, "_h", None):
            self._lib.cbas_enc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the reference call: encoder(x) ---------------------------------------------------------
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward(x)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """backend/cbas.py:672-677: x (B,S,H,W) float32 in [0,1] -> (B,S,D) float32."""
        B, S, H, W = x.shape
        self._fit_frame(H, W)
        x = x.to(self.device, dtype=torch.float32).contiguous().reshape(B * S, H, W)
        out = torch.empty((B * S, self.config.hidden_size), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        for i in range(0, B * S, self.max_batch):
            n = min(self.max_batch, B * S - i)
            _lib.check(self._lib.cbas_enc_forward_f32(self._h, x[i:i + n].data_ptr(), n, H, W,
                                                      out[i:i + n].data_ptr(), None, stream),
                       "cbas_enc_forward_f32")
        return out.reshape(B, S, self.config.hidden_size)

    # -- uint8 fast paths -------------------------------------------------------------------------
    def encode_u8(self, frames: torch.Tensor, channel: int = 1, want_f32: bool = True):
        """frames: uint8 device tensor (n,H,W,3) [decord layout; ``channel`` selects green] or (n,H,W).
        Returns (cls_f16 (n,D) torch.float16, cls_f32 (n,D) or None)."""
        assert frames.dtype == torch.uint8 and frames.is_cuda
        frames = frames.contiguous()
        if frames.dim() == 4:
            n, H, W, Cn = frames.shape
            strides = (H * W * Cn, W * Cn, Cn)
            base_off = channel
        else:
            n, H, W = frames.shape
            strides = (H * W, W, 1)
            base_off = 0
        self._fit_frame(H, W)
        D = self.config.hidden_size
        out16 = torch.empty((n, D), dtype=torch.float16, device=self.device)
        out32 = torch.empty((n, D), dtype=torch.float32, device=self.device) if want_f32 else None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        for i in range(0, n, self.max_batch):
            m = min(self.max_batch, n - i)
            _lib.check(self._lib.cbas_enc_forward_u8(
                self._h, frames[i:i + m].data_ptr() + base_off, m, H, W, strides[0], strides[1], strides[2],
                out32[i:i + m].data_ptr() if want_f32 else None, out16[i:i + m].data_ptr(), stream),
                "cbas_enc_forward_u8")
        return out16, out32

    def cls_attention(self, frames: torch.Tensor, channel: int = 1, per_head: bool = False, layer=None):
        """The CLS rows plus the last layer's attention from the CLS token to the patch tokens, averaged over the heads - what
        ``output_attentions=True`` gives the reference's encoder comparison tool - computed on the device from the query and keys
        of the forward itself (cbas_enc_forward_u8_attn / cbas_enc_forward_f32_attn).

        frames: the uint8 device tensors ``encode_u8`` takes ((n,H,W,3) with ``channel`` picking green, or (n,H,W)), or the
        reference-form float32 (B,1,H,W) tensor in [0, 1].  Returns ``(cls_f16, cls_f32, maps)`` with ``maps`` a float32
        (n, nh, nw) device tensor over the patch grid; with ``per_head=True`` a fourth element, the (n, NH, T) softmax rows
        over all T tokens (CLS and registers first).  The CLS rows are bit for bit ``encode_u8``'s.  Every ViT precision is served;
        a precision-2 encoder's map is the map of that MX-fp8 encoder, not of the fp16 one.  ConvNeXt encoders have no attention:
        ``ValueError``.

        ``layer=None`` is the path above, the pruned last layer included.  ``layer=l`` (1 .. L, or negative from the end) gives
        layer l's map (and rows) instead, ``layer="all"`` every layer's: ``maps`` (n, L, nh, nw) and the rows (n, L, NH, T) - one
        unpruned forward (cbas_enc_forward_*_layers) beside the ``encode_u8`` forward that gives the CLS rows their bits.
        Precision 2 is refused there, as for ``hidden_state``; n may not exceed ``max_batch``."""
        if is_convnext(self.config):
            raise ValueError("a ConvNeXt encoder has no attention: CLS attention maps exist for the ViT families only")
        if layer is not None:
            return self._cls_attention_layers(frames, channel, per_head, layer)
        frames, n, H, W, strides, base_off = _frame_args(frames, channel, "cls_attention")
        self._fit_frame(H, W)
        cfg = self.config
        D, NH, ps = cfg.hidden_size, cfg.num_attention_heads, cfg.patch_size
        nh, nw = H // ps, W // ps
        T = cfg.num_tokens(H, W)
        out16 = torch.empty((n, D), dtype=torch.float16, device=self.device)
        out32 = torch.empty((n, D), dtype=torch.float32, device=self.device)
        maps = torch.empty((n, nh, nw), dtype=torch.float32, device=self.device)
        heads = torch.empty((n, NH, T), dtype=torch.float32, device=self.device) if per_head else None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        for i in range(0, n, self.max_batch):
            m = min(self.max_batch, n - i)
            hp = heads[i:i + m].data_ptr() if per_head else None
            if strides is None:
                _lib.check(self._lib.cbas_enc_forward_f32_attn(self._h, frames[i:i + m].data_ptr(), m, H, W, out32[i:i + m].data_ptr(),
                                                               out16[i:i + m].data_ptr(), stream, hp, maps[i:i + m].data_ptr()),
                           "cbas_enc_forward_f32_attn")
            else:
                _lib.check(self._lib.cbas_enc_forward_u8_attn(self._h, frames[i:i + m].data_ptr() + base_off, m, H, W, *strides,
                                                              out32[i:i + m].data_ptr(), out16[i:i + m].data_ptr(), stream, hp,
                                                              maps[i:i + m].data_ptr()), "cbas_enc_forward_u8_attn")
        return (out16, out32, maps, heads) if per_head else (out16, out32, maps)

    # -- per-layer outputs: one cbas_enc_forward_*_layers call ---------------------------------------
    def _layers_refusals(self, what: str) -> None:
        if is_convnext(self.config):
            raise ValueError(f"a ConvNeXt encoder has no transformer layers: {what} exists for the ViT families only "
                             "(its stage outputs are a different object)")
        if self.precision == 2:
            raise ValueError("precision 2 serves CLS rows only: the token rows of its MX-fp8 layers are a different encoder's "
                             "(use precision 0)")

    def _layers_call(self, frames, channel, what, hidden=None, attn=None, rollout=None):
        """hidden = (layers, norm, dtype) -> (len, n, T, D); attn = (layers, per_head) -> maps (len, n, P), heads (len, n, NH, T) or
        None; rollout = (start_layer, query) -> (n, nh, nw) and the scratch.  Returns a dict of what was asked for."""
        self._layers_refusals(what)
        frames, n, H, W, strides, base_off = _frame_args(frames, channel, what)
        if n > self.max_batch:
            raise ValueError(f"{what} is one library call: {n} frames exceed max_batch = {self.max_batch}")
        self._fit_frame(H, W)
        cfg = self.config
        D, NH, ps = cfg.hidden_size, cfg.num_attention_heads, cfg.patch_size
        nh, nw = H // ps, W // ps
        T = cfg.num_tokens(H, W)
        a = _lib.LayersArgs()
        a.struct_bytes = C.sizeof(_lib.LayersArgs)
        out = {"grid": (nh, nw, T - nh * nw)}
        if hidden is not None:
            layers, norm, dtype = hidden
            if dtype not in (torch.float32, torch.float16):
                raise ValueError("hidden states come as torch.float32 or torch.float16")
            idx = (C.c_int32 * len(layers))(*layers)
            hs = torch.empty((len(layers), n, T, D), dtype=dtype, device=self.device)
            a.hidden_layers, a.n_hidden_layers, a.hidden_norm = C.cast(idx, C.c_void_p), len(layers), int(bool(norm))
            a.hidden_f32_dev, a.hidden_f16_dev = (hs.data_ptr(), None) if dtype == torch.float32 else (None, hs.data_ptr())
            a.ld_hidden, a.hidden_layer_stride = D, n * T * D
            out["hidden"] = hs
        if attn is not None:
            layers, per_head = attn
            idx = (C.c_int32 * len(layers))(*layers)
            maps = torch.empty((len(layers), n, nh * nw), dtype=torch.float32, device=self.device)
            heads = torch.empty((len(layers), n, NH, T), dtype=torch.float32, device=self.device) if per_head else None
            a.attn_layers, a.n_attn_layers = C.cast(idx, C.c_void_p), len(layers)
            a.attn_map_dev, a.attn_heads_dev = maps.data_ptr(), heads.data_ptr() if per_head else None
            out["maps"], out["heads"] = maps, heads
        if rollout is not None:
            start, query = rollout
            need = int(self._lib.cbas_enc_layers_scratch_bytes(self._h, n, H, W))
            if need < 0:
                _lib.check(need, "cbas_enc_layers_scratch_bytes")
            scratch = torch.empty((need,), dtype=torch.uint8, device=self.device)
            roll = torch.empty((n, nh, nw), dtype=torch.float32, device=self.device)
            qidx = None
            if query is not None:
                qidx = torch.full((n,), query_token_index(cfg, H, W, query), dtype=torch.int32, device=self.device)
            a.rollout_dev, a.rollout_start_layer = roll.data_ptr(), int(start)
            a.rollout_query_dev = qidx.data_ptr() if qidx is not None else None
            a.scratch_dev, a.scratch_bytes = scratch.data_ptr(), need
            out["rollout"], out["scratch"] = roll, scratch
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if strides is None:
            _lib.check(self._lib.cbas_enc_forward_f32_layers(self._h, frames.data_ptr(), n, H, W, C.byref(a), stream), "cbas_enc_forward_f32_layers")
        else:
            _lib.check(self._lib.cbas_enc_forward_u8_layers(self._h, frames.data_ptr() + base_off, n, H, W, *strides, C.byref(a), stream),
                       "cbas_enc_forward_u8_layers")
        return out

    def hidden_states(self, frames: torch.Tensor, layers=None, norm: bool = False, channel: int = 1,
                      dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """What ``output_hidden_states=True`` returns, as one (len(layers), n, T, D) device tensor in ``dtype`` (float32 or float16):
        index 0 is the embeddings output (prefix rows and patch embeddings, the residual stream before block 0), index l the
        stream after block l - transformers' numbering, 0 .. L.  ``layers=None``: all L + 1; negative indices count from the end.
        ``norm=False``: the raw rows, as transformers returns them; ``norm=True``: each layer's rows through the encoder's final
        LayerNorm (DINO's ``get_intermediate_layers(norm=True)``) - ``hidden_states(frames, layers=[L], norm=True)[0]`` is
        ``hidden_state(frames)`` bit for bit.  Frames and refusals as ``hidden_state``; ConvNeXt encoders are refused (their stage
        outputs are a different object).  One library call: n may not exceed ``max_batch``."""
        self._layers_refusals("hidden_states")
        lay = normalize_layers(layers, self.config.num_hidden_layers)
        return self._layers_call(frames, channel, "hidden_states", hidden=(lay, norm, dtype))["hidden"]

    def _cls_attention_layers(self, frames, channel, per_head, layer):
        self._layers_refusals("per-layer CLS attention")
        L = self.config.num_hidden_layers
        every = isinstance(layer, str) and layer == "all"
        lay = normalize_layers(layer, L, 1, "attention")
        if not every and len(lay) != 1:
            raise ValueError("cls_attention takes one layer, or layer='all'")
        r = self._layers_call(frames, channel, "cls_attention", attn=(lay, per_head))
        nh, nw, _ = r["grid"]
        maps = r["maps"].permute(1, 0, 2).reshape(r["maps"].shape[1], len(lay), nh, nw).contiguous()
        heads = r["heads"].permute(1, 0, 2, 3).contiguous() if per_head else None
        if not every:
            maps, heads = maps[:, 0], heads[:, 0] if per_head else None
        if frames.dtype == torch.uint8:
            out16, out32 = self.encode_u8(frames, channel)
        else:
            out32 = self.forward(frames.reshape(frames.shape[0], 1, *frames.shape[-2:]))[:, 0]
            out16 = out32.to(torch.float16)
        return (out16, out32, maps, heads) if per_head else (out16, out32, maps)

    def attention_rollout(self, frames: torch.Tensor, query=None, start_layer: int = 1, channel: int = 1) -> torch.Tensor:
        """Attention rollout (Abnar and Zuidema) as a float32 (n, nh, nw) device tensor: with A_l the head mean of layer l's softmax
        rows (T x T) and A^_l = 0.5 A_l + 0.5 I, the query's row of A^_L A^_(L-1) ... A^_(start_layer) on the patch columns, no
        renormalisation (every A^_l is row-stochastic).  ``query=None``: the CLS row; ``query=(y, x)`` in pixels: the patch under
        that pixel, as ``similarity_map`` resolves it.  ``start_layer`` 1 .. L (negative from the end).  Computed on the device
        from the queries and keys of the forward itself; served and refused as ``hidden_states``."""
        self._layers_refusals("attention rollout")
        start = normalize_layers(start_layer, self.config.num_hidden_layers, 1, "rollout start")[0]
        return self._layers_call(frames, channel, "attention_rollout", rollout=(start, query))["rollout"]

    def _tokens(self, frames, channel, dtype, query=None, want_map=False):
        """One cbas_enc_forward_*_tokens call: the (n, T, D) image in ``dtype`` and, with ``want_map``, the (n, nh, nw) cosine map."""
        if dtype not in (torch.float32, torch.float16):
            raise ValueError("hidden states come as torch.float32 or torch.float16")
        if not is_convnext(self.config) and self.precision == 2:
            raise ValueError("precision 2 serves CLS rows only: the token rows of its MX-fp8 layers are a different encoder's "
                             "(use precision 0)")
        frames, n, H, W, strides, base_off = _frame_args(frames, channel, "hidden_state")
        self._fit_frame(H, W)
        nh, nw, P0 = token_grid(self.config, H, W)
        D = self.config.hidden_size
        out = torch.empty((n, P0 + nh * nw, D), dtype=dtype, device=self.device)
        p32, p16 = (out.data_ptr(), None) if dtype == torch.float32 else (None, out.data_ptr())
        maps = torch.empty((n, nh, nw), dtype=torch.float32, device=self.device) if want_map else None
        qidx = None
        if want_map and query is not None:
            qidx = torch.full((n,), query_token_index(self.config, H, W, query), dtype=torch.int32, device=self.device)
        tail = (p32, p16, D, qidx.data_ptr() if qidx is not None else None, maps.data_ptr() if want_map else None,
                torch.cuda.current_stream(self.device).cuda_stream)
        if strides is None:
            _lib.check(self._lib.cbas_enc_forward_f32_tokens(self._h, frames.data_ptr(), n, H, W, *tail), "cbas_enc_forward_f32_tokens")
        else:
            _lib.check(self._lib.cbas_enc_forward_u8_tokens(self._h, frames.data_ptr() + base_off, n, H, W, *strides, *tail),
                       "cbas_enc_forward_u8_tokens")
        return out, maps, (nh, nw, P0)

    def hidden_state(self, frames: torch.Tensor, channel: int = 1, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """What ``transformers`` calls the encoder's output: ``last_hidden_state``, the final-LayerNorm'd row of EVERY token, as an
        (n, T, D) device tensor in ``dtype`` (float32 or float16) - cbas_enc_forward_u8_tokens / cbas_enc_forward_f32_tokens.

        frames: as ``cls_attention`` takes them.  ViT: T = CLS + registers + patches in row-major grid order.  ConvNeXt:
        T = 1 + (H // 32) * (W // 32) - the pooled row, then the last stage's grid, as ``DINOv3ConvNextModel`` returns them.  Row 0
        is the CLS row of this encoder with an unpruned last layer.  The call runs the last layer on every row for itself only;
        ``encode_u8`` before and after it gives the same bits.  One library call: n may not exceed ``max_batch``.  Precision 2
        is refused (its MX-fp8 layers serve the CLS row; their token rows are a different encoder's)."""
        return self._tokens(frames, channel, dtype)[0]

    def patch_tokens(self, frames: torch.Tensor, channel: int = 1, dtype: torch.dtype = torch.float32, layer=None,
                     norm: Optional[bool] = None):
        """``hidden_state`` split the way dense-feature users want it: ``(patches, prefix)`` with ``patches`` (n, nh, nw, D) over the
        patch grid and ``prefix`` (n, P0, D) the rows in front of them (CLS and registers; ConvNeXt: the pooled row).  Both are views
        of one tensor.  ``layer=l`` (0 .. L, negative from the end; ViT only): the same split of ``hidden_states(layers=[l], norm=norm)``,
        ``norm`` defaulting to False as there.  Without ``layer`` the rows are ``hidden_state``'s, which are normalised: ``norm=False``
        is refused there rather than ignored (``layer=-1, norm=False`` gives the last layer's raw rows)."""
        if layer is None and norm is not None and not norm:
            raise ValueError("patch_tokens without layer= returns hidden_state's rows, which are normalised; "
                             "pass layer=-1, norm=False for the last layer's raw rows")
        if layer is not None:
            self._layers_refusals("patch_tokens(layer=)")
            lay = normalize_layers(layer, self.config.num_hidden_layers)
            if len(lay) != 1:
                raise ValueError("patch_tokens takes one layer")
            r = self._layers_call(frames, channel, "patch_tokens", hidden=(lay, bool(norm), dtype))
            out, (nh, nw, P0) = r["hidden"][0], r["grid"]
            return out[:, P0:].reshape(out.shape[0], nh, nw, out.shape[2]), out[:, :P0]
        out, _, (nh, nw, P0) = self._tokens(frames, channel, dtype)
        return out[:, P0:].reshape(out.shape[0], nh, nw, out.shape[2]), out[:, :P0]

    def similarity_map(self, frames: torch.Tensor, query=None, channel: int = 1) -> torch.Tensor:
        """Cosine similarity of one token's final hidden state to every patch token's, as a float32 (n, nh, nw) device tensor: the
        picture of what an encoder looks at that ConvNeXt encoders can give too.  ``query=None``: the CLS row (ConvNeXt: the
        pooled row); ``query=(y, x)`` in pixels: the patch under that pixel.  Computed on the device from the fp32 rows."""
        return self._tokens(frames, channel, torch.float32, query, True)[1]

    @property
    def stamp(self) -> str:
        """The encoder stamp of this encoder's files (``encode_files.run_stamp``: the model identifier, tagged for MX-fp8 rows) with
        the precision: what a ``PatchPCABasis`` remembers of the encoder it was fitted on.  It names the checkpoint, as the files'
        stamp does, not the weights: every encoder built by ``from_weights`` is ``<in-memory>@pN``, so two different in-memory
        encoders of one width and precision cannot be told apart by it."""
        from .encode_files import run_stamp
        return f"{run_stamp(getattr(self, 'model_identifier', '<in-memory>'), self.precision, self.fp8_plan or None)}@p{self.precision}"

    def patch_pca(self, frames: torch.Tensor, n_components: int = 3, scope: str = "frame", basis: Optional[PatchPCABasis] = None,
                  iters: Optional[int] = None, channel: int = 1):
        """PCA of the patch rows of ``hidden_state(frames)``, fitted and projected on the device (cbas_patch_pca_fit /
        cbas_patch_pca_project): the picture of what the encoder separates, and the one every family has.

        Returns ``(scores, basis)``: ``scores`` float32 (n, nh, nw, n_components) on the device, the centred patch rows' coordinates
        along the leading principal components; ``basis`` a ``PatchPCABasis``.  ``scope="frame"`` fits one basis per frame (a
        frame's result does not depend on its batch), ``scope="batch"`` one for all frames.  With ``basis=`` given nothing is
        fitted: the rows are projected on it (one basis for every frame, or one per frame) - a basis fitted on one batch colours a
        whole clip consistently; its ``n_components`` and ``scope`` are the ones used.  A basis of another width or encoder is refused.
        ``iters``: rounds of subspace iteration (default ``PCA_DEFAULT_ITERS``).  Frames, families and precisions: as
        ``hidden_state``; ``encode_u8`` before and after gives the same bits.

        The two entry points read rows, mean and components as 16-byte vectors and have no scalar fallback: pointers must be
        16-byte aligned and the row stride a multiple of 4 floats, or the call is refused (CBAS_EINVAL).  This method always
        meets that - it allocates the rows itself and copies a given basis into contiguous tensors - but a caller of
        ``cbas_patch_pca_fit`` / ``cbas_patch_pca_project`` with rows in a view at an odd offset must copy them first."""
        if basis is None and scope not in ("frame", "batch"):
            raise ValueError(f"scope {scope!r}: 'frame' or 'batch'")
        D = self.config.hidden_size
        if basis is not None:
            basis.check(D, self.stamp)
        tokens, _, (nh, nw, P0) = self._tokens(frames, channel, torch.float32)
        n, T, _ = tokens.shape
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if basis is None:
            k = int(n_components)
            sc = _lib.PCA_BATCH if scope == "batch" else _lib.PCA_FRAME
            nb = 1 if scope == "batch" else n
            ws, need = _lib.workspace("cbas_patch_pca_workspace_bytes", self.device, n, T, P0, D, k, sc)
            f32 = dict(dtype=torch.float32, device=self.device)
            basis = PatchPCABasis(torch.empty((nb, D), **f32), torch.empty((nb, k, D), **f32), torch.empty((nb, k), **f32),
                                  torch.empty((nb,), **f32), scope, self.stamp)
            _lib.check(self._lib.cbas_patch_pca_fit(tokens.data_ptr(), n, T, P0, D, D, k, sc, int(PCA_DEFAULT_ITERS if iters is None else iters),
                                                    basis.mean.data_ptr(), basis.components.data_ptr(), basis.eigenvalues.data_ptr(),
                                                    basis.total_variance.data_ptr(), ws.data_ptr(), need, stream), "cbas_patch_pca_fit")
        elif basis.n_bases not in (1, n):
            raise ValueError(f"a basis of {basis.n_bases} frames cannot colour {n} frames (one basis, or one per frame)")
        k = basis.n_components
        mean, comp = (t.to(self.device, torch.float32).contiguous() for t in (basis.mean, basis.components))
        scores = torch.empty((n, nh, nw, k), dtype=torch.float32, device=self.device)
        _lib.check(self._lib.cbas_patch_pca_project(tokens.data_ptr(), n, T, P0, D, D, k, basis.n_bases, mean.data_ptr(), comp.data_ptr(),
                                                    scores.data_ptr(), stream), "cbas_patch_pca_project")
        return scores, basis

    def patch_clusters(self, frames: torch.Tensor, n_clusters: int = 4, scope: str = "frame", clusters: Optional[PatchClusters] = None,
                       iters: Optional[int] = None, normalize: bool = True, channel: int = 1):
        """k-means of the patch rows of ``hidden_state(frames)``, fitted and assigned on the device (cbas_patch_kmeans_fit /
        cbas_patch_kmeans_assign): a cluster label per patch - which patches belong together.

        Returns ``(labels, clusters)``: ``labels`` int32 (n, nh, nw) on the device, cluster 0 the largest; ``clusters`` a
        ``PatchClusters``.  ``scope="frame"`` fits one set per frame (a frame's result does not depend on its batch),
        ``scope="batch"`` one for all frames.  With ``clusters=`` given nothing is fitted and the rows are only assigned (one set for
        every frame, or one per frame): a set fitted on one batch labels a whole clip consistently; its ``n_clusters``, ``scope`` and
        ``normalize`` are the ones used.  A set of another width or encoder is refused.  ``iters``: Lloyd rounds, exactly that many
        (default ``KMEANS_DEFAULT_ITERS``); ``normalize``: compare rows scaled to unit length (cosine geometry, the usual choice
        for DINO features).  The start is deterministic farthest-point seeding, so two calls give the same bits.  Frames,
        families and precisions: as ``hidden_state``; ``encode_u8`` before and after gives the same bits."""
        if clusters is None and scope not in ("frame", "batch"):
            raise ValueError(f"scope {scope!r}: 'frame' or 'batch'")
        D = self.config.hidden_size
        if clusters is not None:
            clusters.check(D, self.stamp)
        tokens, _, (nh, nw, P0) = self._tokens(frames, channel, torch.float32)
        n, T, _ = tokens.shape
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if clusters is None:
            k, rounds = int(n_clusters), int(KMEANS_DEFAULT_ITERS if iters is None else iters)
            sc = _lib.PCA_BATCH if scope == "batch" else _lib.PCA_FRAME
            nb = 1 if scope == "batch" else n
            need = _lib.workspace_bytes("cbas_patch_kmeans_workspace_bytes", n, T, P0, D, k, sc)      # a refused shape first
            if rounds < 0:
                raise ValueError(f"iters = {rounds}: at least 0")
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            i32 = dict(dtype=torch.int32, device=self.device)
            clusters = PatchClusters(torch.empty((nb, k, D), dtype=torch.float32, device=self.device), torch.empty((nb, k), **i32),
                                     torch.empty((nb, rounds + 1), dtype=torch.float32, device=self.device), torch.empty((nb, k), **i32),
                                     scope, normalize, self.stamp)
            _lib.check(self._lib.cbas_patch_kmeans_fit(tokens.data_ptr(), n, T, P0, D, D, k, sc, rounds, int(bool(normalize)),
                                                       clusters.centroids.data_ptr(), clusters.counts.data_ptr(), clusters.inertia.data_ptr(),
                                                       clusters.init_index.data_ptr(), ws.data_ptr(), need, stream), "cbas_patch_kmeans_fit")
        elif clusters.n_sets not in (1, n):
            raise ValueError(f"a cluster set of {clusters.n_sets} frames cannot label {n} frames (one set, or one per frame)")
        cent = clusters.centroids.to(self.device, torch.float32).contiguous()
        labels = torch.empty((n, nh, nw), dtype=torch.int32, device=self.device)
        _lib.check(self._lib.cbas_patch_kmeans_assign(tokens.data_ptr(), n, T, P0, D, D, clusters.n_clusters, clusters.n_sets,
                                                      int(clusters.normalize), cent.data_ptr(), labels.data_ptr(), None, stream),
                   "cbas_patch_kmeans_assign")
        return labels, clusters

    def submit_host(self, slot: int, frames: np.ndarray, channel: int = 1) -> None:
        """Queue one host chunk (uint8 (n,H,W,3) or (n,H,W), C-contiguous) on ``slot``."""
        assert frames.dtype == np.uint8 and frames.flags.c_contiguous
        if frames.ndim == 4:
            n, H, W, Cn = frames.shape
            strides, off = (H * W * Cn, W * Cn, Cn), channel
        else:
            n, H, W = frames.shape
            strides, off = (H * W, W, 1), 0
        self._fit_frame(H, W)
        _lib.check(self._lib.cbas_enc_submit_u8_host(self._h, slot, frames.ctypes.data + off, n, H, W, *strides),
                   "cbas_enc_submit_u8_host")
        self._slot_n = getattr(self, "_slot_n", {})
        self._slot_n[slot] = n

    def submit_dev(self, slot: int, frames: torch.Tensor, out16: Optional[torch.Tensor], out32: Optional[torch.Tensor] = None,
                   channel: int = 1) -> None:
        """Asynchronous encode of one device batch (<= max_batch frames, uint8 (n,H,W,3) or (n,H,W)) into the
        given output rows, on one of the handle's two compute lanes, ordered after the current torch stream.
        Call ``wait_stream(slot)`` before anything reads the outputs or overwrites the frames."""
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.is_contiguous()
        if frames.dim() == 4:
            n, H, W, Cn = frames.shape
            strides, off = (H * W * Cn, W * Cn, Cn), channel
        else:
            n, H, W = frames.shape
            strides, off = (H * W, W, 1), 0
        if H > self.max_frame[0] or W > self.max_frame[1]:
            raise RuntimeError(f"frames of {H}x{W} exceed the encoder workspace {self.max_frame}; create the encoder with "
                               "max_frame=(H, W) (the asynchronous form cannot rebuild the handle with batches in flight)")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.cbas_enc_submit_u8(self._h, slot, frames.data_ptr() + off, n, H, W, *strides,
                                                out32.data_ptr() if out32 is not None else None,
                                                out16.data_ptr() if out16 is not None else None, stream),
                   "cbas_enc_submit_u8")

    def set_lanes(self, n: int) -> None:
        """1 or 2 compute lanes for the asynchronous forms (default 2: two batches in flight)."""
        _lib.check(self._lib.cbas_enc_set_lanes(self._h, int(n)), "cbas_enc_set_lanes")

    def set_prune_last_layer(self, enable: bool) -> None:
        """Default on: the last layer computes q/attention/MLP for the CLS rows only (bit-identical CLS)."""
        _lib.check(self._lib.cbas_enc_set_prune_last_layer(self._h, int(bool(enable))), "cbas_enc_set_prune_last_layer")

    def debug_option(self, name: str, value: int) -> None:
        """Bring-up / tests: switch an implementation detail whose settings are bit-identical (cbas_enc_debug_option;
        debug build of the library only)."""
        _lib.require_debug("cbas_enc_debug_option")
        _lib.check(self._lib.cbas_enc_debug_option(self._h, name.encode(), int(value)), "cbas_enc_debug_option")

    def wait_stream(self, slot: int) -> None:
        """The current torch stream waits for ``slot``'s batch (no host synchronisation); frees the slot."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.cbas_enc_wait_stream(self._h, slot, stream), "cbas_enc_wait_stream")

    def wait(self, slot: int, want_f32: bool = False):
        n = getattr(self, "_slot_n", {}).pop(slot, None)
        if n is None:
            raise RuntimeError(f"cbas_enc_wait: slot {slot} has no submitted work")
        D = self.config.hidden_size
        o16 = np.empty((n, D), np.float16)
        o32 = np.empty((n, D), np.float32) if want_f32 else None
        _lib.check(self._lib.cbas_enc_wait(self._h, slot, o16.ctypes.data, o32.ctypes.data if want_f32 else None),
                   "cbas_enc_wait")
        return o16, o32

    def check_finite(self) -> None:
        """Raise if a batch completed since the last check produced a NaN / infinite CLS row (an activation left the range of
        the arithmetic mode: cbas_enc_check_finite).  ``wait`` and the fused session's waits check by themselves; callers of the
        stream-ordered forms (``encode_u8``, ``submit`` + ``wait_stream``) call this after synchronising."""
        _lib.check(self._lib.cbas_enc_check_finite(self._h), "cbas_enc_check_finite")

    # -- per-kernel timing (HIP events inside the library) ------------------------------------------
    def profile(self, enable: bool) -> None:
        _lib.check(self._lib.cbas_enc_profile(self._h, int(bool(enable))), "cbas_enc_profile")

    def profile_read(self, reset: bool = True) -> Dict[str, Dict[str, float]]:
        n = len(_lib.PROF_CATS)
        ms = (C.c_double * n)()
        cnt = (C.c_int64 * n)()
        fl = (C.c_double * n)()
        _lib.check(self._lib.cbas_enc_profile_read(self._h, ms, cnt, fl, int(reset)), "cbas_enc_profile_read")
        return {name: {"ms": ms[i], "launches": int(cnt[i]), "flops": fl[i]}
                for i, name in enumerate(_lib.PROF_CATS) if cnt[i] > 0}

    # -- bring-up taps -----------------------------------------------------------------------------
    def debug_tap(self, frames: torch.Tensor, stop_layer: int, stop_stage: int, which: int, channel: int = 1):
        _lib.require_debug("cbas_enc_debug_forward_u8")
        n, H, W = frames.shape[:3]
        if frames.dim() == 4:
            Cn = frames.shape[3]
            strides, off = (H * W * Cn, W * Cn, Cn), channel
        else:
            strides, off = (H * W, W, 1), 0
        torch.cuda.synchronize(self.device)
        _lib.check(self._lib.cbas_enc_debug_forward_u8(self._h, frames.data_ptr() + off, n, H, W, *strides,
                                                       stop_layer, stop_stage), "cbas_enc_debug_forward_u8")
        if is_convnext(self.config):
            # stop_layer 0: the stem after its LayerNorm, 1 + i: stage i; which = 4 + stop_layer (cbas_mi355x_debug.h)
            (h, w), Cw = self.config.stage_grids(H, W)[max(0, stop_layer - 1)], self.config.hidden_sizes[max(0, stop_layer - 1)]
            out = np.empty((n * h * w, Cw), np.float32)
            _lib.check(self._lib.cbas_enc_debug_read(self._h, which, out.ctypes.data, out.nbytes), "cbas_enc_debug_read")
            return out
        T = self.config.num_tokens(H, W)
        D, F = self.config.hidden_size, self.config.intermediate_size
        if self.precision == 4 and which in (1, 3):
            raise RuntimeError("precision 4 keeps the LayerNorm / GELU buffers in the GEMM's split hi|lo tile order; tap precision 3")
        act = np.float32 if self.precision >= 3 else np.float16        # precision 3 / 4 keep every activation buffer fp32
        shape, dt = {0: ((n * T, D), np.float32), 1: ((n * T, D), act), 2: ((n * T, 3 * D), act),
                     3: ((n * T, F), act)}[which]
        out = np.empty(shape, dt)
        _lib.check(self._lib.cbas_enc_debug_read(self._h, which, out.ctypes.data, out.nbytes), "cbas_enc_debug_read")
        return out
