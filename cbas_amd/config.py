"""Configuration records for the encoders (DINOv3 ViT, DINOv2 with and without registers, DINOv3 ConvNeXt) and the classifier head.

The field names follow the HF ``config.json`` of a DINOv3 ViT checkpoint
(``transformers/models/dinov3_vit/configuration_dinov3_vit.py:74-101``) so that a
checkpoint directory can be read without importing ``transformers``; the head fields
follow the constructor of ``ClassifierLSTMDeltas`` (reference
``backend/classifier_head.py:62-64``).
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, asdict, replace
from typing import Tuple


# the two HF DINOv2 model types: same blocks, same state-dict keys (minus the register tokens of the plain one)
DINOV2_FAMILIES = ("dinov2_with_registers", "dinov2")


@dataclass(frozen=True)
class ViTConfig:
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    num_register_tokens: int = 4
    patch_size: int = 16
    image_size: int = 224
    layer_norm_eps: float = 1e-5
    rope_theta: float = 100.0
    query_bias: bool = True
    key_bias: bool = False
    value_bias: bool = True
    proj_bias: bool = True
    mlp_bias: bool = True
    use_gated_mlp: bool = False
    hidden_act: str = "gelu"
    num_channels: int = 3
    # encoder family: "dinov3_vit" (RoPE, no additive position embedding) or "dinov2_with_registers"
    # (learned position embedding on a pos_embed_grid x pos_embed_grid lattice, bicubically
    # interpolated to the frame's patch grid; no RoPE; key bias) - CBAS's default project encoder
    # (reference backend/cbas.py:1030-1033) - or "dinov2" (the same without register tokens, and with the
    # position embedding interpolated WITHOUT antialiasing: HF modeling_dinov2.py:86-91)
    model_type: str = "dinov3_vit"
    use_rope: bool = True
    pos_embed_grid: int = 0

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads

    @property
    def num_prefix_tokens(self) -> int:
        return 1 + self.num_register_tokens

    def num_patches(self, height: int, width: int) -> int:
        return (height // self.patch_size) * (width // self.patch_size)

    def num_tokens(self, height: int, width: int) -> int:
        return self.num_prefix_tokens + self.num_patches(height, width)

    def flops_per_frame(self, height: int, width: int) -> float:
        """Algorithmic FLOPs (MAC = 2) per frame: SURVEY.md §8(a) 'Encoder totals'."""
        D, F, L = self.hidden_size, self.intermediate_size, self.num_hidden_layers
        P, T = self.num_patches(height, width), self.num_tokens(height, width)
        patch = P * self.num_channels * self.patch_size ** 2 * D
        mlp = (3 if self.use_gated_mlp else 2) * T * D * F       # gated: gate_proj, up_proj and down_proj
        per_layer = 4 * T * D * D + mlp + 2 * T * T * D
        return 2.0 * (patch + L * per_layer)

    def validate(self) -> None:
        if self.use_gated_mlp:
            # DINOv3ViTGatedMLP ([tf] modeling_dinov3_vit.py:360-373): down_proj(silu(gate_proj(x)) * up_proj(x)) - ViT-S+ / H+
            if self.model_type in DINOV2_FAMILIES:
                raise NotImplementedError("DINOv2 SwiGLU checkpoints (use_swiglu_ffn) are not built: HF's Dinov2SwiGLUFFN keeps gate "
                                          "and up in one weights_in tensor (another weight layout) and its hidden width "
                                          "(int(4 D * 2 / 3) rounded up to 8) is not a multiple of 128 at any supported width")
            if self.hidden_act != "silu":
                raise NotImplementedError(f"gated MLP with hidden_act={self.hidden_act!r}; the gated (SwiGLU) MLP of DINOv3 "
                                          "ViT-S+ / H+ is built with 'silu' only")
        elif self.hidden_act != "gelu":
            raise NotImplementedError(f"hidden_act={self.hidden_act!r}; only exact-erf 'gelu' is implemented")
        if self.head_dim != 64:
            raise NotImplementedError("head_dim must be 64 (all DINOv3 ViT-S/B/L checkpoints)")
        if self.patch_size not in (14, 16):
            raise NotImplementedError("patch_size must be 14 (DINOv2) or 16 (DINOv3)")
        if self.model_type not in ("dinov3_vit",) + DINOV2_FAMILIES:
            raise NotImplementedError(f"model_type={self.model_type!r} is not built")
        if self.model_type == "dinov2" and self.num_register_tokens != 0:
            raise NotImplementedError("model_type='dinov2' has no register tokens (that is 'dinov2_with_registers')")
        if self.use_rope == (self.pos_embed_grid > 0):
            raise NotImplementedError("exactly one of RoPE / learned position embedding is expected")
        if not (self.query_bias and self.value_bias and self.proj_bias and self.mlp_bias):
            raise NotImplementedError("query/value/proj/mlp biases are expected (DINOv3 defaults)")

    def to_json(self) -> str:
        d = asdict(self)
        if self.model_type in DINOV2_FAMILIES:               # write the fields HF's config class reads back
            d.update(mlp_ratio=self.intermediate_size // self.hidden_size, qkv_bias=self.query_bias,
                     use_swiglu_ffn=self.use_gated_mlp)
        return json.dumps(d, indent=2)

    @classmethod
    def from_json_file(cls, path: str) -> "ViTConfig":
        with open(path, "r") as f:
            raw = json.load(f)
        mt = raw.get("model_type", "dinov3_vit")
        if mt not in ("dinov3_vit",) + DINOV2_FAMILIES:
            raise NotImplementedError(f"model_type={mt!r}: only DINOv3 ViT and DINOv2 (with or without registers) encoders are built")
        known = {k: raw[k] for k in cls.__dataclass_fields__ if k in raw}
        for key in ("patch_size", "image_size"):
            if isinstance(known.get(key), (list, tuple)):
                known[key] = int(known[key][0])
        if mt in DINOV2_FAMILIES:
            # HF Dinov2WithRegistersConfig (configuration_dinov2_with_registers.py) and Dinov2Config (configuration_dinov2.py):
            # mlp_ratio, qkv_bias, use_swiglu_ffn; plain DINOv2 has no register tokens
            hs = int(raw.get("hidden_size", 768))
            qkv_bias = bool(raw.get("qkv_bias", True))
            known.update(intermediate_size=hs * int(raw.get("mlp_ratio", 4)), query_bias=qkv_bias, key_bias=qkv_bias,
                         value_bias=qkv_bias, use_gated_mlp=bool(raw.get("use_swiglu_ffn", False)), use_rope=False,
                         layer_norm_eps=float(raw.get("layer_norm_eps", 1e-6)),
                         num_register_tokens=int(raw.get("num_register_tokens", 4)) if mt == "dinov2_with_registers" else 0,
                         patch_size=int(known.get("patch_size", 16)), image_size=int(known.get("image_size", 224)))
            known["pos_embed_grid"] = known["image_size"] // known["patch_size"]
        return cls(**known)


VIT_S16 = ViTConfig(hidden_size=384, intermediate_size=1536, num_hidden_layers=12, num_attention_heads=6)
VIT_B16 = ViTConfig(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12)
VIT_L16 = ViTConfig(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16)
# The gated-MLP family (use_gated_mlp, hidden_act "silu"; shapes from the public model cards of
# facebook/dinov3-vits16plus-pretrain-lvd1689m and facebook/dinov3-vith16plus-pretrain-lvd1689m)
VIT_S16PLUS = ViTConfig(hidden_size=384, intermediate_size=1536, num_hidden_layers=12, num_attention_heads=6,
                        use_gated_mlp=True, hidden_act="silu")
VIT_H16PLUS = ViTConfig(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20,
                        use_gated_mlp=True, hidden_act="silu")
# Tiny gated config (not a published architecture): F = 384 makes the fused gate | up GEMM N = 768 - three 256-column tiles -
# and gives the down projection K = 384
VIT_TINY_GATED = ViTConfig(hidden_size=128, intermediate_size=384, num_hidden_layers=2, num_attention_heads=2,
                           image_size=64, use_gated_mlp=True, hidden_act="silu")
# Tiny config for fast oracle/kernel parity (not a published architecture).
VIT_TINY = ViTConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                     image_size=64)

# DINOv2-with-registers (CBAS's default encoder, "facebook/dinov2-with-registers-base"): ViT-B/14 trained at 518
DINOV2_REG_B14 = ViTConfig(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                           patch_size=14, image_size=518, layer_norm_eps=1e-6, key_bias=True,
                           model_type="dinov2_with_registers", use_rope=False, pos_embed_grid=37)
DINOV2_REG_TINY = ViTConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                            patch_size=14, image_size=70, layer_norm_eps=1e-6, key_bias=True,
                            model_type="dinov2_with_registers", use_rope=False, pos_embed_grid=5)
# Plain DINOv2 ("facebook/dinov2-base", the third encoder the reference's cbas_config.yaml.example names): the R = 0 twins
DINOV2_B14 = replace(DINOV2_REG_B14, model_type="dinov2", num_register_tokens=0)
DINOV2_TINY = replace(DINOV2_REG_TINY, model_type="dinov2", num_register_tokens=0)

NAMED_VIT = {"vits16": VIT_S16, "vitb16": VIT_B16, "vitl16": VIT_L16, "tiny": VIT_TINY,
             "vits16plus": VIT_S16PLUS, "vith16plus": VIT_H16PLUS, "tiny_gated": VIT_TINY_GATED,
             "dinov2regb14": DINOV2_REG_B14, "dinov2regtiny": DINOV2_REG_TINY,
             "dinov2b14": DINOV2_B14, "dinov2tiny": DINOV2_TINY}


@dataclass(frozen=True)
class ConvNextConfig:
    """HF ``DINOv3ConvNextConfig`` (transformers models/dinov3_convnext/configuration_dinov3_convnext.py): the four-stage
    DINOv3 ConvNeXt whose ``DINOv3ConvNextModel`` puts LayerNorm(global mean pool of the last stage) at row 0 of
    ``last_hidden_state`` - the row the reference keeps (backend/cbas.py:677).  Defaults are ConvNeXt-T."""
    hidden_sizes: Tuple[int, ...] = (96, 192, 384, 768)
    depths: Tuple[int, ...] = (3, 3, 9, 3)
    layer_norm_eps: float = 1e-6
    layer_scale_init_value: float = 1e-6
    drop_path_rate: float = 0.0
    hidden_act: str = "gelu"
    num_channels: int = 3
    image_size: int = 224
    model_type: str = "dinov3_convnext"

    @property
    def hidden_size(self) -> int:
        """Width of the row the encoder emits (the last stage's)."""
        return int(self.hidden_sizes[-1])

    def stage_grids(self, height: int, width: int):
        """(h, w) of the four stages: the 4x4 / stride-4 stem, then three 2x2 / stride-2 downsamples (floor, as PyTorch)."""
        h, w, out = height // 4, width // 4, []
        for i in range(4):
            if i:
                h, w = h // 2, w // 2
            out.append((h, w))
        return out

    def flops_per_frame(self, height: int, width: int) -> float:
        """Algorithmic FLOPs (MAC = 2): stem + downsamples + sum of depth * HW * (49 C + 8 C^2)."""
        mac, prev = 0, self.num_channels
        for i, ((h, w), C, d) in enumerate(zip(self.stage_grids(height, width), self.hidden_sizes, self.depths)):
            mac += h * w * C * prev * (16 if i == 0 else 4)
            mac += d * h * w * (49 * C + 8 * C * C)
            prev = C
        return 2.0 * mac

    def validate(self) -> None:
        if self.model_type != "dinov3_convnext":
            raise NotImplementedError(f"model_type={self.model_type!r} is not a DINOv3 ConvNeXt")
        if len(self.hidden_sizes) != 4 or len(self.depths) != 4:
            raise NotImplementedError("a DINOv3 ConvNeXt with 4 stages is expected")
        if any(c <= 0 or c % 32 or c > 1536 for c in self.hidden_sizes):
            raise NotImplementedError(f"hidden_sizes={tuple(self.hidden_sizes)}: every width must be a multiple of 32 (<= 1536)")
        if any(d < 1 or d > 64 for d in self.depths):
            raise NotImplementedError(f"depths={tuple(self.depths)} outside [1, 64]")
        if self.hidden_act != "gelu":
            raise NotImplementedError(f"hidden_act={self.hidden_act!r}; only exact-erf 'gelu' is implemented")
        if self.num_channels != 3:
            raise NotImplementedError("num_channels must be 3 (the reference replicates the green plane 3 times)")

    def to_json(self) -> str:
        d = asdict(self)
        d.update(hidden_sizes=list(self.hidden_sizes), depths=list(self.depths), num_stages=4)
        return json.dumps(d, indent=2)

    @classmethod
    def from_json_file(cls, path: str) -> "ConvNextConfig":
        with open(path, "r") as f:
            raw = json.load(f)
        mt = raw.get("model_type")
        if mt != "dinov3_convnext":
            raise NotImplementedError(f"model_type={mt!r} is not a DINOv3 ConvNeXt")
        known = {k: raw[k] for k in cls.__dataclass_fields__ if k in raw}
        for key in ("hidden_sizes", "depths"):
            if key in known:
                known[key] = tuple(int(v) for v in known[key])
        if isinstance(known.get("image_size"), (list, tuple)):
            known["image_size"] = int(known["image_size"][0])
        return cls(**known)


CONVNEXT_T = ConvNextConfig()
CONVNEXT_S = ConvNextConfig(depths=(3, 3, 27, 3))
# Tiny config for fast kernel parity (not a published architecture)
CONVNEXT_TINY = ConvNextConfig(hidden_sizes=(32, 64, 128, 256), depths=(1, 1, 2, 1), image_size=64)

NAMED_CONVNEXT = {"convnext_t": CONVNEXT_T, "convnext_s": CONVNEXT_S, "convnext_tiny": CONVNEXT_TINY}


def encoder_config_from_json(path: str):
    """The encoder config of a checkpoint's ``config.json``, by its ``model_type``: ``ConvNextConfig`` for
    ``dinov3_convnext``, else ``ViTConfig`` (which refuses the families that are not built)."""
    with open(path, "r") as f:
        mt = json.load(f).get("model_type", "dinov3_vit")
    if mt == "dinov3_convnext":
        return ConvNextConfig.from_json_file(path)
    return ViTConfig.from_json_file(path)


def is_convnext(cfg) -> bool:
    return isinstance(cfg, ConvNextConfig)


@dataclass(frozen=True)
class HeadConfig:
    """``ClassifierLSTMDeltas(in_features, out_features, seq_len, ...)``: classifier_head.py:62-64."""
    in_features: int = 768
    out_features: int = 9
    seq_len: int = 31
    bottleneck_dim: int = 128
    use_acceleration: bool = True
    ema_alpha: float = 0.3
    center_window_size: int = 5
    lstm_hidden_size: int = 64
    lstm_layers: int = 1
    lin0_dim: int = 256

    @property
    def hsl(self) -> int:
        return self.seq_len // 2

    @property
    def centre_lo(self) -> int:
        return max(0, self.hsl - self.center_window_size)

    @property
    def centre_hi(self) -> int:
        return min(self.seq_len, self.hsl + self.center_window_size + 1)

    def flops_per_frame_naive(self) -> float:
        """Naive (per-window) head FLOPs, SURVEY.md §8(a) 'Head totals' definition."""
        T, I, Bn, C, h = self.seq_len, self.in_features, self.bottleneck_dim, self.out_features, self.lstm_hidden_size
        n_streams = 3 if self.use_acceleration else 2
        mac = T * I * Bn * n_streams                        # bottlenecks
        mac += T * Bn * n_streams * self.lin0_dim           # lin0
        mac += 2 * T * (self.lin0_dim * 4 * h + h * 4 * h)  # BiLSTM
        mac += (self.centre_hi - self.centre_lo) * I * C    # lin1 on the centre window
        mac += 2 * h * C + (self.centre_hi - self.centre_lo) * 2 * h
        return 2.0 * mac

    def validate(self) -> None:
        if not 1 <= self.lstm_layers <= 4:
            raise NotImplementedError("lstm_layers must be in [1, 4]")
        if self.lstm_hidden_size < 16 or self.lstm_hidden_size > 128 or self.lstm_hidden_size % 16:
            raise NotImplementedError("lstm_hidden_size must be a multiple of 16 in [16, 128]")
        if self.seq_len < 3:
            raise NotImplementedError("seq_len < 3 (replicate-pad delta mode) is not implemented")
        if self.centre_lo >= self.centre_hi:
            raise NotImplementedError("empty centre window")


def find_checkpoint_dir(model_identifier: str) -> str:
    """Resolve ``model_identifier`` the way ``AutoModel.from_pretrained`` would *offline*.

    A local directory is used as is; a hub name is looked up in the HF cache
    (``$HF_HOME/hub/models--org--name/snapshots/<rev>/``).  No network access is attempted.
    Mirrors the reference call at backend/cbas.py:657.
    """
    if os.path.isdir(model_identifier):
        return model_identifier
    hf_home = os.environ.get("HF_HOME", os.path.join(os.path.expanduser("~"), ".cache", "huggingface"))
    hub = os.environ.get("HF_HUB_CACHE", os.path.join(hf_home, "hub"))
    snap = os.path.join(hub, "models--" + model_identifier.replace("/", "--"), "snapshots")
    if os.path.isdir(snap):
        revs = sorted(os.listdir(snap))
        for rev in reversed(revs):
            cand = os.path.join(snap, rev)
            if os.path.exists(os.path.join(cand, "config.json")):
                return cand
    raise FileNotFoundError(
        f"encoder checkpoint {model_identifier!r} is neither a local directory nor present in the "
        f"Hugging Face cache ({snap}); this build never downloads")


# ---- MX-fp8 plans (precision 2): which projection GEMMs of a layer take MX-fp8 operands -------------------------------------
# bits of include/cbas_mi355x.h CBAS_FP8_PLAN_*; the activations follow their consumers (cbas_enc_set_fp8_plan)
FP8_PLAN_BITS = {"qkv": 1, "proj": 2, "up": 4, "down": 8}
FP8_PLANS = {"all": 15, "mlp": 12, "mlp_qkv": 13, "up": 4, "down": 8}
FP8_PLAN_DEFAULT = FP8_PLANS["all"]             # every release's precision 2


def parse_fp8_plan(plan) -> int:
    """A plan name (FP8_PLANS), a '+'-joined list of GEMM names ('qkv+up') or a mask 0..15 (int or decimal string) -> the mask.
    None is the default plan.  Anything else is a ValueError naming what is accepted."""
    if plan is None:
        return FP8_PLAN_DEFAULT
    if isinstance(plan, bool):
        raise ValueError(f"fp8 plan {plan!r}: a name ({', '.join(FP8_PLANS)}), GEMM names joined by '+' or a mask 0..15")
    if isinstance(plan, int):
        mask = plan
    else:
        text = str(plan).strip().lower()
        if text in FP8_PLANS:
            return FP8_PLANS[text]
        if text.isdigit():
            mask = int(text)
        elif text and all(t in FP8_PLAN_BITS for t in text.split("+")):
            mask = 0
            for t in text.split("+"):
                mask |= FP8_PLAN_BITS[t]
        else:
            raise ValueError(f"fp8 plan {plan!r}: a name ({', '.join(FP8_PLANS)}), GEMM names ({', '.join(FP8_PLAN_BITS)}) joined "
                             "by '+' or a mask 0..15")
    if not 0 <= mask <= 15:
        raise ValueError(f"fp8 plan mask {mask}: 0..15 (1 qkv, 2 proj, 4 up, 8 down)")
    return mask


def fp8_plan_name(mask: int) -> str:
    """The name a plan is written under (file stamps, study records): its FP8_PLANS name, else 'p<mask>'."""
    mask = parse_fp8_plan(mask)
    for name, m in FP8_PLANS.items():
        if m == mask:
            return name
    return f"p{mask}"
