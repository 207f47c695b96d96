"""Float64 restatement of the gated-MLP DINOv3 layer (test infrastructure): transformers' DINOv3ViTGatedMLP,
``down_proj(silu(gate_proj(x)) * up_proj(x))`` (modeling_dinov3_vit.py:360-373), inside the layer of :419-445.  Everything that is
not the MLP - embeddings, RoPE tables, LayerNorm, attention - is oracle/vit_oracle.py's, imported; only the gated MLP is written
here, in float64, independently of the library and of its blob order (it reads the tensors by their checkpoint names).

Pinned by tests/test_gated_mlp_host.py against tests/golden/gated_tiny.npz (transformers' own rows)."""
from typing import Dict, Optional

import numpy as np

from oracle import vit_oracle as V

F64 = np.float64


def silu(g: np.ndarray) -> np.ndarray:
    """x * sigmoid(x) without overflow for g -> -large: exp(-|g|) only."""
    g = g.astype(F64)
    e = np.exp(-np.abs(g))
    return np.where(g >= 0, g / (1.0 + e), g * e / (1.0 + e))


def gated_mlp(h: np.ndarray, w: Dict[str, np.ndarray], pre: str, taps: Optional[dict] = None, tag: str = "") -> np.ndarray:
    """(.., D) -> (.., D) float64; taps[tag + 'act'] = silu(gate) * up, the tensor the fused GEMM stores."""
    h = h.astype(F64)
    g = h @ w[pre + "gate_proj.weight"].astype(F64).T + w[pre + "gate_proj.bias"].astype(F64)
    u = h @ w[pre + "up_proj.weight"].astype(F64).T + w[pre + "up_proj.bias"].astype(F64)
    act = silu(g) * u
    if taps is not None:
        taps[tag + "act"] = act.copy()
    return act @ w[pre + "down_proj.weight"].astype(F64).T + w[pre + "down_proj.bias"].astype(F64)


def layer(x: np.ndarray, w: Dict[str, np.ndarray], i: int, cfg, cos, sin, taps: Optional[dict] = None) -> np.ndarray:
    pre = f"model.layer.{i}."
    h = V.layer_norm(x, w[pre + "norm1.weight"], w[pre + "norm1.bias"], cfg.layer_norm_eps)
    a = V.attention(h, w, pre + "attention.", cfg.num_attention_heads, cos, sin)
    x = (a * w[pre + "layer_scale1.lambda1"] + x).astype(V.F32)
    h = V.layer_norm(x, w[pre + "norm2.weight"], w[pre + "norm2.bias"], cfg.layer_norm_eps)
    d = gated_mlp(h, w, pre + "mlp.", taps, f"l{i}.")
    x = (d * w[pre + "layer_scale2.lambda1"].astype(F64) + x).astype(V.F32)
    if taps is not None:
        taps[f"l{i}.out"] = x.copy()
    return x


def forward(frames_u8: np.ndarray, w: Dict[str, np.ndarray], cfg, taps: Optional[dict] = None) -> np.ndarray:
    """uint8 (n, H, W, 3) frames -> last_hidden_state (n, T, D) float32, fed the way the reference's DinoEncoder feeds the model."""
    px = np.repeat(V.preprocess_green(frames_u8)[:, None], 3, 1)
    H, Wd = px.shape[2:]
    x = V.embeddings(px, w, cfg.patch_size)
    cos, sin = V.rope_cos_sin(H // cfg.patch_size, Wd // cfg.patch_size, cfg.hidden_size // cfg.num_attention_heads, cfg.rope_theta)
    for i in range(cfg.num_hidden_layers):
        x = layer(x, w, i, cfg, cos, sin, taps)
    return V.layer_norm(x, w["norm.weight"], w["norm.bias"], cfg.layer_norm_eps).astype(V.F32)
