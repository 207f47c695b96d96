"""CPU restatement of a precision-2 forward under an fp8 plan (shared by test_fp8_plan_host.py and test_gpu_fp8_plans.py).

``oracle.mx_oracle.vit_forward_mx`` with ``mx_quant`` applied only to the operands of the GEMMs in the plan: bit 1 q|k|v
(LayerNorm 1 rows and the three weights), 2 o_proj (attention context), 4 up (LayerNorm 2 rows), 8 down (GELU output).
Plan 15 is ``vit_forward_mx``, plan 0 ``vit_oracle.vit_forward``; both identities are tested on the CPU.
"""
import numpy as np

from oracle import mx_oracle as MX, vit_oracle as V

F32 = np.float32
QKV, PROJ, UP, DOWN = 1, 2, 4, 8


_GEMM_WEIGHTS = ("attention.q_proj.weight", "attention.k_proj.weight", "attention.v_proj.weight", "attention.o_proj.weight",
                 "mlp.up_proj.weight", "mlp.down_proj.weight")


def quantised_weights(w, cfg):
    """mx_quant of every projection weight, once: what a caller that restates several plans passes as ``wq``."""
    return {f"model.layer.{i}.{k}": MX.mx_quant(w[f"model.layer.{i}.{k}"])[0]
            for i in range(cfg.num_hidden_layers) for k in _GEMM_WEIGHTS}


def vit_forward_plan(pixels, w, cfg, plan, wq=None):
    def q_if(bit, t):
        return MX.mx_quant(t)[0] if plan & bit else t

    def wt(bit, key):
        if not plan & bit:
            return w[key]
        return wq[key] if wq is not None else MX.mx_quant(w[key])[0]

    x = V.embeddings(pixels.astype(F32), w, cfg.patch_size)
    H, W_ = pixels.shape[2:]
    nh = cfg.num_attention_heads
    cos, sin = V.rope_cos_sin(H // cfg.patch_size, W_ // cfg.patch_size, cfg.hidden_size // nh, cfg.rope_theta)
    for i in range(cfg.num_hidden_layers):
        pre = f"model.layer.{i}."
        a = pre + "attention."
        B, T, D = x.shape
        h = q_if(QKV, V.layer_norm(x, w[pre + "norm1.weight"], w[pre + "norm1.bias"], cfg.layer_norm_eps))
        q = h @ wt(QKV, a + "q_proj.weight").T + w[a + "q_proj.bias"]
        k = h @ wt(QKV, a + "k_proj.weight").T
        v = h @ wt(QKV, a + "v_proj.weight").T + w[a + "v_proj.bias"]
        q, k, v = (t.reshape(B, T, nh, D // nh).transpose(0, 2, 1, 3) for t in (q, k, v))
        npf = T - cos.shape[0]
        qp, kp = q[:, :, npf:], k[:, :, npf:]
        q = np.concatenate([q[:, :, :npf], qp * cos + V._rotate_half(qp) * sin], axis=2)
        k = np.concatenate([k[:, :, :npf], kp * cos + V._rotate_half(kp) * sin], axis=2)
        s = (q @ k.transpose(0, 1, 3, 2)) * F32((D // nh) ** -0.5)
        s = s - s.max(-1, keepdims=True)
        p = np.exp(s)
        p = p / p.sum(-1, keepdims=True)
        ctx = q_if(PROJ, (p @ v).transpose(0, 2, 1, 3).reshape(B, T, D).astype(F32))
        o = ctx @ wt(PROJ, a + "o_proj.weight").T + w[a + "o_proj.bias"]
        x = (o * w[pre + "layer_scale1.lambda1"] + x).astype(F32)
        h = q_if(UP, V.layer_norm(x, w[pre + "norm2.weight"], w[pre + "norm2.bias"], cfg.layer_norm_eps))
        u = q_if(DOWN, V.gelu_erf(h @ wt(UP, pre + "mlp.up_proj.weight").T + w[pre + "mlp.up_proj.bias"]))
        d = u @ wt(DOWN, pre + "mlp.down_proj.weight").T + w[pre + "mlp.down_proj.bias"]
        x = (d * w[pre + "layer_scale2.lambda1"] + x).astype(F32)
    return V.layer_norm(x, w["norm.weight"], w["norm.bias"], cfg.layer_norm_eps).astype(F32)


def encode_frames_plan(frames_u8, w, cfg, plan, batch=4, wq=None):
    """CLS rows (n, D) of uint8 frames, as mx_oracle.encode_frames_mx does for plan 15."""
    g = V.preprocess_green(frames_u8)
    outs = []
    for i in range(0, g.shape[0], batch):
        outs.append(vit_forward_plan(np.repeat(g[i:i + batch, None], 3, axis=1), w, cfg, plan, wq)[:, 0, :])
    return np.concatenate(outs, axis=0)
