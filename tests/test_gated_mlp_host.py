"""Gated-MLP DINOv3 encoders (ViT-S+/16, ViT-H+/16), host side: config parsing and round trip, the refusals that stay, parameter
names / shapes / blob length against the HF module and the library, the unchanged C boundary, the FLOP count."""
import ctypes
import json
import os
from dataclasses import replace

import numpy as np
import pytest

from cbas_amd import config as C, weights as W
from cbas_amd.encoder import pack_encoder_weights


def _write_cfg(tmp_path, **over):
    raw = dict(model_type="dinov3_vit", hidden_size=384, intermediate_size=1536, num_hidden_layers=12, num_attention_heads=6,
               num_register_tokens=4, patch_size=16, image_size=224, layer_norm_eps=1e-5, rope_theta=100.0, query_bias=True,
               key_bias=False, value_bias=True, proj_bias=True, mlp_bias=True, use_gated_mlp=True, hidden_act="silu")
    raw.update(over)
    p = tmp_path / "config.json"
    p.write_text(json.dumps(raw))
    return str(p)


def test_gated_config_parses_validates_and_round_trips(tmp_path):
    cfg = C.ViTConfig.from_json_file(_write_cfg(tmp_path))
    assert cfg == C.NAMED_VIT["vits16plus"]
    cfg.validate()                                            # raised NotImplementedError before gated MLPs were built
    transformers = pytest.importorskip("transformers")
    hf = transformers.DINOv3ViTConfig(**json.loads(cfg.to_json()))
    assert hf.use_gated_mlp is True and hf.hidden_act == "silu"
    p2 = tmp_path / "rt"
    p2.mkdir()
    hf.save_pretrained(str(p2))
    assert C.ViTConfig.from_json_file(str(p2 / "config.json")) == cfg


def test_named_gated_configs():
    s, h, t = C.NAMED_VIT["vits16plus"], C.NAMED_VIT["vith16plus"], C.NAMED_VIT["tiny_gated"]
    assert (s.hidden_size, s.intermediate_size, s.num_attention_heads, s.num_hidden_layers) == (384, 1536, 6, 12)
    assert (h.hidden_size, h.intermediate_size, h.num_attention_heads, h.num_hidden_layers) == (1280, 5120, 20, 32)
    assert (t.hidden_size, t.intermediate_size, t.num_attention_heads, t.num_hidden_layers, t.image_size) == (128, 384, 2, 2, 64)
    for c in (s, h, t):
        assert c.use_gated_mlp and c.hidden_act == "silu" and c.head_dim == 64
        c.validate()


def test_refusals_that_stay():
    with pytest.raises(NotImplementedError):
        C.ViTConfig(use_gated_mlp=True).validate()                                  # gated with the default "gelu"
    with pytest.raises(NotImplementedError):
        replace(C.VIT_S16PLUS, hidden_act="gelu_new").validate()
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        replace(C.DINOV2_B14, use_gated_mlp=True).validate()                        # DINOv2 use_swiglu_ffn
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        replace(C.DINOV2_B14, use_gated_mlp=True, hidden_act="silu").validate()
    with pytest.raises(NotImplementedError):
        replace(C.VIT_S16, hidden_act="silu").validate()                            # not gated: exact-erf gelu only


def test_param_shapes_match_the_hf_module():
    transformers = pytest.importorskip("transformers")
    cfg = C.VIT_TINY_GATED
    hcfg = transformers.DINOv3ViTConfig(**json.loads(cfg.to_json()))
    sd = transformers.DINOv3ViTModel(hcfg).state_dict()
    ours = W.encoder_param_shapes(cfg)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v) for k, v in ours.items()}
    # the MLP's tensors in the module's own order: gate_proj immediately before up_proj, then down_proj
    mlp = lambda keys: [k for k in keys if k.startswith("model.layer.0.mlp.")]      # noqa: E731
    assert mlp(ours) == mlp(sd) == ["model.layer.0.mlp." + k for k in
                                    ("gate_proj.weight", "gate_proj.bias", "up_proj.weight", "up_proj.bias", "down_proj.weight", "down_proj.bias")]
    w = W.synth_encoder_weights(cfg, 7)
    assert set(w) == set(ours) and all(w[k].shape == tuple(ours[k]) for k in ours)


def _enc_config_c(cfg, hw=64, precision=0):
    from cbas_amd import _lib
    return _lib.EncConfig(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                          cfg.num_register_tokens, cfg.patch_size, cfg.layer_norm_eps, cfg.rope_theta, 4, hw, hw, precision,
                          int(cfg.use_rope), int(cfg.pos_embed_grid))


def test_weight_counts_and_blob_order_agree_with_the_library():
    from cbas_amd import _lib
    lib = _lib.load()
    for cfg in (C.VIT_TINY_GATED, C.VIT_S16PLUS):
        w = W.synth_encoder_weights(cfg, 11)
        blob = pack_encoder_weights(cfg, w)
        cc = _enc_config_c(cfg)
        assert lib.cbas_enc_weights_count_mlp(ctypes.byref(cc), _lib.MLP_SWIGLU) == blob.shape[0]
        # mlp = 0 is cbas_enc_weights_count exactly; the gated blob is one (F, D) weight and one (F,) bias per layer longer
        plain = lib.cbas_enc_weights_count(ctypes.byref(cc))
        assert lib.cbas_enc_weights_count_mlp(ctypes.byref(cc), _lib.MLP_GELU) == plain
        F, D, L = cfg.intermediate_size, cfg.hidden_size, cfg.num_hidden_layers
        assert blob.shape[0] - plain == L * (F * D + F)
    # gate weight | gate bias immediately before up weight | up bias in layer 0
    cfg = C.VIT_TINY_GATED
    w = W.synth_encoder_weights(cfg, 11)
    blob = pack_encoder_weights(cfg, w)
    D, F, R, p = cfg.hidden_size, cfg.intermediate_size, cfg.num_register_tokens, cfg.patch_size
    off = D + R * D + D * 3 * p * p + D + 2 * D + 4 * (D * D + D) + D + 2 * D
    for k in ("gate_proj.weight", "gate_proj.bias", "up_proj.weight", "up_proj.bias"):
        t = w["model.layer.0.mlp." + k].reshape(-1)
        np.testing.assert_array_equal(blob[off:off + t.size], t)
        off += t.size
    # the refusals of the count (same rule as create): precision 2, precision 1, ConvNeXt, an unknown kind
    for cc, mlp in ((_enc_config_c(cfg, precision=2), 1), (_enc_config_c(cfg, precision=1), 1), (_enc_config_c(cfg), 2)):
        assert lib.cbas_enc_weights_count_mlp(ctypes.byref(cc), mlp) == -1
        assert lib.cbas_last_error()
    cnx = _enc_config_c(cfg, precision=4)
    cnx.family = 1
    assert lib.cbas_enc_weights_count_mlp(ctypes.byref(cnx), 1) == -1


def test_c_boundary_is_unchanged():
    from cbas_amd import _lib
    assert ctypes.sizeof(_lib.EncConfig) == 14 * 4 + 4 + 16 + 16
    assert _lib.EXPECTED_ABI == 11
    assert _lib.load().cbas_abi_version() == 11
    for name in ("cbas_enc_weights_count_mlp", "cbas_enc_create_mlp", "cbas_enc_get_mlp"):
        assert name in _lib.SIGNATURES


def test_precision_2_is_refused_before_any_library_call():
    from cbas_amd.encoder import DinoEncoder
    cfg = C.VIT_TINY_GATED
    with pytest.raises(ValueError, match="gated"):
        DinoEncoder.from_weights(cfg, W.synth_encoder_weights(cfg, 3), "cuda", precision=2)


def test_flops_per_frame_counts_three_mlp_gemms():
    cfg = C.VIT_S16PLUS
    P, T, D, F, L = 196, 201, 384, 1536, 12
    macs = P * 3 * 256 * D + L * (4 * T * D * D + 3 * T * D * F + 2 * T * T * D)
    assert cfg.flops_per_frame(224, 224) == 2.0 * macs
    assert cfg.flops_per_frame(224, 224) - C.VIT_S16.flops_per_frame(224, 224) == 2.0 * L * T * D * F


def test_float64_restatement_against_the_transformers_rows(golden_dir):
    """tests/gated_ref.py (the gated MLP in float64, everything else oracle/vit_oracle.py's) against transformers' own rows in
    gated_tiny.npz: the activation product silu(gate) * up and each layer's output to the absolute bound of
    tests/test_oracle_golden.py::test_vit_tiny_stagewise (1e-5), the CLS rows to the bound that file holds vits16_224 to
    (relative row error 1e-5).  The fixture stores the weights' seed: it stands for them as long as synth_encoder_weights is
    bit-stable, which the recorded frame hashes and these bounds together would show if it were not."""
    import hashlib
    from cbas_amd import synth
    import gated_ref as G
    g = np.load(os.path.join(golden_dir, "gated_tiny.npz"), allow_pickle=False)
    cfg = C.VIT_TINY_GATED
    w = W.synth_encoder_weights(cfg, int(g["enc_seed"]))
    for tag in ("a", "b"):
        fr = synth.cage_frames(int(g[f"{tag}_seed"]), 2, int(g[f"{tag}_height"]), int(g[f"{tag}_width"]))
        assert hashlib.sha256(np.ascontiguousarray(fr).tobytes()).hexdigest() == str(g[f"{tag}_frames_sha"])
        taps = {}
        out = G.forward(fr, w, cfg, taps)
        for i in range(cfg.num_hidden_layers):
            np.testing.assert_allclose(taps[f"l{i}.act"], g[f"{tag}_act{i}"], atol=1e-5)
            np.testing.assert_allclose(taps[f"l{i}.out"], g[f"{tag}_layer{i}"], atol=1e-5)
        cls, ref = out[:, 0].astype(np.float64), g[f"{tag}_cls"].astype(np.float64)
        rel = np.linalg.norm(cls - ref, axis=1) / np.linalg.norm(ref, axis=1)
        assert rel.max() < 1e-5, rel.max()
