"""DINOv3 ConvNeXt encoders, host side (no GPU): config parsing, FLOPs, the state-dict key set, the weight blob's length
against the library's cbas_enc_weights_count, the ABI 11 config struct, and the refusal of precisions 0 / 1 / 2."""
import ctypes
import json
import os

import numpy as np
import pytest

from cbas_amd import config as C, weights as W, _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_config_json_parses_to_convnext_t():
    cfg = C.encoder_config_from_json(os.path.join(GOLDEN, "convnext_t_config.json"))
    assert isinstance(cfg, C.ConvNextConfig)
    assert tuple(cfg.hidden_sizes) == (96, 192, 384, 768) and tuple(cfg.depths) == (3, 3, 9, 3)
    assert cfg.hidden_size == 768 and cfg.layer_norm_eps == 1e-6 and cfg.hidden_act == "gelu"
    assert cfg.num_channels == 3 and cfg.model_type == "dinov3_convnext"
    cfg.validate()
    assert cfg == C.CONVNEXT_T


def test_config_round_trips_through_to_json(tmp_path):
    p = tmp_path / "config.json"
    p.write_text(C.CONVNEXT_S.to_json())
    assert C.encoder_config_from_json(str(p)) == C.CONVNEXT_S


def test_unknown_model_types_are_still_refused(tmp_path):
    for mt in ("convnext", "dinov3_convnext_v2", "swin"):
        p = tmp_path / f"{mt}.json"
        p.write_text(json.dumps({"model_type": mt, "hidden_size": 768}))
        with pytest.raises(NotImplementedError):
            C.encoder_config_from_json(str(p))


def test_validate_refuses_unbuilt_variants():
    with pytest.raises(NotImplementedError, match="multiple of 32"):
        C.ConvNextConfig(hidden_sizes=(96, 200, 384, 768)).validate()
    with pytest.raises(NotImplementedError, match="gelu"):
        C.ConvNextConfig(hidden_act="relu").validate()


def test_flops_per_frame():
    assert round(C.CONVNEXT_T.flops_per_frame(224, 224) / 1e9, 3) == 8.910
    assert round(C.CONVNEXT_T.flops_per_frame(256, 256) / 1e9, 3) == 11.637


def test_synthesised_key_set_is_the_hf_state_dict():
    ref = {}
    with open(os.path.join(GOLDEN, "convnext_t_keys.txt")) as f:
        for line in f:
            name, shape = line.split()
            ref[name] = tuple(int(s) for s in shape.split(","))
    assert {k: tuple(v) for k, v in W.convnext_param_shapes(C.CONVNEXT_T).items()} == ref
    # the synthesiser draws exactly those tensors (checked on the tiny config: the draw is the same code for every config, and
    # ConvNeXt-T's 28 M values would take seconds of CPU here); LayerNorm gains / offsets, biases and gamma are randomised,
    # so no block is an identity
    cfg = C.CONVNEXT_TINY
    w = W.synth_convnext_weights(cfg, 1)
    assert {k: tuple(v.shape) for k, v in w.items()} == {k: tuple(v) for k, v in W.convnext_param_shapes(cfg).items()}
    g = w["model.stages.0.layers.0.gamma"]
    assert g.min() > 0.1 and np.unique(g).size > 1


def _cnx_config(cfg, precision=4):
    return _lib.EncConfig(hidden_size=cfg.hidden_size, layer_norm_eps=cfg.layer_norm_eps, max_batch=2, max_height=64,
                          max_width=64, precision=precision, family=1,
                          stage_widths=(ctypes.c_int32 * 4)(*cfg.hidden_sizes), stage_depths=(ctypes.c_int32 * 4)(*cfg.depths))


@pytest.mark.parametrize("cfg", [C.CONVNEXT_TINY, C.CONVNEXT_T], ids=["tiny", "convnext_t"])
def test_blob_length_matches_the_library(cfg):
    from cbas_amd.encoder import pack_encoder_weights
    lib = _lib.load()
    zeros = {k: np.zeros(shape, np.float32) for k, shape in W.convnext_param_shapes(cfg).items()}     # the length is the point
    blob = pack_encoder_weights(cfg, zeros)
    assert lib.cbas_enc_weights_count(ctypes.byref(_cnx_config(cfg))) == blob.shape[0]


def test_abi_11_config_struct():
    assert _lib.EXPECTED_ABI == 11 and _lib.load().cbas_abi_version() == 11
    vit = _lib.EncConfig(768, 3072, 12, 12, 4, 16, 1e-5, 100.0, 8, 224, 224, 4, 1, 0)     # ABI 10's 14 positional fields
    assert vit.family == 0 and list(vit.stage_widths) == [0] * 4 and list(vit.stage_depths) == [0] * 4
    assert ctypes.sizeof(_lib.EncConfig) == 4 * (14 + 1 + 8)


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_precisions_0_1_2_are_refused_before_any_device_call(precision, tmp_path, monkeypatch):
    from cbas_amd.encoder import DinoEncoder
    cfg = C.CONVNEXT_TINY
    with pytest.raises(ValueError, match="precision 3"):
        DinoEncoder.from_weights(cfg, W.synth_convnext_weights(cfg, 1), "cpu", precision=precision)
    d = str(tmp_path / "ckpt")
    W.save_encoder_checkpoint(d, cfg, W.synth_convnext_weights(cfg, 1))
    loaded_cfg, loaded_w = W.load_encoder_checkpoint(d)
    assert loaded_cfg == cfg and set(loaded_w) == set(W.convnext_param_shapes(cfg))
    if precision == 0:
        monkeypatch.setenv("CBAS_PRECISION", "0")
        with pytest.raises(ValueError, match="precision 3"):
            DinoEncoder(d, device="cpu")


def test_task_model_prefix_is_stripped(tmp_path):
    from safetensors.numpy import save_file
    cfg = C.CONVNEXT_TINY
    d = tmp_path / "task"
    d.mkdir()
    (d / "config.json").write_text(cfg.to_json())
    save_file({"dinov3_convnext." + k: v for k, v in W.synth_convnext_weights(cfg, 1).items()}, str(d / "model.safetensors"))
    _, w = W.load_encoder_checkpoint(str(d))
    assert set(w) == set(W.convnext_param_shapes(cfg))
