"""Per-layer hidden states, per-layer CLS attention and attention rollout: what can be checked without a GPU - the library
surface, the recorded fixture (tests/golden/make_goldens_layers.py) and the pure-Python argument handling."""
import os
import re

import numpy as np
import pytest

from cbas_amd import _lib, attention_maps as A, config as C
from cbas_amd.encoder import normalize_layers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cbas_enc_forward_u8_layers", "cbas_enc_forward_f32_layers", "cbas_enc_layers_scratch_bytes")
NEW_DEBUG = ("cbas_debug_attention_mean", "cbas_debug_rollout_step")
TINY = ("vit_tiny", "gated_tiny", "dinov2reg_tiny", "dinov2_tiny")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_library_surface():
    header, dbg = read("include", "cbas_mi355x.h"), read("include", "cbas_mi355x_debug.h")
    for name in NEW:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", header), name
    for name in NEW_DEBUG:
        assert name in _lib.DEBUG_SIGNATURES and re.search(rf"\b{name}\(", dbg) and name not in _lib.SIGNATURES, name
    assert "global: cbas_*;" in read("cbas_amd", "csrc", "exports.map")      # every cbas_ symbol is exported, nothing else
    assert _lib.EXPECTED_ABI == 11 and re.search(r"#define CBAS_ABI_VERSION\s+11\b", header)
    readme = read("README.md")
    assert f"{len(_lib.SIGNATURES)} entry points" in readme and "attention_rollout" in readme
    # the ctypes mirror of cbas_enc_layers_args has the header's fields in the header's order
    body = re.search(r"typedef struct cbas_enc_layers_args \{(.*?)\} cbas_enc_layers_args;", header, re.S).group(1)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f[0] for f in _lib.LayersArgs._fields_]


def rollout64(attn_mean):
    Amean = np.asarray(attn_mean, np.float64)
    eye = np.eye(Amean.shape[-1])
    R = 0.5 * Amean[0] + 0.5 * eye
    for l in range(1, Amean.shape[0]):
        R = np.matmul(0.5 * Amean[l] + 0.5 * eye, R)
    return R


def test_fixture(golden_dir):
    path = os.path.join(golden_dir, "encoder_layers.npz")
    assert os.path.getsize(path) < 1_000_000
    g, hs = np.load(path), np.load(os.path.join(golden_dir, "hidden_state.npz"))
    assert list(g["names"]) == list(TINY) + ["vitb16"]
    for name in g["names"]:
        for k in ("n", "height", "width", "seed", "frames_sha", "rows"):
            assert np.array_equal(g[f"{name}_{k}"], hs[f"{name}_{k}"]), (name, k)      # hidden_state.npz's own frames and rows
    for name, cfg in zip(TINY, (C.VIT_TINY, C.VIT_TINY_GATED, C.DINOV2_REG_TINY, C.DINOV2_TINY)):
        L, NP = cfg.num_hidden_layers, cfg.num_prefix_tokens
        am = g[f"{name}_attn_mean"]
        assert am.shape[0] == L and list(g[f"{name}_hs_layers"]) == list(range(L + 1))
        assert np.abs(am.astype(np.float64).sum(-1) - 1.0).max() < 1e-6
        R = rollout64(am)
        q = int(g[f"{name}_patch_query"])
        assert np.abs(R[:, 0, NP:] - g[f"{name}_rollout_cls"]).max() <= 1e-12
        assert np.abs(R[:, q, NP:] - g[f"{name}_rollout_patch"]).max() <= 1e-12
        # the recorded CLS rows and map are row 0 of the recorded attentions
        heads = g[f"{name}_cls_heads"]
        assert np.abs(heads.astype(np.float64).mean(2) - am[:, :, 0].astype(np.float64)).max() < 1e-7
        assert np.abs(heads[:, :, :, NP:].astype(np.float64).mean(2) - g[f"{name}_cls_map"]).max() < 1e-7
        from cbas_amd.encoder import query_token_index
        assert query_token_index(cfg, int(g[f"{name}_height"]), int(g[f"{name}_width"]), tuple(g[f"{name}_patch_pixel"])) == q


@pytest.mark.parametrize("name,cfg", [("vit_tiny", C.VIT_TINY), ("gated_tiny", C.VIT_TINY_GATED), ("dinov2reg_tiny", C.DINOV2_REG_TINY),
                                      ("dinov2_tiny", C.DINOV2_TINY), ("vitb16", C.VIT_B16)])
def test_fixture_last_state_normalises_to_hidden_state(golden_dir, name, cfg):
    """LayerNorm of the last raw hidden state, with the fixture's own final-norm weights, is hidden_state.npz's rows."""
    from cbas_amd import weights as W
    g, hs = np.load(os.path.join(golden_dir, "encoder_layers.npz")), np.load(os.path.join(golden_dir, "hidden_state.npz"))
    w = dict(W.canonical_encoder_weights(cfg, W.synth_encoder_weights(cfg, int(g["enc_seed"]))))
    x = g[f"{name}_hidden"][-1].astype(np.float64)
    assert int(g[f"{name}_hs_layers"][-1]) == cfg.num_hidden_layers
    c = x - x.mean(-1, keepdims=True)
    y = c / np.sqrt((c * c).mean(-1, keepdims=True) + cfg.layer_norm_eps) * w["norm.weight"].astype(np.float64) + w["norm.bias"].astype(np.float64)
    ref = hs[f"{name}_hidden"].astype(np.float64)
    assert np.abs(y - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max())      # both recorded in fp32: a few ulps of the rows' magnitude


def test_normalize_layers():
    assert normalize_layers(None, 12) == list(range(13)) and normalize_layers("all", 12, 1, "attention") == list(range(1, 13))
    assert normalize_layers([0, -1, 6], 12) == [0, 12, 6] and normalize_layers(-13, 12) == [0] and normalize_layers(3, 12) == [3]
    assert normalize_layers(-12, 12, 1) == [1] and normalize_layers(np.int64(2), 4) == [2]
    for bad, lo in (([13], 0), ([-14], 0), ([0], 1), ([-13], 1), ([], 0), ("every", 0)):
        with pytest.raises(ValueError):
            normalize_layers(bad, 12, lo)


def test_refuse_kind_and_cli():
    assert "rollout" in A.KINDS and A.refuse_kind(C.VIT_B16, "rollout") is None
    assert "similarity" in A.refuse_kind(C.CONVNEXT_T, "rollout") and "pca" in A.refuse_kind(C.CONVNEXT_T, "rollout")
    base = ["--video", "v.npy", "--frame", "0", "--encoder", "e", "--out", "o.png"]
    a = A.parse_cli(base + ["--layer", "all"])[1]
    assert a.kind == "attention" and a.layer == "all" and a.query is None
    assert A.parse_cli(base + ["--layer", "-2"])[1].layer == -2 and A.parse_cli(base)[1].layer is None
    a = A.parse_cli(base + ["--kind", "rollout", "--query", "17,40"])[1]
    assert a.kind == "rollout" and a.query == (17, 40) and a.layer is None
    for bad in (["--kind", "rollout", "--layer", "3"], ["--layer", "two"], ["--kind", "pca", "--query", "1,2"], ["--kind", "similarity", "--layer", "1"]):
        with pytest.raises(SystemExit):
            A.parse_cli(base + bad)
