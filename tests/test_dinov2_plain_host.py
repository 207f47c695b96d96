"""Plain DINOv2 (HF model_type "dinov2", e.g. "facebook/dinov2-base": the third encoder the reference's
cbas_config.yaml.example names) on the host: config / checkpoint plumbing, the weight blob without a register block, and the
position-table builder - F.interpolate(mode="bicubic", align_corners=False) WITHOUT antialiasing (HF modeling_dinov2.py:86-91),
where the with-registers family passes antialias=True.  Fixtures: tests/golden/make_goldens_dinov2_plain.py (transformers'
Dinov2Model and the reference's own DinoEncoder wrapper).

Also holds the small numpy restatement of Dinov2Model the GPU tests take their stage taps from (tests/test_gpu_dinov2_plain.py);
it is pinned here against the recorded HF outputs."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from cbas_amd import _lib, config as C, weights as W, synth
from oracle import vit_oracle as V

F32 = np.float32
POS_AA, POS_PLAIN = _lib.POS_INTERP_BICUBIC_AA, _lib.POS_INTERP_BICUBIC
# the table fixture's input (make_goldens_dinov2_plain.py: TABLE_SEED, TABLE_GRID, TABLE_DIM)
TABLE_SEED, TABLE_GRID, TABLE_DIM = 77, 37, 16
TABLE_SIZES = ((16, 16), (18, 18), (18, 20), (40, 40))
# Bound of the builder against torch, fixed before measuring: an output is two nested 4-tap sums, 8 products and 8 additions of
# terms no larger than the largest entry, each rounded to <= 1/2 ulp of it -> 4 ulps of the largest table entry.  Nothing else
# differs (same fp32 coefficients up to their own last bit, same tap order).  Measured: 2.5 ulps (18 x 20, 40 x 40).
TABLE_ULPS = 4


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def rel_rows(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


# ------------------------------------------------------------------------------------------------------------------------
# numpy restatement of HF Dinov2Model (modeling_dinov2.py): embeddings :97-116 with interpolate_pos_encoding :57-95, then the
# blocks shared with the other ViT families (oracle/vit_oracle.py: no RoPE, key bias), then the final LayerNorm
# ------------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """One fused multiply-add in float32 (the product of two float32 is exact in float64)."""
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def _cubic_coeffs(t):
    """ATen get_cubic_upsample_coefficients (UpSample.h), a = -0.75, in float32.  The outer taps' polynomial cancels to a few
    1e-4; it is evaluated with fused multiply-adds, as ATen's x86 builds contract it and as the library writes it."""
    A, one, two = F32(-0.75), F32(1), F32(2)

    def c1(x):
        return ((A + two) * x - (A + F32(3))) * x * x + one

    def c2(x):
        return _fma(_fma(_fma(A, x, -F32(5) * A), x, F32(8) * A), x, -F32(4) * A)
    return [c2(t + one), c1(t), c1(one - t), c2((one - t) + one)]


def bicubic_taps(in_size, out_size):
    """[(4 clamped source indices, 4 float32 weights)] per output index: upsample_bicubic2d, align_corners=False, scale from
    the sizes (HF passes size=), source index not clamped, taps clamped."""
    scale = F32(in_size) / F32(out_size)
    out = []
    for i in range(out_size):
        real = _fma(scale, F32(i) + F32(0.5), -F32(0.5))
        idx = min(int(np.floor(real)), in_size - 1)
        t = F32(min(max(real - F32(idx), F32(0)), F32(1)))
        out.append(([min(max(idx - 1 + k, 0), in_size - 1) for k in range(4)], _cubic_coeffs(t)))
    return out


def plain_pos_table(pos, grid, nh, nw):
    """modeling_dinov2.py:57-95: pos (1 + grid * grid, D) -> (1 + nh * nw, D); the stored table when the grids match."""
    pos = pos.reshape(1 + grid * grid, -1).astype(F32)
    if nh == grid and nw == grid:
        return pos
    patch = pos[1:].reshape(grid, grid, -1)
    ty, tx = bicubic_taps(grid, nh), bicubic_taps(grid, nw)
    out = np.zeros((nh, nw, patch.shape[-1]), F32)
    for y, (iy, wy) in enumerate(ty):
        for x, (ix, wx) in enumerate(tx):
            acc = np.zeros(patch.shape[-1], F32)
            for a in range(4):
                row = np.zeros(patch.shape[-1], F32)
                for b in range(4):
                    row = row + wx[b] * patch[iy[a], ix[b]]
                acc = acc + wy[a] * row
            out[y, x] = acc
    return np.concatenate([pos[:1], out.reshape(nh * nw, -1)], axis=0)


def plain_forward(frames, w, cfg, taps=None):
    """frames (n, H, W, 3) uint8 -> last_hidden_state (n, 1 + P, D); ``w`` in the canonical key names.  taps: "pos",
    "embeddings" and vit_oracle's per-layer taps (l{i}.ln1 ... l{i}.out)."""
    px = np.repeat(V.preprocess_green(frames)[:, None], 3, 1).astype(F32)
    B, Cn, H, Wd = px.shape
    p = cfg.patch_size
    nh, nw = H // p, Wd // p
    x = px[:, :, :nh * p, :nw * p].reshape(B, Cn, nh, p, nw, p).transpose(0, 2, 4, 1, 3, 5).reshape(B, nh * nw, Cn * p * p)
    wk = w["embeddings.patch_embeddings.weight"].reshape(-1, Cn * p * p)
    pe = (x @ wk.T + w["embeddings.patch_embeddings.bias"]).astype(F32)
    D = wk.shape[0]
    pos = plain_pos_table(w["embeddings.position_embeddings"], cfg.pos_embed_grid, nh, nw)
    cls = np.broadcast_to(w["embeddings.cls_token"].reshape(1, 1, D), (B, 1, D))
    x = (np.concatenate([cls, pe], axis=1) + pos[None]).astype(F32)
    if taps is not None:
        taps["pos"], taps["embeddings"] = pos, x.copy()
    for i in range(cfg.num_hidden_layers):
        x = V.layer(x, w, i, cfg.num_attention_heads, cfg.layer_norm_eps, None, None, taps)
    return V.layer_norm(x, w["norm.weight"], w["norm.bias"], cfg.layer_norm_eps).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------
# config and weights
# ------------------------------------------------------------------------------------------------------------------------
# config.json of "facebook/dinov2-base" as the hub serves it (settings only)
HUB_DINOV2_BASE = {
    "architectures": ["Dinov2Model"], "attention_probs_dropout_prob": 0.0, "drop_path_rate": 0.0, "hidden_act": "gelu",
    "hidden_dropout_prob": 0.0, "hidden_size": 768, "image_size": 518, "initializer_range": 0.02, "layer_norm_eps": 1e-06,
    "layerscale_value": 1.0, "mlp_ratio": 4, "model_type": "dinov2", "num_attention_heads": 12, "num_channels": 3,
    "num_hidden_layers": 12, "patch_size": 14, "qkv_bias": True, "torch_dtype": "float32", "use_swiglu_ffn": False}


def _write_config(tmp_path, **over):
    p = tmp_path / "config.json"
    p.write_text(json.dumps({**HUB_DINOV2_BASE, **over}))
    return str(p)


def test_hub_config_parses_to_the_named_config(tmp_path):
    p = _write_config(tmp_path)
    cfg = C.ViTConfig.from_json_file(p)
    assert cfg == C.DINOV2_B14 == C.NAMED_VIT["dinov2b14"] and C.encoder_config_from_json(p) == cfg
    cfg.validate()
    assert cfg.num_register_tokens == 0 and cfg.num_prefix_tokens == 1 and not cfg.use_rope and cfg.key_bias
    assert cfg.pos_embed_grid == 37 and cfg.layer_norm_eps == 1e-6 and cfg.intermediate_size == 3072
    assert [cfg.num_tokens(s, s) for s in (224, 256, 518)] == [257, 325, 1370]
    tiny = C.NAMED_VIT["dinov2tiny"]
    assert tiny == C.DINOV2_TINY and tiny.num_register_tokens == 0 and tiny.pos_embed_grid == 5
    # the R = 0 twins: nothing else differs
    from dataclasses import replace
    assert replace(C.DINOV2_REG_B14, model_type="dinov2", num_register_tokens=0) == C.DINOV2_B14
    # a stray num_register_tokens in a plain-DINOv2 config.json is not a register count
    assert C.ViTConfig.from_json_file(_write_config(tmp_path, num_register_tokens=4)) == C.DINOV2_B14


def test_swiglu_checkpoint_is_still_refused(tmp_path):
    cfg = C.ViTConfig.from_json_file(_write_config(tmp_path, use_swiglu_ffn=True))
    assert cfg.use_gated_mlp
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        cfg.validate()
    from dataclasses import replace
    with pytest.raises(NotImplementedError, match="register"):
        replace(C.DINOV2_TINY, num_register_tokens=4).validate()


def test_state_dict_keys_and_canonical_names():
    cfg = C.DINOV2_TINY
    w = W.synth_encoder_weights(cfg, 1234)
    reg = W.synth_encoder_weights(C.DINOV2_REG_TINY, 1234)
    assert set(reg) - set(w) == {"embeddings.register_tokens"} and set(w) <= set(reg)
    for k in w:                                             # same seeded tensors as the with-registers twin
        assert np.array_equal(w[k], reg[k]), k
    assert w["embeddings.mask_token"].shape == (1, cfg.hidden_size)
    cw = W.canonical_encoder_weights(cfg, w)
    assert "embeddings.patch_embeddings.weight" in cw and "model.layer.1.attention.k_proj.bias" in cw and "norm.bias" in cw
    assert "embeddings.register_tokens" not in cw and len(cw) == len(w)


def test_checkpoint_roundtrip_through_us(tmp_path):
    cfg = C.DINOV2_TINY
    w = W.synth_encoder_weights(cfg, 3)
    W.save_encoder_checkpoint(str(tmp_path / "ck"), cfg, w)
    cfg2, w2 = W.load_encoder_checkpoint(str(tmp_path / "ck"))
    assert cfg2 == cfg and set(w2) == set(w)
    for k in w:
        assert np.array_equal(w[k], w2[k]), k
    assert json.load(open(tmp_path / "ck" / "config.json"))["model_type"] == "dinov2"


def test_checkpoint_roundtrip_through_transformers(tmp_path):
    """A directory we write loads in transformers' Dinov2Model (through AutoModel, as the reference loads it), and a directory
    Dinov2Model.save_pretrained writes loads here - equal tensors both ways."""
    transformers = pytest.importorskip("transformers")
    import torch
    cfg = C.DINOV2_TINY
    w = W.synth_encoder_weights(cfg, 5)
    W.save_encoder_checkpoint(str(tmp_path / "ours"), cfg, w)
    m = transformers.AutoModel.from_pretrained(str(tmp_path / "ours"))
    assert type(m).__name__ == "Dinov2Model" and m.config.model_type == "dinov2"
    assert m.config.mlp_ratio == 4 and m.config.layer_norm_eps == 1e-6 and not m.config.use_swiglu_ffn
    sd = m.state_dict()
    assert set(sd) == set(w)
    for k, v in w.items():
        assert torch.equal(sd[k], torch.from_numpy(v)), k
    m.save_pretrained(str(tmp_path / "theirs"))
    cfg2, w2 = W.load_encoder_checkpoint(str(tmp_path / "theirs"))
    assert cfg2 == cfg
    for k, v in w.items():
        assert np.array_equal(w2[k], v), k


def _enc_config_c(cfg, max_hw=70):
    return _lib.EncConfig(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                          cfg.num_register_tokens, cfg.patch_size, cfg.layer_norm_eps, cfg.rope_theta, 8, max_hw, max_hw, 0,
                          int(cfg.use_rope), cfg.pos_embed_grid)


def test_blob_has_an_empty_register_block():
    from cbas_amd.encoder import pack_encoder_weights
    lib = _lib.load()
    cfg, reg = C.DINOV2_TINY, C.DINOV2_REG_TINY
    w = W.synth_encoder_weights(cfg, 1)
    blob = pack_encoder_weights(cfg, w)
    assert lib.cbas_enc_weights_count(ctypes.byref(_enc_config_c(cfg))) == blob.shape[0]
    D = cfg.hidden_size
    assert lib.cbas_enc_weights_count(ctypes.byref(_enc_config_c(reg))) - blob.shape[0] == reg.num_register_tokens * D
    # cls_token, then straight the position embeddings
    assert np.array_equal(blob[:D], w["embeddings.cls_token"].reshape(-1))
    assert np.array_equal(blob[D:D + (1 + 25) * D], w["embeddings.position_embeddings"].reshape(-1))
    # ViT-B/14 by shapes alone (no 86 M-element blob here)
    n = sum(int(np.prod(s)) for k, s in W.encoder_param_shapes(C.DINOV2_B14).items() if not k.endswith("mask_token"))
    assert lib.cbas_enc_weights_count(ctypes.byref(_enc_config_c(C.DINOV2_B14, 518))) == n


def test_set_pos_interp_rejects_a_null_handle_without_gpu():
    lib = _lib.load()
    assert lib.cbas_enc_set_pos_interp(None, POS_PLAIN) == -1
    assert ctypes.sizeof(_lib.EncConfig) == 4 * (14 + 1 + 8) and lib.cbas_abi_version() == 11      # the choice is not a config field


# ------------------------------------------------------------------------------------------------------------------------
# the position table
# ------------------------------------------------------------------------------------------------------------------------
def lib_matrix(mode, n_in, n_out):
    _lib.require_debug("cbas_debug_pos_interp_matrix")
    Wm = np.zeros((n_out, n_in), F32)
    _lib.check(_lib.load().cbas_debug_pos_interp_matrix(mode, n_in, n_out, Wm.ctypes.data), "cbas_debug_pos_interp_matrix")
    return Wm


def lib_table(mode, src, grid, nh, nw):
    _lib.require_debug("cbas_debug_pos_table")
    src = np.ascontiguousarray(src, F32)
    out = np.full((nh * nw, src.shape[1]), np.nan, F32)
    _lib.check(_lib.load().cbas_debug_pos_table(mode, src.ctypes.data, grid, src.shape[1], nh, nw, out.ctypes.data),
               "cbas_debug_pos_table")
    return out


def table_grid():
    return W.synth_normal(TABLE_SEED, "pos_table_grid", (TABLE_GRID * TABLE_GRID, TABLE_DIM), 0.3)


def test_plain_matrix_properties():
    for gin, gout in ((37, 16), (37, 18), (37, 20), (37, 40), (5, 4), (5, 6)):
        Wm = lib_matrix(POS_PLAIN, gin, gout)
        np.testing.assert_allclose(Wm.sum(1), 1.0, atol=2e-6)
        # symmetric under reflection up to the fp32 source index: near index 36 its ulp is 3.8e-6, and so is the tap phase's
        np.testing.assert_allclose(Wm, Wm[::-1, ::-1], atol=1e-5)
        assert ((Wm != 0).sum(1) <= 4).all()                            # four taps, never widened (no antialiasing)
        for i, (idx, co) in enumerate(bicubic_taps(gin, gout)):         # the restatement above, tap by tap
            want = np.zeros(gin, F32)
            for j, c in zip(idx, co):
                want[j] += c
            np.testing.assert_allclose(Wm[i], want, atol=2e-6)
    assert np.array_equal(lib_matrix(POS_PLAIN, 37, 37), np.eye(37, dtype=F32))
    # the antialiased builder widens its support when it downsamples: 37 -> 18 reaches 8 to 9 source rows
    assert ((lib_matrix(POS_AA, 37, 18) != 0).sum(1) > 4).any()


def test_plain_table_matches_torch_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "dinov2_pos_tables.npz"))
    src = table_grid()
    assert sha(src) == str(g["grid_sha"])
    worst = 0.0
    for nh, nw in TABLE_SIZES:
        ref = g[f"t{nh}x{nw}"]
        got = lib_table(POS_PLAIN, src, TABLE_GRID, nh, nw)
        ulp = float(np.spacing(F32(np.abs(ref).max())))
        d = float(np.abs(got - ref).max())
        worst = max(worst, d / ulp)
        print(f"[plain table {nh}x{nw}] max |d| = {d:.3e} = {d / ulp:.2f} ulp of the largest entry ({np.abs(ref).max():.3f})")
        assert d <= TABLE_ULPS * ulp, (nh, nw, d / ulp)
        # the test's own restatement, used for the GPU stage taps
        mine = plain_pos_table(np.concatenate([np.zeros((1, TABLE_DIM), F32), src]), TABLE_GRID, nh, nw)[1:]
        assert np.abs(mine - ref).max() <= TABLE_ULPS * ulp
    print(f"[plain table] worst {worst:.2f} ulp (bound {TABLE_ULPS})")


def test_antialiased_table_is_a_different_table_at_cbas_video_size(golden_dir):
    """The check above can tell the two filters apart: at 18 x 18 (CBAS's standard 256 x 256 video) the antialiased builder misses
    the plain fixture by orders of magnitude more than the bound, and so it does at every downsampled size."""
    g = np.load(os.path.join(golden_dir, "dinov2_pos_tables.npz"))
    src = table_grid()
    for nh, nw in ((18, 18), (16, 16), (18, 20)):
        ref = g[f"t{nh}x{nw}"]
        bound = TABLE_ULPS * float(np.spacing(F32(np.abs(ref).max())))
        d = float(np.abs(lib_table(POS_AA, src, TABLE_GRID, nh, nw) - ref).max())
        print(f"[aa vs plain {nh}x{nw}] max |d| = {d:.3e} = {d / bound:.1e} x the bound")
        assert d > 1e4 * bound


def test_native_grid_returns_the_stored_table_exactly():
    src = table_grid()
    for mode in (POS_PLAIN, POS_AA):
        assert np.array_equal(lib_table(mode, src, TABLE_GRID, TABLE_GRID, TABLE_GRID), src)
    lib = _lib.load()
    assert lib.cbas_debug_pos_table(2, src.ctypes.data, TABLE_GRID, TABLE_DIM, 4, 4, src.ctypes.data) == -1      # unknown mode


# ------------------------------------------------------------------------------------------------------------------------
# the restatement against the recorded HF outputs (it supplies the GPU tests' stage taps)
# ------------------------------------------------------------------------------------------------------------------------
def tiny_case(g, tag):
    H, Wd, seed = int(g[f"{tag}_height"]), int(g[f"{tag}_width"]), int(g[f"{tag}_seed"])
    fr = synth.cage_frames(seed, 2, H, Wd)
    assert sha(fr) == str(g[f"{tag}_frames_sha"])
    return fr


@pytest.mark.parametrize("tag", ["r", "n"])
def test_restatement_reproduces_tiny_fixture(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "dinov2_tiny.npz"))
    cfg = C.DINOV2_TINY
    w = W.canonical_encoder_weights(cfg, W.synth_encoder_weights(cfg, 1234))
    taps = {}
    out = plain_forward(tiny_case(g, tag), w, cfg, taps)
    if tag == "n":
        assert np.array_equal(taps["pos"], w["embeddings.position_embeddings"].reshape(26, -1))     # the skip branch
        assert np.array_equal(g["n_pos"], taps["pos"])
    np.testing.assert_allclose(taps["pos"], g[f"{tag}_pos"], atol=1e-6)
    np.testing.assert_allclose(taps["embeddings"], g[f"{tag}_emb"], atol=2e-5)
    np.testing.assert_allclose(taps["l0.out"], g[f"{tag}_layer0"], atol=3e-5)
    np.testing.assert_allclose(taps["l1.out"], g[f"{tag}_layer1"], atol=3e-5)
    np.testing.assert_allclose(out, g[f"{tag}_last"], atol=3e-5)
    # the library's builder on the same stored table
    nh, nw = int(g[f"{tag}_height"]) // 14, int(g[f"{tag}_width"]) // 14
    stored = w["embeddings.position_embeddings"].reshape(26, -1)
    got = lib_table(POS_PLAIN, stored[1:], 5, nh, nw)
    ulp = float(np.spacing(F32(np.abs(g[f"{tag}_pos"]).max())))
    assert np.abs(got - g[f"{tag}_pos"][1:]).max() <= TABLE_ULPS * ulp


def test_restatement_reproduces_b14_non_square_row(golden_dir):
    g = np.load(os.path.join(golden_dir, "dinov2_b14.npz"))
    cfg = C.DINOV2_B14
    w = W.canonical_encoder_weights(cfg, W.synth_encoder_weights(cfg, 1234))
    fr = synth.cage_frames(int(g["r252x280_seed"]), 1, 252, 280)
    assert rel_rows(plain_forward(fr, w, cfg)[:, 0], g["r252x280_cls"][:1]).max() < 2e-5


def test_e2e_fixture_is_not_near_a_tie_and_its_labels_follow_from_its_rows(golden_dir):
    from oracle import pipeline_oracle as PO
    g = np.load(os.path.join(golden_dir, "e2e_dinov2_b14.npz"))
    n = int(g["n"])
    assert 256 <= n <= 512 and int(g["hw"]) == 256
    srt = np.sort(g["probs"].astype(np.float64), axis=1)
    margin = float((srt[:, -1] - srt[:, -2]).min())
    assert margin >= 1e-3 and abs(margin - float(g["min_margin"])) < 1e-9       # checked when the fixture was made; stored
    assert np.array_equal(g["cls_every8"].astype(np.float16), g["cls_f16"][::8])
    probs = PO.classify_cls(g["cls_f16"], W.synth_head_weights(C.HeadConfig(in_features=768), 4321), 31, 1.0)
    np.testing.assert_allclose(probs, g["probs"], atol=1e-5)
    assert (probs.argmax(1) == g["labels"]).all() and len(set(g["labels"].tolist())) >= 2
    cfg = C.DINOV2_B14
    w = W.canonical_encoder_weights(cfg, W.synth_encoder_weights(cfg, 1234))
    fr = synth.cage_frames(int(g["frame_seed"]), 1, 256, 256, first=8)
    assert rel_rows(plain_forward(fr, w, cfg)[:, 0], g["cls_every8"][1:2]).max() < 2e-5
