"""DINOv3 ConvNeXt encoders (family 1 of cbas_enc; cbas_amd/csrc/convnext_f32.hip + the fp32 / split GEMMs) in precision 3
and 4 against transformers' DINOv3ConvNextModel run in fp32 on the CPU (tests/golden/make_goldens_convnext.py): stage by stage
on a tiny config, row 0 of ConvNeXt-T, batch invariance, the file paths end to end through a checkpoint directory, the range
fallback and the refusals."""
import os

import numpy as np
import pytest
import torch

from cbas_amd import config as C, weights as W, synth

pytestmark = pytest.mark.gpu

CLS_TOL_F32 = 5e-6          # per-frame ||d||2 / ||ref||2 against the reference's fp32 CPU rows (the ViT modes' bar)
PRECISIONS = (3, 4)
NAMES = ["eating", "drinking", "rearing", "climbing", "digging", "nesting", "resting", "grooming", "exploring"]


def rel_rows(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def make_enc(cfg, hw, max_batch, precision, weights=None):
    from cbas_amd.encoder import DinoEncoder
    w = weights if weights is not None else W.synth_convnext_weights(cfg, 1234)
    return DinoEncoder.from_weights(cfg, w, "cuda", max_batch=max_batch, max_frame=hw, precision=precision)


def make_head(dim):
    from cbas_amd.head import ClassifierLSTMDeltas
    head = ClassifierLSTMDeltas(dim, 9)
    head.load_state_dict(W.synth_head_weights(C.HeadConfig(in_features=dim), 4321))
    head.to("cuda")
    return head


@pytest.mark.parametrize("precision", PRECISIONS)
def test_convnext_tiny_stagewise(golden_dir, precision):
    """Stem (+ its LayerNorm), every stage's output and row 0 of a tiny ConvNeXt (widths 32 / 64 / 128 / 256: every GEMM N below
    the 128-column tile), at 64 x 64 and at 72 x 88 (odd grids: the downsamples drop the last row / column)."""
    from cbas_amd import _lib
    _lib.require_debug("ConvNeXt taps")
    g = load(golden_dir, "convnext_tiny")
    cfg = C.CONVNEXT_TINY
    for tag in ("a", "b"):
        H, W_ = int(g[f"{tag}_height"]), int(g[f"{tag}_width"])
        frames = synth.cage_frames(int(g["frame_seed"]), int(g["n"]), H, W_)
        enc = make_enc(cfg, (H, W_), 4, precision)
        try:
            fr = torch.from_numpy(frames).cuda()
            for stop, key in ((0, "stem"), (1, "stage0"), (2, "stage1"), (3, "stage2"), (4, "stage3")):
                got = enc.debug_tap(fr, stop, 0, 4 + stop)
                ref = g[f"{tag}_{key}"]
                assert got.shape == ref.shape, (tag, key)
                err = np.abs(got - ref).max() / np.abs(ref).max()
                assert err < 2e-5, (tag, key, err)
            _, c32 = enc.encode_u8(fr)
            torch.cuda.synchronize()
            r = rel_rows(c32.cpu().numpy(), g[f"{tag}_row0"])
            print(f"[p{precision} tiny {tag}] row 0 rel max {r.max():.2e}")
            assert r.max() < CLS_TOL_F32
        finally:
            enc.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_convnext_t_row0(golden_dir, precision):
    """ConvNeXt-T row 0 within 5e-6 of the reference's fp32 CPU rows, at 224^2, 256^2 and 250 x 250."""
    g = load(golden_dir, "convnext_t")
    cfg = C.CONVNEXT_T
    enc = make_enc(cfg, (256, 256), 8, precision)
    try:
        for tag in ("r224", "r256", "r250"):
            n, S = int(g[f"{tag}_n"]), int(g[f"{tag}_size"])
            frames = synth.cage_frames(int(g[f"{tag}_seed"]), n, S, S)
            _, c32 = enc.encode_u8(torch.from_numpy(frames).cuda())
            torch.cuda.synchronize()
            r = rel_rows(c32.cpu().numpy(), g[f"{tag}_cls"])
            print(f"[p{precision} ConvNeXt-T {tag}] per-frame rel {np.array2string(r, precision=2)}")
            assert r.max() < CLS_TOL_F32, (tag, r)
    finally:
        enc.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_convnext_batch_invariance(precision):
    """A frame's row is bit-identical alone, at position 5 of 7 and in a batch of 64 (different GEMM kernels by M)."""
    cfg = C.CONVNEXT_T
    enc = make_enc(cfg, (224, 224), 64, precision)
    try:
        frames = torch.from_numpy(synth.cage_frames(9, 64, 224, 224)).cuda()
        big16, big32 = enc.encode_u8(frames)
        mid16, mid32 = enc.encode_u8(frames[:7])
        one16, one32 = enc.encode_u8(frames[5:6])
        torch.cuda.synchronize()
        assert torch.equal(one32[0], mid32[5]) and torch.equal(one32[0], big32[5])
        assert torch.equal(one16[0], mid16[5]) and torch.equal(one16[0], big16[5])
        assert torch.isfinite(big32).all()
    finally:
        enc.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_convnext_reference_call_matches_u8_path(precision):
    """encoder(t), t float32 (B, 1, H, W) in [0, 1] (backend/cbas.py:672-677) -> (B, 1, 768), equal to the u8 path's rows."""
    cfg = C.CONVNEXT_T
    enc = make_enc(cfg, (224, 224), 8, precision)
    try:
        frames = synth.cage_frames(12, 6, 224, 224)
        t = torch.from_numpy(frames[:, :, :, 1] / 255.0).float().unsqueeze(1)
        out = enc(t)
        _, c32 = enc.encode_u8(torch.from_numpy(frames).cuda())
        torch.cuda.synchronize()
        assert tuple(out.shape) == (6, 1, 768)
        assert torch.equal(out[:, 0], c32)
    finally:
        enc.close()


def _ckpt(tmp_path, cfg, w):
    d = str(tmp_path / "dinov3-convnext-tiny-pretrain-lvd1689m")
    W.save_encoder_checkpoint(d, cfg, w)
    return d


@pytest.mark.parametrize("precision", PRECISIONS)
def test_convnext_e2e_file_paths_labels_identical(golden_dir, tmp_path, precision, monkeypatch):
    """e2e_convnext_t.npz (the reference's own DinoEncoder + infer_file, 512 frames at 256^2): DinoEncoder(<checkpoint dir>)
    + encode_infer_file (fused session) and encode_file + infer_file - f16 rows as the reference's, every label identical,
    the `_cls.h5` stamped with the model identifier."""
    from conftest import assert_labels_match
    from cbas_amd import pipeline as P, h5io
    from cbas_amd.encoder import DinoEncoder
    g = load(golden_dir, "e2e_convnext_t")
    cfg = C.CONVNEXT_T
    n, S = int(g["n"]), int(g["height"])
    frames = synth.cage_frames(int(g["frame_seed"]), n, S, S)
    ckpt = _ckpt(tmp_path, cfg, W.synth_convnext_weights(cfg, 1234))
    monkeypatch.setenv("CBAS_PRECISION", str(precision))
    enc = DinoEncoder(ckpt, device="cuda", max_frame=(S, S))
    head = make_head(768)
    P.set_project_stamp(ckpt)
    try:
        assert enc.precision == precision
        for sub in ("a", "b"):
            (tmp_path / sub).mkdir()
            np.save(str(tmp_path / sub / "vid.npy"), frames)
        h5a, csva = P.encode_infer_file(enc, head, str(tmp_path / "a" / "vid.npy"), "ds", NAMES)
        h5b = P.encode_file(enc, str(tmp_path / "b" / "vid.npy"))
        csvb = P.infer_file(h5b, head, "ds", NAMES, 31)
        for h5 in (h5a, h5b):
            with h5io.ClsReader(h5) as r:
                rows = r.read(0, n)
                assert r.attrs.get("encoder_model_identifier") == ckpt
            ref16 = g["cls_f16"]
            differ = rows != ref16
            d = np.abs(rows.astype(np.float32) - ref16.astype(np.float32))
            print(f"[p{precision}] f16 elements differing from the reference's: {differ.mean() * 100:.4f} %, max |d| {d.max():.2e}")
            # where a row differs it is by one rounding step of the fp16 store (rows agree to ~3e-7 before it; near zero the
            # subnormal steps are smaller than that agreement, hence the absolute term)
            assert (d <= np.spacing(np.abs(ref16)).astype(np.float32) + 2e-6).all()
            assert differ.mean() < 1e-2
        import pandas as pd
        for csv in (csva, csvb):
            probs = pd.read_csv(csv).to_numpy(dtype=np.float64).astype(np.float32)
            n_mis, _ = assert_labels_match(probs, g["probs"], 5e-3, margin=0.0)     # margin 0: EVERY frame
            assert n_mis == 0
            assert (probs.argmax(1) == g["labels"]).all()
        # the f32 rows of every 8th frame against the reference's
        _, c32 = enc.encode_u8(torch.from_numpy(frames[::8]).cuda())
        torch.cuda.synchronize()
        assert rel_rows(c32.cpu().numpy(), g["cls_every8"]).max() < CLS_TOL_F32
    finally:
        P.set_project_stamp(None)
        enc.close(); head.close()


def test_convnext_range_fallback_is_a_convnext(tmp_path, capsys):
    """A precision-4 ConvNeXt whose GELU output leaves the split operands' range (one pointwise_conv1 bias at 4e4) re-encodes
    the file in precision 3 OF THE SAME FAMILY: rows bit-identical to a precision-3 ConvNeXt encoder's for the same weights."""
    from cbas_amd import pipeline as P, h5io
    cfg = C.CONVNEXT_TINY
    w = {k: v.copy() for k, v in W.synth_convnext_weights(cfg, 1234).items()}
    w["model.stages.0.layers.0.pointwise_conv1.bias"][3] = 40000.0       # GELU(40 000) x 4 overflows the fp16 high half
    w["model.stages.0.layers.0.pointwise_conv2.weight"][:, 3] *= 1e-4
    frames = synth.cage_frames(3, 40, 64, 64)
    enc = make_enc(cfg, (64, 64), 16, 4, weights=w)
    ref = make_enc(cfg, (64, 64), 16, 3, weights=w)
    try:
        np.save(str(tmp_path / "vid.npy"), frames)
        out = P.encode_file(enc, str(tmp_path / "vid.npy"))
        assert "re-encoded in precision 3" in capsys.readouterr().out
        twin = enc.range_fallback()
        assert twin.precision == 3 and twin._cfg_c.family == 1
        with h5io.ClsReader(out) as r:
            rows = r.read(0, 40)
        r16, _ = ref.encode_u8(torch.from_numpy(frames).cuda())
        torch.cuda.synchronize()
        assert np.array_equal(rows.view(np.uint16), r16.cpu().numpy().view(np.uint16))
    finally:
        enc.close(); ref.close()


def test_convnext_refusals():
    """Widths that are not multiples of 32 and precisions outside {3, 4} come back as CBAS_EINVAL with a message."""
    import ctypes
    from cbas_amd import _lib
    lib = _lib.load()

    def create(widths, precision):
        depths = (1, 1, 1, 1)
        cfg = _lib.EncConfig(hidden_size=widths[3], layer_norm_eps=1e-6, max_batch=2, max_height=64, max_width=64,
                             precision=precision, family=1, stage_widths=(ctypes.c_int32 * 4)(*widths),
                             stage_depths=(ctypes.c_int32 * 4)(*depths))
        n = lib.cbas_enc_weights_count(ctypes.byref(cfg))
        blob = np.zeros(max(int(n), 1), np.float32)
        h = ctypes.c_void_p()
        rc = lib.cbas_enc_create(ctypes.byref(cfg), blob.ctypes.data, int(n), 0, ctypes.byref(h))
        if rc == 0:
            lib.cbas_enc_destroy(h)
        return rc, lib.cbas_last_error().decode()

    rc, msg = create((48, 64, 128, 256), 4)
    assert rc == -1 and "multiple of 32" in msg
    rc, msg = create((32, 64, 128, 256), 0)
    assert rc == -1 and "precision 3" in msg
    rc, msg = create((32, 64, 128, 256), 3)
    assert rc == 0, msg
