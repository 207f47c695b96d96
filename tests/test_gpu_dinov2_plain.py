"""Plain DINOv2 (HF model_type "dinov2": one prefix row, position table resampled without antialiasing) on the GPU, in every
mode the with-registers family runs in.  The device arithmetic is the existing ViT path; what is new on the device is the
1-row prefix (T = 1 + P: 257 at 224^2, 325 at 256^2, 1 370 at 518^2) and the table the patch GEMM's epilogue adds.
Fixtures: tests/golden/make_goldens_dinov2_plain.py (transformers' Dinov2Model, the reference's DinoEncoder + infer_file);
stage taps come from the numpy restatement pinned in tests/test_dinov2_plain_host.py.  The gates are the ones the project
already holds the with-registers family to - no new numbers."""
import functools
import os

import numpy as np
import pytest
import torch

from cbas_amd import _lib, config as C, weights as W, synth
from test_dinov2_plain_host import plain_forward, rel_rows, sha, tiny_case, TABLE_ULPS

pytestmark = pytest.mark.gpu

CLS_TOL = 1e-3              # precision 0 / 1: tests/test_gpu_parity.py CLS_TOL, the gate tests/test_dinov2.py applies
CLS_TOL_F32 = 5e-6          # precision 3 / 4: tests/test_gpu_fp32.py
NAMES = ["eating", "drinking", "rearing", "climbing", "digging", "nesting", "resting", "grooming", "exploring"]
B14_CASES = (("r224", 224, 224), ("r256", 256, 256), ("r252x280", 252, 280), ("r518", 518, 518))


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


@functools.lru_cache(maxsize=1)
def b14_weights():
    return W.synth_encoder_weights(C.DINOV2_B14, 1234)


def make_b14(precision, max_frame=(256, 256), max_batch=4, cfg=C.DINOV2_B14, weights=None):
    from cbas_amd.encoder import DinoEncoder
    return DinoEncoder.from_weights(cfg, weights if weights is not None else b14_weights(), "cuda", max_batch=max_batch,
                                    max_frame=max_frame, precision=precision)


def make_head(dim=768):
    from cbas_amd.head import ClassifierLSTMDeltas
    head = ClassifierLSTMDeltas(dim, 9)
    head.load_state_dict(W.synth_head_weights(C.HeadConfig(in_features=dim), 4321))
    head.to("cuda")
    return head


def encode(enc, frames):
    _, c32 = enc.encode_u8(torch.from_numpy(frames).cuda())
    torch.cuda.synchronize()
    enc.check_finite()
    return c32.cpu().numpy()


@pytest.mark.parametrize("precision", [0, 3, 4])
def test_tiny_stagewise(golden_dir, precision):
    """Every tap of the tiny model at a resampled grid (56 x 84: 4 x 6 patches, a different matrix per axis) and at the native
    grid (the stored table), with NP = 1: the prefix row bit for bit, the position table as the device holds it, the
    embeddings against HF's, then every stage of both layers against the restatement."""
    from cbas_amd.encoder import DinoEncoder
    g = load(golden_dir, "dinov2_tiny")
    cfg = C.DINOV2_TINY
    raw = W.synth_encoder_weights(cfg, 1234)
    w = W.canonical_encoder_weights(cfg, raw)
    D = cfg.hidden_size
    f32 = precision >= 3
    # precision 3 / 4: tests/test_gpu_fp32.py's stagewise 2e-6 and its 2e-5 on the embeddings; precision 0: tests/test_gpu_parity.py's
    # stagewise tolerances and tests/test_dinov2.py's 2e-3 on the embeddings
    tol_x, tol_ln, tol_mm, tol_emb = (2e-6, 2e-6, 2e-6, 2e-5) if f32 else (3e-4, 6e-4, 8e-4, 2e-3)
    enc = DinoEncoder.from_weights(cfg, raw, "cuda", max_batch=4, max_frame=(84, 84), precision=precision)

    def close(got, want, tol, what):
        got, want = got.astype(np.float64), want.reshape(-1, want.shape[-1]).astype(np.float64)
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        assert err < tol, (what, err)
    try:
        for tag in ("r", "n", "r"):                               # back to the first grid: the per-resolution table cache
            fr = tiny_case(g, tag)
            n, H, Wd = fr.shape[:3]
            T = cfg.num_tokens(H, Wd)
            assert T == 1 + (H // 14) * (Wd // 14)
            taps = {}
            last = plain_forward(fr, w, cfg, taps)
            fd = torch.from_numpy(fr).cuda()
            emb = enc.debug_tap(fd, 0, 0, 0).reshape(n, T, D)
            # the prefix row: cls_token + its position embedding, one float32 addition on the host - bit for bit, every frame
            prefix = (w["embeddings.cls_token"].reshape(D) + w["embeddings.position_embeddings"].reshape(-1, D)[0]).astype(np.float32)
            assert all(np.array_equal(emb[f, 0], prefix) for f in range(n)), tag
            assert np.abs(emb - g[f"{tag}_emb"]).max() < tol_emb
            # the position table as the device holds it: a black frame's patch rows are bias + table (the GEMM adds exact zeros)
            black = enc.debug_tap(torch.zeros((1, H, Wd, 3), dtype=torch.uint8, device="cuda"), 0, 0, 0).reshape(T, D)
            bias = w["embeddings.patch_embeddings.bias"].astype(np.float32)
            want_tab = g[f"{tag}_pos"][1:]
            ulp = float(np.spacing(np.float32(np.abs(want_tab).max())))
            tab_err = float(np.abs(black[1:] - (bias + want_tab).astype(np.float32)).max())
            print(f"[precision {precision} tiny {tag}] device table + bias vs HF: max |d| = {tab_err:.3e}")
            # the table's own bound (tests/test_dinov2_plain_host.py) + one rounding of the sum bias + table
            assert tab_err <= TABLE_ULPS * ulp + float(np.spacing(np.float32(np.abs(bias + want_tab).max())))
            if tag == "n":
                assert np.array_equal(black[1:], (bias + w["embeddings.position_embeddings"].reshape(-1, D)[1:]).astype(np.float32))
            for l in range(cfg.num_hidden_layers):
                if precision != 4:        # precision 4 keeps its GEMM / attention operands as split images: the fp32 residual stream only
                    close(enc.debug_tap(fd, l, 1, 1), taps[f"l{l}.ln1"], tol_ln, f"l{l}.ln1")
                    qkv = enc.debug_tap(fd, l, 2, 2).astype(np.float32)
                    close(qkv[:, :D] * 8.0, taps[f"l{l}.q_rope"], tol_mm, f"l{l}.q")        # q is stored pre-scaled by 1/8 (exact)
                    close(qkv[:, D:2 * D], taps[f"l{l}.k_rope"], tol_mm, f"l{l}.k")
                    close(qkv[:, 2 * D:], taps[f"l{l}.v"], tol_mm, f"l{l}.v")
                    close(enc.debug_tap(fd, l, 3, 1), taps[f"l{l}.ctx"], tol_mm, f"l{l}.ctx")
                close(enc.debug_tap(fd, l, 4, 0), taps[f"l{l}.after_attn"], tol_x, f"l{l}.after_attn")
                if precision != 4:
                    close(enc.debug_tap(fd, l, 5, 1), taps[f"l{l}.ln2"], tol_ln, f"l{l}.ln2")
                    close(enc.debug_tap(fd, l, 6, 3), taps[f"l{l}.up"], tol_mm, f"l{l}.up")
                close(enc.debug_tap(fd, l, 7, 0), taps[f"l{l}.out"], tol_x, f"l{l}.out")
            r = rel_rows(encode(enc, fr), g[f"{tag}_last"][:, 0])
            r2 = rel_rows(encode(enc, fr), last[:, 0])
            print(f"[precision {precision} tiny {tag}] CLS rel err max {r.max():.3e} (HF), {r2.max():.3e} (restatement)")
            assert r.max() < (CLS_TOL_F32 if f32 else CLS_TOL)
            # the reference's call form: encoder(x) with float32 frames
            x = torch.from_numpy(fr[:, :, :, 1].astype(np.float32) / np.float32(255.0)).cuda().unsqueeze(1)
            assert rel_rows(enc(x).squeeze(1).cpu().numpy(), g[f"{tag}_last"][:, 0]).max() < (CLS_TOL_F32 if f32 else CLS_TOL)
    finally:
        enc.close()


@pytest.mark.parametrize("precision", [0, 1, 3, 4])
def test_b14_row0_at_four_sizes(golden_dir, precision):
    """ViT-B/14 row 0 against HF Dinov2Model / the reference's wrapper at 224^2 (T = 257), 256^2 (T = 325, CBAS's standard), 252 x 280
    (a different matrix per axis) and 518^2 (T = 1 370, the stored table): <= 5e-6 in precisions 3 and 4, <= 1e-3 in 0 and 1."""
    g = load(golden_dir, "dinov2_b14")
    gate = CLS_TOL_F32 if precision >= 3 else CLS_TOL
    enc = make_b14(precision, max_frame=(518, 518))
    try:
        for tag, H, Wd in B14_CASES:
            n = int(g[f"{tag}_n"])
            fr = synth.cage_frames(int(g[f"{tag}_seed"]), n, H, Wd)
            assert sha(fr) == str(g[f"{tag}_frames_sha"]) and enc.config.num_tokens(H, Wd) == 1 + (H // 14) * (Wd // 14)
            r = rel_rows(encode(enc, fr), g[f"{tag}_cls"])
            print(f"[precision {precision} dinov2_b14 {H}x{Wd}] CLS rel err max {r.max():.3e} (gate {gate:.0e})")
            assert r.max() <= gate, (tag, r.max())
    finally:
        enc.close()


@pytest.mark.parametrize("precision", [0, 3, 4])
def test_batch_position_and_pruning_invariance(precision):
    """A frame's row does not depend on its batch, on its place in it or on the pruned last layer (NP = 1: the CLS-row path reads
    row b * T of a 325-row frame): bit-exact, as for the other families."""
    fr = synth.cage_frames(61, 4, 256, 256)
    enc = make_b14(precision)
    try:
        whole = encode(enc, fr)
        assert np.isfinite(whole).all() and len({whole[i].tobytes() for i in range(4)}) == 4
        for i in range(4):
            assert np.array_equal(encode(enc, fr[i:i + 1])[0], whole[i]), ("batch of one", i)
        perm = [2, 0, 3, 1]
        assert np.array_equal(encode(enc, np.ascontiguousarray(fr[perm])), whole[perm])
        assert np.array_equal(encode(enc, fr[1:3]), whole[1:3])
        enc.set_prune_last_layer(False)
        assert np.array_equal(encode(enc, fr), whole), "full last layer"
        enc.set_prune_last_layer(True)
        # the asynchronous lanes (two batches in flight) give the same rows
        o16 = [torch.empty((2, 768), dtype=torch.float16, device="cuda") for _ in range(2)]
        o32 = [torch.empty((2, 768), dtype=torch.float32, device="cuda") for _ in range(2)]
        fd = torch.from_numpy(fr).cuda()
        for s in range(2):
            enc.submit_dev(s, fd[2 * s:2 * s + 2], o16[s], o32[s])
        for s in range(2):
            enc.wait_stream(s)
        torch.cuda.synchronize()
        assert np.array_equal(torch.cat(o32).cpu().numpy(), whole)
    finally:
        enc.close()


def test_wrong_filter_is_caught(golden_dir):
    """The silent error this family invites: the with-registers table rule (antialiased) on plain-DINOv2 weights.  It is still
    reachable - the with-registers family with no register tokens - and at 256^2 its rows miss the fixture by far more than
    the gate the right rule meets."""
    from dataclasses import replace
    g = load(golden_dir, "dinov2_b14")
    fr = synth.cage_frames(int(g["r256_seed"]), int(g["r256_n"]), 256, 256)
    wrong_cfg = replace(C.DINOV2_REG_B14, num_register_tokens=0)
    enc = make_b14(3, cfg=wrong_cfg)
    try:
        assert enc.config.num_tokens(256, 256) == 325
        r_wrong = rel_rows(encode(enc, fr), g["r256_cls"])
    finally:
        enc.close()
    enc = make_b14(3)
    try:
        r_right = rel_rows(encode(enc, fr), g["r256_cls"])
        # the rule is fixed once a table exists; asking again for the one in force is fine
        assert enc._lib.cbas_enc_set_pos_interp(enc._h, _lib.POS_INTERP_BICUBIC) == 0
        assert enc._lib.cbas_enc_set_pos_interp(enc._h, _lib.POS_INTERP_BICUBIC_AA) == -1
        assert b"before the first batch" in enc._lib.cbas_last_error()
    finally:
        enc.close()
    print(f"[wrong filter] antialiased table on plain weights: CLS rel err {r_wrong.min():.3e} ... {r_wrong.max():.3e}; "
          f"right table {r_right.max():.3e}")
    assert r_right.max() <= CLS_TOL_F32 and r_wrong.min() > 1e3 * CLS_TOL_F32


def test_range_fallback_twin_is_a_plain_dinov2(golden_dir):
    """The precision-3 twin the file paths fall back to keeps the family and its table rule: bit-identical to a precision-3
    encoder built directly.  So does the handle rebuilt for larger frames."""
    g = load(golden_dir, "dinov2_b14")
    fr = synth.cage_frames(int(g["r256_seed"]), int(g["r256_n"]), 256, 256)
    enc4 = make_b14(4, max_frame=(224, 224))
    direct = make_b14(3)
    try:
        want = encode(direct, fr)
        twin = enc4.range_fallback()
        assert twin.precision == 3 and enc4.precision == 4 and twin.config.model_type == "dinov2"
        assert np.array_equal(encode(twin, fr), want)
        assert rel_rows(want, g["r256_cls"]).max() <= CLS_TOL_F32
        # 256 x 256 frames exceed enc4's 224 x 224 workspace: the rebuilt handle must resample the same way
        assert rel_rows(encode(enc4, fr), g["r256_cls"]).max() <= CLS_TOL_F32 and enc4.max_frame == (256, 256)
    finally:
        enc4.close(); direct.close()


def _csv_probs(path):
    lines = open(path).read().splitlines()
    assert lines[0] == ",".join(NAMES)
    return np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]], np.float32)


@pytest.mark.parametrize("precision", ["default", 3, 0])
def test_e2e_checkpoint_directory_through_the_file_paths(golden_dir, tmp_path, monkeypatch, precision):
    """A plain-DINOv2 checkpoint directory the reference's way - DinoEncoder(path), mode from the environment - then
    encode_file + infer_file, encode_infer_file, encode_files and ClipStream on the clip of tests/golden/e2e_dinov2_b14.npz (the
    reference's own wrapper + infer_file; its smallest top-2 margin is >= 1e-3, checked when it was made).  Precisions 4 (the
    default) and 3: EVERY label the reference's, fp16 rows that round differently < 2 % (the with-registers e2e bound);
    precision 0: the <= 1 % near-tie rule."""
    from conftest import assert_labels_match
    from cbas_amd import pipeline as P, h5io, dist as cdist
    from cbas_amd.encoder import DinoEncoder
    from cbas_amd.stream import ClipStream
    g = load(golden_dir, "e2e_dinov2_b14")
    n, hw = int(g["n"]), int(g["hw"])
    assert float(g["min_margin"]) >= 1e-3
    frames = synth.cage_frames(int(g["frame_seed"]), n, hw, hw)
    assert sha(frames) == str(g["frames_sha"])
    ck = str(tmp_path / "dinov2-base")
    W.save_encoder_checkpoint(ck, C.DINOV2_B14, b14_weights())
    if precision == "default":
        monkeypatch.delenv("CBAS_PRECISION", raising=False)
    else:
        monkeypatch.setenv("CBAS_PRECISION", str(precision))
    enc = DinoEncoder(ck, device="cuda", max_batch=32, max_frame=(hw, hw))
    head = make_head()
    try:
        assert enc.config == C.DINOV2_B14 and enc.precision == (4 if precision == "default" else precision)
        for sub in ("a", "b", "c"):
            (tmp_path / sub).mkdir()
            np.save(str(tmp_path / sub / "vid.npy"), frames)
        out = P.encode_file(enc, str(tmp_path / "a" / "vid.npy"))
        with h5io.ClsReader(out) as r:
            assert r.shape == (n, 768)
            rows = r.read(0, n)
        csv = P.infer_file(out, head, "ds", NAMES, 31, device="cuda")
        h5b, csvb = P.encode_infer_file(enc, head, str(tmp_path / "b" / "vid.npy"), "ds", NAMES)
        assert open(out, "rb").read() == open(h5b, "rb").read() and open(csv, "rb").read() == open(csvb, "rb").read()
        recs = cdist.encode_files([str(tmp_path / "c" / "vid.npy")], enc, head=head, dataset_name="ds", behaviors=NAMES)
        assert recs[0]["status"] == "ok" and open(recs[0]["cls_file"], "rb").read() == open(out, "rb").read()
        assert open(recs[0]["csv_file"], "rb").read() == open(csv, "rb").read()
        st = ClipStream(enc, head, capacity=n)
        for i in range(0, n, 32):
            st.push_u8(torch.from_numpy(frames[i:i + 32]).cuda())
        cls16, sprobs = st.finish()
        torch.cuda.synchronize()
        assert np.array_equal(cls16.cpu().numpy(), rows)
        probs = _csv_probs(csv)
        share = float((rows != g["cls_f16"]).mean())
        r = rel_rows(rows[::8].astype(np.float32), g["cls_every8"])
        tag = f"e2e_dinov2_b14 precision {enc.precision}"
        if enc.precision >= 3:
            n_mis, _ = assert_labels_match(probs, g["probs"], 5e-3, margin=0.0)        # margin 0: EVERY frame
            print(f"[{tag}] {n_mis} of {n} labels differ; fp16 rows: {share * 100:.3f} % of elements round differently from the "
                  f"reference's; CLS (f16 rows vs f32 reference) rel err max {r.max():.3e}")
            assert n_mis == 0 and (probs.argmax(1) == g["labels"]).all()
            assert (sprobs.cpu().numpy().argmax(1) == g["labels"]).all()
            assert r.max() < 2.0 ** -11 + 1e-5          # fp16 storage rounding of rows that agree to ~1e-6
            assert share < 2e-2
        else:
            n_mis, _ = assert_labels_match(probs, g["probs"], 5e-2)
            print(f"[{tag}] {n_mis} of {n} labels differ; {share * 100:.1f} % of the fp16 elements differ; CLS rel err max {r.max():.3e}")
            assert r.max() < CLS_TOL + 5e-4
            assert n_mis <= max(2, n // 100)
    finally:
        enc.close(); head.close()
