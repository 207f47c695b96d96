"""Every token's final hidden state, the parts that need no GPU: the library surface of the two entry points, the recorded
fixture against the configurations, the pixel -> token index of a similarity query, and the command line's refusals."""
import os
import re

import numpy as np
import pytest

from cbas_amd import _lib, attention_maps as A, config as C, synth
from cbas_amd.encoder import DinoEncoder, query_token_index, token_grid

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {"vit_tiny": C.VIT_TINY, "gated_tiny": C.VIT_TINY_GATED, "dinov2reg_tiny": C.DINOV2_REG_TINY,
            "dinov2_tiny": C.DINOV2_TINY, "convnext_tiny": C.CONVNEXT_TINY, "vitb16": C.VIT_B16, "convnext_t": C.CONVNEXT_T}


def test_library_surface():
    header = open(os.path.join(REPO, "include", "cbas_mi355x.h")).read()
    debug_header = open(os.path.join(REPO, "include", "cbas_mi355x_debug.h")).read()
    p, i, i64 = _lib.c_void_p, _lib.c_int, _lib.c_int64
    tail = [p, p, i64, p, p, p]          # tokens_f32_dev, tokens_f16_dev, ld_tokens, query_idx_dev, sim_map_dev, stream
    for name, plain in (("cbas_enc_forward_u8_tokens", "cbas_enc_forward_u8"), ("cbas_enc_forward_f32_tokens", "cbas_enc_forward_f32")):
        decl = re.search(r"\bint %s\(([^;]+)\);" % name, header)
        assert decl, name
        res, args = _lib.SIGNATURES[name]
        assert res is i and len(args) == decl.group(1).count(",") + 1
        # the frames exactly as the CLS form takes them (everything before its three trailing cls_f32 / cls_f16 / stream), then the tail
        assert args == _lib.SIGNATURES[plain][1][:-3] + tail
        assert re.search(r"float\* tokens_f32_dev, uint16_t\* tokens_f16_dev, int64_t ld_tokens,\s+const int32_t\* query_idx_dev, "
                         r"float\* sim_map_dev, void\* stream$", decl.group(1)), decl.group(1)
        assert name not in debug_header
    assert int(re.search(r"#define CBAS_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.EXPECTED_ABI == 11
    ops = dict(re.findall(r"(CBAS_DEBUG_ROWS_\w+) = (\d+)", debug_header))
    assert ops["CBAS_DEBUG_ROWS_CNX_POOL_LN"] == "10" and ops["CBAS_DEBUG_ROWS_TOKEN_ROWS"] == "11" and ops["CBAS_DEBUG_ROWS_TOKEN_SIM"] == "12"
    readme = open(os.path.join(REPO, "README.md")).read()
    assert f"{len(_lib.SIGNATURES)} entry points" in readme and "hidden_state" in readme
    for method in ("hidden_state", "patch_tokens", "similarity_map"):
        assert callable(getattr(DinoEncoder, method))


def test_product_library_exports_the_new_names():
    import subprocess
    from cbas_amd import build as B
    path = B.build_library(debug=False)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"cbas_enc_forward_u8_tokens", "cbas_enc_forward_f32_tokens"} <= names


def test_fixture_matches_the_configurations(golden_dir):
    path = os.path.join(golden_dir, "hidden_state.npz")
    assert os.path.getsize(path) < 1_000_000
    g = np.load(path)
    assert sorted(str(x) for x in g["names"]) == sorted(FIXTURES)
    for name, cfg in FIXTURES.items():
        n, H, Wd = (int(g[f"{name}_{k}"]) for k in ("n", "height", "width"))
        nh, nw, P0 = token_grid(cfg, H, Wd)
        T = P0 + nh * nw
        if C.is_convnext(cfg):
            assert (nh, nw) == cfg.stage_grids(H, Wd)[-1] and P0 == 1
        else:
            assert T == cfg.num_tokens(H, Wd) and P0 == 1 + cfg.num_register_tokens
        rows, hidden = g[f"{name}_rows"], g[f"{name}_hidden"]
        assert hidden.shape == (n, len(rows), cfg.hidden_size) and hidden.dtype == np.float32 and np.isfinite(hidden).all()
        assert rows[0] == 0 and (np.diff(rows) > 0).all() and rows[-1] < T
        assert set(range(P0 + 1)) <= set(rows.tolist())                    # the prefix rows and the first patch: always kept
        if name in ("vitb16", "convnext_t"):
            assert (n, H, Wd) == (1, 224, 224) and set(range(P0, T, 7)) <= set(rows.tolist())
        else:
            assert n == 3 and len(rows) == T and (nh != nw or name == "convnext_tiny")
    assert token_grid(C.VIT_TINY, 72, 88) == (4, 5, 5) and token_grid(C.DINOV2_REG_TINY, 72, 88) == (5, 6, 5)
    assert token_grid(C.CONVNEXT_TINY, 72, 88) == (2, 2, 1) and token_grid(C.CONVNEXT_T, 224, 224) == (7, 7, 1)


def test_query_pixel_to_token_index():
    # (config, H, W, pixel) -> index: prefix rows first, then the grid in row-major order, cell = patch size (ConvNeXt: 32)
    cases = [(C.VIT_B16, 224, 224, (0, 0), 5), (C.VIT_B16, 224, 224, (15, 15), 5), (C.VIT_B16, 224, 224, (16, 0), 5 + 14),
             (C.VIT_B16, 224, 224, (223, 223), 5 + 195), (C.VIT_TINY, 72, 88, (63, 79), 5 + 19), (C.VIT_TINY, 72, 88, (20, 50), 5 + 5 + 3),
             (C.DINOV2_REG_TINY, 72, 88, (14, 13), 5 + 6), (C.DINOV2_REG_TINY, 72, 88, (69, 83), 5 + 29),
             (C.DINOV2_TINY, 72, 88, (14, 14), 1 + 7), (C.DINOV2_B14, 224, 224, (223, 0), 1 + 15 * 16),
             (C.CONVNEXT_TINY, 72, 88, (0, 0), 1), (C.CONVNEXT_TINY, 72, 88, (63, 63), 4), (C.CONVNEXT_TINY, 72, 88, (31, 32), 2),
             (C.CONVNEXT_T, 224, 224, (100, 200), 1 + 3 * 7 + 6)]
    for cfg, H, Wd, px, want in cases:
        assert query_token_index(cfg, H, Wd, px) == want, (cfg.model_type, px)
        assert query_token_index(cfg, H, Wd, None) == 0
    # pixels of the margin whole patches leave uncovered, and pixels outside the frame, have no token
    for cfg, H, Wd, px in ((C.VIT_TINY, 72, 88, (64, 0)), (C.VIT_TINY, 72, 88, (0, 80)), (C.DINOV2_TINY, 72, 88, (70, 0)),
                           (C.CONVNEXT_TINY, 72, 88, (64, 0)), (C.CONVNEXT_TINY, 72, 88, (0, 64)), (C.VIT_B16, 224, 224, (-1, 0)),
                           (C.VIT_B16, 224, 224, (0, 224))):
        with pytest.raises(ValueError, match="outside"):
            query_token_index(cfg, H, Wd, px)


def test_command_line_kinds(tmp_path, capsys):
    vid = str(tmp_path / "clip.npy")
    np.save(vid, synth.cage_frames(5, 4, 64, 64))
    out = str(tmp_path / "o.png")
    cnx, vit = tmp_path / "cnx", tmp_path / "vit"
    for d, cfg in ((cnx, C.CONVNEXT_TINY), (vit, C.VIT_TINY)):
        d.mkdir()
        (d / "config.json").write_text(cfg.to_json())
    base = ["--video", vid, "--frame", "0", "--out", out]
    for extra in ([], ["--kind", "attention"]):                  # refused from the config alone: no weights are read, no GPU is touched
        with pytest.raises(SystemExit) as e:
            A.main(base + ["--encoder", str(cnx)] + extra)
        err = capsys.readouterr().err
        assert e.value.code == 2 and "ConvNeXt" in err and "similarity" in err
    with pytest.raises(SystemExit) as e:                         # one ConvNeXt among ViTs is enough
        A.main(base + ["--encoder", str(vit), "--encoder", str(cnx)])
    assert e.value.code == 2 and "similarity" in capsys.readouterr().err
    for bad, msg in ((["--kind", "attention", "--query", "3,4"], "--kind similarity"), (["--kind", "similarity", "--query", "3"], "Y,X"),
                     (["--kind", "similarity", "--query", "a,b"], "Y,X"), (["--kind", "cosine"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            A.main(base + ["--encoder", str(vit)] + bad)
        assert e.value.code == 2 and msg in capsys.readouterr().err
    assert not os.path.exists(out)
    assert A.refuse_kind(C.CONVNEXT_T, "similarity") is None and A.refuse_kind(C.VIT_B16, "attention") is None
    assert "similarity" in A.refuse_kind(C.CONVNEXT_T, "attention")

    class Enc:
        config = C.CONVNEXT_TINY
    with pytest.raises(ValueError, match="similarity"):          # frame_maps refuses before it opens the video
        A.frame_maps(Enc(), vid, [0], kind="attention")
