"""CLS attention maps, the parts that need no GPU: the library surface of the two new entry points, render_map, the command
line's argument handling, and the sanity of the recorded fixtures."""
import fnmatch
import glob
import os
import re

import numpy as np
import pytest

from cbas_amd import _lib, attention_maps as A, config as C, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cbas_enc_forward_u8_attn", "cbas_enc_forward_f32_attn")
DEBUG = "cbas_debug_cls_attention"


def test_library_surface():
    header = open(os.path.join(REPO, "include", "cbas_mi355x.h")).read()
    debug_header = open(os.path.join(REPO, "include", "cbas_mi355x_debug.h")).read()
    exported = re.search(r"global:\s*([^;]+);", open(os.path.join(REPO, "cbas_amd", "csrc", "exports.map")).read()).group(1).split()
    for name, n_args in zip(NEW, (13, 10)):
        assert re.search(r"\bint %s\(cbas_enc\* h," % name, header), name
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported)
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.c_int and len(args) == n_args
        # the arguments of the form without maps, then the two attention pointers
        assert args[:-2] == _lib.SIGNATURES[name[:-len("_attn")]][1] and args[-2:] == [_lib.c_void_p, _lib.c_void_p]
        assert name not in debug_header
    assert "compare_encoders.py:36-49" in header
    assert DEBUG in _lib.DEBUG_SIGNATURES and DEBUG not in _lib.SIGNATURES
    assert re.search(r"\bint %s\(" % DEBUG, debug_header) and DEBUG not in header
    assert int(re.search(r"#define CBAS_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.EXPECTED_ABI == 11
    readme = open(os.path.join(REPO, "README.md")).read()
    assert f"{len(_lib.SIGNATURES)} entry points" in readme and "cbas_amd.attention_maps" in readme


def test_product_library_exports_the_new_names_and_not_the_debug_one():
    import subprocess
    from cbas_amd import build as B
    path = B.build_library(debug=False)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW) <= names and DEBUG not in names


def test_map_to_bytes_before_the_resize():
    """What render_map hands to the resize (no Pillow needed): a map with max > min reaches 0 and 255, a constant map is
    not normalised - value * 255, truncated - and nothing divides by zero."""
    m = np.linspace(0.03, 0.07, 20, dtype=np.float32).reshape(4, 5)
    u8 = A._to_u8(m)
    assert u8.shape == (4, 5) and u8.dtype == np.uint8 and u8.min() == 0 and u8.max() == 255
    assert u8[0, 0] == 0 and u8[-1, -1] == 255 and (np.diff(u8.reshape(-1).astype(int)) >= 0).all()
    with np.errstate(all="raise"):
        for v, want in ((0.05, 12), (0.0, 0), (1.0, 255)):
            flat = A._to_u8(np.full((3, 3), v, np.float32))
            assert flat.dtype == np.uint8 and (flat == want).all(), (v, np.unique(flat))


def test_render_map_shape_range_and_constant():
    pytest.importorskip("PIL")
    m = np.linspace(0.03, 0.07, 20, dtype=np.float32).reshape(4, 5)
    pic = A.render_map(m, (88, 72))                      # size = (width, height), as Pillow takes it
    assert pic.shape == (72, 88) and pic.dtype == np.uint8
    assert pic[0, 0] <= 2 and pic[-1, -1] >= 253         # the corners of a ramp stay its extremes
    # a constant map: no normalisation and no division by zero - value * 255, truncated, everywhere
    for v, want in ((0.05, 12), (0.0, 0), (1.0, 255)):
        flat = A.render_map(np.full((3, 3), v, np.float32), (30, 20))
        assert flat.shape == (20, 30) and (flat == want).all(), (v, np.unique(flat))
    with pytest.raises(ValueError):
        A.render_map(np.zeros((2, 3, 4), np.float32), (8, 8))


def test_command_line_argument_handling(tmp_path, capsys):
    vid = str(tmp_path / "clip.npy")
    np.save(vid, synth.cage_frames(5, 6, 32, 32))
    out = str(tmp_path / "o.png")
    with pytest.raises(SystemExit) as e:                 # no encoder given
        A.main(["--video", vid, "--frame", "0", "--out", out])
    assert e.value.code == 2 and "--encoder" in capsys.readouterr().err
    for frame in ("6", "-1"):                            # frame index out of range: refused before any encoder is loaded
        with pytest.raises(SystemExit) as e:
            A.main(["--video", vid, "--frame", frame, "--encoder", str(tmp_path / "no_such_checkpoint"), "--out", out])
        assert e.value.code == 2 and "out of range" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        A.main(["--video", str(tmp_path / "missing.npy"), "--frame", "0", "--encoder", "x", "--out", out])
    assert e.value.code == 2 and "no such video" in capsys.readouterr().err
    assert not os.path.exists(out)
    with pytest.raises(ValueError):
        A.compare_encoders(vid, 0, {}, out)


FIXTURES = {"vit_tiny": C.VIT_TINY, "gated_tiny": C.VIT_TINY_GATED, "dinov2reg_tiny": C.DINOV2_REG_TINY,
            "dinov2_tiny": C.DINOV2_TINY, "vitb16": C.VIT_B16}


def test_fixture_sanity(golden_dir):
    found = sorted(os.path.basename(p) for p in glob.glob(os.path.join(golden_dir, "cls_attention_*.npz")))
    assert found == sorted(f"cls_attention_{k}.npz" for k in FIXTURES)
    for name, cfg in FIXTURES.items():
        path = os.path.join(golden_dir, f"cls_attention_{name}.npz")
        assert os.path.getsize(path) < (1 << 20)
        g = np.load(path)
        NP = 1 + cfg.num_register_tokens
        for t in (str(x) for x in g["tags"]):
            n, H, Wd = int(g[f"{t}_n"]), int(g[f"{t}_height"]), int(g[f"{t}_width"])
            heads, mp, cls = g[f"{t}_heads"], g[f"{t}_map"], g[f"{t}_cls"]
            T = cfg.num_tokens(H, Wd)
            assert heads.shape == (n, cfg.num_attention_heads, T) and heads.dtype == np.float32
            assert mp.shape == (n, T - NP) and cls.shape == (n, cfg.hidden_size)
            assert np.abs(heads.astype(np.float64).sum(-1) - 1.0).max() < 1e-5
            assert np.abs(heads[:, :, NP:].astype(np.float64).mean(1) - mp).max() <= 2.0 ** -24 * np.abs(mp).max()
            assert (heads > 0).all() and np.isfinite(cls).all()
    g = np.load(os.path.join(golden_dir, "cls_attention_vit_tiny.npz"))
    assert (int(g["b_height"]) // 16, int(g["b_width"]) // 16) == (4, 5)          # the non-square grid
