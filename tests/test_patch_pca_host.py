"""Patch-feature PCA, the parts that need no GPU: the float64 restatement of the device's fit against numpy.linalg.eigh on every
fixture the GPU tests use (which is where the default number of rounds comes from), the fixtures' own eigenvalue-ratio condition,
the sign rule, the library surface and the refusals of ``PatchPCABasis`` and of the command line.

The default rounds: the smallest power of two at which every fixture's sine is <= 1e-9 in float64 is 32
(16 rounds: 1.7e-7; 32 rounds: 1.5e-13, the level of eigh itself), doubled for real features' narrower gaps: 64."""
import os
import re

import numpy as np
import pytest
import torch

import patch_pca_ref as R
from cbas_amd import _lib, attention_maps as A, config as C, synth
from cbas_amd.encoder import PCA_DEFAULT_ITERS, DinoEncoder, PatchPCABasis

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINE_GATE = 1e-9


@pytest.fixture(scope="module")
def fits():
    """(D, k, M) -> (eigh eigenvalues, eigh components, the whole spectrum, C) of every eigenpair fixture, computed once."""
    out = {}
    for case in R.EIGEN_CASES:
        _, Cm = R.covariance64(R.eigen_fixture(*case)[:, :case[0]])
        out[case] = R.eigh_topk(Cm, case[1]) + (Cm,)
    return out


def test_default_rounds_meet_the_gate_on_every_fixture(fits):
    worst = {}
    for (D, k, M), (w, V, _, Cm) in fits.items():
        for iters in (PCA_DEFAULT_ITERS // 4, PCA_DEFAULT_ITERS // 2, PCA_DEFAULT_ITERS):
            lam, comp = R.subspace_fit(Cm, k, iters)
            s = float(R.sines(comp, V).max())
            worst[iters] = max(worst.get(iters, 0.0), s)
            if iters == PCA_DEFAULT_ITERS:
                print(f"D {D} k {k} M {M}: sine {s:.2e}  eigenvalue error {np.abs(lam - w).max() / w[0]:.2e}")
                assert s <= SINE_GATE, (D, k, M, s)
                assert np.abs(lam - w).max() <= 1e-12 * w[0]
    print("worst sine by rounds:", {i: f"{s:.2e}" for i, s in worst.items()})
    # the rule that chose the default: half of it is the smallest power of two inside the gate, a quarter is outside
    assert PCA_DEFAULT_ITERS == 64 and worst[PCA_DEFAULT_ITERS // 2] <= SINE_GATE < worst[PCA_DEFAULT_ITERS // 4]


def test_fixtures_keep_their_eigenvalue_ratio(fits):
    for (D, k, M), (_, _, spectrum, _) in fits.items():
        top = spectrum[:k + 1]
        ratios = top[:-1] / np.maximum(top[1:], np.finfo(np.float64).tiny)
        assert ratios.min() >= 2.0, (D, k, M, ratios)
        # and the mean is what makes an uncentred fit fail: its square dwarfs the leading eigenvalue
        X = R.eigen_fixture(D, k, M)[:, :D].astype(np.float64)
        assert np.linalg.norm(X.mean(axis=0)) ** 2 > 50 * spectrum[0]


def test_start_pattern_and_sign_rule():
    P = R.start_pattern(1536, 8)
    assert P.shape == (8, 1536) and (np.abs(P) < 1).all() and np.linalg.matrix_rank(P) == 8
    assert (P * 2.0 ** 23 == np.round(P * 2.0 ** 23)).all()                 # 24-bit values: exact in fp32
    c = R.sign_rule(np.array([[1.0, -3.0, 2.0], [-2.0, 2.0, 1.0], [0.5, 1.0, -1.0], [0.0, 0.0, 0.0]]))
    assert c.tolist() == [[-1.0, 3.0, -2.0], [2.0, -2.0, -1.0], [0.5, 1.0, -1.0], [0.0, 0.0, 0.0]]      # ties: the lowest index decides
    Q = R.mgs(R.mgs(P[:, :96]))
    assert np.abs(Q @ Q.T - np.eye(8)).max() < 1e-14


def test_library_surface():
    header = open(os.path.join(REPO, "include", "cbas_mi355x.h")).read()
    debug_header = open(os.path.join(REPO, "include", "cbas_mi355x_debug.h")).read()
    for name, res in (("cbas_patch_pca_workspace_bytes", _lib.c_int64), ("cbas_patch_pca_fit", _lib.c_int), ("cbas_patch_pca_project", _lib.c_int)):
        decl = re.search(r"\b(?:int|int64_t) %s\(([^;]+)\);" % name, header)
        assert decl, name
        r, args = _lib.SIGNATURES[name]
        assert r is res and len(args) == decl.group(1).count(",") + 1 and name not in debug_header
    assert int(re.search(r"#define CBAS_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.EXPECTED_ABI == 11
    assert (int(re.search(r"#define CBAS_PCA_FRAME (\d)", header).group(1)), int(re.search(r"#define CBAS_PCA_BATCH (\d)", header).group(1))) \
        == (_lib.PCA_FRAME, _lib.PCA_BATCH)
    kernels_h = open(os.path.join(REPO, "cbas_amd", "csrc", "kernels.h")).read()
    for name, val in (("PCA_CHUNK", _lib.PCA_CHUNK), ("PCA_MEAN_CHUNK", _lib.PCA_MEAN_CHUNK), ("PCA_MAX_K", _lib.PCA_MAX_K), ("PCA_MAX_D", _lib.PCA_MAX_D)):
        assert int(re.search(r"\b%s = (\d+)" % name, kernels_h).group(1)) == val
    assert (R.CHUNK, R.MEAN_CHUNK) == (_lib.PCA_CHUNK, _lib.PCA_MEAN_CHUNK)
    from cbas_amd import build as B
    assert "patch_pca.hip" in B.SOURCES and B.EXTRA_FLAGS["patch_pca.hip"] == B.NO_PACKED
    readme = open(os.path.join(REPO, "README.md")).read()
    assert f"{len(_lib.SIGNATURES)} entry points" in readme and "patch_pca" in readme
    assert "## 16." in open(os.path.join(REPO, "DESIGN.md")).read()
    assert callable(DinoEncoder.patch_pca)


def _basis(b=1, k=3, D=64, scope="batch", stamp="enc@p4"):
    return PatchPCABasis(torch.zeros(b, D), torch.zeros(b, k, D), torch.ones(b, k), torch.full((b,), 4.0), scope, stamp)


def test_basis_refusals():
    bs = _basis()
    assert (bs.n_bases, bs.n_components, bs.dim) == (1, 3, 64)
    assert bs.explained_variance_ratio.shape == (1, 3) and float(bs.explained_variance_ratio.sum()) == 0.75
    bs.check(64, "enc@p4")
    with pytest.raises(ValueError, match="width 64"):
        bs.check(96, "enc@p4")
    with pytest.raises(ValueError, match="fitted on encoder"):
        bs.check(64, "other@p4")
    with pytest.raises(ValueError, match="fitted on encoder"):
        bs.check(64, "enc@p0")                                             # the same checkpoint in another precision is another encoder
    with pytest.raises(ValueError, match="scope"):
        _basis(scope="clip")
    with pytest.raises(ValueError, match="one basis"):
        _basis(b=2, scope="batch")
    with pytest.raises(ValueError, match="a basis is"):
        PatchPCABasis(torch.zeros(1, 64), torch.zeros(1, 3, 32), torch.ones(1, 3), torch.ones(1), "frame", "s")
    assert _basis(b=2, scope="frame").n_bases == 2


def test_render_and_command_line(tmp_path, capsys):
    rng = np.random.default_rng(3)
    pic = A.render_pca(rng.standard_normal((4, 5, 3)).astype(np.float32), (80, 64))
    assert pic.shape == (64, 80, 3) and pic.dtype == np.float32 and pic.min() >= 0.0 and pic.max() <= 1.0 and pic.max() > 0.9
    flat = A.render_pca(np.ones((4, 5, 3), np.float32), (80, 64))
    assert (flat == 0).all()                                               # a constant component has no range to stretch
    with pytest.raises(ValueError, match="k >= 3"):
        A.render_pca(np.ones((4, 5, 2), np.float32), (80, 64))
    assert "pca" in A.KINDS and A.refuse_kind(C.CONVNEXT_T, "pca") is None and A.refuse_kind(C.VIT_B16, "pca") is None
    assert "pca" in A.refuse_kind(C.CONVNEXT_T, "attention")
    vid = str(tmp_path / "clip.npy")
    np.save(vid, synth.cage_frames(5, 4, 64, 64))
    vit = tmp_path / "vit"
    vit.mkdir()
    (vit / "config.json").write_text(C.VIT_TINY.to_json())
    base = ["--video", vid, "--frame", "0", "--out", str(tmp_path / "o.png"), "--encoder", str(vit)]
    for bad, msg in ((["--pca-scope", "batch"], "--kind pca"), (["--kind", "pca", "--pca-scope", "clip"], "invalid choice"),
                     (["--kind", "pca", "--query", "1,2"], "--kind similarity")):
        with pytest.raises(SystemExit) as e:
            A.main(base + bad)
        assert e.value.code == 2 and msg in capsys.readouterr().err

    class Enc:
        config = C.VIT_TINY
    with pytest.raises(ValueError, match="scope"):
        A.frame_maps(Enc(), vid, [0], kind="pca", pca_scope="clip")
