"""Patch-feature k-means, the parts that need no GPU: the library surface, the float64 reference's own checks (a planted partition
is recovered, the inertia never rises, duplicate rows tie to the lowest index, an emptied cluster keeps its centroid), where the
default number of rounds comes from, and the refusals of ``PatchClusters``, ``render_labels`` and the command line.

The default rounds: on the tiny encoders' recorded hidden states (tests/golden/hidden_state.npz, every
family, per frame and as one batch, k = 2, 3, 4, 8, both normalisations) the labels stop changing after at most 2 rounds; on rows
whose clusters touch (patch_kmeans_ref.tiny_patch_rows, 320 rows, k = 2 .. 16) after at most 8.  The smallest power of two that
covers both is 8, doubled for real features: 16."""
import os
import re

import numpy as np
import pytest
import torch

import patch_kmeans_ref as R
from cbas_amd import _lib, attention_maps as A, config as C, synth
from cbas_amd.encoder import KMEANS_DEFAULT_ITERS, DinoEncoder, PatchClusters

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_surface():
    header = open(os.path.join(REPO, "include", "cbas_mi355x.h")).read()
    debug_header = open(os.path.join(REPO, "include", "cbas_mi355x_debug.h")).read()
    ctype = {"int": _lib.c_int, "int64_t": _lib.c_int64, "int32_t*": _lib.c_void_p, "float*": _lib.c_void_p, "void*": _lib.c_void_p}
    for name, res in (("cbas_patch_kmeans_workspace_bytes", _lib.c_int64), ("cbas_patch_kmeans_fit", _lib.c_int),
                      ("cbas_patch_kmeans_assign", _lib.c_int)):
        decl = re.search(r"\b(?:int|int64_t) %s\(([^;]+)\);" % name, header)
        assert decl, name
        r, args = _lib.SIGNATURES[name]
        declared = [ctype[re.sub(r"\bconst\s+", "", a.strip()).rsplit(" ", 1)[0].replace(" *", "*")] for a in decl.group(1).split(",")]
        assert r is res and args == declared and name not in debug_header, name
    assert int(re.search(r"#define CBAS_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.EXPECTED_ABI == 11
    assert "#define CBAS_KMEANS_FRAME CBAS_PCA_FRAME" in header and "#define CBAS_KMEANS_BATCH CBAS_PCA_BATCH" in header
    assert int(re.search(r"#define CBAS_KMEANS_CHUNK (\d+)", header).group(1)) == _lib.KMEANS_CHUNK == R.CHUNK
    assert int(re.search(r"#define CBAS_KMEANS_MAX_K (\d+)", header).group(1)) == _lib.KMEANS_MAX_K == R.MAX_K == len(A.LABEL_PALETTE)
    kernels_h = open(os.path.join(REPO, "cbas_amd", "csrc", "kernels.h")).read()
    for name, val in (("KMEANS_CHUNK", _lib.KMEANS_CHUNK), ("KMEANS_MAX_K", _lib.KMEANS_MAX_K)):
        assert int(re.search(r"\b%s = (\d+)" % name, kernels_h).group(1)) == val
    from cbas_amd import build as B
    assert "patch_kmeans.hip" in B.SOURCES and B.EXTRA_FLAGS["patch_kmeans.hip"] == B.NO_PACKED
    readme = open(os.path.join(REPO, "README.md")).read()
    assert f"{len(_lib.SIGNATURES)} entry points" in readme and "patch_clusters" in readme
    assert "## 18." in open(os.path.join(REPO, "DESIGN.md")).read()
    assert callable(DinoEncoder.patch_clusters)


@pytest.mark.parametrize("k,normalize", [(2, 0), (5, 1), (16, 0)])
def test_reference_recovers_a_planted_partition(k, normalize):
    X, planted = R.planted(5 + k, k, 40 * k, 32)
    out = R.fit(X, k, 3, normalize)
    # the same partition, named by size: planted blob j is the j-th largest, and so is output cluster j
    assert np.array_equal(out["labels"], planted) and (np.diff(out["counts"]) < 0).all()
    assert out["counts"].tolist() == np.bincount(planted).tolist()
    assert out["margin"] > 1.0 and out["seed_margin"] > 0
    assert sorted(planted[out["init_index"]].tolist()) == list(range(k))       # farthest-point seeding: one seed per blob


def test_reference_inertia_never_rises_and_empty_clusters_stay():
    for s in range(4):
        X = R.tiny_patch_rows(s, 200, 32)
        for normalize in (0, 1):
            inertia = R.fit(X, 6, 12, normalize)["inertia"]
            assert (np.diff(inertia) <= 1e-9 * inertia[0]).all(), inertia
    # three distinct points, k = 3 seeds of which two coincide: the duplicate seed owns no row and keeps its centroid
    U = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 0.0], [0.0, 0.0]])
    out = R.lloyd(U, [0, 1, 2], 2)
    assert out["counts"].tolist() == [2, 2, 0] and np.array_equal(out["seeding_centroids"][2], U[2])
    assert out["order"].tolist() == [0, 1, 2] and out["labels"].tolist() == [0, 1, 1, 0]


def test_reference_ties_go_to_the_lowest_index():
    X = np.array([[1.0, 0.0], [5.0, 0.0], [5.0, 0.0], [1.0, 0.0], [-3.0, 0.0], [9.0, 0.0]])
    chosen, _ = R.seed(X, 2)
    # the mean is 3: rows 4 and 5 are both 6 away and the lower one is taken; then row 5, the farthest from row 4
    assert chosen == [4, 5]
    lab, _ = R.assign(X, np.array([[1.0, 0.0], [1.0, 0.0], [5.0, 0.0]]))
    assert lab.tolist() == [0, 2, 2, 0, 0, 2]                                   # centroids 0 and 1 coincide: 0 wins
    lab, _ = R.assign(np.array([[3.0, 0.0]]), np.array([[1.0, 0.0], [5.0, 0.0]]))
    assert lab.tolist() == [0]                                                   # equidistant: the lowest
    assert R.working_rows(np.array([[0.0, 0.0], [3.0, 4.0]]), 1).tolist() == [[0.0, 0.0], [0.6, 0.8]]


def test_default_rounds():
    z = np.load(os.path.join(REPO, "tests", "golden", "hidden_state.npz"))
    worst_golden = 0
    for name in z["names"]:
        H = z[f"{name}_hidden"]
        for X in [H.reshape(-1, H.shape[-1])] + list(H):
            for k in (2, 3, 4, 8):
                if k <= len(X):
                    worst_golden = max(worst_golden, max(R.rounds_until_stable(X, k, nz) for nz in (0, 1)))
    worst_touching = max(R.rounds_until_stable(R.tiny_patch_rows(s, 320, 128), k, 1) for s in range(6) for k in (2, 4, 8, 16))
    print(f"rounds until the labels stop changing: recorded tiny-encoder rows {worst_golden}, touching clusters {worst_touching}")
    worst = max(worst_golden, worst_touching)
    # the rule that chose the default: half of it is the smallest power of two that covers every fixture, a quarter does not
    assert KMEANS_DEFAULT_ITERS == 16 and KMEANS_DEFAULT_ITERS // 4 < worst <= KMEANS_DEFAULT_ITERS // 2


def _clusters(b=1, k=4, D=64, scope="batch", stamp="enc@p4", iters=3):
    return PatchClusters(torch.zeros(b, k, D), torch.zeros(b, k, dtype=torch.int32), torch.zeros(b, iters + 1),
                         torch.zeros(b, k, dtype=torch.int32), scope, True, stamp)


def test_clusters_refusals():
    cl = _clusters()
    assert (cl.n_sets, cl.n_clusters, cl.dim, cl.normalize, cl.scope) == (1, 4, 64, True, "batch")
    cl.check(64, "enc@p4")
    with pytest.raises(ValueError, match="width 64"):
        cl.check(96, "enc@p4")
    with pytest.raises(ValueError, match="fitted on encoder"):
        cl.check(64, "other@p4")
    with pytest.raises(ValueError, match="fitted on encoder"):
        cl.check(64, "enc@p0")                                             # the same checkpoint in another precision is another encoder
    with pytest.raises(ValueError, match="scope"):
        _clusters(scope="clip")
    with pytest.raises(ValueError, match="one set"):
        _clusters(b=2, scope="batch")
    with pytest.raises(ValueError, match="a cluster set is"):
        PatchClusters(torch.zeros(1, 4, 64), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(1, 2), torch.zeros(1, 4, dtype=torch.int32),
                      "frame", True, "s")
    assert _clusters(b=2, scope="frame").n_sets == 2


def test_render_and_command_line(tmp_path, capsys):
    lab = np.array([[0, 1, 1], [2, 15, 0]], np.int32)
    pic = A.render_labels(lab, (30, 20))
    assert pic.shape == (20, 30, 3) and pic.dtype == np.uint8
    # nearest neighbour: every pixel is one of the palette's colours, a cell is one colour, the same label is the same colour
    assert np.array_equal(pic[0, 0], A.LABEL_PALETTE[0]) and np.array_equal(pic[19, 29], A.LABEL_PALETTE[0])
    assert np.array_equal(pic[15, 15], A.LABEL_PALETTE[15]) and np.array_equal(pic[3, 12], A.LABEL_PALETTE[1])
    assert {tuple(c) for c in pic.reshape(-1, 3)} == {tuple(A.LABEL_PALETTE[j]) for j in (0, 1, 2, 15)}
    assert len({tuple(c) for c in A.LABEL_PALETTE}) == 16
    with pytest.raises(ValueError, match="integer labels"):
        A.render_labels(np.zeros((2, 3), np.float32), (30, 20))
    with pytest.raises(ValueError, match="integer labels"):
        A.render_labels(np.zeros((2, 3, 1), np.int32), (30, 20))
    with pytest.raises(ValueError, match="outside"):
        A.render_labels(np.full((2, 3), 16, np.int32), (30, 20))
    assert "clusters" in A.KINDS and A.refuse_kind(C.CONVNEXT_T, "clusters") is None and A.refuse_kind(C.VIT_B16, "clusters") is None
    vid = str(tmp_path / "clip.npy")
    np.save(vid, synth.cage_frames(5, 4, 64, 64))
    vit = tmp_path / "vit"
    vit.mkdir()
    (vit / "config.json").write_text(C.VIT_TINY.to_json())
    base = ["--video", vid, "--frame", "0", "--out", str(tmp_path / "o.png"), "--encoder", str(vit)]
    for bad, msg in ((["--cluster-scope", "batch"], "--kind clusters"), (["--clusters", "3"], "--kind clusters"),
                     (["--kind", "pca", "--clusters", "3"], "--kind clusters"), (["--kind", "clusters", "--cluster-scope", "clip"], "invalid choice"),
                     (["--kind", "clusters", "--clusters", "1"], "2 .. 16"), (["--kind", "clusters", "--clusters", "17"], "2 .. 16"),
                     (["--kind", "clusters", "--pca-scope", "batch"], "--kind pca"), (["--kind", "clusters", "--query", "1,2"], "--kind similarity")):
        with pytest.raises(SystemExit) as e:
            A.main(base + bad)
        assert e.value.code == 2 and msg in capsys.readouterr().err, bad
    _, a = A.parse_cli(base + ["--kind", "clusters", "--clusters", "5", "--cluster-scope", "batch"])
    assert (a.kind, a.clusters, a.cluster_scope) == ("clusters", 5, "batch")

    class Enc:
        config = C.VIT_TINY
    with pytest.raises(ValueError, match="scope"):
        A.frame_maps(Enc(), vid, [0], kind="clusters", cluster_scope="clip")
