"""The host side of the k-means over resident CLS rows: the float64 restatement against brute force, the library surface, and the
parts of cbas_amd.motifs that need no GPU."""
import os
import re
import types

import numpy as np
import pytest
import torch

import rows_kmeans_ref as R
from cbas_amd import _lib, motifs, postprocess, search as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cbas_rows_kmeans_workspace_bytes", "cbas_rows_kmeans_fit", "cbas_rows_kmeans_assign")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [0, 1])
def test_assign_against_brute_force(normalize):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((40, 32)).astype(np.float16)
    x[7] = 0
    cent = rng.standard_normal((5, 32))
    labels, dist2, gap = R.assign(x, cent, normalize)
    want, want_d2 = R.brute_assign(x, cent, normalize)
    assert np.array_equal(labels, want) and np.abs(dist2 - want_d2).max() < 1e-12 and (gap >= 0).all()


def test_ties_go_to_the_lowest():
    x = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 3, 0], [0, 0, 3, 0]], np.float64)
    cent = np.array([[0, 0, 0, 1], [1, 1, 0, 0], [1, 1, 0, 0]], np.float64)          # centroids 1 and 2 coincide
    assert R.assign(x, cent, 0)[0].tolist() == [1, 1, 1, 0, 0]
    picks = R.seed(x, 3, 0)
    assert picks[0] == 3                                                             # rows 3 and 4 tie: the lowest
    assert R.order([5, 9, 9, 0]).tolist() == [1, 2, 0, 3]


def test_lloyd_keeps_an_empty_cluster_and_orders_by_count():
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.standard_normal((30, 8)) * 0.1 + 5, rng.standard_normal((10, 8)) * 0.1 - 5])
    c0 = np.stack([np.full(8, -5.0), np.full(8, 100.0), np.full(8, 5.0)])
    out = R.lloyd(x, c0, 3, 0)
    assert out["counts"].tolist() == [30, 10, 0] and out["order"].tolist() == [2, 0, 1]
    assert np.array_equal(out["centroids"][2], c0[1]) and np.array_equal(out["cur"][1], c0[1])
    assert np.bincount(out["labels"], minlength=3).tolist() == [30, 10, 0] and out["inertia"].shape == (4,)
    assert (np.diff(out["inertia"]) <= 1e-12).all()
    brute = np.stack([x[:30].mean(axis=0), x[30:].mean(axis=0)])
    assert np.abs(out["centroids"][:2] - brute).max() < 1e-12


def test_fit_recovers_planted_groups():
    rng = np.random.default_rng(6)
    proto = rng.standard_normal((4, 16)) * 3
    group = np.repeat(np.arange(4), (40, 25, 10, 5))
    x = (proto[group] + 0.05 * rng.standard_normal((80, 16))).astype(np.float16)
    for normalize in (0, 1):
        out = R.fit(x, 4, 5, normalize)
        assert out["counts"].tolist() == [40, 25, 10, 5] and sorted(group[out["init_index"]].tolist()) == [0, 1, 2, 3]
        assert np.array_equal(out["labels"], group)


def test_bounds_are_small_and_grow_with_the_width():
    rng = np.random.default_rng(8)
    for D in (32, 768, 1536):
        x = rng.standard_normal((6, D)).astype(np.float16)
        c = rng.standard_normal((3, D)) / np.sqrt(D)
        b = R.score_bound(x, c, 1)
        assert b.shape == (6, 3) and (b > 0).all() and b.max() < 1e-3
    assert R.g(10) > 10 * R.E and R.TILE == motifs.TILE and R.SEGMENT == motifs.SEGMENT


# ---- the library surface -----------------------------------------------------------------------------------------------------------
def test_signatures_header_and_readme():
    from ctypes import c_int, c_int32, c_int64, c_void_p
    for name in NAMES:
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES[NAMES[0]] == (c_int64, [c_int64, c_int32, c_int32])
    res, args = _lib.SIGNATURES[NAMES[1]]
    assert res is c_int and len(args) == 17 and args[:7] == [c_void_p, c_int64, c_int32, c_int64, c_int32, c_int32, c_int32]
    assert args[7:15] == [c_void_p] * 8 and args[15:] == [c_int64, c_void_p]
    res, args = _lib.SIGNATURES[NAMES[2]]
    assert res is c_int and args == [c_void_p, c_int64, c_int32, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]
    with open(os.path.join(ROOT, "include", "cbas_mi355x.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\(", header), name
    assert re.search(r"#define CBAS_ROWS_KMEANS_SEGMENT (\d+)", header).group(1) == str(motifs.SEGMENT)
    assert re.search(r"#define CBAS_ABI_VERSION\s+11\b", header)                  # additive entry points: the version stays
    with open(os.path.join(ROOT, "README.md")) as f:
        assert f"{len(_lib.SIGNATURES)} entry points" in f.read()
    from cbas_amd import build
    assert "rows_kmeans.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "rows_kmeans.hip"))


# ---- cbas_amd.motifs without a GPU ---------------------------------------------------------------------------------------------------
def test_clusters_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    a = motifs.FrameClusters(rng.standard_normal((3, 32)), [9, 5, 1], [3.0, 2.0], [("a_cls.h5", 4), ("b:c_cls.h5", 0), ("a_cls.h5", 7)], 32, True)
    path = str(tmp_path / "c.npz")
    a.save(path)
    b = motifs.FrameClusters.load(path)
    assert b.centroids.tobytes() == a.centroids.tobytes() and b.centroids.dtype == np.float32 and b.counts.tolist() == [9, 5, 1]
    assert b.inertia.tolist() == [3.0, 2.0] and b.seed_rows == a.seed_rows and b.dim == 32 and b.normalize is True and b.n_clusters == 3
    c = motifs.FrameClusters(a.centroids, a.counts, a.inertia, None, 32, False)
    c.save(path)
    d = motifs.FrameClusters.load(path)
    assert d.seed_rows is None and d.normalize is False
    with pytest.raises(ValueError, match="width"):
        motifs.FrameClusters(np.zeros((3, 16)), [1, 1, 1], [0.0], None, 32, True)
    assert motifs.motif_names(3) == ["motif_00", "motif_01", "motif_02"]


def test_cli_parser():
    _, a = motifs.parse_cli(["--dir", "rec", "--clusters", "12", "--out", "f.csv"])
    assert (a.dir, a.clusters, a.iters, a.no_normalize, a.smooth, a.load, a.save, a.runs, a.exemplars, a.write_outputs) == \
        ("rec", 12, 20, False, 1, None, None, None, None, None)
    _, a = motifs.parse_cli(["--files", "a_cls.h5", "b_cls.h5", "--load", "c.npz", "--out", "f.csv", "--no-normalize", "--smooth", "5", "--runs",
                             "r.csv", "--exemplars", "e.csv", "--write-outputs", "m", "--iters", "3", "--save", "s.npz"])
    assert a.files == ["a_cls.h5", "b_cls.h5"] and a.load == "c.npz" and a.clusters is None and a.no_normalize and a.smooth == 5
    assert (a.runs, a.exemplars, a.write_outputs, a.iters, a.save) == ("r.csv", "e.csv", "m", 3, "s.npz")
    for bad in (["--dir", "rec", "--out", "f.csv"], ["--dir", "rec", "--clusters", "4", "--load", "c.npz", "--out", "f.csv"],
                ["--dir", "rec", "--clusters", "1", "--out", "f.csv"], ["--dir", "rec", "--clusters", "65", "--out", "f.csv"],
                ["--dir", "rec", "--clusters", "4", "--out", "f.csv", "--smooth", "4"], ["--dir", "rec", "--clusters", "4", "--out", "f.csv", "--iters", "-1"],
                ["--dir", "rec", "--clusters", "4"], ["--clusters", "4", "--out", "f.csv"]):
        with pytest.raises(SystemExit):
            motifs.parse_cli(bad)


def test_runs_host_arithmetic():
    rng = np.random.default_rng(9)
    table = np.array([(0, 50), (50, 3), (53, 0), (53, 40)], np.int64)
    labels = np.repeat(rng.integers(0, 4, 31), 3)[:93]
    for w, least in ((1, 1), (5, 1), (5, 4), (7, 2)):
        runs = motifs.runs_host(labels, table, w, least)
        assert len(runs) == 4 and runs[2] == []
        for (first, n), got in zip(table, runs):
            smooth = postprocess.median_host(labels[first:first + n], w)
            want = [(lab, a, b) for a, b, lab, _ in postprocess.label_runs_host(smooth, np.ones(n, np.float32)) if b - a + 1 >= least]
            assert got == want and all(0 <= a <= b < n for _, a, b in got)
        if least == 1:                                                       # the bouts of a file tile it: no bout crosses a file
            assert [sum(b - a + 1 for _, a, b in r) for r in runs] == [50, 3, 0, 40]


def fake_index(device="cpu", dim=64, n=10):
    return types.SimpleNamespace(device=torch.device(device), dim=dim, n_rows=n, files=["a_cls.h5"], _table=np.array([[0, n]], np.int64))


def test_refusals_without_a_gpu():
    index = fake_index()
    with pytest.raises(RuntimeError, match="GPU"):
        motifs.cluster_frames(index, n_clusters=4)
    clusters = motifs.FrameClusters(np.zeros((4, 64)), np.zeros(4), np.zeros(1), None, 64, True)
    with pytest.raises(RuntimeError, match="GPU"):
        motifs.cluster_frames(index, clusters=clusters)
    with pytest.raises(RuntimeError, match="GPU"):
        motifs.motif_runs(index, np.zeros(10, np.int32), clusters)
    assert S.FrameIndex.cluster is not None and "clusters" in S.FrameIndex.cluster.__code__.co_varnames
    with pytest.raises(ValueError, match="odd"):
        motifs._smoothing(4, 4)
    with pytest.raises(ValueError, match="classes"):
        motifs._smoothing(3, postprocess.MAX_CLASSES + 1)
    with pytest.raises(ValueError, match="init of shape"):
        motifs._init_centroids(index, np.zeros((4, 32)), 4)
    with pytest.raises(ValueError, match="finite"):
        motifs._init_centroids(index, np.full((4, 64), np.nan), 4)
    # transition counts are integer torch ops: they run wherever the labels are
    idx = types.SimpleNamespace(device=torch.device("cpu"), n_rows=7, _table=np.array([[0, 4], [4, 0], [4, 3]], np.int64))
    t = motifs.transition_counts(idx, np.array([0, 1, 1, 2, 2, 0, 0]), 3)
    assert t.tolist() == [[1, 1, 0], [0, 1, 1], [1, 0, 0]]
    with pytest.raises(ValueError, match="label outside"):
        motifs.transition_counts(idx, np.array([0, 1, 1, 2, 2, 0, 3]), 3)
