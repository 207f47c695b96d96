"""The host side of the linear probe over resident CLS rows: the library surface, the float64 restatement against itself (central
differences, Nesterov's theorem), and the parts of cbas_amd.probe that need no GPU."""
import os
import re
import types

import numpy as np
import pytest
import torch

import rows_probe_ref as R
from cbas_amd import _lib, knn, probe, search as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cbas_rows_probe_workspace_bytes", "cbas_rows_probe_fit", "cbas_rows_probe_predict")


planted = R.planted


# ---- the library surface -----------------------------------------------------------------------------------------------------------
def test_signatures_header_and_readme():
    from ctypes import c_float, c_int, c_int32, c_int64, c_void_p
    for name in NAMES:
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES[NAMES[0]] == (c_int64, [c_int64, c_int32, c_int32])
    res, args = _lib.SIGNATURES[NAMES[1]]
    assert res is c_int and len(args) == 17 and args[:9] == [c_void_p, c_int64, c_int32, c_int64, c_void_p, c_void_p, c_int32, c_float, c_int32]
    assert args[9:15] == [c_void_p] * 6 and args[15:] == [c_int64, c_void_p]
    res, args = _lib.SIGNATURES[NAMES[2]]
    assert res is c_int and args == [c_void_p, c_int64, c_int32, c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]
    with open(os.path.join(ROOT, "include", "cbas_mi355x.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\(", header), name
    assert re.search(r"#define CBAS_ROWS_PROBE_SEGMENT (\d+)", header).group(1) == str(probe.SEGMENT) == str(R.SEGMENT)
    assert re.search(r"#define CBAS_ABI_VERSION\s+11\b", header)                  # additive entry points: the version stays
    with open(os.path.join(ROOT, "cbas_amd", "csrc", "exports.map")) as f:
        assert "cbas_*" in f.read()
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert f"{len(_lib.SIGNATURES)} entry points" in readme and "cbas_amd.probe" in readme
    from cbas_amd import build
    assert "rows_probe.hip" in build.SOURCES and build.EXTRA_FLAGS["rows_probe.hip"] == build.NO_PACKED
    assert os.path.exists(os.path.join(build.CSRC, "rows_probe.hip")) and R.TILE == probe.TILE


# ---- the restatement against itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_gradient_against_central_differences(weighted):
    rng, x, y = planted(3, 60, 32, 5)
    x[7] = 0                                                                    # a zero row: only the bias sees it
    omega = rng.uniform(0.0, 2.0, 60) * (rng.random(60) > 0.2) if weighted else None
    W, b, l2 = 0.3 * rng.standard_normal((5, 32)), 0.3 * rng.standard_normal(5), 1e-2
    gW, gb = R.gradient(x, y, omega, W, b, l2)
    h = 1e-6
    for c, d in ((0, 0), (2, 17), (4, 31)):
        Wp, Wm = W.copy(), W.copy()
        Wp[c, d] += h
        Wm[c, d] -= h
        num = (R.objective(x, y, omega, Wp, b, l2) - R.objective(x, y, omega, Wm, b, l2)) / (2 * h)
        assert abs(num - gW[c, d]) <= 1e-8 * max(1.0, abs(num))
    for c in range(5):
        bp, bm = b.copy(), b.copy()
        bp[c] += h
        bm[c] -= h
        num = (R.objective(x, y, omega, W, bp, l2) - R.objective(x, y, omega, W, bm, l2)) / (2 * h)
        assert abs(num - gb[c]) <= 1e-8 * max(1.0, abs(num))
    probs, z = R.predict(x, W, b)
    assert np.abs(probs.sum(axis=1) - 1).max() < 1e-12 and np.array_equal(z[7], b)      # the zero row's logits are the bias


def test_fit_meets_the_theorem():
    """The documented (l2, iters) of the GPU convergence test, on its data: the float64 restatement itself is inside the bound."""
    C, D, l2, iters = 16, 96, 1e-2, 80
    _, x, y = planted(11, 3 * R.SEGMENT + 37, D, C)
    omega = R.balanced(y, C)[y]
    fstar, _, _ = R.optimum(x, y, omega, l2, C)
    W, b, loss = R.fit(x, y, omega, l2, iters, C=C)
    f0 = R.objective(x, y, omega, np.zeros((C, D)), np.zeros(C), l2)
    bound = R.theorem_bound(l2, iters, f0, fstar)
    assert loss.shape == (iters + 1,) and abs(loss[0] - f0) < 1e-12 and abs(f0 - np.log(C)) < 1e-12
    assert 0 <= loss[-1] - fstar <= bound and 1e-4 < bound < 5e-3
    L, inv_l, beta = R.constants(l2)
    assert L == 1.01 and abs(inv_l * L - 1) < 1e-15 and 0 < beta < 1
    # iters = 0 returns the start and its loss
    W0, b0, l0 = R.fit(x[:50], y[:50], None, l2, 0, W0=W, b0=b)
    assert np.array_equal(W0, W) and l0.shape == (1,)


def test_planted_project_is_separable_in_float64():
    """The data of the GPU suite's report test: the float64 restatement predicts every frame, and every held-out entry, correctly."""
    C, D, stride, folds, l2, iters = 4, 64, 2, 3, 1e-3, 100
    rows_of, labels_of = R.planted_project(5, (300, 420, 260), D, C)
    x, y, group = R.project_bank(rows_of, labels_of, stride)
    assert len(y) == 490 and group.max() == 48 and sorted(set(y.tolist())) == [0, 1, 2, 3]
    W, b, _ = R.fit(x, y, R.balanced(y, C)[y], l2, iters, C=C)
    z = R.logits(np.concatenate(rows_of), W, b)
    part = np.partition(z, -2, axis=1)
    assert np.array_equal(z.argmax(axis=1), np.concatenate(labels_of))
    assert (part[:, -1] - part[:, -2]).min() > 100 * R.logit_bound(np.concatenate(rows_of), W, b).max()       # far from any tie
    fold_of = R.deal_folds(group, folds)
    for f in range(folds):
        hold = fold_of == f
        om = np.where(hold, 0.0, R.balanced(y[~hold], C)[y])
        W, b, _ = R.fit(x, y, om, l2, iters, C=C)
        z = R.logits(x[hold], W, b)
        part = np.partition(z, -2, axis=1)
        assert np.array_equal(z.argmax(axis=1), y[hold]) and (part[:, -1] - part[:, -2]).min() > 100 * R.logit_bound(x[hold], W, b).max()


def test_bounds_are_small_and_positive():
    rng = np.random.default_rng(8)
    for D, C in ((32, 2), (768, 64), (1536, 17)):
        x = rng.standard_normal((6, D)).astype(np.float16)
        x[3] = 0
        y = rng.integers(0, C, 6)
        W, b = rng.standard_normal((C, D)) / np.sqrt(D), rng.standard_normal(C)
        dz, dp = R.logit_bound(x, W, b), R.prob_bound(x, W, b)
        assert dz.shape == dp.shape == (6, C) and (dz[3] == 0).all() and (np.delete(dz, 3, axis=0) > 0).all() and dz.max() < 1e-3
        assert (dp > 0).all() and dp.max() < 1e-3
        dW, db = R.gradient_bound(x, y, None, W, b, 1e-3)
        assert dW.shape == (C, D) and db.shape == (C,) and (db > 0).all() and max(dW.max(), db.max()) < 1e-3
        assert 0 < R.loss_bound(x, y, None, W, b, 1e-3) < 1e-2
    assert R.g(10) > 10 * R.E


# ---- cbas_amd.probe without a GPU ----------------------------------------------------------------------------------------------------
def test_probe_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    a = probe.LinearProbe(rng.standard_normal((3, 32)), rng.standard_normal(3), ["rear", "groom: face", "eat"], 32, 1e-3, 7,
                          rng.standard_normal(8), [1.0, 0.0, 2.5])
    path = str(tmp_path / "p.npz")
    a.save(path)
    b = probe.LinearProbe.load(path)
    assert b.weights.tobytes() == a.weights.tobytes() and b.weights.dtype == np.float32 and b.bias.tobytes() == a.bias.tobytes()
    assert b.behaviors == a.behaviors and (b.dim, b.l2, b.iters, b.n_classes) == (32, 1e-3, 7, 3)
    assert b.loss.tobytes() == a.loss.tobytes() and b.class_weights.tolist() == [1.0, 0.0, 2.5]
    c = probe.LinearProbe(a.weights, a.bias, a.behaviors, 32, 1e-3, 7, a.loss)
    c.save(path)
    assert probe.LinearProbe.load(path).class_weights is None
    with pytest.raises(ValueError, match="width"):
        probe.LinearProbe(np.zeros((3, 16)), np.zeros(3), ["a", "b", "c"], 32, 1e-3, 0, [0.0])
    with pytest.raises(ValueError, match="class_weights"):
        probe.LinearProbe(np.zeros((3, 32)), np.zeros(3), ["a", "b", "c"], 32, 1e-3, 0, [0.0], [1.0, 2.0])


def test_balanced_weights_with_an_empty_class():
    labels = np.array([0, 0, 0, 2, 2, 3])
    w = probe.balanced_weights(labels, 5)
    assert w.dtype == np.float32 and np.allclose(w, [6 / 15, 0, 6 / 10, 6 / 5, 0]) and np.allclose(w, R.balanced(labels, 5))
    omega, cw = probe.sample_weights(labels, 5)
    assert np.array_equal(cw, w) and np.array_equal(omega, w[labels]) and omega.dtype == np.float32
    hold = np.array([False, False, True, False, False, True])                   # class 3 has no entry that trains
    omega, cw = probe.sample_weights(labels, 5, "balanced", hold)
    assert np.allclose(cw, [4 / 10, 0, 4 / 10, 0, 0]) and omega[2] == 0 and omega[5] == 0 and np.allclose(omega[[0, 3]], [0.4, 0.4])
    assert probe.sample_weights(labels, 5, None) == (None, None)
    omega, cw = probe.sample_weights(labels, 5, None, hold)
    assert cw is None and omega.tolist() == [1, 1, 0, 1, 1, 0]
    omega, cw = probe.sample_weights(labels, 5, [1, 2, 3, 4, 5])
    assert omega.tolist() == [1, 1, 1, 3, 3, 4]
    for bad in ("uniform", [1, 2, 3], [1, 2, 3, -1, 5], [1, 2, 3, np.nan, 5]):
        with pytest.raises(ValueError, match="class_weights"):
            probe.sample_weights(labels, 5, bad)
    with pytest.raises(ValueError, match="holdout"):
        probe.sample_weights(labels, 5, None, np.zeros(5, bool))
    with pytest.raises(ValueError, match="holdout"):
        probe.sample_weights(labels, 5, None, np.zeros(6, np.int64))


def test_fold_dealing():
    groups = np.array([9, 4, 4, 30, 9, 7, 12, 30])                              # sorted ids 4 7 9 12 30 -> folds 0 1 2 0 1 (3 folds)
    assert probe.deal_folds(groups, 3).tolist() == [2, 0, 0, 1, 2, 1, 0, 1] == R.deal_folds(groups, 3).tolist()
    assert probe.deal_folds(groups, 5).tolist() == [2, 0, 0, 4, 2, 1, 3, 4]
    rng = np.random.default_rng(1)
    many = rng.integers(-5, 40, 300)
    for folds in (2, 5, 7):
        assert np.array_equal(probe.deal_folds(many, folds), R.deal_folds(many, folds))
    for bad in (1, 0, 6):
        with pytest.raises(ValueError, match="folds"):
            probe.deal_folds(groups, bad)
        with pytest.raises(ValueError, match="folds"):
            R.deal_folds(groups, bad)


def test_cli_parser():
    _, a = probe.parse_cli(["--dir", "rec", "--instances", "l.csv", "--report", "r.json"])
    assert (a.dir, a.instances, a.l2, a.iters, a.stride, a.group, a.folds, a.report, a.save, a.load, a.write_outputs) == \
        ("rec", "l.csv", 1e-4, 1000, 1, "instance", 5, "r.json", None, None, None)
    _, a = probe.parse_cli(["--files", "a_cls.h5", "b_cls.h5", "--labels-yaml", "l.yaml", "--project-root", "p", "--l2", "1e-3", "--iters", "50",
                            "--stride", "4", "--group", "file", "--folds", "3", "--save", "p.npz", "--write-outputs", "probe"])
    assert a.files == ["a_cls.h5", "b_cls.h5"] and (a.l2, a.iters, a.stride, a.group, a.folds, a.save, a.write_outputs) == \
        (1e-3, 50, 4, "file", 3, "p.npz", "probe")
    _, a = probe.parse_cli(["--dir", "rec", "--load", "p.npz", "--write-outputs", "probe"])          # --load needs no labels
    assert a.load == "p.npz" and a.instances is None and a.labels_yaml is None
    for bad in (["--dir", "rec", "--instances", "l.csv"],                                            # nothing to do
                ["--instances", "l.csv", "--report", "r.json"],                                      # no rows
                ["--dir", "rec", "--report", "r.json"],                                              # no labels, no probe
                ["--dir", "rec", "--load", "p.npz", "--report", "r.json"],                           # a report needs labels
                ["--dir", "rec", "--load", "p.npz", "--save", "q.npz"],
                ["--dir", "rec", "--load", "p.npz", "--instances", "l.csv", "--save", "q.npz"],
                ["--dir", "rec", "--labels-yaml", "l.yaml", "--report", "r.json"],                   # no --project-root
                ["--dir", "rec", "--instances", "l.csv", "--labels-yaml", "l.yaml", "--project-root", "p", "--report", "r.json"],
                ["--dir", "rec", "--instances", "l.csv", "--report", "r.json", "--l2", "0"],
                ["--dir", "rec", "--instances", "l.csv", "--report", "r.json", "--l2", "nan"],
                ["--dir", "rec", "--instances", "l.csv", "--report", "r.json", "--iters", "-1"],
                ["--dir", "rec", "--instances", "l.csv", "--report", "r.json", "--stride", "0"],
                ["--dir", "rec", "--instances", "l.csv", "--report", "r.json", "--folds", "1"],
                ["--dir", "rec", "--instances", "l.csv", "--report", "r.json", "--group", "clip"]):
        with pytest.raises(SystemExit):
            probe.parse_cli(bad)


def fake_index(device="cpu", dim=8, n=40):
    return types.SimpleNamespace(device=torch.device(device), dim=dim, n_rows=n, files=["a_cls.h5"], _table=np.array([[0, n]], np.int64))


def fake_bank(label, group, dim=8, behaviors=("a", "b", "c")):
    label = np.asarray(label, np.int32)
    return knn.LabelBank(torch.zeros((label.size, dim), dtype=torch.float16), torch.from_numpy(label),
                         None if group is None else torch.from_numpy(np.asarray(group, np.int32)), None, np.arange(label.size), behaviors, dim,
                         None if group is None else "instance")


def test_report_plumbing_through_a_stub(monkeypatch):
    """Every entry is predicted exactly once, by the probe of the fold that held it out; the report is report_from_predictions'."""
    label = np.array([0, 0, 1, 1, 2, 2, 0, 1, 2, 0])
    group = np.array([5, 5, 6, 6, 7, 7, 8, 9, 10, 11])                         # 7 groups -> 3 folds: 5 8 11 | 6 9 | 7 10
    bank, index = fake_bank(label, group), fake_index()
    fits = []

    def fit_stub(idx, bk, l2, iters, class_weights, holdout):
        assert idx is index and bk is bank and (l2, iters, class_weights) == (1e-3, 9, None)
        fits.append(np.array(holdout, copy=True))
        return len(fits) - 1                                                    # the "probe": the number of its fold

    def predict_stub(rows, fitted):
        assert rows is bank.rows
        # a held-out entry gets its own label - but for entry 4, which is given class 0; an entry that trained gets a wrong one: any
        # prediction taken from a probe that trained on the entry shows
        out = np.zeros((label.size, 3), np.float32)
        hold = fits[fitted]
        guess = np.where(hold, label, (label + 1) % 3)
        guess[4] = 0
        out[np.arange(label.size), guess] = 1.0
        return out

    monkeypatch.setattr(probe, "fit_probe", fit_stub)
    monkeypatch.setattr(probe, "predict_rows", predict_stub)
    report = probe.probe_report(index, bank, folds=3, l2=1e-3, iters=9, class_weights=None)
    assert len(fits) == 3 and np.array_equal(np.sum(fits, axis=0), np.ones(10))                      # every entry held out once
    assert [np.flatnonzero(h).tolist() for h in fits] == [[0, 1, 6, 9], [2, 3, 7], [4, 5, 8]]
    want = label.copy()
    want[4] = 0
    assert report == knn.report_from_predictions(label, want, bank.behaviors)
    assert report["accuracy"] == 0.9 and report["confusion_matrix"][2][0] == 1 and set(report) >= {"a", "b", "c", "macro avg", "weighted avg"}
    with pytest.raises(ValueError, match="folds"):
        probe.probe_report(index, bank, folds=8)
    with pytest.raises(ValueError, match="folds"):
        probe.probe_report(index, bank, folds=1)
    with pytest.raises(ValueError, match="group"):
        probe.probe_report(index, fake_bank(label, None), folds=3)


def test_refusals_without_a_gpu():
    index, bank = fake_index(), fake_bank([0, 1, 2, 0], [0, 1, 2, 3])
    fitted = probe.LinearProbe(np.zeros((3, 8)), np.zeros(3), ["a", "b", "c"], 8, 1e-4, 0, [0.0])
    with pytest.raises(RuntimeError, match="GPU"):
        probe.fit_probe(index, bank)
    with pytest.raises(RuntimeError, match="GPU"):
        probe.probe_labels(index, fitted)
    with pytest.raises(ValueError, match="GPU"):
        probe.predict_rows(bank.rows, fitted)
    assert "bank" in S.FrameIndex.linear_probe.__code__.co_varnames and "probe" in S.FrameIndex.probe_labels.__code__.co_varnames
    with pytest.raises(ValueError, match="init of shapes"):
        probe._start((np.zeros((3, 4)), np.zeros(3)), 3, 8)
    with pytest.raises(ValueError, match="finite"):
        probe._start((np.full((3, 8), np.inf), np.zeros(3)), 3, 8)
    w, b = probe._start(fitted, 3, 8)
    assert w.dtype == np.float32 and w.shape == (3, 8) and probe._start(None, 3, 8) == (None, None)
