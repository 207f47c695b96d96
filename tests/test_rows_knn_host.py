"""The k-NN labels over resident CLS rows, the parts that need no GPU: the library surface, knn.LabelBank.from_instances on files
written with h5io, the report's arithmetic against a hand-worked confusion matrix, the command line, the naming of the output
files, and the select / vote64 restatements of rows_knn_ref against brute-force loops."""
import math
import os
import re

import numpy as np
import pytest

import rows_knn_ref as K
from cbas_amd import _lib, h5io, knn, search as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_surface():
    header = open(os.path.join(REPO, "include", "cbas_mi355x.h")).read()
    ctype = {"int64_t": _lib.c_int64, "int32_t": _lib.c_int32, "float": _lib.c_float, "void*": _lib.c_void_p, "int32_t*": _lib.c_void_p,
             "float*": _lib.c_void_p}
    for name, res in (("cbas_rows_knn_workspace_bytes", _lib.c_int64), ("cbas_rows_knn", _lib.c_int)):
        decl = re.search(r"\b(?:int|int64_t) %s\(([^;]+)\);" % name, header)
        assert decl, name
        r, args = _lib.SIGNATURES[name]
        declared = [ctype[re.sub(r"\bconst\s+", "", a.strip()).rsplit(" ", 1)[0].replace(" *", "*")] for a in decl.group(1).split(",")]
        assert r is res and args == declared, name
        assert name not in open(os.path.join(REPO, "include", "cbas_mi355x_debug.h")).read()
    assert len(_lib.SIGNATURES["cbas_rows_knn"][1]) == 21
    for word in ("excluded", "neighbours", "the vote", "(2 D + 8) 2^-24", "SYNCHRONISES"):
        assert word in header[header.index("Weighted k-nearest-neighbour"):header.index("cbas_rows_knn(")], word
    assert int(re.search(r"#define CBAS_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.EXPECTED_ABI == 11
    from cbas_amd import build as B
    assert "rows_knn.hip" in B.SOURCES and B.EXTRA_FLAGS["rows_knn.hip"] == B.NO_PACKED
    source = open(os.path.join(REPO, "cbas_amd", "csrc", "rows_knn.hip")).read()
    assert int(re.search(r"\bRK_TILE = (\d+)", source).group(1)) == K.TILE == knn.TILE
    assert int(re.search(r"\bRK_BLOCK = (\d+)", source).group(1)) == K.BLOCK == knn.BLOCK
    assert (knn.MAX_BANK, knn.MAX_K, knn.MAX_CLASSES) == (K.MAX_M, K.MAX_K, K.MAX_C) == (65536, 64, 64)
    readme = open(os.path.join(REPO, "README.md")).read()
    assert f"{len(_lib.SIGNATURES)} entry points" in readme and "cbas_amd.knn" in readme
    assert "## 20." in open(os.path.join(REPO, "DESIGN.md")).read()


# ---- LabelBank.from_instances ---------------------------------------------------------------------------------------------------------
@pytest.fixture()
def index(tmp_path):
    rng = np.random.default_rng(4)
    paths, rows = [], []
    for name, n in (("a", 30), ("b", 50), ("c", 20)):
        rows.append(rng.standard_normal((n, 32)).astype(np.float16))
        paths.append(str(tmp_path / f"{name}_cls.h5"))
        with h5io.ClsWriter(paths[-1], 32) as w:
            w.append(rows[-1])
    return S.FrameIndex(paths, "cpu"), paths, np.concatenate(rows)


def test_label_bank(index, tmp_path, capsys):
    ix, paths, rows = index
    inst = [(paths[0], 2, 10, "groom"),            # 0: frames 2, 5, 8
            (paths[1], 45, 60, "rear "),           # 1: clipped to the file's 50 frames: 45, 48; the label is stripped
            (paths[1], -1, 7, "groom"),            # 2: skipped, no warning
            (paths[2], 0, 5, "fly"),               # 3: unknown label
            (str(tmp_path / "zzz_cls.h5"), 0, 5, "groom"),      # 4: not in the index
            (paths[2], 19, 19, "groom")]           # 5: one frame
    bank = knn.LabelBank.from_instances(ix, inst, ["groom", "rear"], stride=3, group="instance")
    out = capsys.readouterr().out
    assert "WARNING: The label 'fly'" in out and "is not in the master behavior list. This instance will be SKIPPED." in out
    assert f"Warning: H5 file not found, skipping instances for {tmp_path / 'zzz_cls.h5'}" in out
    assert bank.store_row.tolist() == [2, 5, 8, 30 + 45, 30 + 48, 80 + 19] and len(bank) == 6
    assert bank.label.tolist() == [0, 0, 0, 1, 1, 0] and bank.label.dtype.is_floating_point is False
    assert bank.group.tolist() == [0, 0, 0, 1, 1, 5]
    rg = bank.row_group.numpy()
    want = np.full(100, -1, np.int32)
    want[2:11] = 0
    want[75:80] = 1
    want[99] = 5
    assert rg.dtype == np.int32 and np.array_equal(rg, want)
    assert np.array_equal(bank.rows.numpy(), rows[bank.store_row]) and (bank.dim, bank.behaviors, bank.group_kind) == (32, ["groom", "rear"], "instance")
    by_file = knn.LabelBank.from_instances(ix, inst, ["groom", "rear"], stride=1, group="file")
    assert len(by_file) == 9 + 5 + 1 and by_file.group.tolist() == [0] * 9 + [1] * 5 + [2]
    assert np.array_equal(by_file.row_group.numpy(), np.repeat([0, 1, 2], [30, 50, 20]))
    plain = knn.LabelBank.from_instances(ix, inst, ["groom", "rear"], group=None)
    assert plain.group is None and plain.row_group is None and len(plain) == 15
    with pytest.raises(ValueError, match="empty"):
        knn.LabelBank.from_instances(ix, inst[2:5], ["groom", "rear"])
    with pytest.raises(ValueError, match="stride"):
        knn.LabelBank.from_instances(ix, inst, ["groom"], stride=0)
    with pytest.raises(ValueError, match="group"):
        knn.LabelBank.from_instances(ix, inst, ["groom"], group="clip")
    with pytest.raises(ValueError, match="behaviours"):
        knn.LabelBank.from_instances(ix, inst, [str(i) for i in range(65)])
    with pytest.raises(RuntimeError, match="runs on a GPU"):
        ix.knn_labels(bank)


def test_label_bank_too_large(tmp_path):
    path = str(tmp_path / "long_cls.h5")
    with h5io.ClsWriter(path, 32) as w:
        w.append(np.zeros((70000, 32), np.float16))
    ix = S.FrameIndex([path], "cpu")
    with pytest.raises(ValueError, match=r"70000 labelled frames, a bank holds 65536: raise stride \(now 1\)"):
        knn.LabelBank.from_instances(ix, [(path, 0, 69999, "x")], ["x"])
    assert len(knn.LabelBank.from_instances(ix, [(path, 0, 69999, "x")], ["x"], stride=2)) == 35000


# ---- the report ------------------------------------------------------------------------------------------------------------------------
def test_report_by_hand():
    # truth rows, predicted columns; class "c" is never predicted, one frame of "a" has no neighbour (-1)
    #        a  b  c
    #   a    3  1  0   (+ one -1)
    #   b    1  2  0
    #   c    0  2  0
    y_true = [0, 0, 0, 0, 0, 1, 1, 1, 2, 2]
    y_pred = [0, 0, 0, 1, -1, 0, 1, 1, 1, 1]
    r = knn.report_from_predictions(y_true, y_pred, ["a", "b", "c"])
    assert r["confusion_matrix"] == [[3, 1, 0], [1, 2, 0], [0, 2, 0]]
    pa, ra = 3 / 4, 3 / 5
    pb, rb = 2 / 5, 2 / 3
    fa, fb = 2 * pa * ra / (pa + ra), 2 * pb * rb / (pb + rb)
    assert r["a"] == {"precision": pa, "recall": ra, "f1-score": pytest.approx(fa, abs=1e-15), "support": 5}
    assert r["b"] == {"precision": pb, "recall": pytest.approx(rb, abs=1e-15), "f1-score": pytest.approx(fb, abs=1e-15), "support": 3}
    assert r["c"] == {"precision": 0.0, "recall": 0.0, "f1-score": 0.0, "support": 2}          # zero_division = 0
    assert r["accuracy"] == 5 / 10
    assert r["macro avg"] == {"precision": pytest.approx((pa + pb) / 3), "recall": pytest.approx((ra + rb) / 3),
                              "f1-score": pytest.approx((fa + fb) / 3), "support": 10}
    assert r["weighted avg"] == {"precision": pytest.approx(0.5 * pa + 0.3 * pb), "recall": pytest.approx(0.5 * ra + 0.3 * rb),
                                 "f1-score": pytest.approx(0.5 * fa + 0.3 * fb), "support": 10}
    assert set(r) == {"a", "b", "c", "accuracy", "macro avg", "weighted avg", "confusion_matrix"}
    empty = knn.report_from_predictions([1, 1], [-1, -1], ["a", "b"])                           # a class without support, nothing predicted
    assert empty["a"]["f1-score"] == 0.0 and empty["accuracy"] == 0.0 and empty["confusion_matrix"] == [[0, 0], [0, 0]]


# ---- the command line and the output names ---------------------------------------------------------------------------------------------
def test_command_line(tmp_path, capsys):
    _, a = knn.parse_cli(["--dir", "rec", "--instances", "l.csv", "--report", "r.json"])
    assert (a.k, a.temperature, a.stride, a.group, a.write_outputs, a.dir, a.files) == (20, 0.07, 1, "instance", None, "rec", None)
    _, a = knn.parse_cli(["--files", "a_cls.h5", "b_cls.h5", "--labels-yaml", "labels.yaml", "--project-root", "proj", "--k", "5", "--temperature",
                          "0.5", "--stride", "4", "--group", "file", "--write-outputs", "knn"])
    assert (a.files, a.labels_yaml, a.project_root, a.k, a.temperature, a.stride, a.group, a.write_outputs, a.report) == (
        ["a_cls.h5", "b_cls.h5"], "labels.yaml", "proj", 5, 0.5, 4, "file", "knn", None)
    base = ["--dir", "rec", "--instances", "l.csv", "--report", "r.json"]
    for bad, msg in ((base + ["--k", "0"], "1 .. 64"), (base + ["--k", "65"], "1 .. 64"), (base + ["--temperature", "0"], "greater than 0"),
                     (base + ["--temperature", "nan"], "greater than 0"), (base + ["--stride", "0"], "at least 1"),
                     (base + ["--group", "clip"], "invalid choice"), (base[:4], "nothing to do"), (base[2:], "--dir"),
                     (base + ["--labels-yaml", "y"], "not allowed with"), (["--dir", "rec", "--labels-yaml", "y", "--report", "r"], "--project-root")):
        with pytest.raises(SystemExit) as e:
            knn.parse_cli(bad)
        assert e.value.code == 2 and msg in capsys.readouterr().err, bad
    p = tmp_path / "l.csv"
    p.write_text("file,start,end,label\na_cls.h5,3,9,groom\nb_cls.h5,0,4, rear\na_cls.h5,20,29,groom\n")
    assert knn.read_instances_csv(str(p)) == ([("a_cls.h5", 3, 9, "groom"), ("b_cls.h5", 0, 4, "rear"), ("a_cls.h5", 20, 29, "groom")], ["groom", "rear"])
    (tmp_path / "bad.csv").write_text("file,start,end\n")
    with pytest.raises(ValueError, match="file,start,end,label"):
        knn.read_instances_csv(str(tmp_path / "bad.csv"))
    pytest.importorskip("yaml")
    y = tmp_path / "labels.yaml"
    y.write_text("behaviors: [groom, rear]\nlabels:\n  groom:\n  - {video: day1/m1.mp4, start: 3, end: 9, label: groom}\n  rear:\n"
                 "  - {video: day1/m2.mp4, start: 0, end: 4, label: rear}\n")
    inst, names = knn.read_labels_yaml(str(y), "proj")
    assert names == ["groom", "rear"] and inst == [(os.path.join("proj", "day1/m1_cls.h5"), 3, 9, "groom"),
                                                    (os.path.join("proj", "day1/m2_cls.h5"), 0, 4, "rear")]


def test_write_outputs_naming(index, monkeypatch):
    ix, paths, _ = index
    written = []
    from cbas_amd import pipeline
    monkeypatch.setattr(pipeline, "write_probs_csv", lambda path, probs, behaviors, threads=1: written.append((path, probs.copy(), behaviors)))
    probs = np.arange(200, dtype=np.float32).reshape(100, 2)
    out = knn.write_outputs(ix, probs, ["groom", "rear"], "knn20")
    assert out == [p.replace("_cls.h5", "_knn20_outputs.csv") for p in paths] == [w[0] for w in written]
    assert [w[1].shape[0] for w in written] == [30, 50, 20] and np.array_equal(np.concatenate([w[1] for w in written]), probs)
    assert all(w[2] == ["groom", "rear"] for w in written) and knn.outputs_path("x/y_cls.h5", "m") == "x/y_m_outputs.csv"
    with pytest.raises(ValueError, match="shape"):
        knn.write_outputs(ix, probs[:99], ["groom", "rear"], "knn20")


# ---- the restatements against brute force ----------------------------------------------------------------------------------------------
def brute_select(sims, bank_group, row_group, k):
    N, M = sims.shape
    index, score = [], []
    for m in range(N):
        cand = [j for j in range(M) if not (bank_group is not None and row_group is not None and row_group[m] >= 0 and bank_group[j] == row_group[m])]
        best = []
        for _ in range(min(k, len(cand))):
            top = None
            for j in cand:
                if j in best:
                    continue
                if top is None or sims[m, j] > sims[m, top] or (sims[m, j] == sims[m, top] and j < top):
                    top = j
            best.append(top)
        index.append(best + [-1] * (k - len(best)))
        score.append([sims[m, j] for j in best] + [-np.inf] * (k - len(best)))
    return np.asarray(index, np.int32), np.asarray(score, np.float32)


@pytest.mark.parametrize("seed", range(3))
def test_select_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    N, M = 12, 23
    sims = (rng.integers(0, 5 if seed else 1000, (N, M)) / 8.0 - 0.25).astype(np.float32)       # few distinct values: ties everywhere
    sims[0, :4] = [0.0, -0.0, 0.0, -0.0]
    bg = rng.integers(0, 4, M).astype(np.int32)
    rg = rng.integers(-1, 4, N).astype(np.int32)
    bg[:] = np.where(rng.random(M) < 0.1, -1, bg)                                               # a group of -1 excludes nothing
    full = np.zeros(M, np.int32)
    for k in (1, 5, 23, 64):
        for groups in ((None, None), (bg, rg), (bg, None), (full, np.zeros(N, np.int32))):
            got, want = K.select(sims, *groups, k), brute_select(sims, *groups, k)
            assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes() and got[0].dtype == np.int32, (k, groups[0] is None)
    idx, sc = K.select(sims, full, np.zeros(N, np.int32), 3)                                    # the whole bank excluded
    assert (idx == -1).all() and np.isneginf(sc).all()


def test_vote64_against_brute_force():
    rng = np.random.default_rng(9)
    N, k, C, T = 6, 5, 4, 0.07
    labels = rng.integers(0, C, 30)
    index = np.stack([rng.choice(30, k, replace=False) for _ in range(N)]).astype(np.int32)
    score = -np.sort(-rng.random((N, k)).astype(np.float32), axis=1)
    index[1, 3:] = -1
    index[2, :] = -1
    cw = np.array([1.0, 2.0, 0.5, 3.0])
    for weights in (None, cw):
        got = K.vote64(index, score, labels, weights, T, C)
        for m in range(N):
            num, Z = [0.0] * C, 0.0
            for r in range(k):
                if index[m, r] < 0:
                    break
                w = math.exp((float(score[m, r]) - float(score[m, 0])) / T) * (1.0 if weights is None else weights[labels[index[m, r]]])
                num[labels[index[m, r]]] += w
                Z += w
            want = [x / Z for x in num] if Z else [0.0] * C
            assert np.allclose(got[m], want, rtol=0, atol=1e-15), m
    assert (K.vote64(index, score, labels, None, T, C)[2] == 0).all()
    assert K.prob_bound(0.07, 20) == (8 / 0.07 + 48) * 2.0 ** -24 and K.cos_bound(768) == 1544 * 2.0 ** -24
    x = np.array([[3, 4, 0, 0], [0, 0, 0, 0]], np.float16)
    assert K.cos64(x, np.array([[6, 8, 0, 0], [0, 0, 0, 0], [-3, -4, 0, 0]], np.float16)).tolist() == [[1.0, 0.0, -1.0], [0.0, 0.0, 0.0]]
