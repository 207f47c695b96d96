"""The search over resident CLS rows, the parts that need no GPU: the numpy selection of rows_search_ref against a brute-force
restatement of the rule, datasets.plan_files, the refusals, locate and query_from of search.FrameIndex on files written with
h5io, the command line and the CSV, and the library surface."""
import fnmatch
import os
import re

import numpy as np
import pytest

import rows_search_ref as R
from cbas_amd import _lib, datasets, h5io, search as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute(trace, table, mask, gap, threshold, k):
    """The rule of include/cbas_mi355x.h word for word: O(N gap) loops, one row at a time."""
    trace = np.asarray(trace, np.float32).reshape(-1, np.shape(trace)[-1])
    index, score = [], []
    for t in trace:
        found = []
        for first, n in table:
            for m in range(first, first + n):
                peak = True
                for m2 in range(max(first, m - gap), min(first + n - 1, m + gap) + 1):
                    if m2 != m and not (t[m2] < t[m] or (t[m2] == t[m] and m2 > m)):
                        peak = False
                if peak and (mask is None or mask[m]) and (threshold is None or t[m] >= np.float32(threshold)):
                    found.append((-float(t[m]), m))
        found.sort()
        found = found[:k]
        index.append([m for _, m in found] + [-1] * (k - len(found)))
        score.append([t[m] for _, m in found] + [-np.inf] * (k - len(found)))
    return np.asarray(index, np.int64), np.asarray(score, np.float32)


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1].dtype == b[1].dtype == np.float32 and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("seed", range(4))
def test_select_random_traces(seed):
    rng = np.random.default_rng(seed)
    N = 300
    # few distinct values: ties everywhere
    trace = (rng.integers(0, 7 if seed % 2 else 1000, (2, N)) / 8.0).astype(np.float32)
    table = [(5, 60), (65, 1), (66, 0), (80, 150), (230, 70)]                # rows 0 - 4 and 66 - 79 outside every clip
    mask = (rng.random(N) > 0.2).astype(np.uint8)
    for gap in (0, 1, 3, 15, 200):
        for k in (1, 5, 64):
            for m, thr in ((None, None), (mask, None), (mask, 0.4)):
                assert same(R.select(trace, table, m, gap, thr, k), brute(trace, table, m, gap, thr, k)), (gap, k, thr)


def test_select_adversarial():
    # a plateau longer than the gap: only its first row is a peak (an equal score at a lower row wins over every later one
    # within the gap, and the rows further on lose to their own predecessors)
    t = np.zeros(40, np.float32)
    t[10:30] = 1.0
    idx, sc = R.select(t, [(0, 40)], None, 5, None, 4)
    assert same((idx, sc), brute(t, [(0, 40)], None, 5, None, 4)) and idx[0].tolist()[:1] == [10] and sc[0, 0] == 1.0
    assert 0 in idx[0] and all(m not in idx[0] for m in range(11, 30))
    # equal scores across a clip boundary: windows never cross clips, so both are peaks; the lower row comes first
    t = np.array([0, 1, 2, 3, 3, 2, 1, 0], np.float32)
    idx, sc = R.select(t, [(0, 4), (4, 4)], None, 3, None, 3)
    assert idx[0].tolist() == [3, 4, -1] and sc[0].tolist() == [3.0, 3.0, -np.inf]
    assert same((idx, sc), brute(t, [(0, 4), (4, 4)], None, 3, None, 3))
    # as one clip the later of the two loses
    assert R.select(t, [(0, 8)], None, 3, None, 3)[0][0].tolist() == [3, -1, -1]
    # a gap of at least the clip's length: one peak per clip, its first maximum
    t = np.array([1, 5, 5, 2, 9, 3, 3], np.float32)
    for gap in (4, 7, 65535):
        idx, _ = R.select(t, [(0, 4), (4, 3)], None, gap, None, 5)
        assert idx[0].tolist() == [4, 1, -1, -1, -1], gap
    # k greater than the number of peaks pads; min_gap 0 is plain top-k with ties to the lowest row
    idx, sc = R.select(t, [(0, 7)], None, 0, None, 9)
    assert idx[0].tolist() == [4, 1, 2, 5, 6, 3, 0, -1, -1] and np.isneginf(sc[0, 7:]).all()
    # a masked maximum is not returned but still suppresses its neighbours
    t = np.array([0, 1, 4, 9, 4, 1, 0, 2, 0], np.float32)
    mask = np.ones(9, np.uint8)
    mask[3] = 0
    idx, _ = R.select(t, [(0, 9)], mask, 2, None, 3)
    assert idx[0].tolist() == [7, -1, -1] and same(R.select(t, [(0, 9)], mask, 2, None, 3), brute(t, [(0, 9)], mask, 2, None, 3))
    # -0 and +0 are equal scores
    t = np.array([-0.0, 0.0, -0.0], np.float32)
    assert R.select(t, [(0, 3)], None, 0, None, 3)[0][0].tolist() == [0, 1, 2]
    # the threshold is compared in float32
    t = np.array([0.1, 0.7, 0.1], np.float32)
    assert R.select(t, [(0, 3)], None, 1, 0.7, 2)[0][0].tolist() == [1, -1]
    assert R.select(t, [(0, 3)], None, 1, np.nextafter(np.float32(0.7), np.float32(1)), 2)[0][0].tolist() == [-1, -1]


def test_scores64():
    rows = np.array([[3, 4, 0, 0], [0, 0, 0, 0], [-3, -4, 0, 0], [0, 0, 1, 0]], np.float16)
    q = np.array([[6, 8, 0, 0], [0, 0, 0, 0]], np.float32)
    assert R.scores64(rows, q).tolist() == [[1.0, 0.0, -1.0, 0.0], [0.0, 0.0, 0.0, 0.0]]
    assert R.score_bound(768) == 1544 * 2.0 ** -24


def _write(path, rows, dtype="f2"):
    with h5io.ClsWriter(str(path), rows.shape[1], dtype=dtype) as w:
        w.append(rows.astype({"f2": np.float16, "f4": np.float32}[dtype]))
    return str(path)


@pytest.fixture()
def files(tmp_path):
    rng = np.random.default_rng(3)
    rows = [rng.standard_normal((n, 32)).astype(np.float16) for n in (7, 12, 5)]
    rows[1][4] = 0                                                            # a zero row
    (tmp_path / "rec" / "day2").mkdir(parents=True)
    names = ["rec/a_cls.h5", "rec/day2/b_cls.h5", "rec/day2/c_cls.h5"]       # in sorted order
    return [_write(tmp_path / name, r) for name, r in zip(names, rows)], rows


def test_plan_files(files, tmp_path):
    paths, rows = files
    plan = datasets.plan_files(paths + [paths[0]])
    assert plan.files == {paths[0]: (0, 7), paths[1]: (7, 12), paths[2]: (19, 5)} and (plan.total_rows, plan.dim) == (24, 32)
    assert plan.nbytes == 24 * 32 * 2 and not plan.not_half and not plan.unreadable
    assert datasets.plan_files(paths, 32).files == plan.files
    with pytest.raises(ValueError, match="width 64"):
        datasets.plan_files(paths, 64)
    wide = _write(tmp_path / "wide_cls.h5", np.zeros((3, 64), np.float16))
    with pytest.raises(ValueError, match="wide_cls.h5"):
        datasets.plan_files(paths + [wide])
    single = _write(tmp_path / "single_cls.h5", np.zeros((3, 32), np.float32), "f4")
    plan = datasets.plan_files([str(tmp_path / "missing_cls.h5"), single, paths[2]])
    assert plan.unreadable == [str(tmp_path / "missing_cls.h5")] and plan.not_half == [single] and plan.total_rows == 8


def test_frame_index_refusals(files, tmp_path):
    paths, _ = files
    with pytest.raises(ValueError, match="not a directory"):
        S.FrameIndex(paths[0], "cpu")
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match=r"no \*_cls.h5"):
        S.FrameIndex(str(empty), "cpu")
    with pytest.raises(ValueError, match="no files"):
        S.FrameIndex([], "cpu")
    with pytest.raises(ValueError, match="cannot be read"):
        S.FrameIndex(paths + [str(tmp_path / "missing_cls.h5")], "cpu")
    single = _write(tmp_path / "single_cls.h5", np.zeros((3, 32), np.float32), "f4")
    with pytest.raises(ValueError, match="half-precision"):
        S.FrameIndex(paths + [single], "cpu")
    wide = _write(tmp_path / "wide_cls.h5", np.zeros((3, 64), np.float16))
    with pytest.raises(ValueError, match="same row width"):
        S.FrameIndex(paths + [wide], "cpu")
    odd = _write(tmp_path / "odd_cls.h5", np.zeros((3, 48), np.float16))
    with pytest.raises(ValueError, match="multiples of 32"):
        S.FrameIndex([odd], "cpu")
    # the memory rule's own words (train._fit_line)
    with pytest.raises(MemoryError, match=r"host loader \(24 rows need 0 MB, 0 MB may be used\)"):
        S.FrameIndex(paths, "cpu", max_gb=1e-9)
    index = S.FrameIndex(str(tmp_path / "rec"), "cpu", max_gb=1.0)           # the directory form finds the three files, sorted
    assert index.files == paths and (index.n_rows, index.dim) == (24, 32)
    with pytest.raises(RuntimeError, match="runs on a GPU"):
        index.search(np.ones(32, np.float32))


def test_locate_and_query_from(files):
    paths, rows = files
    index = S.FrameIndex(paths, "cpu")
    assert index.rows.dtype.is_floating_point and np.array_equal(index.rows.numpy(), np.concatenate(rows))
    assert index._table.tolist() == [[0, 7], [7, 12], [19, 5]]
    assert [index.locate(m) for m in (0, 6, 7, 18, 19, 23)] == [(paths[0], 0), (paths[0], 6), (paths[1], 0), (paths[1], 11), (paths[2], 0),
                                                                 (paths[2], 4)]
    for bad in (-1, 24):
        with pytest.raises(ValueError, match="outside the 24 rows"):
            index.locate(bad)
    x = rows[1][2:6].astype(np.float64)                                       # frames 2 .. 5; frame 4 is the zero row
    n = np.sqrt((x * x).sum(1, keepdims=True))
    want = (np.divide(x, n, out=np.zeros_like(x), where=n > 0)).mean(0).astype(np.float32)
    got = index.query_from(paths[1], 2, 5)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    one = rows[2][3].astype(np.float64)
    assert np.array_equal(index.query_from(paths[2], 3), (one / np.sqrt((one * one).sum())).astype(np.float32))
    assert np.array_equal(index._queries([(paths[2], 3), (paths[1], 2, 5)]), np.stack([index.query_from(paths[2], 3), got]))
    for bad in ((paths[1], 12), (paths[1], -1), (paths[1], 5, 4), (paths[0], 3, 7)):
        with pytest.raises(ValueError, match="lie outside"):
            index.query_from(*bad)
    with pytest.raises(ValueError, match="not one of the 3 files"):
        index.query_from("elsewhere_cls.h5", 0)
    mask = index._mask([(paths[0], 5, 6), (paths[2], 0, 0)])
    assert np.flatnonzero(mask == 0).tolist() == [5, 6, 19] and index._mask(None) is None
    with pytest.raises(ValueError, match="queries of shape"):
        index._queries(np.zeros((2, 16), np.float32))
    with pytest.raises(ValueError, match="not finite"):
        index._queries(np.full(32, np.nan, np.float32))


def test_command_line_and_csv(tmp_path, capsys):
    base = ["--files", "a_cls.h5", "b_cls.h5", "--out", "hits.csv"]
    _, a = S.parse_cli(base + ["--like", "a_cls.h5:12", "--like", "C:/x/b_cls.h5:3-9", "--exclude", "a_cls.h5:0-40", "--k", "5", "--min-gap", "0",
                               "--threshold", "0.5"])
    assert a.like == [("a_cls.h5", 12, None), ("C:/x/b_cls.h5", 3, 9)] and a.exclude == [("a_cls.h5", 0, 40)]
    assert (a.k, a.min_gap, a.threshold, a.files, a.dir, a.out) == (5, 0, 0.5, ["a_cls.h5", "b_cls.h5"], None, "hits.csv")
    _, a = S.parse_cli(["--dir", "rec", "--like", "x:1", "--out", "o.csv"])
    assert (a.k, a.min_gap, a.threshold, a.exclude, a.dir) == (20, 15, None, [], "rec")
    for bad, msg in ((base, "--like"), (base + ["--like", "a_cls.h5"], "FILE:FRAME"), (base + ["--like", "a_cls.h5:x"], "FILE:FRAME"),
                     (base + ["--like", "a_cls.h5:9-3"], "FIRST <= LAST"), (base + ["--like", "a:1", "--exclude", "a:4"], "FIRST-LAST"),
                     (base + ["--like", "a:1", "--k", "0"], "1 .. 64"), (base + ["--like", "a:1", "--k", "65"], "1 .. 64"),
                     (base + ["--like", "a:1", "--min-gap", "70000"], "0 .. 65535"), (["--like", "a:1", "--out", "o.csv"], "--dir"),
                     (["--dir", "d", "--files", "f", "--like", "a:1", "--out", "o.csv"], "not allowed with")):
        with pytest.raises(SystemExit) as e:
            S.parse_cli(bad)
        assert e.value.code == 2 and msg in capsys.readouterr().err, bad
    out = tmp_path / "hits.csv"
    S.write_csv(str(out), [[{"file": "a,b_cls.h5", "frame": 7, "score": 0.987654321}, {"file": "c_cls.h5", "frame": 0, "score": -0.5}], [],
                           [{"file": "c_cls.h5", "frame": 3, "score": 1.0}]])
    assert out.read_text() == ('query,rank,file,frame,score\n0,0,"a,b_cls.h5",7,0.987654\n0,1,c_cls.h5,0,-0.500000\n2,0,c_cls.h5,3,1.000000\n')
    assert S.CSV_COLUMNS == ["query", "rank", "file", "frame", "score"]


def test_library_surface():
    header = open(os.path.join(REPO, "include", "cbas_mi355x.h")).read()
    debug_header = open(os.path.join(REPO, "include", "cbas_mi355x_debug.h")).read()
    ctype = {"int64_t": _lib.c_int64, "int32_t": _lib.c_int32, "float": _lib.c_float, "uint16_t*": _lib.c_void_p, "float*": _lib.c_void_p,
             "int64_t*": _lib.c_void_p, "uint8_t*": _lib.c_void_p, "void*": _lib.c_void_p}
    for name, res in (("cbas_rows_search_workspace_bytes", _lib.c_int64), ("cbas_rows_search", _lib.c_int)):
        decl = re.search(r"\b(?:int|int64_t) %s\(([^;]+)\);" % name, header)
        assert decl, name
        r, args = _lib.SIGNATURES[name]
        declared = [ctype[re.sub(r"\bconst\s+", "", a.strip()).rsplit(" ", 1)[0].replace(" *", "*")] for a in decl.group(1).split(",")]
        assert r is res and args == declared and name not in debug_header, name
        exports = open(os.path.join(REPO, "cbas_amd", "csrc", "exports.map")).read()
        patterns = re.search(r"global:([^;]+);", exports).group(1).split()
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns) and name in exports
    assert int(re.search(r"#define CBAS_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.EXPECTED_ABI == 11
    assert (S.MAX_QUERIES, S.MAX_K, S.MAX_GAP) == (R.MAX_Q, R.MAX_K, R.MAX_GAP) == (64, 64, 65535)
    source = open(os.path.join(REPO, "cbas_amd", "csrc", "rows_search.hip")).read()
    assert int(re.search(r"\bRS_CHUNK = (\d+)", source).group(1)) == R.CHUNK
    from cbas_amd import build as B
    assert "rows_search.hip" in B.SOURCES and B.EXTRA_FLAGS["rows_search.hip"] == B.NO_PACKED
    readme = open(os.path.join(REPO, "README.md")).read()
    assert f"{len(_lib.SIGNATURES)} entry points" in readme and "cbas_amd.search" in readme
    assert "## 19." in open(os.path.join(REPO, "DESIGN.md")).read()
    assert "cbas_rows_search" in open(os.path.join(REPO, "INTEGRATION.md")).read()
