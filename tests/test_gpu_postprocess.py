"""Events, pre-labels and actogram bins on the device: cbas_labels_median, cbas_label_runs and cbas_activity_bins against the
numpy routines of cbas_amd.postprocess on the same float32 arrays (everything identical, confidences bit-equal) and against
what the reference's own methods returned (tests/golden/postprocess.npz: records and bins identical, confidences within
2^-24 relative, the CSV's decimals); then ``prelabel_file``, ``activity_bins`` over files and ``install(postprocess=True)``."""
import ctypes as C
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

import postprocess_cases as PC
from cbas_amd import config as CFG, postprocess as P, synth, weights as W

pytestmark = pytest.mark.gpu

EINVAL = -1
GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "postprocess.npz"))
REL = 2.0 ** -24


def golden(key):
    return json.loads(str(GOLDEN[key]))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------
# the median
# ---------------------------------------------------------------------------------------------------------------
MEDIAN_CLIPS = [1, 2, 5, 1000, 40, 40, 3000]       # 3000 frames: three tiles of 1024, the last one partial


def median_case(n_classes):
    rng = np.random.default_rng(100 + n_classes)
    parts = []
    for n in MEDIAN_CLIPS:
        x = np.repeat(rng.integers(0, n_classes, n // 9 + 1), 9)[:n]
        x = np.where(rng.random(n) < 0.1, rng.integers(0, n_classes, n), x)          # flicker
        x[rng.random(n) < 0.04] = -1                                                    # rows without a label
        parts.append(x.astype(np.int32))
    parts[2][:] = n_classes - 1                      # the 5-frame clip: one class, != 0 for C > 1
    # two clips of 40 whose junction would change the result if a window crossed it: all of one class against all of another
    parts[4][:] = n_classes - 1
    parts[5][:] = min(1, n_classes - 1)
    parts[5][:3] = -1
    table = np.array([[sum(MEDIAN_CLIPS[:k]), n] for k, n in enumerate(MEDIAN_CLIPS)], np.int64)
    return parts, table


@pytest.mark.parametrize("n_classes", [1, 9, 64])
def test_median_equals_the_numpy_routine_and_scipy(n_classes):
    parts, table = median_case(n_classes)
    flat = dev(np.concatenate(parts))
    try:
        from scipy.signal import medfilt
    except ImportError:
        medfilt = None
    for k in (1, 3, 7, 31, 2001):
        got = P.labels_median(flat, table, n_classes, k).cpu().numpy()
        assert got.dtype == np.int32
        for (base, n), x in zip(table, parts):
            want = P.median_host(x, k)
            assert np.array_equal(got[base:base + n], want), (n_classes, k, n)
            if medfilt is not None and k <= 31:
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", UserWarning)
                    assert np.array_equal(medfilt(x.astype(np.int64), kernel_size=k), want)
        if k == 1:
            assert np.array_equal(got, np.concatenate(parts))
    # the clips in another order of the table, with a gap: windows follow the table, not the memory
    shuffled = table[[3, 0, 6, 2]]
    got = P.labels_median(flat, shuffled, n_classes, 7)
    for base, n in shuffled:
        assert np.array_equal(got[base:base + n].cpu().numpy(), P.median_host(np.concatenate(parts)[base:base + n], 7))


def test_median_zero_padding_and_junction():
    x = np.array([3, 1, 3, 3, 1, 3] + [5] * 6 + [1, 5, 5, 5, 5, 5], np.int32)
    table = [(0, 6), (6, 6), (12, 6)]
    got = P.labels_median(dev(x), table, 9, 3).cpu().numpy()
    assert list(got[:6]) == [1, 3, 3, 3, 3, 1]                    # (0, 3, 1) and (1, 3, 0): the ends move towards 0
    assert list(got[6:12]) == [5] * 6 and list(got[12:]) == [1, 5, 5, 5, 5, 5]        # (0, 1, 5): the 5 before the junction is not seen
    one = P.labels_median(dev(x), [(0, 18)], 9, 3).cpu().numpy()  # as ONE clip the window (5, 1, 5) removes the 1
    assert list(one) == [int(v) for v in P.median_host(x, 3)] and one[12] == 5
    assert list(P.labels_median(dev(x), table, 9, 13).cpu().numpy()) == [0] * 18        # 7 of 13 values are padding everywhere
    parts, tab = median_case(9)
    joined = P.median_host(np.concatenate(parts[4:6]), 7)
    assert joined[40] != P.median_host(parts[5], 7)[0]             # the junction of median_case's clips 4 | 5 tells the two apart


def test_median_refusals():
    from cbas_amd import _lib
    lib = _lib.load()
    x = dev(np.array([0, 1, 2, 1, 0, -1], np.int32))
    out = torch.empty_like(x)
    table = dev(np.array([[0, 6]], np.int64))

    def call(pred=x, n=6, tab=table, n_clips=1, n_classes=3, k=3, o=out):
        return lib.cbas_labels_median(pred.data_ptr(), n, tab.data_ptr(), n_clips, n_classes, k, o.data_ptr(), None)
    assert call() == 0
    for kw in (dict(k=4), dict(k=0), dict(k=-3), dict(n_classes=0), dict(n_classes=65), dict(n_clips=0), dict(n=-1), dict(o=x)):
        assert call(**kw) == EINVAL, kw
    assert call(n_classes=2) == EINVAL and b"outside [-1, 2)" in lib.cbas_last_error()           # the value 2
    assert call(pred=dev(np.array([0, 1, -2, 1, 0, 0], np.int32))) == EINVAL
    for bad in ([[0, 7]], [[-1, 3]], [[4, 3]], [[0, -1]], [[7, 0]]):
        assert call(tab=dev(np.array(bad, np.int64))) == EINVAL and b"table" in lib.cbas_last_error(), bad
    assert call(tab=dev(np.array([[6, 0]], np.int64))) == 0                                        # an empty clip at the end


# ---------------------------------------------------------------------------------------------------------------
# the runs
# ---------------------------------------------------------------------------------------------------------------
def runs_case():
    rng = np.random.default_rng(5)
    sizes = [1, 2, 40, 600, 300, 10, 0, 257]
    keys, confs = [], []
    for n in sizes:
        k = np.repeat(rng.integers(0, 9, n // 6 + 1), 6)[:n]
        k = np.where(rng.random(n) < 0.15, rng.integers(0, 9, n), k)
        k[rng.random(n) < 0.05] = -1
        keys.append(k.astype(np.int32))
        confs.append((1.0 / 64 + rng.random(n) * (1 - 1.0 / 64)).astype(np.float32))
    keys[3][:] = 4                                   # a run that is the whole clip (600 frames: three tiles)
    confs[3][:] = 0.8
    keys[4][:] = np.arange(300) % 2                  # single-frame runs
    keys[2][-6] = 3
    keys[2][-5:] = 7                                 # a run ending on the last frame
    confs[2][-5:] = 0.9
    keys[5][:] = [1, 1, 1, 2, 2, 2, 2, 1, 1, 1]      # the label changes at 3 and 7 with the probability above the threshold,
    confs[5][:] = [.9, .9, .9, .9, .9, .2, .9, .9, .9, .9]      # and it drops at 5 inside a label
    table = np.array([[sum(sizes[:i]), n] for i, n in enumerate(sizes)], np.int64)
    return keys, confs, table


@pytest.mark.parametrize("threshold", [None, 0.5, 0.0, 2.0])
def test_runs_equal_the_numpy_routine_bit_for_bit(threshold):
    keys, confs, table = runs_case()
    dk, dc = dev(np.concatenate(keys)), dev(np.concatenate(confs))
    got = P.label_runs(dk, dc, table, 9, threshold)
    again = P.label_runs(dk, dc, table, 9, threshold)
    assert got.tobytes() == again.tobytes()
    want = [(c, a, b, label, conf) for c, (k, p) in enumerate(zip(keys, confs)) for a, b, label, conf in P.label_runs_host(k, p, threshold)]
    assert [tuple(r)[:4] for r in got.tolist()] == [w[:4] for w in want]
    assert got["confidence"].tobytes() == np.array([w[4] for w in want], np.float64).tobytes()
    if threshold == 2.0:
        assert len(got) == 0                                       # an empty result
    if threshold is None:
        assert (3, 0, 599, 4) in [tuple(r)[:4] for r in got.tolist()] and got[got["clip"] == 4].shape[0] == 300
        assert tuple(got[got["clip"] == 2][-1])[1:4] == (35, 39, 7)
    if threshold == 0.5:
        assert [tuple(r)[1:4] for r in got[got["clip"] == 5].tolist()] == [(0, 2, 1), (3, 4, 2), (6, 6, 2), (7, 9, 1)]


def test_runs_capacity_count_query_and_refusals():
    from cbas_amd import _lib
    lib = _lib.load()
    keys, confs, table = runs_case()
    dk, dc, dt = dev(np.concatenate(keys)), dev(np.concatenate(confs)), dev(table)
    n, n_clips = int(dk.shape[0]), int(table.shape[0])
    full = P.label_runs(dk, dc, table, 9, 0.5)
    needed = C.c_int64(-5)

    def call(cap, buf, key=dk, tab=dt, n_classes=9, use=1, thr=0.5, clips=n_clips):
        return lib.cbas_label_runs(key.data_ptr(), dc.data_ptr(), n, tab.data_ptr(), clips, n_classes, use, thr,
                                   buf.data_ptr() if buf is not None else None, cap, C.byref(needed), None)
    assert call(0, None) == EINVAL and needed.value == len(full) > 50          # the count query: "N records, the buffer holds 0"
    assert b"records" in lib.cbas_last_error()
    buf = torch.zeros(len(full) * 24, dtype=torch.uint8, device="cuda")
    assert call(len(full), buf) == len(full) and buf.cpu().numpy().view(P.LABEL_RUN_DTYPE).tobytes() == full.tobytes()
    small = torch.full((10 * 24 + 24,), 7, dtype=torch.uint8, device="cuda")
    assert call(10, small) == EINVAL and needed.value == len(full)
    assert bytes(small[-24:].cpu().numpy()) == b"\x07" * 24                     # nothing past the capacity was written
    assert call(5, None) == EINVAL and call(-1, buf) == EINVAL
    assert call(len(full), buf, n_classes=0) == EINVAL and call(len(full), buf, n_classes=65) == EINVAL
    assert call(len(full), buf, clips=0) == EINVAL and call(len(full), buf, thr=float("nan")) == EINVAL
    assert call(len(full), buf, n_classes=8) == EINVAL and b"key" in lib.cbas_last_error()       # keys reach 8
    bad = table.copy()
    bad[3, 1] = n
    assert call(len(full), buf, tab=dev(bad)) == EINVAL and b"table" in lib.cbas_last_error()
    empty = P.label_runs(dev(np.full(5, -1, np.int32)), dev(np.ones(5, np.float32)), [(0, 5)], 3)
    assert empty.shape == (0,)


@pytest.mark.parametrize("seed,n,n_classes,threshold", PC.EVENT_CASES)
def test_events_on_the_device_equal_the_references(seed, n, n_classes, threshold):
    p = PC.probabilities(seed, n, n_classes)
    assert P.predictions_to_instances(dev(p), PC.names(n_classes), f"ev{seed}.mp4", threshold) == golden(f"events/{seed}")


@pytest.mark.parametrize("seed,n,n_classes,window", PC.BLOCK_CASES)
def test_blocks_on_the_device_equal_the_references_and_the_host(seed, n, n_classes, window, monkeypatch):
    p = PC.probabilities(seed, n, n_classes)
    want = golden(f"blocks/{seed}")
    got, df = P.predictions_to_instances_with_confidence(dev(p), PC.names(n_classes), f"bl{seed}.mp4", smoothing_window=window)
    assert [{k: v for k, v in g.items() if k != "confidence"} for g in got] == [{k: v for k, v in w.items() if k != "confidence"} for w in want]
    assert all(abs(g["confidence"] - w["confidence"]) <= REL * w["confidence"] for g, w in zip(got, want))
    assert list(df.columns) == golden(f"blocks/{seed}/columns")
    monkeypatch.setattr(P, "_gpu", lambda: False)
    host, hdf = P.predictions_to_instances_with_confidence(p, PC.names(n_classes), f"bl{seed}.mp4", smoothing_window=window)
    assert got == host and df.equals(hdf)                          # confidences bit-equal, every column identical


def test_a_nan_row_goes_to_the_numpy_routine():
    p = PC.probabilities(2, 60, 4)
    p[7, 1] = np.nan
    names = PC.names(4)
    pred, conf = P.top1_host(p)
    want = [{"video": "v.mp4", "start": a, "label": names[k], "end": b} for a, b, k, _c in P.label_runs_host(pred, conf, 0.5)]
    assert P.predictions_to_instances(dev(p), names, "v.mp4", 0.5) == want and len(want) > 2


# ---------------------------------------------------------------------------------------------------------------
# the bins
# ---------------------------------------------------------------------------------------------------------------
def bins_case(n_classes, n=1000):
    p = PC.probabilities(40 + n_classes, n, n_classes)
    if n_classes > 1:
        p[3] = p[3, 0]                                # every column equal: a tie with everyone
        p[10, 1] = np.nan                             # a NaN in another column
        p[11, 0] = np.nan                             # a NaN probability
        p[12] = np.nan
    else:
        p[11, 0] = np.nan
    return p


@pytest.mark.parametrize("n_classes", [1, 2, 9, 64])
def test_bins_equal_the_numpy_routine(n_classes):
    p = bins_case(n_classes)
    d = dev(p)
    for b in sorted({0, n_classes - 1}):
        for threshold in (0.5, 0.0, -1.0, 0.123):
            for bin_frames in (1, 7, 64, 100, 1000, 5000):
                got = P.activity_bins_device(d, b, threshold, bin_frames).cpu().numpy()
                want = P.activity_bins_host(p, b, threshold, bin_frames)
                assert got.dtype == np.int64 and np.array_equal(got, want), (n_classes, b, threshold, bin_frames)
    ties = np.array([[.5, .5], [.4, .6], [.6, .4]] * 3, np.float32)
    assert list(P.activity_bins_device(dev(ties), 0, 0.5, 3).cpu().numpy()) == [1, 1, 1]          # a tie is no maximum
    assert list(P.activity_bins_device(dev(ties), 0, 0.0, 4).cpu().numpy()) == [4, 4, 1]          # threshold 0: every frame
    assert list(P.activity_bins_device(dev(ties[:, :1]), 0, 0.5, 9).cpu().numpy()) == [0]         # C = 1


def test_bins_refusals():
    from cbas_amd import _lib
    lib = _lib.load()
    p = dev(PC.probabilities(1, 20, 3))
    bins = torch.zeros(4, dtype=torch.int64, device="cuda")

    def call(n=20, n_classes=3, b=0, bin_frames=7, n_bins=3):
        return lib.cbas_activity_bins(p.data_ptr(), n, n_classes, b, 0.5, bin_frames, bins.data_ptr(), n_bins, None)
    assert call() == 0
    for kw in (dict(n=0), dict(n_classes=0), dict(n_classes=65), dict(b=-1), dict(b=3), dict(bin_frames=0), dict(n_bins=2), dict(n_bins=4)):
        assert call(**kw) == EINVAL, kw


@pytest.mark.parametrize("seed,n,n_classes,b,threshold,framerate,minutes", PC.ACTO_DF_CASES)
def test_bins_on_the_device_equal_the_references(seed, n, n_classes, b, threshold, framerate, minutes):
    p = PC.probabilities(seed, n, n_classes)
    names = PC.names(n_classes)
    for source in (dev(p), p):                                     # a device tensor, and an array that is uploaded
        assert np.array_equal(np.array(P.activity_bins(source, None, names, names[b], framerate, minutes, threshold)), GOLDEN[f"acto_df/{seed}"])


# ---------------------------------------------------------------------------------------------------------------
# flows
# ---------------------------------------------------------------------------------------------------------------
DIM, SEQ = 128, 31


def make_head():
    from cbas_amd.head import ClassifierLSTMDeltas
    model = ClassifierLSTMDeltas(DIM, 9, seq_len=SEQ)
    model.load_state_dict(W.synth_head_weights(CFG.HeadConfig(in_features=DIM, out_features=9, seq_len=SEQ), 21))
    return model.to("cuda")


def test_prelabel_file_writes_infer_files_csv_and_returns_the_routines_blocks(tmp_path, monkeypatch):
    from cbas_amd import h5io, pipeline as PL
    names = PC.names(9)
    model = make_head()
    # 14 walks of 50 frames, each around another base row: this head changes its label often enough that blocks remain after
    # a median over 31 frames (one 700-frame walk is one block then; the numpy oracle counts 111 / 64 / 38 blocks here)
    rows = np.concatenate([synth.cls_walk(100 + k, 50, DIM) for k in range(14)])
    for sub in ("dev", "host"):
        os.makedirs(tmp_path / sub / "day1")
        with h5io.ClsWriter(str(tmp_path / sub / "day1" / "cam_cls.h5"), DIM) as w:
            w.append(rows)
    h5 = str(tmp_path / "dev" / "day1" / "cam_cls.h5")
    csv_host = PL.infer_file(file_path=h5.replace("dev", "host"), model=model, dataset_name="job", behaviors=names, seq_len=SEQ,
                             device="cuda", temperature=1.3)
    probs = np.loadtxt(csv_host, delimiter=",", skiprows=1, dtype=np.float64).astype(np.float32)
    for window in (1, 5, 30):
        got, df = P.prelabel_file(h5, model, "job", names, SEQ, smoothing_window=window, temperature=1.3,
                                  project_path=str(tmp_path / "dev"))
        assert open(h5.replace("_cls.h5", "_job_outputs.csv"), "rb").read() == open(csv_host, "rb").read()
        os.remove(h5.replace("_cls.h5", "_job_outputs.csv"))
        monkeypatch.setattr(P, "_gpu", lambda: False)
        want, wdf = P.predictions_to_instances_with_confidence(probs, names, "day1/cam.mp4", smoothing_window=window)
        monkeypatch.undo()
        assert got == want and len(got) > 3 and got[0]["video"] == "day1/cam.mp4" and df.equals(wdf)
        cols = names + ["predicted_label", "max_prob"] + (["predicted_index", "smoothed_index"] if window > 1 else []) + \
            ["label_for_grouping", "block_start"]
        assert list(df.columns) == cols and len(df) == 700
    with pytest.raises(ValueError):
        P.prelabel_file(h5, model, "job", names, SEQ + 2)
    model.close()


def test_activity_bins_over_files_first_call_and_cached(tmp_path, monkeypatch):
    from cbas_amd import pipeline as PL
    P.clear_cache()
    n_classes, b, threshold, framerate, minutes = PC.ACTO_DIR_CASES[0]
    names = PC.names(n_classes)
    for name, seed, n in PC.ACTO_DIR_FILES:
        PL.write_probs_csv(str(tmp_path / name), PC.probabilities(seed, n, n_classes), names)
    first = P.activity_bins(str(tmp_path), PC.MODEL, None, names[b], framerate, minutes, threshold)
    assert np.array_equal(np.array(first), GOLDEN["acto_dir/0"]) and len(P._cache) == 1
    reads = []
    real = P.read_outputs_csv
    monkeypatch.setattr(P, "read_outputs_csv", lambda path: reads.append(path) or real(path))
    assert P.activity_bins(str(tmp_path), PC.MODEL, None, names[b], framerate, minutes, threshold) == first and reads == []
    n_classes, b, threshold, framerate, minutes = PC.ACTO_DIR_CASES[1]       # another behaviour, threshold and bin size: no file is read
    assert np.array_equal(np.array(P.activity_bins(str(tmp_path), PC.MODEL, None, names[b], framerate, minutes, threshold)), GOLDEN["acto_dir/1"])
    assert reads == []
    name, seed, n = PC.ACTO_DIR_FILES[1]
    PL.write_probs_csv(str(tmp_path / name), PC.probabilities(seed + 50, n + 1, n_classes), names)       # a file changed: read again
    changed = P.activity_bins(str(tmp_path), PC.MODEL, None, names[b], framerate, minutes, threshold)
    assert len(reads) == 3 and changed != list(GOLDEN["acto_dir/1"])
    monkeypatch.setenv("CBAS_ACTOGRAM_CACHE_MB", "0")
    P.clear_cache()
    assert P.activity_bins(str(tmp_path), PC.MODEL, None, names[b], framerate, minutes, threshold) == changed and len(P._cache) == 0
    P.clear_cache()


def test_mixed_headers_on_the_device_do_not_depend_on_the_order_of_calls(tmp_path):
    """A recording whose files differ in their columns: two behaviours asked for in both orders, each from a cold cache, give
    what each gives alone; a recording with one header that lacks a behaviour gives [] for it before and after it is cached."""
    from cbas_amd import pipeline as PL
    nine, two = PC.probabilities(31, 70, 9), PC.probabilities(32, 45, 2)
    mixed, plain = tmp_path / "mixed", tmp_path / "plain"
    os.makedirs(mixed), os.makedirs(plain)
    PL.write_probs_csv(str(mixed / "rec_1_m_outputs.csv"), nine, PC.names(9))
    PL.write_probs_csv(str(mixed / "rec_2_m_outputs.csv"), two, ["x", "beh4"])
    PL.write_probs_csv(str(mixed / "rec_3_m_outputs.csv"), nine[:30], PC.names(9))
    want4 = P._rebin(np.concatenate([P.activity_bins_host(nine, 4, 0.3, 1), P.activity_bins_host(two, 1, 0.3, 1),
                                     P.activity_bins_host(nine[:30], 4, 0.3, 1)]), 6)
    wantx = [float(v) for v in P.activity_bins_host(two, 0, 0.3, 6)]
    want0 = P._rebin(np.concatenate([P.activity_bins_host(nine, 0, 0.3, 1), P.activity_bins_host(nine[:30], 0, 0.3, 1)]), 6)
    assert sum(want4) > 0 and sum(wantx) > 0 and sum(want0) > 0
    for order in (("beh4", "x", "beh0"), ("x", "beh4", "beh0"), ("beh0", "x", "beh4", "x")):
        P.clear_cache()
        for b in order:
            assert P.activity_bins(str(mixed), "m", None, b, 0.1, 1, 0.3) == {"beh4": want4, "x": wantx, "beh0": want0}[b], (order, b)
        assert len(P._cache) == 0                                  # nothing of a mixed recording is kept
    PL.write_probs_csv(str(plain / "rec_1_m_outputs.csv"), nine, PC.names(9))
    PL.write_probs_csv(str(plain / "rec_2_m_outputs.csv"), nine[:30], PC.names(9))
    for order in (("x", "beh0"), ("beh0", "x")):
        P.clear_cache()
        for b in order + order:
            assert P.activity_bins(str(plain), "m", None, b, 0.1, 1, 0.3) == ([] if b == "x" else want0), (order, b)
        assert len(P._cache) == 1
    # a file that is not float32 text keeps the whole recording on the host, whatever was cached before
    (plain / "rec_3_m_outputs.csv").write_text(",".join(PC.names(9)) + "\n" + ",".join(["0.7000"] + ["0.0375"] * 8) + "\n")
    assert P.activity_bins(str(plain), "m", None, "beh0", 0.1, 1, 0.3)[-1] == want0[-1] + 1 and len(P._cache) == 1
    P.clear_cache()
    assert P.activity_bins(str(plain), "m", None, "beh0", 0.1, 1, 0.3)[-1] == want0[-1] + 1 and len(P._cache) == 0


def test_install_postprocess_patches_and_plain_install_does_not(tmp_path, monkeypatch):
    from cbas_amd import integration as I, pipeline as PL

    class Dataset:
        def __init__(self, behaviors):
            self.config = {"behaviors": behaviors}

        def predictions_to_instances(self, csv_path, model_name, threshold=0.7):
            return "reference"

        def predictions_to_instances_with_confidence(self, csv_path, model_name, threshold=0.5, smoothing_window=1):
            return "reference"

    class Actogram:
        def __init__(self, *a, **k):
            self.binned_activity = "reference"

    cbas, head = types.ModuleType("cbas"), types.ModuleType("classifier_head")
    cbas.Dataset, cbas.Actogram = Dataset, Actogram
    gui = types.ModuleType("gui_state")
    gui.proj = types.SimpleNamespace(path=str(tmp_path))
    for name, mod in (("cbas", cbas), ("classifier_head", head), ("gui_state", gui)):
        monkeypatch.setitem(sys.modules, name, mod)
    monkeypatch.setitem(sys.modules, "workthreads", None)          # importing it fails: install() goes on without it
    originals = (Dataset.predictions_to_instances, Dataset.predictions_to_instances_with_confidence, Actogram.__init__)
    assert I.install() is True
    assert (Dataset.predictions_to_instances, Dataset.predictions_to_instances_with_confidence, Actogram.__init__) == originals
    assert I.install(postprocess=True) is True and I.install(postprocess=True) is True
    seed, n, n_classes, window = PC.BLOCK_CASES[1]
    names = PC.names(n_classes)
    csv = str(tmp_path / f"bl{seed}_{PC.MODEL}_outputs.csv")
    PL.write_probs_csv(csv, PC.probabilities(seed, n, n_classes), names)
    got, df = Dataset(names).predictions_to_instances_with_confidence(csv, PC.MODEL, smoothing_window=window)
    want = golden(f"blocks/{seed}")
    assert [(g["video"], g["start"], g["end"], g["label"]) for g in got] == [(w["video"], w["start"], w["end"], w["label"]) for w in want]
    assert list(df.columns) == golden(f"blocks/{seed}/columns")
    events = Dataset(names).predictions_to_instances(csv, PC.MODEL, 0.6)
    assert events and events[0]["video"] == str(tmp_path / f"bl{seed}.mp4")
    os.makedirs(tmp_path / "recording")
    for name, s, frames in PC.ACTO_DIR_FILES:
        PL.write_probs_csv(str(tmp_path / "recording" / name), PC.probabilities(s, frames, 9), PC.names(9))
    n_classes, b, threshold, framerate, minutes = PC.ACTO_DIR_CASES[0]
    acto = Actogram(PC.names(9)[b], framerate, 0, minutes, threshold, "LD", directory=str(tmp_path / "recording"), model=PC.MODEL)
    assert np.array_equal(np.array(acto.binned_activity), GOLDEN["acto_dir/0"]) and acto.blob is None and acto.binsize_frames == 6
    I.uninstall()
    assert (Dataset.predictions_to_instances, Dataset.predictions_to_instances_with_confidence, Actogram.__init__) == originals
    P.clear_cache()
