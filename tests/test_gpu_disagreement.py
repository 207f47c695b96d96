"""The disagreement report on the device: cbas_disagreement_runs and cbas_probs_top1 against the pandas restatement of the
reference (tests/disagreement_ref.py, itself checked against the reference's records in tests/test_disagreement_host.py), and
``disagreement_report`` from resident rows against the host path, the restatement and ``infer_file``'s CSV bytes.  (The final
sort is one line shared by both paths; that equal confidences keep their order is checked in the host test.)"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pd = pytest.importorskip("pandas")

import disagreement_ref as R  # noqa: E402
from cbas_amd import config as CFG, synth, weights as W  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = -1
NAMES = {3: ["walk", "eat", "drink"],                                        # sorted: drink, eat, walk
         9: ["walk", "eat", "drink", "rear", "groom", "dig", "sniff", "climb", "bite"]}
SIZES = [1, 40, 97, 20000]


def scan_case(n_classes):
    """pred / conf of four clips back to back and the instances of the issue's list, as (clip, start, end, label index)."""
    rng = np.random.default_rng(n_classes)
    pred, conf, table, base = [], [], [], 0
    for n in SIZES:
        p = rng.integers(0, n_classes, n)
        stretch = np.repeat(rng.integers(0, n_classes, n // 7 + 1), 7)[:n]
        p = np.where(rng.random(n) < 0.6, stretch, p)                       # runs of equal predictions and single outliers
        p[rng.random(n) < 0.03] = -1                                        # frames without a prediction
        pred.append(p)
        # top-1 probabilities lie in [1 / C, 1]: their float64 sums are exact (see the kernel file)
        conf.append((1.0 / 64 + rng.random(n) * (1 - 1.0 / 64)).astype(np.float32))
        table.append((base, n))
        base += n
    pred[0][0] = 1
    c40 = pred[1]
    c40[0:9] = [0, 0, 0, 1, 1, 1, 2, 2, 2]          # a three-way tie: index order says class 0, name order "drink" (2)
    c40[9] = -1
    c40[10:20] = [1, 1, 1, 0, 2, 0, 0, 1, 1, 1]      # frames 13 - 16 differ from label 1 across the seam of 10-14 | 15-19
    c40[20:30] = 1
    c40[30:32] = [0, 2]
    inst = [(0, 0, 0, 2),                                    # start == end, wrong
            (0, 0, 0, 1),                                    # start == end, right
            (0, 0, 5, -1),                                   # end past the clip
            (0, 1, 3, 0),                                    # start past the clip: no record
            (1, 0, 8, -1),                                   # the tie, a label that is no behaviour
            (1, 0, 39, -1),                                  # every frame wrong
            (1, 20, 29, 1),                                  # no frame wrong
            (1, 15, 31, 1),                                  # runs that touch both ends
            (1, 10, 14, 1), (1, 15, 19, 1),                  # abutting: 13-14 and 15-16 must not merge
            (1, 10, 17, 1), (1, 12, 19, 1),                  # overlapping: each reports its own
            (1, 9, 9, 0),                                    # a run of one frame without a prediction
            (3, 0, 19999, 1),                                # many runs over 79 tiles
            (3, 0, 19999, -1),                               # one run of 20 000 frames
            (3, 255, 20100, 0)]
    for _ in range(40):
        a = int(rng.integers(0, 97))
        inst.append((2, a, a + int(rng.integers(0, 40)), int(rng.integers(-1, n_classes))))
    return np.concatenate(pred), np.concatenate(conf), np.array(table, np.int64), np.array(inst, np.int64), pred, conf


def restated_runs(pred_parts, conf_parts, inst, names):
    """[(instance, start, end, prediction name, confidence)] in the order of the kernel's records."""
    tables = [R.frame_table_from(p, c, names) for p, c in zip(pred_parts, conf_parts)]
    out = []
    for i, (clip, start, end, label) in enumerate(inst.tolist()):
        for r in R.instance_records(tables[clip], "v", start, end, names[label] if label >= 0 else "flying"):
            out.append((i, r["start_frame"], r["end_frame"], r["model_prediction"], r["model_confidence"]))
    return out


@pytest.fixture(scope="module", params=[3, 9])
def case(request):
    n_classes = request.param
    pred, conf, table, inst, pred_parts, conf_parts = scan_case(n_classes)
    return n_classes, pred, conf, table, inst, restated_runs(pred_parts, conf_parts, inst, NAMES[n_classes])


def test_runs_equal_the_restatement_and_repeat_bit_for_bit(case):
    from cbas_amd import train as T
    n_classes, pred, conf, table, inst, want = case
    names = NAMES[n_classes]
    rank = T.name_ranks(names)
    dp, dc = torch.from_numpy(pred.astype(np.int32)).cuda(), torch.from_numpy(conf).cuda()
    got = T.disagreement_runs(dp, dc, table, inst[:, 0], inst[:, 1], inst[:, 2], inst[:, 3], rank)
    again = T.disagreement_runs(dp, dc, table, inst[:, 0], inst[:, 1], inst[:, 2], inst[:, 3], rank)
    assert got.tobytes() == again.tobytes()
    assert len(got) == len(want), (len(got), len(want))
    assert [(int(g["instance"]), int(g["start_frame"]), int(g["end_frame"])) for g in got] == [w[:3] for w in want]
    assert [names[g["model_prediction"]] if g["model_prediction"] >= 0 else None for g in got] == [w[3] for w in want]
    gaps = [abs(float(g["model_confidence"]) - w[4]) / w[4] for g, w in zip(got, want)]
    print(f"C={n_classes}: {len(got)} records, largest relative confidence gap to the restatement {max(gaps):.2e}")
    assert all(abs(float(g["model_confidence"]) - w[4]) <= R.confidence_bound(w[4]) for g, w in zip(got, want))
    # what the fixture was built to hold
    by_inst = {}
    for g in got:
        by_inst.setdefault(int(g["instance"]), []).append((int(g["start_frame"]), int(g["end_frame"]), int(g["model_prediction"])))
    assert by_inst[0] == [(0, 0, 1)] and 1 not in by_inst
    assert by_inst[2][0][:2] == (0, 0) and 3 not in by_inst and 6 not in by_inst
    assert by_inst[4] == [(0, 8, 2)] and by_inst[5][0][:2] == (0, 39)
    assert [r[:2] for r in by_inst[7]] == [(15, 16), (30, 31)]
    assert [r[:2] for r in by_inst[8]] == [(13, 14)] and [r[:2] for r in by_inst[9]] == [(15, 16)]
    assert [r[:2] for r in by_inst[10]] == [(13, 16)] and [r[:2] for r in by_inst[11]] == [(13, 16)]
    assert by_inst[12] == [(9, 9, -1)]
    assert len(by_inst[13]) > 256 and [r[:2] for r in by_inst[14]] == [(0, 19999)] and by_inst[15][-1][1] == 19999
    # the sums of these confidences are exact in float64, so the mean is the one summed in ascending frame order
    host = []
    base = dict(enumerate(table[:, 0].tolist()))
    for clip, start, end, label in inst.tolist():
        n = int(table[clip, 1])
        host += T.disagreement_runs_host(pred[base[clip]:base[clip] + n], conf[base[clip]:base[clip] + n], start, end, label, rank)
    assert [float(g["model_confidence"]) for g in got] == [h[3] for h in host]


def test_runs_refusals(case):
    from cbas_amd import _lib, train as T
    n_classes, pred, conf, table, inst, want = case
    lib = _lib.load()
    dev = torch.device("cuda")
    dp, dc = torch.from_numpy(pred.astype(np.int32)).to(dev), torch.from_numpy(conf).to(dev)
    rank = torch.from_numpy(T.name_ranks(NAMES[n_classes])).to(dev)
    tab = torch.from_numpy(table).to(dev)
    records = torch.empty(64 * T.RUN_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(instances, capacity=64, null=None, needed=None):
        a = [torch.tensor([i[k] for i in instances], dtype=torch.int32, device=dev) for k in range(4)]
        args = [dp.data_ptr(), dc.data_ptr(), int(dp.shape[0]), tab.data_ptr(), len(table), a[0].data_ptr(), a[1].data_ptr(),
                a[2].data_ptr(), a[3].data_ptr(), len(instances), rank.data_ptr(), n_classes, records.data_ptr(), capacity,
                C.byref(needed) if needed is not None else None, stream]
        if null is not None:
            args[null] = None
        return lib.cbas_disagreement_runs(*args)

    good = [(1, 0, 8, -1), (1, 15, 31, 1)]
    needed = C.c_int64(-5)
    assert call(good, needed=needed) == 3 and needed.value == 3
    for null in (0, 1, 3, 5, 6, 7, 8, 10, 12):
        assert call(good, null=null) == EINVAL, null
    for bad in ((4, 0, 3, 0), (-1, 0, 3, 0), (1, 0, 3, n_classes), (1, 0, 3, -2), (1, -1, 3, 0), (1, 5, 4, 0)):
        assert call(good + [bad]) == EINVAL, bad
        assert lib.cbas_last_error()
    needed = C.c_int64(0)
    assert call(good, capacity=2, needed=needed) == EINVAL and needed.value == 3
    assert call(good, capacity=0, null=12, needed=needed) == EINVAL and needed.value == 3        # asking for the count
    assert call([(1, 20, 29, 1)], capacity=0, null=12) == 0                                      # no record: nothing to hold
    bad_table = torch.tensor([[0, 1], [1, 40], [41, 97], [138, 20001]], dtype=torch.int64, device=dev)
    tab, keep = bad_table, tab
    assert call([(3, 0, 5, 0)]) == EINVAL
    tab = keep
    assert call(good) == 3 and lib.cbas_abi_version() == 11


def test_probs_top1_first_maximum_nan_and_class_counts():
    from cbas_amd import train as T
    rng = np.random.default_rng(1)
    for n_classes in (1, 9, 64):
        p = rng.random((777, n_classes)).astype(np.float32)
        if n_classes > 1:
            for r in range(0, 777, 5):                                     # exact ties: the first index wins
                order = np.argsort(p[r])
                p[r, order[-2]] = p[r, order[-1]]
            p[10] = p[10, 0]                                               # a row of equal values
        pred, conf, flags = T.probs_top1(torch.from_numpy(p).cuda())
        frame = pd.DataFrame(p.astype(np.float64), columns=[f"c{i:02d}" for i in range(n_classes)])
        assert pred.dtype == torch.int32 and conf.dtype == torch.float32 and int(flags.item()) == 0
        assert [f"c{i:02d}" for i in pred.cpu().tolist()] == frame.idxmax(axis=1).tolist()
        assert np.array_equal(pred.cpu().numpy(), torch.from_numpy(p).argmax(1).numpy())
        assert np.array_equal(conf.cpu().numpy(), p.max(axis=1))
        if n_classes > 1:
            p[[3, 500], [0, n_classes - 1]] = np.nan
            pred2, conf2, flags = T.probs_top1(torch.from_numpy(p).cuda())
            assert int(flags.item()) == T.TOP1_FLAG_NAN
            keep = np.ones(777, bool)
            keep[[3, 500]] = False
            assert pred2.cpu().numpy()[~keep].tolist() == [-1, -1] and np.isnan(conf2.cpu().numpy()[~keep]).all()
            assert np.array_equal(pred2.cpu().numpy()[keep], pred.cpu().numpy()[keep])
            assert np.array_equal(conf2.cpu().numpy()[keep], conf.cpu().numpy()[keep])
    lib = __import__("cbas_amd")._lib.load()
    z = torch.zeros(4, 3).cuda()
    out = torch.zeros(4, dtype=torch.int32).cuda()
    assert lib.cbas_probs_top1(z.data_ptr(), 4, 65, out.data_ptr(), z.data_ptr(), out.data_ptr(), None) == EINVAL
    assert lib.cbas_probs_top1(None, 4, 3, out.data_ptr(), z.data_ptr(), out.data_ptr(), None) == EINVAL


# ---------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------
DIM, SEQ, BEHAVIORS, TASK = 128, 31, NAMES[9], "job"
CLIPS = {"a.mp4": 40, "sub/b.mp4": 97, "c.mp4": 600, "stale.mp4": 40}


def make_project(root):
    from cbas_amd import h5io
    from cbas_amd.pipeline import format_probs_csv
    paths = {}
    for k, (video, n) in enumerate(CLIPS.items()):
        stem = os.path.splitext(os.path.join(root, video))[0]
        os.makedirs(os.path.dirname(stem), exist_ok=True)
        with h5io.ClsWriter(stem + "_cls.h5", DIM) as w:
            w.append(synth.cls_walk(50 + k, n, DIM))
        paths[video] = stem + "_cls.h5"
    rng = np.random.default_rng(9)
    stale = rng.random((50, 9)).astype(np.float32)
    stale /= stale.sum(axis=1, keepdims=True)
    stale_csv = os.path.join(root, f"stale_{TASK}_outputs.csv")
    with open(stale_csv, "w") as f:
        f.write(format_probs_csv(stale, BEHAVIORS))                        # 50 rows for a 40-row clip: whatever was there is read
    inst = []
    for video, n in CLIPS.items():
        a = 0
        while a < n:
            b = min(n - 1, a + int(rng.integers(2, 30)))
            inst.append({"video": video, "start": a, "end": b, "label": BEHAVIORS[int(rng.integers(0, 9))]})
            a = b + 1
    inst += [{"video": "c.mp4", "start": 590, "end": 700, "label": "walk"}, {"video": "c.mp4", "start": 100, "end": 300, "label": "fly"},
             {"video": "c.mp4", "start": -20, "end": -5, "label": "eat"}, {"video": "sub/b.mp4", "start": "x", "end": 4, "label": "eat"},
             {"video": "stale.mp4", "start": 35, "end": 49, "label": "dig"}, {"video": "noh5.mp4", "start": 0, "end": 5, "label": "eat"}]
    return paths, stale_csv, inst


def test_report_from_resident_rows_equals_host_path_restatement_and_infer_file(tmp_path, monkeypatch):
    from cbas_amd import datasets as D, h5io, train as T
    from cbas_amd.head import ClassifierLSTMDeltas
    cfg = CFG.HeadConfig(in_features=DIM, out_features=9, seq_len=SEQ)
    model = ClassifierLSTMDeltas(DIM, 9, seq_len=SEQ)
    model.load_state_dict(W.synth_head_weights(cfg, 21))
    model.to("cuda")
    dev_root, host_root = str(tmp_path / "dev"), str(tmp_path / "host")
    paths, stale_csv, inst = make_project(dev_root)
    make_project(host_root)
    stale_bytes = open(stale_csv, "rb").read()
    device = torch.device("cuda")

    opened = []

    class Counting(h5io.ClsReader):
        def __init__(self, path, *a, **k):
            opened.append(path)
            super().__init__(path, *a, **k)

    monkeypatch.delenv("CBAS_TRAIN_RESIDENT", raising=False)
    logged = []
    with T.keep_rows() as cache:
        # the store a training run leaves behind: it holds a and c, not b
        manifest = D.make_manifest([(paths[v], 0, CLIPS[v] - 1, "walk") for v in ("a.mp4", "c.mp4")], SEQ, BEHAVIORS)
        store = T.open_store([D.LazyStandardDataset(manifest, SEQ)], ("training",), SEQ, DIM, device, lambda line: None)
        assert store is not None and set(store.files) == {paths["a.mp4"], paths["c.mp4"]}
        monkeypatch.setattr(h5io, "ClsReader", Counting)
        ours = T.disagreement_report(model, inst, BEHAVIORS, SEQ, dev_root, TASK, device=device, log=logged.append)
        monkeypatch.undo()
        assert cache.store is store
    assert opened == [paths["sub/b.mp4"]], opened                          # a and c came from the store, b was uploaded once
    assert sum("malformed" in line for line in logged) == 1, logged

    monkeypatch.setenv("CBAS_TRAIN_RESIDENT", "0")
    host = T.disagreement_report(model, inst, BEHAVIORS, SEQ, host_root, TASK, device=device, log=lambda line: None)
    monkeypatch.delenv("CBAS_TRAIN_RESIDENT", raising=False)
    assert len(ours) > 20 and {o["video_path"] for o in ours} == set(CLIPS)
    worst = R.assert_same_report(ours, host)
    print(f"{len(ours)} records; largest relative confidence gap, resident against host path: {worst:.2e}")

    csv_of = {v: os.path.splitext(os.path.join(dev_root, v))[0] + f"_{TASK}_outputs.csv" for v in CLIPS}
    for v in ("a.mp4", "sub/b.mp4", "c.mp4"):                                # what infer_file wrote on the host path
        assert open(csv_of[v], "rb").read() == open(csv_of[v].replace(dev_root, host_root), "rb").read(), v
    assert open(stale_csv, "rb").read() == stale_bytes
    restated = R.report({v: R.frame_table(csv_of[v], BEHAVIORS) for v in CLIPS}, inst)
    worst = R.assert_same_report(ours, restated)
    print(f"largest relative confidence gap, resident against the restatement on the written CSVs: {worst:.2e}")
    assert any(o["video_path"] == "stale.mp4" and o["end_frame"] == 49 for o in ours)               # rows only the stale file has
    model.close()
