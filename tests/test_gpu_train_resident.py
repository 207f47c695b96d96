"""Head training from CLS rows resident in device memory: the window gather kernel (cbas_rows_gather_windows) against numpy
slicing, cbas_head_train_step_rows against cbas_head_train_step on the same windows, and train_lstm_model on manifest
datasets with the rows resident against the host loader (CBAS_TRAIN_RESIDENT=0: the unchanged path) - identical results,
the memory rule, ordinary datasets, and the time of an epoch on either path."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest
import torch

from cbas_amd import config as CFG, synth, weights as W

pytestmark = pytest.mark.gpu

EINVAL = -1


def random_halves(seed, n, dim):
    """Every kind of finite half and the infinities (bit patterns drawn uniformly; NaNs replaced): zeros of both signs,
    subnormals, the largest values."""
    bits = np.random.default_rng(seed).integers(0, 1 << 16, (n, dim), dtype=np.uint16)
    nan = ((bits & 0x7C00) == 0x7C00) & ((bits & 0x03FF) != 0)
    bits[nan] &= 0xFC00                                   # -> +-infinity
    bits[0, :4] = [0x0000, 0x8000, 0x0001, 0x7BFF]
    return bits.view(np.float16)


def gather_ref(rows, first, T):
    """numpy: window w = rows[first[w] : first[w] + T] as float32, rows outside the store zeros."""
    n, dim = rows.shape
    out = np.zeros((len(first), T, dim), np.float32)
    for w, f in enumerate(first):
        for t in range(T):
            r = int(f) + t
            if 0 <= r < n:
                out[w, t] = rows[r].astype(np.float32)
    return out


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("D", [768, 384, 1000, 100, 13])     # 100, 13: rows that do not start on 16-byte boundaries
@pytest.mark.parametrize("T", [3, 31, 63, 95])
def test_gather_is_bit_identical_to_numpy_slicing(D, T):
    from cbas_amd.train import gather_windows
    files = [150, 97, 211]                                 # rows per file, back to back in the store
    n = sum(files)
    rows = random_halves(D * 1000 + T, n, D)
    dev = torch.from_numpy(rows).cuda()
    rng = np.random.default_rng(T)
    edges = [0, n - T, files[0] - T, files[0], files[0] - T // 2, files[0] + files[1] - 1, files[0] + files[1] - T + 1]
    assert all(0 <= e <= n - T for e in edges)
    for B in (1, 37, 512):
        if B == 1:
            batches = [[e] for e in edges[:5]]             # the first and last row of the store, across a file boundary
        else:
            batches = [edges + rng.integers(0, n - T + 1, B - len(edges)).tolist()]
        for first in batches:
            got = gather_windows(dev, torch.tensor(first, dtype=torch.int64), T)
            want = np.stack([rows[f:f + T] for f in first]).astype(np.float32)
            assert same_bits(got.cpu().numpy(), want), (D, T, B, first[:8])
    # a reused, larger output buffer: only the first B windows are written
    buf = torch.full((40, T, D), 7.0, device="cuda")
    got = gather_windows(dev, torch.tensor(edges, dtype=torch.int64), T, out=buf)
    assert got.data_ptr() == buf.data_ptr() and same_bits(got.cpu().numpy(), np.stack([rows[f:f + T] for f in edges]).astype(np.float32))
    assert bool((buf[len(edges):] == 7.0).all())


@pytest.mark.parametrize("D", [768, 100])
def test_rows_outside_the_store_come_out_as_zeros(D):
    """Indices outside the LOGICAL store: it is the middle of a larger allocation whose other rows are non-zero, so a read
    that ignored the bounds would land in allocated memory and show up as a non-zero value."""
    from cbas_amd import _lib
    lib = _lib.load()
    T, n, pad = 31, 200, 64
    phys = random_halves(5, n + 2 * pad, D)
    phys[:pad] = np.float16(3.0)
    phys[pad + n:] = np.float16(-5.0)
    dev = torch.from_numpy(phys).cuda()
    logical = dev[pad:pad + n]
    first = [-T - 5, -T, -T + 1, -3, 0, n - T, n - T + 2, n - 1, n, n + 1000, -2 ** 62, 2 ** 62, 2 ** 63 - 1, -2 ** 63, -2 ** 63 + 5,
             2 ** 63 - T]
    f = torch.tensor(first, dtype=torch.int64).cuda()
    out = torch.full((len(first), T, D), 9.0, device="cuda")
    rc = lib.cbas_rows_gather_windows(logical.data_ptr(), n, D, f.data_ptr(), len(first), T, out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.cbas_last_error()
    got = out.cpu().numpy()
    want = gather_ref(phys[pad:pad + n], first, T)
    assert same_bits(got, want)
    for w in (0, 1, 8, 9, 10, 11, 12, 13, 14, 15):         # wholly outside: nothing but zeros
        assert not got[w].any(), first[w]
    assert not got[2, :T - 1].any() and got[2, T - 1].any() and not got[7, 1:].any() and got[7, 0].any()
    # an empty logical store: every window is zeros
    rc = lib.cbas_rows_gather_windows(logical.data_ptr(), 0, D, f.data_ptr(), len(first), T, out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and not out.cpu().numpy().any()


def test_argument_errors_return_einval():
    from cbas_amd import _lib
    from cbas_amd.train import HeadTrainer
    lib = _lib.load()
    rows = torch.zeros((64, 768), dtype=torch.float16, device="cuda")
    f = torch.zeros(4, dtype=torch.int64, device="cuda")
    y = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros((4, 31, 768), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    R, F, O = rows.data_ptr(), f.data_ptr(), out.data_ptr()
    for args in [(None, 64, 768, F, 4, 31, O), (R, 64, 768, None, 4, 31, O), (R, 64, 768, F, 4, 31, None), (R, -1, 768, F, 4, 31, O),
                 (R, 64, 0, F, 4, 31, O), (R, 64, 768, F, 0, 31, O), (R, 64, 768, F, -2, 31, O), (R, 64, 768, F, 4, 0, O),
                 (R, 64, 768, F, 4, 1 << 17, O), (R, 64, 1 << 20, F, 4, 31, O)]:
        assert lib.cbas_rows_gather_windows(*args, st) == EINVAL, args
        assert lib.cbas_last_error()
    hcfg = CFG.HeadConfig(in_features=768, out_features=9)
    tr = HeadTrainer(hcfg, W.synth_head_weights(hcfg, 4321), "cuda", max_batch=4)
    Y = y.data_ptr()
    for args in [(None, R, 64, 768, F, Y, 4, 31), (tr._h, None, 64, 768, F, Y, 4, 31), (tr._h, R, 64, 768, None, Y, 4, 31),
                 (tr._h, R, 64, 768, F, None, 4, 31), (tr._h, R, 64, 384, F, Y, 4, 31), (tr._h, R, 64, 768, F, Y, 4, 33),
                 (tr._h, R, 64, 768, F, Y, 5, 31), (tr._h, R, 64, 768, F, Y, 0, 31), (tr._h, R, -1, 768, F, Y, 4, 31)]:
        assert lib.cbas_head_train_step_rows(*args, 0, None, st) == EINVAL, args[1:]
        assert lib.cbas_last_error()
    assert tr.step_rows(rows, f, y.long(), update=False) is not None          # and the well-formed call goes through
    with pytest.raises(ValueError):
        tr.step_rows(rows.float(), f, y.long())
    tr.close()


@pytest.mark.parametrize("tag", ["h64", "h48_noacc_l2"])                       # two of test_gpu_train.py's CASES
def test_step_rows_equals_step_on_the_same_windows(tag):
    from cbas_amd.train import HeadTrainer
    h, nl, acc = {"h64": (64, 1, True), "h48_noacc_l2": (48, 2, False)}[tag]
    hcfg = CFG.HeadConfig(in_features=768, out_features=9, lstm_hidden_size=h, lstm_layers=nl, use_acceleration=acc)
    hw = W.synth_head_weights(hcfg, 4321)
    rows = synth.cls_walk(3, 400, 768)
    rng = np.random.default_rng(8)
    first = np.concatenate([[0, 400 - 31], rng.integers(0, 370, 35)]).astype(np.int64)
    labels = rng.integers(0, 9, len(first)).astype(np.int64)
    x = np.stack([rows[f:f + 31] for f in first]).astype(np.float32)          # the windows, gathered by numpy
    dev_rows = torch.from_numpy(rows).cuda()
    res = []
    for by_rows in (False, True):
        tr = HeadTrainer(hcfg, hw, "cuda", lr=1e-3, weight_decay=1e-2, label_smoothing=0.05, max_batch=64, seed=6, dropout=True)

        def step(update):
            if by_rows:
                return tr.step_rows(dev_rows, torch.from_numpy(first), torch.from_numpy(labels), update=update)
            return tr.step(torch.from_numpy(x), torch.from_numpy(labels), update=update)
        loss0 = step(False)
        grads = tr.grads()
        losses = [step(True) for _ in range(3)]
        res.append((loss0, grads, losses, tr.weights()))
        tr.close()
    (l0a, ga, la, wa), (l0b, gb, lb, wb) = res
    assert l0a == l0b and la == lb, (l0a, l0b, la, lb)
    for k in hw:
        assert np.array_equal(ga[k], gb[k]) and np.array_equal(wa[k], wb[k]), k
    assert any(not np.array_equal(wa[k], np.asarray(hw[k], np.float32)) for k in hw)       # the steps did move the weights


# ---------------------------------------------------------------------------------------------------------------
# train_lstm_model on manifests
# ---------------------------------------------------------------------------------------------------------------
BEHAVIORS = ["a", "b", "c", "d"]


@pytest.fixture(scope="module")
def manifests(tmp_path_factory):
    """Three readable files and one that is not an HDF5 file; a train manifest over files 0, 1 and the bad one, a
    validation manifest over file 2 and the bad one."""
    from cbas_amd.datasets import make_manifest
    root = str(tmp_path_factory.mktemp("resident_project"))
    paths, labels = synth.cls_project(root, [400, 500, 300], 768, 4, 21)
    bad = os.path.join(root, "broken_cls.h5")
    with open(bad, "wb") as f:
        f.write(b"not an HDF5 file " * 64)
    inst = [[(p, a, b, BEHAVIORS[c]) for a, b, c in synth.label_runs(l)] for p, l in zip(paths, labels)]
    train = make_manifest(inst[0] + inst[1], 31, BEHAVIORS)
    val = make_manifest(inst[2], 31, BEHAVIORS)
    train = train[:300] + [(bad, 40 + i, i % 4) for i in range(25)] + train[300:]
    val = val[:100] + [(bad, 90 + i, 1) for i in range(10)] + val[100:]
    return train, val


def run_training(monkeypatch, manifests, env, epochs=3):
    from cbas_amd import datasets as D
    from cbas_amd.train import train_lstm_model
    for k in ("CBAS_TRAIN_RESIDENT", "CBAS_TRAIN_RESIDENT_MAX_GB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    train, val = manifests
    lines = []
    model, reports, best = train_lstm_model(D.LazyBalancedDataset(train, 31, BEHAVIORS), D.LazyStandardDataset(val, 31), 31, BEHAVIORS,
                                            threading.Event(), batch_size=64, lr=2e-3, epochs=epochs, device="cuda", patience=5,
                                            seed=4, log=lines.append)
    sd = {k: v.numpy().copy() for k, v in model.state_dict().items()}
    model.close()
    D.close_readers()
    return sd, reports, best, [l for l in lines if l.startswith("training data:")]


def assert_same_run(a, b):
    (sda, ra, ba, _), (sdb, rb, bb, _) = a, b
    assert ba == bb and len(ra) == len(rb) == 3
    for x, y in zip(ra, rb):
        assert np.array_equal(x.train_cm, y.train_cm) and np.array_equal(x.val_cm, y.val_cm)
        assert x.train_report == y.train_report and x.val_report == y.val_report
    assert set(sda) == set(sdb)
    for k in sda:
        assert np.array_equal(sda[k].view(np.uint32), sdb[k].view(np.uint32)), k


@pytest.fixture(scope="module")
def host_run(manifests):
    mp = pytest.MonkeyPatch()
    try:
        return run_training(mp, manifests, {"CBAS_TRAIN_RESIDENT": "0"})
    finally:
        mp.undo()


def test_resident_and_host_loader_runs_are_identical(monkeypatch, manifests, host_run):
    res = run_training(monkeypatch, manifests, {"CBAS_TRAIN_RESIDENT": "1"})
    assert len(host_run[3]) == 1 and host_run[3][0] == "training data: host loader (CBAS_TRAIN_RESIDENT=0)"
    assert len(res[3]) == 1 and res[3][0] == "training data: resident in HBM (3 files, 1 200 rows, 2 MB)", res[3]
    assert_same_run(host_run, res)
    # the runs dropped the windows of the unreadable file
    train, val = manifests
    assert host_run[1][0].val_cm.sum() == len(val) - 10
    n_train = len(train) + (-len(train)) % 4            # the balanced length; some of its draws hit the unreadable file
    assert 0 < int(host_run[1][0].train_cm.sum()) < n_train
    # without either switch the rows are resident too
    default = run_training(monkeypatch, manifests, {}, epochs=3)
    assert default[3][0].startswith("training data: resident")
    assert_same_run(host_run, default)


def test_memory_rule_selects_the_host_loader(monkeypatch, manifests, host_run):
    res = run_training(monkeypatch, manifests, {"CBAS_TRAIN_RESIDENT_MAX_GB": "0.001"})       # 1 MB allowed, 1.8 MB needed
    assert len(res[3]) == 1 and res[3][0].startswith("training data: host loader (1 200 rows need 2 MB, 1 MB may be used"), res[3]
    assert_same_run(host_run, res)
    roomy = run_training(monkeypatch, manifests, {"CBAS_TRAIN_RESIDENT_MAX_GB": "1"})
    assert roomy[3][0].startswith("training data: resident")
    assert_same_run(host_run, roomy)


def test_reference_style_instances_train_without_getitem(monkeypatch, manifests, host_run):
    """Objects with only the reference's attribute names (no resolve(), a __getitem__ that must not run): recognised, and
    the run equals the host loader's on this package's classes."""
    from cbas_amd import datasets as D
    from cbas_amd.train import train_lstm_model
    monkeypatch.delenv("CBAS_TRAIN_RESIDENT", raising=False)
    monkeypatch.delenv("CBAS_TRAIN_RESIDENT_MAX_GB", raising=False)
    train, val = manifests

    class Foreign(torch.utils.data.Dataset):
        def __init__(self, like):
            self.__dict__.update(like.__dict__)
            self._n = len(like)

        def __len__(self):
            return self._n

        def __getitem__(self, i):
            raise AssertionError("the reference's __getitem__ needs h5py: it must not be called")

    lines = []
    tr = Foreign(D.LazyBalancedDataset(train, 31, BEHAVIORS))
    model, reports, best = train_lstm_model(tr, Foreign(D.LazyStandardDataset(val, 31)), 31, BEHAVIORS, threading.Event(),
                                            batch_size=64, lr=2e-3, epochs=3, device="cuda", patience=5, seed=4, log=lines.append)
    sd = {k: v.numpy().copy() for k, v in model.state_dict().items()}
    model.close()
    assert tr.counter == 3 * 2 * len(tr)                   # a training and a scoring pass per epoch advanced the instance's counter
    assert_same_run(host_run, (sd, reports, best, lines))
    assert any(l.startswith("training data: resident") for l in lines)


def test_mixed_row_width_is_refused_by_name(monkeypatch, manifests, tmp_path):
    from cbas_amd import datasets as D, h5io
    from cbas_amd.train import train_lstm_model
    monkeypatch.delenv("CBAS_TRAIN_RESIDENT", raising=False)
    narrow = str(tmp_path / "narrow_cls.h5")
    with h5io.ClsWriter(narrow, 384) as w:
        w.append(synth.cls_walk(1, 100, 384))
    train, val = manifests
    with pytest.raises(ValueError, match="narrow_cls.h5"):
        train_lstm_model(D.LazyStandardDataset(train + [(narrow, 50, 0)], 31), None, 31, BEHAVIORS, threading.Event(), batch_size=64,
                         epochs=1, device="cuda", log=lambda s: None)


def test_ordinary_datasets_keep_the_host_loader(monkeypatch):
    from cbas_amd.train import train_lstm_model
    monkeypatch.delenv("CBAS_TRAIN_RESIDENT", raising=False)
    x, y = synth.train_windows(31, 160, 768, 4, 31)

    class DS(torch.utils.data.Dataset):                    # the DS of tests/test_gpu_train.py
        def __init__(self, a, b):
            self.a, self.b = a, b

        def __len__(self):
            return len(self.b)

        def __getitem__(self, i):
            return torch.from_numpy(self.a[i]), torch.tensor(int(self.b[i]))

    lines = []
    model, reports, best = train_lstm_model(DS(x[:128], y[:128]), DS(x[128:], y[128:]), 31, BEHAVIORS, threading.Event(), batch_size=64,
                                            lr=2e-3, epochs=2, device="cuda", seed=1, log=lines.append)
    assert model is not None and len(reports) == 2 and 0 <= best < 2
    model.close()
    data = [l for l in lines if l.startswith("training data:")]
    assert data == ["training data: host loader (the training set is not a manifest dataset)"]


def test_epoch_rate_resident_next_to_the_host_loader(monkeypatch, tmp_path, capsys):
    """About 20 000 windows over 4 files (T = 31, D = 768, batch 512): one training pass and one scoring pass
    (train_lstm_model with epochs=1 and no validation set, everything it does included) with the rows resident, next to
    the same call through the host loader (CBAS_TRAIN_RESIDENT=0: the unchanged path, the baseline).  Both warmed up by a
    first call.  Asserted only: the resident call is faster."""
    from cbas_amd import datasets as D
    from cbas_amd.train import train_lstm_model
    names = [f"b{i}" for i in range(9)]
    paths, labels = synth.cls_project(str(tmp_path), [5031] * 4, 768, 9, 5)
    manifest = D.make_manifest([(p, a, b, names[c]) for p, l in zip(paths, labels) for a, b, c in synth.label_runs(l)], 31, names)
    assert len(manifest) == 4 * 5001
    monkeypatch.delenv("CBAS_TRAIN_RESIDENT_MAX_GB", raising=False)
    times = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("CBAS_TRAIN_RESIDENT", mode)
        for rep in range(2):
            lines = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model, reports, best = train_lstm_model(D.LazyStandardDataset(manifest, 31), None, 31, names, threading.Event(),
                                                    batch_size=512, epochs=1, device="cuda", seed=2, log=lines.append)
            torch.cuda.synchronize()
            times[mode] = time.perf_counter() - t0
            model.close()
            assert int(reports[0].train_cm.sum()) == len(manifest)
            assert any(l.startswith("training data: resident" if mode == "1" else "training data: host loader") for l in lines)
    D.close_readers()
    n_batches = -(-len(manifest) // 512)
    with capsys.disabled():
        print(f"\ntrain + score pass over {len(manifest)} windows ({n_batches} batches of 512): host loader {times['0']:.3f} s, "
              f"resident {times['1']:.3f} s -> {times['0'] / times['1']:.1f}x")
    assert times["1"] < times["0"]
