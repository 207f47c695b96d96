"""The tail of a training job on the device: cbas_head_score_rows against the existing path (gather + head + host argmax +
sklearn), cbas_logits_nll against float64 numpy, evaluate_on_split and fit_temperature from resident rows against the host
loader and against what the reference produced (tests/golden/evaluate_on_split.npz, fit_temperature.npz), and a whole tail
inside keep_rows() on one store."""
import os

import numpy as np
import pytest
import torch

from cbas_amd import config as CFG, synth, weights as W

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FACTOR = 4.0                    # see tests/test_train_tail_host.py: the same bound holds for the device's closure


def temperature_bound(fx, name):
    t32, t64 = float(fx[f"{name}/temperature"]), float(fx[f"{name}/temperature_f64_logits"])
    return FACTOR * max(abs(t32 - t64), float(np.spacing(np.float32(t32))))


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def make_head(C, seed=3, hidden=64, layers=1):
    from cbas_amd.head import ClassifierLSTMDeltas
    cfg = CFG.HeadConfig(in_features=768, out_features=C, seq_len=31, lstm_hidden_size=hidden, lstm_layers=layers)
    m = ClassifierLSTMDeltas(768, C, seq_len=31, lstm_hidden_size=hidden, lstm_layers=layers)
    m.load_state_dict(W.synth_head_weights(cfg, seed))
    return m.to("cuda").eval()


@pytest.fixture(scope="module")
def rows():
    """A store of 3 000 CLS-like rows, with runs of identical rows so that some windows are constant."""
    r = synth.cls_walk(17, 3000, 768)
    return torch.from_numpy(np.ascontiguousarray(r)).cuda()


def existing_path(model, rows, first, labels, C):
    """gather_windows + model(x) in batches of 512 + host argmax + sklearn: what train_lstm_model's scoring does today."""
    from sklearn.metrics import confusion_matrix
    from cbas_amd.train import gather_windows
    logits = []
    for a in range(0, len(first), 512):
        x = gather_windows(rows, torch.from_numpy(first[a:a + 512]), 31)
        logits.append(model(x)[0].cpu().numpy())
    logits = np.concatenate(logits)
    pred = torch.from_numpy(logits).argmax(1).numpy()
    return logits, pred, confusion_matrix(labels, pred, labels=range(C))


@pytest.mark.parametrize("C", [2, 9])
@pytest.mark.parametrize("n", [1, 511, 512, 513, 20004])
def test_score_rows_equals_gather_forward_argmax_confusion(rows, C, n):
    model = make_head(C, seed=C)
    rng = np.random.default_rng(n * 10 + C)
    first = rng.integers(0, rows.shape[0] - 31 + 1, n).astype(np.int64)
    labels = rng.integers(0, C - 1, n).astype(np.int64)              # class C - 1 never occurs as a label
    want_logits, want_pred, want_cm = existing_path(model, rows, first, labels, C)
    logits, pred, cm = model.score_rows(rows, torch.from_numpy(first), torch.from_numpy(labels), want_logits=True, want_pred=True)
    assert same_bits(logits.cpu().numpy(), want_logits)
    assert pred.dtype == torch.int32 and np.array_equal(pred.cpu().numpy(), want_pred)
    assert cm.dtype == torch.int64 and np.array_equal(cm.cpu().numpy(), want_cm) and int(cm.sum()) == n
    assert int(cm[C - 1].sum()) == 0
    # the matrix alone (what evaluate_on_split asks for), and twice the same
    for _ in range(2):
        _, _, again = model.score_rows(rows, torch.from_numpy(first), torch.from_numpy(labels))
        assert np.array_equal(again.cpu().numpy(), want_cm)
    model.close()


@pytest.mark.parametrize("C", [2, 9])
def test_first_of_tied_maxima_wins(C):
    """Ties made on purpose: with lin2 and lin1 zeroed the logits are the gate-weighted sum of two equal bias vectors, the
    same for every window; the bias holds its maximum twice (and, for C = 9, a third time at the end)."""
    from cbas_amd.head import ClassifierLSTMDeltas
    cfg = CFG.HeadConfig(in_features=768, out_features=C, seq_len=31)
    w = W.synth_head_weights(cfg, 5)
    bias = np.linspace(-1.0, 0.0, C).astype(np.float32)
    tied = [0, 1] if C == 2 else [3, 6, 8]
    bias[tied] = 0.5
    for k in ("lin1.weight", "lin2.weight"):
        w[k] = np.zeros_like(w[k])
    w["lin1.bias"], w["lin2.bias"] = bias.copy(), bias.copy()
    model = ClassifierLSTMDeltas(768, C, seq_len=31)
    model.load_state_dict(w)
    model.to("cuda")
    r = torch.from_numpy(np.ascontiguousarray(synth.cls_walk(3, 700, 768))).cuda()
    first = np.arange(0, 600, dtype=np.int64)
    labels = (first % C).astype(np.int64)
    logits, pred, cm = model.score_rows(r, torch.from_numpy(first), torch.from_numpy(labels), want_logits=True, want_pred=True)
    z = logits.cpu().numpy()
    assert all(np.array_equal(z[:, tied[0]], z[:, t]) for t in tied) and (z.max(axis=1) == z[:, tied[0]]).all()   # the ties are there
    assert (pred.cpu().numpy() == tied[0]).all()
    assert np.array_equal(pred.cpu().numpy(), torch.from_numpy(z).argmax(1).numpy())
    want = np.zeros((C, C), np.int64)
    want[:, tied[0]] = np.bincount(labels, minlength=C)
    assert np.array_equal(cm.cpu().numpy(), want)
    model.close()


def test_score_rows_refusals(rows):
    from cbas_amd import _lib
    model = make_head(3)
    first = torch.arange(0, 40, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="label lies outside"):
        model.score_rows(rows, first, torch.full((40,), 3, dtype=torch.int64))
    with pytest.raises(ValueError):
        model.score_rows(rows, first)                                   # nothing asked for
    with pytest.raises(ValueError):
        model.score_rows(rows[:, :384].contiguous(), first, want_pred=True)
    # a NaN logit row is an error, not a label: rows outside the store read as zeros, so poison the weights instead
    cfg = CFG.HeadConfig(in_features=768, out_features=3, seq_len=31)
    w = W.synth_head_weights(cfg, 3)
    w["lin2.bias"] = np.array([0.0, np.nan, 0.0], np.float32)
    from cbas_amd.head import ClassifierLSTMDeltas
    bad = ClassifierLSTMDeltas(768, 3, seq_len=31)
    bad.load_state_dict(w)
    bad.to("cuda")
    with pytest.raises(RuntimeError, match="NaN"):
        bad.score_rows(rows, first, torch.zeros(40, dtype=torch.int64))
    bad.close()
    # the handle still works after a refusal
    _, pred, _ = model.score_rows(rows, first, want_pred=True)
    assert pred.shape == (40,) and _lib.load().cbas_abi_version() == 11
    model.close()


# ---------------------------------------------------------------------------------------------------------------
# cbas_logits_nll
# ---------------------------------------------------------------------------------------------------------------
def numpy_nll(z32, labels, temp):
    z = z32.astype(np.float64)
    rows = np.arange(len(labels))
    x = z / float(temp)
    x = x - x.max(axis=1, keepdims=True)
    e = np.exp(x)
    p = e / e.sum(axis=1, keepdims=True)
    loss = -(x[rows, labels] - np.log(e.sum(axis=1)))
    slope = (z[rows, labels] - (p * z).sum(axis=1)) / float(temp) ** 2
    return loss, slope


def nll_bounds(z32, labels, temp):
    """Bounds on |device - float64| for the mean loss and the mean derivative, from the float32 arithmetic of the kernel.
    With u = 2^-24 (float32 unit roundoff), C classes, x = z / temp, A = max |x|:
      * a row's loss is log(sum exp(x - m)) - (x_y - m): each x carries one rounding (A u), x - m another (2 A u at most),
        exp and log are accurate to a few ulp (taken as 4 u relative each: 2 ulp functions), the C-term sum adds C u
        relative, and the final subtraction u relative of a value <= 2 A + log C.  Row error <= u (3 A + (C + 8) + (2 A + log C))
        <= u (5 A + C + 8 + log C).
      * a row's derivative is (z_y - sum e z / sum e) / temp^2: the weights e carry (2 A + 4) u relative error each, the two
        C-term sums C u each, the quotient, difference and the division by temp^2 four more; the value is at most
        2 Z / temp^2 with Z = max |z|.  Row error <= u (2 A + 2 C + 12) * 2 Z / temp^2.
      * the sum of n such terms in float32 (a thread's sequential part of at most ceil(n / 256) terms, then trees of depth
        8 + 8) adds u (ceil(n / 256) + 16) relative to the sum of magnitudes, i.e. to the mean of |terms| after the division
        by n, which itself adds u.
    """
    u = 2.0 ** -24
    n, C = z32.shape
    A = float(np.abs(z32.astype(np.float64) / temp).max())
    Z = float(np.abs(z32).max())
    loss, slope = numpy_nll(z32, labels, temp)
    chain = (np.ceil(n / 256) + 17) * u
    b_loss = u * (5 * A + C + 8 + np.log(C)) + chain * float(np.abs(loss).mean())
    row_slope = u * (2 * A + 2 * C + 12) * 2 * Z / temp ** 2
    b_slope = row_slope + chain * (float(np.abs(slope).mean()) + row_slope)
    return float(loss.mean()), float(slope.mean()), b_loss, b_slope


def test_logits_nll_against_float64_and_bitwise_repeatable():
    from cbas_amd.train import device_nll
    fx = np.load(os.path.join(GOLDEN, "fit_temperature.npz"))
    rng = np.random.default_rng(0)
    cases = [(str(n), fx[f"{n}/logits"], fx[f"{n}/labels"]) for n in fx["names"]]
    z = (rng.standard_normal((70001, 20)) * 3).astype(np.float32)          # more rows than one pass of the grid, C = 20
    cases.append(("large", z, rng.integers(0, 20, 70001)))
    for name, z32, labels in cases:
        f = device_nll(torch.from_numpy(z32).cuda(), torch.from_numpy(labels).cuda())
        for temp in (0.05, 0.7, 1.3143, 10.0):
            temp32 = float(np.float32(temp))
            got = f(temp32)
            again = f(temp32)
            want_loss, want_slope, b_loss, b_slope = nll_bounds(z32, labels, temp32)
            print(f"{name} temp {temp}: loss {got[0]:.9g} (float64 {want_loss:.9g}, gap {abs(got[0] - want_loss):.2e}, bound {b_loss:.2e}); "
                  f"slope {got[1]:.9g} (float64 {want_slope:.9g}, gap {abs(got[1] - want_slope):.2e}, bound {b_slope:.2e})")
            assert abs(float(got[0]) - want_loss) <= b_loss, (name, temp)
            assert abs(float(got[1]) - want_slope) <= b_slope, (name, temp)
            assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes(), (name, temp)
    with pytest.raises(ValueError):
        device_nll(torch.zeros(4, 3).cuda(), torch.tensor([0, 1, 2, 3]).cuda())


# ---------------------------------------------------------------------------------------------------------------
# evaluate_on_split / fit_temperature on manifests
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def manifest_project(tmp_path_factory):
    from cbas_amd import datasets as D
    root = str(tmp_path_factory.mktemp("tail_project"))
    behaviors = ["a", "b", "c", "d"]
    paths, labels = synth.cls_project(root, [700, 900, 500], 768, 4, 41)
    inst = [(paths[f], a, b, behaviors[c]) for f, lab in enumerate(labels) for a, b, c in synth.label_runs(lab)]
    manifest = D.make_manifest(inst, 31, behaviors)
    per_file = {p: [m for m in manifest if m[0] == p] for p in paths}
    return D, paths, behaviors, manifest, per_file


def captured(fn, capsys):
    capsys.readouterr()
    out = fn()
    return out, [l for l in capsys.readouterr().out.splitlines() if l.startswith("training data:")]


def test_evaluate_on_split_resident_equals_host_loader(manifest_project, monkeypatch, capsys):
    from cbas_amd.train import evaluate_on_split
    D, paths, behaviors, manifest, per_file = manifest_project
    model = make_head(4, seed=8)
    for ds in (D.LazyStandardDataset(manifest, 31), D.LazyBalancedDataset(per_file[paths[1]], 31, behaviors)):
        monkeypatch.delenv("CBAS_TRAIN_RESIDENT", raising=False)
        res, lines = captured(lambda: evaluate_on_split(model, ds, behaviors, device=torch.device("cuda")), capsys)
        assert len(lines) == 1 and lines[0].startswith("training data: resident in HBM ("), lines
        monkeypatch.setenv("CBAS_TRAIN_RESIDENT", "0")
        if hasattr(ds, "counter"):
            ds.counter = 0
        host, lines = captured(lambda: evaluate_on_split(model, ds, behaviors, device=torch.device("cuda")), capsys)
        assert lines == ["training data: host loader (CBAS_TRAIN_RESIDENT=0)"], lines
        assert res["cm"].dtype == host["cm"].dtype and np.array_equal(res["cm"], host["cm"]) and int(res["cm"].sum()) == len(ds)
        assert res["report"] == host["report"] and set(res["report"]) >= set(behaviors) | {"macro avg", "weighted avg"}
    monkeypatch.delenv("CBAS_TRAIN_RESIDENT", raising=False)
    # nothing to score: an unreadable file behind every entry, an empty dataset
    gone = [(os.path.join(os.path.dirname(paths[0]), "gone_cls.h5"), 40, 1)]
    for ds in (D.LazyStandardDataset(gone, 31), D.LazyStandardDataset([], 31)):
        res = evaluate_on_split(model, ds, behaviors, device=torch.device("cuda"))
        assert res["report"] == {} and res["cm"].size == 0
    model.close()


def test_evaluate_on_split_against_the_reference_fixture(tmp_path, capsys):
    """Matrix equal to the reference's wherever the reference's own top-2 margin exceeds the measured logit error of this
    head; at most 1 % of the windows may lie below it (the fixture was chosen with every margin > 1e-3)."""
    import json
    from cbas_amd import datasets as D
    from cbas_amd.head import ClassifierLSTMDeltas
    from cbas_amd.train import evaluate_on_split, keep_rows, open_store
    fx = np.load(os.path.join(GOLDEN, "evaluate_on_split.npz"))
    behaviors = [str(b) for b in fx["behaviors"]]
    paths, _ = synth.cls_project(str(tmp_path), fx["sizes"].tolist(), int(fx["dim"]), len(behaviors), int(fx["seed"]),
                                 skip_classes=tuple(fx["skip_classes"].tolist()))
    manifest = [(paths[f], int(c), int(l)) for f, c, l in zip(fx["manifest/file"], fx["manifest/centre"], fx["manifest/label"])]
    T = int(fx["seq_len"])
    cfg = CFG.HeadConfig(in_features=int(fx["dim"]), out_features=len(behaviors), seq_len=T)
    model = ClassifierLSTMDeltas(int(fx["dim"]), len(behaviors), seq_len=T)
    model.load_state_dict(W.synth_head_weights(cfg, int(fx["head_seed"])))
    model.to("cuda")
    ds = D.LazyStandardDataset(manifest, T)
    with keep_rows():
        res = evaluate_on_split(model, ds, behaviors, device=torch.device("cuda"))
        store = open_store([ds], ("test",), T, int(fx["dim"]), torch.device("cuda"), lambda line: None)
        first, labels = D.manifest_windows(manifest, T, store.files)
        logits, pred, _ = model.score_rows(store.rows, torch.from_numpy(first), want_logits=True, want_pred=True)
    ref = fx["logits"]
    err = float(np.abs(logits.cpu().numpy() - ref).max())
    top2 = np.sort(ref, axis=1)[:, -2:]
    margin = top2[:, 1] - top2[:, 0]
    clear = margin > err
    print(f"logit error of the head against the reference {err:.3e}; smallest reference margin {margin.min():.3e}; "
          f"{int((~clear).sum())} of {len(clear)} windows below it")
    assert (~clear).mean() <= 0.01
    assert np.array_equal(pred.cpu().numpy()[clear], ref.argmax(1)[clear])
    if clear.all():
        assert np.array_equal(res["cm"], fx["cm"])
        assert res["report"] == json.loads(str(fx["report_json"]))
    model.close()


def fixture_fit(name, fx, resident, tmp_path):
    """fit_temperature end to end on the fixture's logits: a head cannot be made to emit given logits, so the model is
    a stand-in that serves them from the device, as tests/golden/make_goldens_calibration.py serves them to the reference."""
    from cbas_amd.train import fit_temperature
    z, y, batch = torch.from_numpy(fx[f"{name}/logits"]).cuda(), torch.from_numpy(fx[f"{name}/labels"]), int(fx[f"{name}/batch"])

    class Served:
        def to(self, device):
            return self

        def eval(self):
            return self

        def __call__(self, d):
            return z[d.long().reshape(-1)], None

    index = torch.arange(len(y), dtype=torch.float32)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(index, y), batch_size=batch)
    return fit_temperature(Served(), loader, torch.device("cuda"))


def test_fit_temperature_on_device_logits_against_the_reference(tmp_path):
    fx = np.load(os.path.join(GOLDEN, "fit_temperature.npz"))
    failures = []
    for name in [str(n) for n in fx["names"]]:
        temp = fixture_fit(name, fx, False, tmp_path)
        want, bound = float(fx[f"{name}/temperature"]), temperature_bound(fx, name)
        print(f"{name}: temperature {temp:.9f}, reference {want:.9f}, gap {abs(temp - want):.3e}, bound {bound:.3e}")
        assert isinstance(temp, float) and temp == fixture_fit(name, fx, False, tmp_path)          # a second run: the same bits
        if not abs(temp - want) <= bound:
            failures.append((name, temp, want, bound))
    assert not failures, failures


def test_fit_temperature_resident_equals_host_loader_bit_for_bit(manifest_project, monkeypatch, capsys):
    from cbas_amd.train import fit_temperature
    D, paths, behaviors, manifest, per_file = manifest_project
    model = make_head(4, seed=8)
    val = D.LazyStandardDataset(per_file[paths[0]] + per_file[paths[2]], 31)
    dev = torch.device("cuda")

    def loader():
        return torch.utils.data.DataLoader(val, batch_size=200, num_workers=0)

    monkeypatch.delenv("CBAS_TRAIN_RESIDENT", raising=False)
    resident, lines = captured(lambda: fit_temperature(model, loader(), dev), capsys)
    assert len(lines) == 1 and lines[0].startswith("training data: resident in HBM (2 files"), lines
    again = fit_temperature(model, loader(), dev)
    monkeypatch.setenv("CBAS_TRAIN_RESIDENT", "0")
    host, lines = captured(lambda: fit_temperature(model, loader(), dev), capsys)
    assert lines == ["training data: host loader (CBAS_TRAIN_RESIDENT=0)"], lines
    monkeypatch.delenv("CBAS_TRAIN_RESIDENT", raising=False)
    print(f"temperature: resident {resident!r}, host loader {host!r}")
    assert isinstance(resident, float) and resident == again == host and 1e-3 < resident <= 10.0
    # an empty loader, and a window that cannot be served
    assert fit_temperature(model, torch.utils.data.DataLoader(D.LazyStandardDataset([], 31), batch_size=8), dev) == 1.0
    gone = os.path.join(os.path.dirname(paths[0]), "gone_cls.h5")
    broken = D.LazyStandardDataset(per_file[paths[0]][:50] + [(gone, 40, 1)], 31)
    with pytest.raises(ValueError, match="gone_cls.h5"):
        fit_temperature(model, torch.utils.data.DataLoader(broken, batch_size=16), dev)
    model.close()


def test_a_whole_tail_runs_on_one_store(manifest_project, monkeypatch):
    from cbas_amd.train import evaluate_on_split, fit_temperature, keep_rows, train_lstm_model
    D, paths, behaviors, manifest, per_file = manifest_project
    monkeypatch.delenv("CBAS_TRAIN_RESIDENT", raising=False)
    dev = torch.device("cuda")

    def sets():
        return (D.LazyBalancedDataset(per_file[paths[0]] + per_file[paths[1]], 31, behaviors), D.LazyStandardDataset(per_file[paths[2]], 31))

    def train(log):
        train_ds, val_ds = sets()
        return train_lstm_model(train_ds, val_ds, 31, behaviors, None, batch_size=256, epochs=2, device=dev, seed=5, log=log)

    outside_lines = []
    outside, _, _ = train(outside_lines.append)
    lines = []
    printed = []
    monkeypatch.setattr("builtins.print", lambda *a, **k: printed.append(" ".join(str(x) for x in a)))
    with keep_rows() as cache:
        inside, _, best_epoch = train(lines.append)
        kept = cache.store
        # the test split lies in a file of the training manifest here, so that the kept store serves it
        res = evaluate_on_split(inside, D.LazyStandardDataset(per_file[paths[1]][::3], 31), behaviors, device=dev)
        val = D.LazyStandardDataset(per_file[paths[2]], 31)
        temp = fit_temperature(inside, torch.utils.data.DataLoader(val, batch_size=256, num_workers=0), dev)
        assert cache.store is kept
    monkeypatch.undo()
    data_lines = [l for l in lines + printed if l.startswith("training data:")]
    assert sum("resident in HBM" in l for l in data_lines) == 1 and sum("kept rows reused" in l for l in data_lines) == 2, data_lines
    assert cache.store is None
    a, b = outside.state_dict(), inside.state_dict()
    assert a.keys() == b.keys() and all(same_bits(a[k].numpy().reshape(-1), b[k].numpy().reshape(-1)) for k in a)
    assert sum("resident in HBM" in l for l in outside_lines) == 1
    assert int(res["cm"].sum()) == len(per_file[paths[1]][::3]) and isinstance(temp, float) and 1e-3 < temp <= 10.0
    # what the bundle writer reads next (workthreads.py:875-877)
    assert int(getattr(inside.lstm, "hidden_size", -1)) == 64 and int(getattr(inside.lstm, "num_layers", -1)) == 1
    outside.close(), inside.close()
