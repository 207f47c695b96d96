"""The tail of a training job, host side (no GPU): the scalar L-BFGS of cbas_amd.train.fit_temperature against the
temperatures, iteration counts and closure-call counts the reference's fit_temperature produced
(tests/golden/fit_temperature.npz, recorded by tests/golden/make_goldens_calibration.py), the keep_rows() store cache with a
stand-in for the device store, the attributes the reference's bundle writer reads from the head, and install() /
uninstall() of the two new names against the real reference modules."""
import gc
import os
import subprocess
import sys
import textwrap
import weakref

import numpy as np
import pytest

from cbas_amd import synth

GOLD = os.path.join(os.path.dirname(__file__), "golden", "fit_temperature.npz")
REF = "/root/reference"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Tolerance of a restated fit against the reference's temperature.  The fixture holds the reference's own result twice: with
# float32 logits (what CBAS computes) and with the same logits as float64.  The two runs execute the same optimiser on the
# same float32 parameter; only the rounding of the loss and of its gradient differs - which is also the only thing in which
# a statement-for-statement restatement of the optimiser may differ from either.  So the reference's own spread between the
# two is the size of the permitted gap.  The temperature is returned as a float32 number, so a recorded spread of 0 means
# "below one float32 step", not "none": the spread is taken as at least one float32 ulp of the temperature.  FACTOR covers
# that a third way of rounding (float64 numpy here, the device's fp32 sums in tests/test_gpu_train_tail.py) need not fall
# between the two recorded ones: it may miss each of them by the spread on either side, and the trajectory of 50 steps is
# shared, hence 2 x 2.
FACTOR = 4.0


def temperature_bound(fx, name):
    t32, t64 = float(fx[f"{name}/temperature"]), float(fx[f"{name}/temperature_f64_logits"])
    ulp = float(np.spacing(np.float32(t32)))
    return FACTOR * max(abs(t32 - t64), ulp)


def numpy_nll(logits, labels):
    """temp -> (mean cross-entropy of logits / temp, d / d temp) in float64."""
    z = logits.astype(np.float64)
    rows = np.arange(len(labels))

    def f(temp):
        x = z / float(temp)
        x = x - x.max(axis=1, keepdims=True)
        e = np.exp(x)
        p = e / e.sum(axis=1, keepdims=True)
        loss = -(x[rows, labels] - np.log(e.sum(axis=1))).mean()
        slope = ((z[rows, labels] - (p * z).sum(axis=1)) / float(temp) ** 2).mean()
        return loss, slope
    return f


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLD)


def test_fixture_holds_the_cases_the_fit_is_specified_on(fx):
    names = [str(n) for n in fx["names"]]
    assert {int(fx[f"{n}/logits"].shape[1]) for n in names} == {2, 3, 5, 9}
    assert any(fx[f"{n}/logits"].shape[0] == 1 for n in names)
    assert any(int(fx[f"{n}/n_iter"]) < 50 for n in names)                      # ended by a tolerance test
    temps = [float(fx[f"{n}/temperature"]) for n in names]
    assert min(temps) < 1.3143 < max(temps)                                     # fits that moved both ways from the start


def test_scalar_lbfgs_reproduces_the_reference_fit(fx):
    from cbas_amd.train import fit_temperature_from
    failures = []
    for name in [str(n) for n in fx["names"]]:
        temp, n_iter, evals = fit_temperature_from(numpy_nll(fx[f"{name}/logits"], fx[f"{name}/labels"]))
        want, bound = float(fx[f"{name}/temperature"]), temperature_bound(fx, name)
        print(f"{name}: temperature {temp:.9f}, reference {want:.9f}, gap {abs(temp - want):.3e}, bound {bound:.3e}; "
              f"{n_iter} iterations, {evals} closure calls")
        assert isinstance(temp, float)
        assert (n_iter, evals) == (int(fx[f"{name}/n_iter"]), int(fx[f"{name}/func_evals"])), name
        if not abs(temp - want) <= bound:
            failures.append((name, temp, want, bound))
    assert not failures, failures


def test_scalar_lbfgs_matches_torch_on_a_quartic_with_torch_defaults():
    """Independent of the fixture: torch.optim.LBFGS itself on a float32 scalar, with other settings than the fit's (a
    tolerance stop and a max_eval stop among them)."""
    import torch
    from cbas_amd.train import lbfgs_scalar
    for x0, lr, max_iter, max_eval in ((3.0, 0.05, 40, None), (0.5, 1.0, 20, None), (-2.0, 0.3, 30, 7), (1.0, 0.5, 60, None)):
        p = torch.nn.Parameter(torch.tensor([x0]))
        opt = torch.optim.LBFGS([p], lr=lr, max_iter=max_iter, max_eval=max_eval)

        def closure():
            opt.zero_grad()
            loss = ((p - 1.0) ** 4 + 0.5 * (p - 1.0) ** 2).sum()
            loss.backward()
            return loss

        opt.step(closure)
        state = opt.state[p]

        def mine(x):
            q = torch.tensor([float(x)], requires_grad=True)
            loss = ((q - 1.0) ** 4 + 0.5 * (q - 1.0) ** 2).sum()
            loss.backward()
            return float(loss.detach()), float(q.grad)

        x, n_iter, evals = lbfgs_scalar(mine, x0, lr=lr, max_iter=max_iter, max_eval=max_eval)
        assert (n_iter, evals) == (state["n_iter"], state["func_evals"]), (x0, lr)
        assert abs(float(x) - float(p.detach())) <= 4 * float(np.spacing(np.float32(abs(float(p)) + 1.0))), (x0, lr, float(x), float(p.detach()))


def test_calibration_temperature_is_the_reference_expression():
    import torch
    from cbas_amd.train import calibration_chain, calibration_temperature
    for T in (-30.0, -1.0, 0.0, 1.0, 5.0, 9.9, 9.9995, 10.0, 19.0, 25.0):
        t = torch.tensor([T], requires_grad=True)
        temp = torch.clamp(torch.nn.functional.softplus(t) + 1e-3, max=10.0)
        temp.sum().backward()
        assert float(calibration_temperature(T)) == float(temp)
        assert abs(float(calibration_chain(T)) - float(t.grad)) <= 2 * float(np.spacing(np.float32(float(t.grad)))), T
    assert float(calibration_temperature(50.0)) == 10.0 and float(calibration_chain(50.0)) == 0.0


# ---------------------------------------------------------------------------------------------------------------
# keep_rows()
# ---------------------------------------------------------------------------------------------------------------
class FakeRows:
    """Stand-in for train.ResidentRows: records its construction, holds no device memory."""
    built = []

    def __init__(self, plan, device):
        self.device, self.files, self.dim, self.rows = device, dict(plan.files), int(plan.dim), None
        FakeRows.built.append(weakref.ref(self))


@pytest.fixture()
def project(tmp_path, monkeypatch):
    from cbas_amd import datasets as D, train as T
    FakeRows.built = []
    monkeypatch.setattr(T, "ResidentRows", FakeRows)
    monkeypatch.setattr(T, "_resident_budget", lambda device: 1e12)
    monkeypatch.delenv("CBAS_TRAIN_RESIDENT", raising=False)
    paths, labels = synth.cls_project(str(tmp_path), [80, 90, 70], 64, 3, 5)

    def dataset(files):
        manifest = [(paths[f], c, int(labels[f][c])) for f in files for c in range(15, 40)]
        return D.LazyStandardDataset(manifest, 31)
    return T, paths, dataset


def test_outside_keep_rows_every_call_builds_its_store(project):
    T, paths, dataset = project
    lines = []
    a = T.open_store([dataset([0, 1, 2])], ("training",), 31, 64, "cuda", lines.append)
    b = T.open_store([dataset([0, 1])], ("test",), 31, 64, "cuda", lines.append)
    assert a is not b and len(FakeRows.built) == 2 and T._row_cache is None
    assert all(line.startswith("training data: resident in HBM (") for line in lines), lines


def test_keep_rows_reuses_a_store_for_a_subset_and_rebuilds_for_changed_files(project):
    T, paths, dataset = project
    lines = []
    with T.keep_rows():
        a = T.open_store([dataset([0, 1]), dataset([2])], ("training", "test"), 31, 64, "cuda", lines.append)
        b = T.open_store([dataset([1])], ("test",), 31, 64, "cuda", lines.append)
        c = T.open_store([dataset([2, 0])], ("validation",), 31, 64, "cuda", lines.append)
        assert a is b is c and len(FakeRows.built) == 1
        assert [("resident in HBM" in line, "kept rows reused" in line) for line in lines] == [(True, False), (False, True), (False, True)]
        # nested scopes share the outer one's store
        with T.keep_rows():
            assert T.open_store([dataset([0])], ("test",), 31, 64, "cuda", lines.append) is a
        assert T.open_store([dataset([0])], ("test",), 31, 64, "cuda", lines.append) is a and len(FakeRows.built) == 1
        # another device, another row width: not served from the kept store
        assert T.open_store([dataset([0])], ("test",), 31, 64, "cuda:1", lines.append) is not a and len(FakeRows.built) == 2
        a = T.open_store([dataset([0, 1, 2])], ("training",), 31, 64, "cuda", lines.append)
        assert len(FakeRows.built) == 3
        # a file whose mtime changed
        st = os.stat(paths[1])
        os.utime(paths[1], ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
        assert T.open_store([dataset([0])], ("test",), 31, 64, "cuda", lines.append) is a          # file 0 is as it was
        d = T.open_store([dataset([0, 1])], ("test",), 31, 64, "cuda", lines.append)
        assert d is not a and len(FakeRows.built) == 4
        # a file whose size changed (written again with more rows, mtime put back)
        st = os.stat(paths[0])
        synth.cls_project(os.path.dirname(paths[0]), [20000], 64, 3, 5)
        os.utime(paths[0], ns=(st.st_atime_ns, st.st_mtime_ns))
        assert os.stat(paths[0]).st_size != st.st_size
        e = T.open_store([dataset([0, 1])], ("test",), 31, 64, "cuda", lines.append)
        assert e is not d and len(FakeRows.built) == 5
        # a file the kept store does not hold
        assert T.open_store([dataset([0, 1, 2])], ("test",), 31, 64, "cuda", lines.append) is not e and len(FakeRows.built) == 6
    assert sum("resident in HBM" in line for line in lines) == 6


def test_keep_rows_frees_the_store_on_exit_and_on_exception(project):
    T, paths, dataset = project
    with T.keep_rows() as cache:
        T.open_store([dataset([0, 1])], ("training",), 31, 64, "cuda", lambda line: None)
        assert cache.store is not None
    gc.collect()
    assert T._row_cache is None and cache.store is None and FakeRows.built[0]() is None
    with pytest.raises(KeyError):
        with T.keep_rows() as cache:
            T.open_store([dataset([0, 1])], ("training",), 31, 64, "cuda", lambda line: None)
            raise KeyError("boom")
    gc.collect()
    assert T._row_cache is None and cache.store is None and FakeRows.built[1]() is None
    # and the next call outside a scope keeps nothing
    T.open_store([dataset([0])], ("training",), 31, 64, "cuda", lambda line: None)
    gc.collect()
    assert T._row_cache is None and FakeRows.built[2]() is None


def test_host_loader_decisions_are_logged_and_keep_nothing(project, monkeypatch):
    T, paths, dataset = project
    lines = []
    with T.keep_rows() as cache:
        monkeypatch.setenv("CBAS_TRAIN_RESIDENT", "0")
        assert T.open_store([dataset([0])], ("test",), 31, 64, "cuda", lines.append) is None
        monkeypatch.delenv("CBAS_TRAIN_RESIDENT")
        monkeypatch.setattr(T, "_resident_budget", lambda device: 10.0)
        assert T.open_store([dataset([0])], ("test",), 31, 64, "cuda", lines.append) is None
        assert cache.store is None and not FakeRows.built
    assert lines[0] == "training data: host loader (CBAS_TRAIN_RESIDENT=0)" and lines[1].startswith("training data: host loader (80 rows need")


# ---------------------------------------------------------------------------------------------------------------
# what the reference's bundle writer reads from the model (workthreads.py:867-884)
# ---------------------------------------------------------------------------------------------------------------
def test_head_answers_the_bundle_writers_questions():
    from cbas_amd.head import ClassifierLSTMDeltas
    m = ClassifierLSTMDeltas(768, 9, lstm_hidden_size=48, lstm_layers=2)
    assert m.lstm.hidden_size == 48 and m.lstm.num_layers == 2
    assert m.lstm.input_size == 256 and m.lstm.bidirectional is True and m.use_acceleration is True
    assert ClassifierLSTMDeltas(768, 3, use_acceleration=False).use_acceleration is False
    assert int(getattr(ClassifierLSTMDeltas(768, 3).lstm, "hidden_size", -1)) == 64
    with pytest.raises(AttributeError):
        m.lstm.weight_ih_l0
    with pytest.raises(AttributeError):
        m.lstm.hidden_size = 3


CHILD = r'''
import json, os, sys, types
import numpy as np, torch
REF, REPO = sys.argv[1:3]
for name in ("cv2", "decord", "h5py", "eel", "watchdog", "watchdog.observers", "watchdog.events"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["cv2"].VideoCapture = object
sys.modules["decord"].VideoReader = object
sys.modules["decord"].cpu = lambda i=0: None
sys.modules["h5py"].File = object
eel = sys.modules["eel"]
eel.expose = lambda f=None, *a, **k: f
eel.spawn = lambda *a, **k: None
sys.modules["watchdog.observers"].Observer = object
sys.modules["watchdog.events"].FileSystemEventHandler = object
sys.path[:0] = [REPO, REF, os.path.join(REF, "backend")]

import cbas, classifier_head, workthreads            # the reference, unmodified
ref_eval, ref_fit, ref_task = cbas.evaluate_on_split, workthreads.fit_temperature, workthreads.TrainingThread._execute_training_task

import cbas_amd.integration as I
from cbas_amd import train as T
assert I.install() is True
# the worker thread resolves both names through the modules at call time (workthreads.py:675, 851)
assert workthreads.cbas.evaluate_on_split is T.evaluate_on_split and workthreads.fit_temperature is T.fit_temperature
assert workthreads.TrainingThread._execute_training_task is not ref_task

# a training task runs inside keep_rows(): the scope is open while the reference's method body runs and closed after it,
# also when it raises
seen = []
def body(self, task, *a, **k):
    seen.append(T._row_cache is not None)
    if task == "fail":
        raise RuntimeError("task failed")
    return "done"
workthreads.TrainingThread._execute_training_task._cbas_amd_wrapped      # the original is kept for uninstall()
wrapped = I._in_keep_rows(body)
assert wrapped(None, "ok") == "done" and T._row_cache is None
try:
    wrapped(None, "fail")
    raise SystemExit("the task's exception was swallowed")
except RuntimeError:
    pass
assert seen == [True, True] and T._row_cache is None
assert I.install() is True                                               # a second install() does not wrap twice
assert workthreads.TrainingThread._execute_training_task._cbas_amd_wrapped is ref_task

# the model_meta dictionary of workthreads.py:867-884, from the head train_lstm_model returns
best_model = classifier_head.ClassifierLSTMDeltas(768, 4, seq_len=31, lstm_hidden_size=48, lstm_layers=2)
meta = {
    "head_architecture_version": type(best_model).__name__,
    "hyperparameters": {
        "use_acceleration": bool(getattr(best_model, "use_acceleration", True)),
        "lstm_hidden_size": int(getattr(best_model.lstm, "hidden_size", 64)),
        "lstm_layers": int(getattr(best_model.lstm, "num_layers", 1)),
    },
    "calibration": {"temperature": float(1.25)},
}
assert json.loads(json.dumps(meta))["hyperparameters"] == {"use_acceleration": True, "lstm_hidden_size": 48, "lstm_layers": 2}
assert meta["head_architecture_version"] == "ClassifierLSTMDeltas"

I.uninstall()
assert cbas.evaluate_on_split is ref_eval and workthreads.fit_temperature is ref_fit
assert workthreads.TrainingThread._execute_training_task is ref_task
print("OK")
'''


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "backend")), reason="reference tree not present")
def test_install_patches_the_tail_and_uninstall_restores_it():
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(CHILD), REF, REPO], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-4000:]
