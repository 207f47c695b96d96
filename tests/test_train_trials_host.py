"""train_lstm_trials without a device: argument checks, the decision to run the trials one after another and its log line,
the slot scheduler on fake trials, and the library surface (cbas_head_train_step_rows_multi in the header, the export map,
the ctypes table and the built library)."""
import ctypes as C
import fnmatch
import os
import re
import threading

import pytest
import torch

from cbas_amd import _lib, datasets as D, synth, train as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEHAVIORS = ["a", "b", "c", "d", "e"]


class Plain(torch.utils.data.Dataset):
    """No manifest: an ordinary dataset."""

    def __len__(self):
        return 8

    def __getitem__(self, i):
        return torch.zeros(31, 768), torch.tensor(i % 5)


def fake_solo(calls):
    def train_lstm_model(train_set, test_set, seq_len, behaviors, cancel_event, **kw):
        calls.append((kw["seed"], train_set, kw))
        return f"model{kw['seed']}", [], kw["seed"] % 3
    return train_lstm_model


def test_no_seeds_bad_max_concurrent():
    ev = threading.Event()
    assert T.train_lstm_trials(Plain(), None, 31, BEHAVIORS, ev, trial_seeds=[]) == []
    assert T.train_lstm_trials(Plain(), None, 31, BEHAVIORS, ev, trial_seeds=(), max_concurrent=8) == []
    for bad in (0, 9, -1, 2.5, True):
        with pytest.raises(ValueError):
            T.train_lstm_trials(Plain(), None, 31, BEHAVIORS, ev, trial_seeds=[1, 2], max_concurrent=bad)
        with pytest.raises(ValueError):                       # also with nothing to train
            T.train_lstm_trials(Plain(), None, 31, BEHAVIORS, ev, trial_seeds=[], max_concurrent=bad)
    assert _lib.TRAIN_MULTI_MAX == 8


def test_an_empty_training_set_gives_the_reference_triple_per_seed():
    class Empty(Plain):
        def __len__(self):
            return 0
    assert T.train_lstm_trials(Empty(), None, 31, BEHAVIORS, threading.Event(), trial_seeds=[3, 1]) == [(None, None, -1)] * 2


def test_switch_off_runs_one_after_another_in_seed_order(monkeypatch):
    calls, lines = [], []
    monkeypatch.setattr(T, "train_lstm_model", fake_solo(calls))
    monkeypatch.setenv("CBAS_TRAIN_RESIDENT", "0")
    out = T.train_lstm_trials(Plain(), None, 31, BEHAVIORS, threading.Event(), trial_seeds=[7, 3, 11, 3], max_concurrent=2,
                              batch_size=64, lr=2e-3, epochs=2, patience=1, lstm_hidden_size=32, log=lines.append)
    assert [c[0] for c in calls] == [7, 3, 11, 3]
    assert out == [("model7", [], 1), ("model3", [], 0), ("model11", [], 2), ("model3", [], 0)]
    assert lines == ["training trials: 4 one after another (CBAS_TRAIN_RESIDENT=0)"]
    kw = calls[0][2]
    assert (kw["batch_size"], kw["lr"], kw["epochs"], kw["patience"], kw["lstm_hidden_size"]) == (64, 2e-3, 2, 1, 32)
    assert "max_concurrent" not in kw and "trial_seeds" not in kw


def test_ordinary_datasets_run_one_after_another(monkeypatch):
    calls, lines = [], []
    monkeypatch.setattr(T, "train_lstm_model", fake_solo(calls))
    monkeypatch.delenv("CBAS_TRAIN_RESIDENT", raising=False)
    out = T.train_lstm_trials(Plain(), None, 31, BEHAVIORS, threading.Event(), trial_seeds=[5, 6], log=lines.append)
    assert [o[0] for o in out] == ["model5", "model6"]
    assert lines == ["training trials: 2 one after another (the training set is not a manifest dataset)"]


@pytest.fixture(scope="module")
def manifest(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("trials_host_project"))
    paths, labels = synth.cls_project(root, [120, 90], 768, 5, 33)
    inst = [(p, a, b, BEHAVIORS[c]) for p, l in zip(paths, labels) for a, b, c in synth.label_runs(l)]
    return D.make_manifest(inst, 31, BEHAVIORS)


def test_rows_that_do_not_fit_run_one_after_another_each_on_its_own_counter(monkeypatch, manifest):
    calls, lines = [], []
    monkeypatch.setattr(T, "train_lstm_model", fake_solo(calls))
    monkeypatch.setattr(T, "_resident_budget", lambda device: 1000.0)          # bytes
    monkeypatch.delenv("CBAS_TRAIN_RESIDENT", raising=False)
    balanced = D.LazyBalancedDataset(manifest, 31, BEHAVIORS)
    balanced.counter = 3
    out = T.train_lstm_trials(balanced, None, 31, BEHAVIORS, threading.Event(), trial_seeds=[1, 2], log=lines.append)
    assert len(out) == 2 and len(lines) == 1
    assert re.fullmatch(r"training trials: 2 one after another \(210 rows need 0 MB, 0 MB may be used\)", lines[0]), lines
    # a balanced dataset counts its class draws on the instance: every trial gets a copy that starts where the caller's stands
    sets = [c[1] for c in calls]
    assert all(s is not balanced and s.counter == 3 and s.manifest is balanced.manifest and s.buckets is balanced.buckets for s in sets)
    assert sets[0] is not sets[1]
    D.close_readers()


def test_slot_scheduler_keeps_at_most_two_of_five_alive():
    alive, peak, started, steps = set(), [], [], []

    def start(seed):
        def trial():
            alive.add(seed)
            peak.append(len(alive))
            try:
                for i in range(seed % 3 + 1):                  # trials of different lengths: slots free at different times
                    loss = yield seed, i
                    assert loss == ("loss", seed, i)
                return f"result{seed}"
            finally:
                alive.discard(seed)
        started.append(seed)
        return trial()

    def step_many(requests):
        assert 1 <= len(requests) <= 2
        steps.append([s for s, _ in requests])
        return [("loss", s, i) for s, i in requests]

    seeds = [14, 11, 13, 12, 10]
    assert T._run_trial_slots(seeds, 2, start, step_many) == [f"result{s}" for s in seeds]
    assert started == seeds and max(peak) == 2 and not alive
    assert sorted(s for round_ in steps for s in round_) == sorted(s for s in seeds for _ in range(s % 3 + 1))
    assert steps[0] == [14, 11] and any(len(r) == 2 and 14 not in r and 11 not in r for r in steps)     # slots were reused


def test_slot_scheduler_closes_live_trials_when_a_step_fails():
    closed = []

    def start(seed):
        def trial():
            try:
                while True:
                    yield seed
            finally:
                closed.append(seed)
        return trial()

    def step_many(requests):
        raise RuntimeError("device lost")
    with pytest.raises(RuntimeError, match="device lost"):
        T._run_trial_slots([1, 2, 3], 2, start, step_many)
    assert sorted(closed) == [1, 2]


def test_library_surface():
    name = "cbas_head_train_step_rows_multi"
    header = open(os.path.join(REPO, "include", "cbas_mi355x.h")).read()
    assert re.search(r"\bint " + name + r"\(cbas_head_trainer\*\* trainers, int32_t k,", header)
    assert int(re.search(r"#define CBAS_TRAIN_MULTI_MAX\s+(\d+)", header).group(1)) == _lib.TRAIN_MULTI_MAX
    assert int(re.search(r"#define CBAS_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.EXPECTED_ABI
    exported = re.search(r"global:\s*([^;]+);", open(os.path.join(REPO, "cbas_amd", "csrc", "exports.map")).read()).group(1).split()
    assert any(fnmatch.fnmatchcase(name, pat) for pat in exported)
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(args) == 9 and args[1] is C.c_int32
    lib = _lib.load()
    assert lib.cbas_abi_version() == _lib.EXPECTED_ABI and hasattr(lib, name)
    # the README counts the entry points of the product header
    readme = open(os.path.join(REPO, "README.md")).read()
    assert f"{len(_lib.SIGNATURES)} entry points" in readme
    # refusals that need no device: nothing is dereferenced before the checks
    assert lib.cbas_head_train_step_rows_multi(None, 1, None, 0, 768, None, None, None, None) == -1
    assert b"NULL" in lib.cbas_last_error()
