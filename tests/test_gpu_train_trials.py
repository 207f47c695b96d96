"""The trials of a run trained beside each other (train_lstm_trials, cbas_head_train_step_rows_multi): every trial ends bit
for bit where the same seed ends alone - through the public function on manifest datasets (all slots busy, a slot reused
mid-epoch, a two-layer head, early stopping) and through the entry point itself (k = 1, uneven batches with every option of
the loss and of Adam switched on, the smallest trainer leading, a neighbour with huge rows, refusals).  The trial-batched
small kernels have no tolerance to meet: the reference is the same trainer stepped alone, through the single-trial kernels,
and equality is exact.  The arithmetic itself is held to the float64 oracle and the reference fixtures by tests/test_gpu_train.py."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

from cbas_amd import config as CFG, synth, weights as W

pytestmark = pytest.mark.gpu

EINVAL = -1
BEHAVIORS = ["a", "b", "c", "d", "e"]
SEQ, BATCH = 31, 64
HEADS = {"h64": dict(lstm_hidden_size=64, lstm_layers=1), "h32_l2": dict(lstm_hidden_size=32, lstm_layers=2)}
COMMON = dict(batch_size=BATCH, lr=2e-3, epochs=2, device="cuda", patience=5, weight_decay=1e-3, label_smoothing=0.05)


@pytest.fixture(scope="module")
def manifests(tmp_path_factory):
    from cbas_amd.datasets import make_manifest
    root = str(tmp_path_factory.mktemp("trials_project"))
    paths, labels = synth.cls_project(root, [260, 200, 150], 768, len(BEHAVIORS), 77)
    inst = [[(p, a, b, BEHAVIORS[c]) for a, b, c in synth.label_runs(l)] for p, l in zip(paths, labels)]
    train, val = make_manifest(inst[0] + inst[1], SEQ, BEHAVIORS), make_manifest(inst[2], SEQ, BEHAVIORS)
    assert 200 < len(train) < 500 and len(val) > 50
    return train, val


def datasets_of(manifests):
    """Fresh instances: a balanced dataset counts its draws on the instance."""
    from cbas_amd import datasets as D
    train, val = manifests
    ds = D.LazyBalancedDataset(train, SEQ, BEHAVIORS), D.LazyStandardDataset(val, SEQ)
    assert len(ds[0]) % BATCH and len(ds[1]) % BATCH               # the last batch of either pass is partial
    return ds


def outcome(result):
    model, reports, best = result
    sd = None
    if model is not None:
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        model.close()
    return sd, reports, best


class Solo:
    """train_lstm_model alone, once per (head, seed, options): the reference every trial is compared with."""

    def __init__(self, manifests):
        self.manifests, self.runs = manifests, {}

    def __call__(self, head, seed, **options):
        from cbas_amd.train import train_lstm_model
        key = (head, seed, tuple(sorted(options.items())))
        if key not in self.runs:
            train, val = datasets_of(self.manifests)
            kw = {**COMMON, **HEADS[head], **options}
            self.runs[key] = outcome(train_lstm_model(train, val, SEQ, BEHAVIORS, threading.Event(), seed=seed, log=lambda s: None, **kw))
        return self.runs[key]


@pytest.fixture(scope="module")
def solo(manifests):
    return Solo(manifests)


def run_trials(manifests, head, seeds, max_concurrent, **options):
    from cbas_amd.train import train_lstm_trials
    train, val = datasets_of(manifests)
    lines = []
    kw = {**COMMON, **HEADS[head], **options}
    out = train_lstm_trials(train, val, SEQ, BEHAVIORS, threading.Event(), trial_seeds=seeds, max_concurrent=max_concurrent,
                            log=lines.append, **kw)
    return [outcome(r) for r in out], lines


def assert_same_trial(got, want):
    (sda, ra, ba), (sdb, rb, bb) = got, want
    assert ba == bb and len(ra) == len(rb) and sda is not None and sdb is not None
    for x, y in zip(ra, rb):
        assert np.array_equal(x.train_cm, y.train_cm) and np.array_equal(x.val_cm, y.val_cm)
        assert x.train_report == y.train_report and x.val_report == y.val_report
    assert set(sda) == set(sdb)
    for k in sda:
        assert torch.equal(sda[k], sdb[k]), k


@pytest.mark.parametrize("head,max_concurrent", [("h64", 3), ("h64", 2), ("h32_l2", 3)])
def test_trials_equal_solo_runs_bit_for_bit(manifests, solo, head, max_concurrent):
    seeds = (11, 12, 13)
    got, lines = run_trials(manifests, head, seeds, max_concurrent)
    assert [l for l in lines if l.startswith("training")] == [
        "training data: resident in HBM (3 files, 610 rows, 1 MB)", f"training trials: 3 on one row store, up to {max_concurrent} beside each other"]
    for seed, g in zip(seeds, got):
        assert_same_trial(g, solo(head, seed))
    assert len(got[0][1]) == 2                                                   # both epochs were scored
    assert not torch.equal(got[0][0]["lin2.weight"], got[1][0]["lin2.weight"])     # and the seeds do differ


def test_early_stop_frees_the_slot(manifests, solo):
    """patience = 1 with a learning rate that cannot move a prediction: the validation F1 of epoch 2 equals that of epoch 1,
    so every trial stops after 2 of 4 epochs, the third seed takes a freed slot, and all three still equal their solo runs."""
    options = dict(patience=1, epochs=4, lr=1e-7)
    seeds = (21, 22, 23)
    want = [solo("h64", s, **options) for s in seeds]
    assert all(len(w[1]) == 2 and w[2] == 0 for w in want)
    got, lines = run_trials(manifests, "h64", seeds, 2, **options)
    assert sum(l.startswith("Early stopping triggered at epoch 2") for l in lines) == 3
    for g, w in zip(got, want):
        assert_same_trial(g, w)


def test_a_set_cancel_event_ends_every_trial(manifests):
    from cbas_amd.train import train_lstm_trials
    train, val = datasets_of(manifests)
    ev = threading.Event()
    ev.set()
    out = train_lstm_trials(train, val, SEQ, BEHAVIORS, ev, trial_seeds=[1, 2, 3], max_concurrent=2, log=lambda s: None,
                            **{**COMMON, **HEADS["h32_l2"]})
    assert out == [(None, [], -1)] * 3


# ---------------------------------------------------------------------------------------------------------------
# the entry point itself
# ---------------------------------------------------------------------------------------------------------------
def store_and_batches(counts, seed=5, scale_from=None):
    """610 half-precision rows on the device (rows from ``scale_from`` on scaled to magnitude 1e4) and, per count, a table of
    first rows and labels."""
    rows = synth.cls_walk(3, 610, 768).astype(np.float32)
    if scale_from is not None:
        rows[scale_from:] *= 1e4 / np.abs(rows[scale_from:]).max()
    rng = np.random.default_rng(seed)
    hi = (scale_from if scale_from is not None else 610) - SEQ
    batches = [(torch.from_numpy(rng.integers(0, hi + 1, n).astype(np.int64)), torch.from_numpy(rng.integers(0, 5, n).astype(np.int64)))
               for n in counts]
    return torch.from_numpy(rows.astype(np.float16)).cuda(), batches


def make_trainer(hcfg, seed, **kw):
    from cbas_amd.train import HeadTrainer
    return HeadTrainer(hcfg, W.synth_head_weights(hcfg, 4000 + seed), "cuda", max_batch=BATCH, seed=seed, dropout=True, **kw)


def state_of(tr):
    return (tr.weights(), tr.grads()) + tr.adam_moments()


def assert_same_state(a, b):
    for what, (x, y) in zip(("weights", "gradients", "first moment", "second moment"), zip(a, b)):
        for k in x:
            assert np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)), (what, k)


def test_multi_with_one_trainer_equals_step_rows():
    from cbas_amd.train import step_rows_multi
    hcfg = CFG.HeadConfig(in_features=768, out_features=5, lstm_hidden_size=64)
    rows, [(first, labels)] = store_and_batches([37])
    a, b = make_trainer(hcfg, 6, lr=1e-3), make_trainer(hcfg, 6, lr=1e-3)
    la = [a.step_rows(rows, first, labels) for _ in range(3)]
    lb = [step_rows_multi(rows, [(b, first, labels)])[0] for _ in range(3)]
    assert la == lb and all(np.isfinite(l[0]) for l in la)
    assert_same_state(state_of(a), state_of(b))
    assert not np.array_equal(state_of(a)[0]["lin2.weight"], W.synth_head_weights(hcfg, 4006)["lin2.weight"])
    a.close(), b.close()


def test_uneven_trainers_in_one_call_equal_their_own_steps():
    """64, 37 and 1 windows (the last takes the path without the covariance penalty), label smoothing, class weights and
    weight decay on (the gate group's own decay in the batched Adam), a two-layer head without the acceleration stream."""
    from cbas_amd.train import step_rows_multi
    hcfg = CFG.HeadConfig(in_features=768, out_features=5, lstm_hidden_size=32, lstm_layers=2, use_acceleration=False)
    opts = dict(lr=1e-3, weight_decay=1e-2, label_smoothing=0.1, class_weights=[0.5, 1.0, 2.0, 1.5, 0.25])
    rows, batches = store_and_batches([64, 37, 1])
    alone, together = [make_trainer(hcfg, s, **opts) for s in (1, 2, 3)], [make_trainer(hcfg, s, **opts) for s in (1, 2, 3)]
    want = [[t.step_rows(rows, f, y) for _ in range(2)] for t, (f, y) in zip(alone, batches)]
    got = [step_rows_multi(rows, [(t, f, y) for t, (f, y) in zip(together, batches)]) for _ in range(2)]
    for j in range(3):
        assert [got[0][j], got[1][j]] == want[j], j
        assert_same_state(state_of(together[j]), state_of(alone[j]))
    assert want[2][0][2] == 0.0 and want[0][0][2] > 0.0                  # the covariance penalty: off for one window
    # a step without the wait ends in the same place
    for t, (f, y) in zip(alone, batches):
        t.step_rows(rows, f, y, want_loss=False)
    assert step_rows_multi(rows, [(t, f, y) for t, (f, y) in zip(together, batches)], want_loss=False) is None
    for j in range(3):
        assert_same_state(state_of(together[j]), state_of(alone[j]))
    for t in alone + together:
        t.close()


def test_the_smallest_trainer_leads_and_the_larger_ones_are_masked():
    """1, 37 and 64 windows in that order: every table's grid is sized by the last entry and must mask the others, and
    trainer 0 - the leading stream - is the one without the covariance penalty, so its entries in the `cov_offdiag` table and
    in two of the column-sum tables have the count 0."""
    from cbas_amd.train import step_rows_multi
    hcfg = CFG.HeadConfig(in_features=768, out_features=5, lstm_hidden_size=32, lstm_layers=2, use_acceleration=False)
    opts = dict(lr=1e-3, weight_decay=1e-2, label_smoothing=0.1, class_weights=[0.5, 1.0, 2.0, 1.5, 0.25])
    rows, batches = store_and_batches([1, 37, 64])
    alone, together = [make_trainer(hcfg, s, **opts) for s in (1, 2, 3)], [make_trainer(hcfg, s, **opts) for s in (1, 2, 3)]
    want = [[t.step_rows(rows, f, y) for _ in range(2)] for t, (f, y) in zip(alone, batches)]
    got = [step_rows_multi(rows, [(t, f, y) for t, (f, y) in zip(together, batches)]) for _ in range(2)]
    for j in range(3):
        assert [got[0][j], got[1][j]] == want[j], j
        assert_same_state(state_of(together[j]), state_of(alone[j]))
    assert want[0][0][2] == 0.0 and want[2][0][2] > 0.0 and all(np.isfinite(l[0]) for w in want for l in w)
    for t in alone + together:
        t.close()


def test_a_neighbour_with_huge_rows_does_not_touch_a_trial():
    from cbas_amd.train import step_rows_multi
    hcfg = CFG.HeadConfig(in_features=768, out_features=5, lstm_hidden_size=64)
    rows, [(fa, ya), (fb, yb)] = store_and_batches([48, 48], scale_from=400)
    fb = fb % (610 - 400 - SEQ + 1) + 400                                # B's windows lie in the rows of magnitude 1e4
    assert float(rows[400:].abs().max()) > 9e3 and float(rows[:400].abs().max()) < 100 and int(fa.max()) + SEQ <= 400
    alone, a, b = make_trainer(hcfg, 8, lr=1e-3), make_trainer(hcfg, 8, lr=1e-3), make_trainer(hcfg, 9, lr=1e-3)
    want = [alone.step_rows(rows, fa, ya) for _ in range(3)]
    got = [step_rows_multi(rows, [(a, fa, ya), (b, fb, yb)]) for _ in range(3)]
    assert [g[0] for g in got] == want
    assert_same_state(state_of(a), state_of(alone))
    assert all(np.isfinite(g[1]).all() for g in got) and got[0][1][0] > 10 * got[0][0][0]     # B: large, finite
    for t in (alone, a, b):
        t.close()


def test_refusals_by_return_code():
    from cbas_amd import _lib
    lib = _lib.load()
    hcfg = CFG.HeadConfig(in_features=768, out_features=5, lstm_hidden_size=32)
    other = CFG.HeadConfig(in_features=384, out_features=5, lstm_hidden_size=32)
    rows, [(f, y)] = store_and_batches([8])
    f, y = f.cuda(), y.to(torch.int32).cuda()
    torch.cuda.synchronize()
    trs = [make_trainer(hcfg, s) for s in range(9)]
    narrow = make_trainer(other, 1)
    before = trs[0].weights()

    def call(handles, k, dim=768, n=8):
        m = max(len(handles), 1)
        hs = (C.c_void_p * m)(*[h._h.value if h is not None else None for h in handles])
        fs, ys, ns = (C.c_void_p * m)(*[f.data_ptr()] * m), (C.c_void_p * m)(*[y.data_ptr()] * m), (C.c_int32 * m)(*[n] * m)
        rc = lib.cbas_head_train_step_rows_multi(hs, k, rows.data_ptr(), 610, dim, fs, ys, ns, None)
        assert rc == 0 or lib.cbas_last_error()
        return rc
    assert call(trs[:2], 0) == EINVAL and call(trs, 9) == EINVAL and call(trs[:2], -1) == EINVAL
    assert call([trs[0], None], 2) == EINVAL
    assert call([trs[0], narrow], 2) == EINVAL and call([narrow, trs[0]], 2, dim=384) == EINVAL      # different dim
    assert call([trs[0], trs[0]], 2) == EINVAL                                                      # one trainer twice
    assert call(trs[:2], 2, n=0) == EINVAL and call(trs[:2], 2, n=BATCH + 1) == EINVAL
    after = trs[0].weights()
    assert all(np.array_equal(before[k], after[k]) for k in before)       # nothing was queued
    assert call(trs[:8], 8) == 0                                            # the cap itself is served
    assert any(not np.array_equal(before[k], trs[0].weights()[k]) for k in before)
    for t in trs + [narrow]:
        t.close()
