"""cbasx_viterbi_scores / cbasx_viterbi_decode (csrc/seq_viterbi.hip) and cbas_amd/bouts.py on the device, bit for bit against
the serial numpy definition of tests/viterbi_ref.py: clip lengths around the piece size, every class-count path of the kernels,
tie-heavy scores, a forbidden diagonal, clips alone against clips in a batch, the refusals, and one behavioural case."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viterbi_ref as V  # noqa: E402
from test_bouts_host import flicker_clip  # noqa: E402

from cbas_amd import _lib, bouts, postprocess  # noqa: E402

pytestmark = pytest.mark.gpu
CHUNK = bouts.CHUNK
LENGTHS = [1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
CLASSES = [1, 2, 9, 33, 64]                                    # register-column widths 2, 2, 16, 64, 64 of the forward pass
REGIMES = ["random", "ties", "zeros"]


def layout():
    """The lengths back to back in one call, with a clip of no frame, a gap of 5 unowned frames and 3 unowned frames at the end."""
    table, at = [], 0
    for i, n in enumerate(LENGTHS):
        table.append((at, n))
        at += n
        if i == 1:
            table.append((at, 0))
            at += 5
    return np.array(table, np.int64), at + 3


@functools.lru_cache(maxsize=None)
def case(C, regime):
    """``(scores, table, A, prior, reference labels, reference clip scores)``, computed once per (C, regime)."""
    rng = np.random.default_rng(1000 * C + REGIMES.index(regime))
    table, N = layout()
    if regime == "random":
        scores = rng.integers(-8192, 1, size=(N, C))
        A = rng.integers(-3000, 1, size=(C, C))
        prior = rng.integers(-3000, 1, size=C)
    elif regime == "ties":
        scores = rng.integers(-2, 1, size=(N, C))
        A = rng.integers(-2, 1, size=(C, C))
        prior = rng.integers(-2, 1, size=C)
    else:
        scores, A, prior = np.zeros((N, C), int), np.zeros((C, C), int), None
    scores, A = scores.astype(np.int32), A.astype(np.int32)
    prior = None if prior is None else prior.astype(np.int32)
    labels, clip_score = V.viterbi_ref(scores, table, A, prior)
    for x in (scores, table, A, labels, clip_score):
        x.setflags(write=False)
    return scores, table, A, prior, labels, clip_score


def raw_decode(scores, table, A, prior, labels=None, clip_score=None, workspace=None, n_total=None, n_clips=None, C=None, null=()):
    """The raw entry point on numpy inputs: ``(labels, clip_score)`` device tensors.  The keyword arguments override what a
    refusal test wants to get wrong; ``null`` names pointers to pass as NULL."""
    lib, dev = _lib.load(), torch.device("cuda:0")
    s = torch.from_numpy(np.array(scores, np.int32)).to(dev)
    t = torch.from_numpy(np.array(table, np.int64).reshape(-1, 2)).to(dev)
    a = torch.from_numpy(np.array(A, np.int32)).to(dev)
    p = None if prior is None else torch.from_numpy(np.ascontiguousarray(prior, np.int32)).to(dev)
    N = int(s.shape[0]) if n_total is None else n_total
    K = int(t.shape[0]) if n_clips is None else n_clips
    Cn = int(s.shape[1]) if C is None else C
    labels = torch.empty(int(s.shape[0]), dtype=torch.int32, device=dev) if labels is None else labels
    clip_score = torch.empty(int(t.shape[0]), dtype=torch.int64, device=dev) if clip_score is None else clip_score
    if workspace is None:
        need = int(lib.cbasx_viterbi_workspace_bytes(int(s.shape[0]), int(t.shape[0]), int(s.shape[1])))
        assert need > 0
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    ptr = {"scores": s.data_ptr(), "table": t.data_ptr(), "trans": a.data_ptr(), "labels": labels.data_ptr(), "workspace": workspace.data_ptr()}
    for name in null:
        ptr[name] = None
    with torch.cuda.device(dev):
        _lib.check(lib.cbasx_viterbi_decode(ptr["scores"], N, ptr["table"], K, Cn, ptr["trans"], None if p is None else p.data_ptr(),
                                            ptr["labels"], clip_score.data_ptr(), ptr["workspace"], int(workspace.numel()),
                                            torch.cuda.current_stream(dev).cuda_stream), "cbasx_viterbi_decode")
    return labels, clip_score


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("C", CLASSES)
def test_decode_matches_the_reference(C, regime):
    scores, table, A, prior, want, want_score = case(C, regime)
    labels, clip_score = raw_decode(scores, table, A, prior)
    got, got_score = labels.cpu().numpy(), clip_score.cpu().numpy()
    owned = np.zeros(scores.shape[0], bool)
    for first, n in table:
        owned[first:first + n] = True
    assert (got[~owned] == -1).all() and (want[~owned] == -1).all() and (~owned).sum() == 8
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert np.array_equal(got_score, want_score) and got_score[2] == 0            # the clip of no frame
    if regime == "zeros":
        assert (got[owned] == 0).all() and (got_score == 0).all()
    again, again_score = raw_decode(scores, table, A, prior)
    assert torch.equal(again, labels) and torch.equal(again_score, clip_score)


@pytest.mark.parametrize("C", [2, 9, 64])
def test_a_forbidden_diagonal_is_obeyed(C):
    scores, table, A, prior, _, _ = case(C, "random")
    A = A.copy()
    A[np.diag_indices(C)] = -(1 << 20)
    want, want_score = V.viterbi_ref(scores, table, A, prior)
    labels, clip_score = raw_decode(scores, table, A, prior)
    got = labels.cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(clip_score.cpu().numpy(), want_score)
    first, n = table[-1]
    assert (got[first + 1:first + n] != got[first:first + n - 1]).all()           # no state follows itself


@pytest.mark.parametrize("C,regime", [(9, "random"), (9, "ties"), (64, "ties")])
def test_a_clip_alone_decodes_as_in_the_batch(C, regime):
    scores, table, A, prior, want, want_score = case(C, regime)
    for c, (first, n) in enumerate(table):
        if n == 0:
            continue
        labels, clip_score = raw_decode(scores[first:first + n], [(0, n)], A, prior)          # alone, and at another place
        assert np.array_equal(labels.cpu().numpy(), want[first:first + n]), (c, n)
        assert int(clip_score[0]) == want_score[c]


def device_scores(probs):
    dev = torch.device("cuda:0")
    p = torch.from_numpy(np.ascontiguousarray(probs, np.float32)).to(dev)
    scores, flags = bouts.device_scores(p)
    return scores.cpu().numpy(), int(flags.item())


def test_scores_against_float64():
    rng = np.random.default_rng(7)
    p = np.concatenate([rng.random(20000), np.exp2(-33 * rng.random(20000))]).astype(np.float32).reshape(-1, 8)
    got, flag = device_scores(p)
    want = V.scores_ref(p)
    print("scores: max |device - float64| =", int(np.abs(got.astype(np.int64) - want).max()), "differing:", int((got != want).sum()), "of", got.size)
    assert flag == 0 and np.abs(got.astype(np.int64) - want).max() <= 1
    assert got.min() >= -8192 and got.max() <= 0
    powers = np.exp2(-np.arange(41, dtype=np.float64)).astype(np.float32).reshape(-1, 1)
    got, flag = device_scores(powers)
    assert flag == 0 and got[:, 0].tolist() == [max(-256 * k, -8192) for k in range(41)]
    special = np.array([[0.0, 1.0, 1.5, 1e-45, -0.25, 3.0, np.inf, 2.0 ** -32]], np.float32)
    got, flag = device_scores(special)
    assert flag == 0 and got[0].tolist() == [-8192, 0, 0, -8192, -8192, 0, 0, -8192] and np.array_equal(got, V.scores_ref(special))
    got, flag = device_scores(np.array([[0.5, np.nan, 0.25]], np.float32))
    assert flag == bouts.FLAG_NAN and got[0].tolist() == [-256, -8192, -512]


def test_refusals_leave_the_outputs_untouched():
    scores, table, A, prior, _, _ = case(9, "random")
    dev = torch.device("cuda:0")
    N, C = scores.shape
    need = int(_lib.load().cbasx_viterbi_workspace_bytes(N, len(table), C))
    big = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    bad_table_end, bad_table_neg = table.copy(), table.copy()
    bad_table_end[-1, 1] += 4                                   # 3 unowned frames follow the last clip
    bad_table_neg[0, 0] = -1
    bad_A, bad_prior, bad_hi, bad_lo = A.copy(), prior.copy(), scores.copy(), scores.copy()
    bad_A[3, 4] = (1 << 20) + 1
    bad_prior[2] = -(1 << 20) - 1
    bad_hi[N - 1, C - 1] = 1                                    # in no clip: every score is checked
    bad_lo[700, 0] = -8193
    refusals = [
        dict(null=["scores"]), dict(null=["table"]), dict(null=["trans"]), dict(null=["labels"]), dict(null=["workspace"]),
        dict(C=0), dict(C=65), dict(n_total=-1), dict(n_clips=0),
        dict(table=bad_table_end), dict(table=bad_table_neg), dict(A=bad_A), dict(prior=bad_prior), dict(scores=bad_hi), dict(scores=bad_lo),
        dict(workspace=big[:need - 1]), dict(workspace=big[1:need + 1]),
    ]
    for r in refusals:
        labels = torch.full((N,), 77, dtype=torch.int32, device=dev)
        clip_score = torch.full((len(table),), 77, dtype=torch.int64, device=dev)
        kw = {k: v for k, v in r.items() if k not in ("table", "A", "prior", "scores")}
        with pytest.raises(RuntimeError, match="cbasx_viterbi_decode"):
            raw_decode(r.get("scores", scores), r.get("table", table), r.get("A", A), r.get("prior", prior), labels=labels, clip_score=clip_score, **kw)
        torch.cuda.synchronize()
        assert bool((labels == 77).all()) and bool((clip_score == 77).all()), r.keys()
    lib = _lib.load()
    for shape in ((-1, 1, 9), (10, 0, 9), (10, 1, 0), (10, 1, 65)):
        assert lib.cbasx_viterbi_workspace_bytes(*shape) == -1
    assert lib.cbasx_viterbi_workspace_bytes(0, 1, 1) > 0
    # the optional pointers: no prior, no clip_score
    labels, _ = raw_decode(scores, table, A, None)
    with torch.cuda.device(dev):
        s, t, a = (torch.from_numpy(np.array(x)).to(dev) for x in (scores, table, A))
        out = torch.empty(N, dtype=torch.int32, device=dev)
        _lib.check(lib.cbasx_viterbi_decode(s.data_ptr(), N, t.data_ptr(), len(table), C, a.data_ptr(), None, out.data_ptr(), None,
                                            big.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream), "cbasx_viterbi_decode")
    assert torch.equal(out, labels) and np.array_equal(out.cpu().numpy(), V.viterbi_ref(scores, table, A, None)[0])


def test_python_api_matches_the_raw_entry_points(tmp_path):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    table, N = layout()
    C = 9
    probs = rng.dirichlet(np.full(C, 0.3), size=N).astype(np.float32)
    A = bouts.sticky_transitions(C, mean_duration=12)
    prior = bouts.log_scores(np.full(C, 1.0 / C))
    scores, flag = device_scores(probs)
    raw, raw_score = raw_decode(scores, table, A, prior)
    assert np.array_equal(raw.cpu().numpy(), V.viterbi_ref(scores, table, A, prior)[0])
    p_dev = torch.from_numpy(probs).to(dev)
    labels, clip_score = bouts.viterbi_labels(p_dev, table, A, prior, return_scores=True)
    assert labels.is_cuda and labels.dtype == torch.int32 and torch.equal(labels, raw) and torch.equal(clip_score, raw_score)
    # hard labels are one-hot scores
    hard = torch.from_numpy(probs.argmax(1).astype(np.int32)).to(dev)
    one_hot = np.where(probs.argmax(1)[:, None] == np.arange(C)[None, :], 0, -8192)
    assert torch.equal(bouts.viterbi_labels(hard, table, A), raw_decode(one_hot, table, A, None)[0])
    # decode_bouts = label_runs of those labels with the decoded label's probability
    conf = p_dev.gather(1, raw.clamp(min=0).to(torch.int64)[:, None])[:, 0].contiguous()
    want = postprocess.label_runs(raw, conf, table, C)
    got = bouts.decode_bouts(p_dev, table, A, prior)
    assert got.dtype == postprocess.LABEL_RUN_DTYPE and got.tobytes() == want.tobytes() and len(got) > len(table)
    files = [str(tmp_path / f"rec_{i}_cls.h5") for i in range(len(table))]
    index = types.SimpleNamespace(n_rows=N, _table=table, files=files, clip_table=torch.from_numpy(table).to(dev), device=dev)
    assert bouts.index_bouts(index, p_dev, A, prior).tobytes() == want.tobytes()
    # write_outputs -> activity_bins: the one-hot files of the decoded labels count the decoded frames
    names = [f"b{j}" for j in range(C)]
    paths = bouts.write_outputs(index, raw, names, "net_viterbi")
    assert paths == [f.replace("_cls.h5", "_net_viterbi_outputs.csv") for f in files] and all(os.path.exists(p) for p in paths)
    lab = raw.cpu().numpy()
    for b in (0, 4):
        owned = np.concatenate([lab[first:first + n] for first, n in table])
        bins = postprocess.activity_bins(paths, None, None, names[b], 1.0, 1, 0.5)           # bins of 60 frames
        padded = np.zeros(-(-owned.size // 60) * 60, np.int64)
        padded[:owned.size] = owned == b
        assert bins == [float(x) for x in padded.reshape(-1, 60).sum(1)]


def test_sticky_decode_removes_flicker_on_the_device():
    probs, want = flicker_clip()
    dev = torch.device("cuda:0")
    p_dev = torch.from_numpy(probs).to(dev)
    argmax_runs = postprocess.label_runs(p_dev.argmax(1).to(torch.int32), p_dev.max(1).values.contiguous(), [(0, 360)], 3)
    assert len(argmax_runs) > 3
    records = bouts.decode_bouts(p_dev, [(0, 360)], bouts.sticky_transitions(3, mean_duration=50))
    assert [(int(r["start_frame"]), int(r["end_frame"]), int(r["label"])) for r in records] == want
