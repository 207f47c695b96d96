"""The forward-backward pass on the host (cbas_amd/bouts.py): the float64 reference against an enumeration
of all paths, ``posteriors_host`` against the reference, the identities of the definition, ``fit_transitions``, the validation
errors, the command line and the header."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_ref as H  # noqa: E402

from cbas_amd import _lib, bouts, build as B, pipeline, postprocess  # noqa: E402


def small_case(C, T, kind, seed):
    rng = np.random.default_rng(seed)
    A = H.make_transitions(kind, C, rng)
    prior = rng.dirichlet(np.ones(C))
    probs = H.make_probs(["softmax", "one_hot", "uniform"][seed % 3], T, C, rng)
    return probs, A, prior


@pytest.mark.parametrize("C,T", [(1, 5), (2, 1), (2, 2), (2, 9), (3, 4), (3, 7)])
@pytest.mark.parametrize("kind", H.TRANSITIONS)
def test_reference_equals_enumeration(C, T, kind):
    assert C ** T <= 3 ** 7
    for seed in range(3):
        probs, A, prior = small_case(C, T, kind, 10 * T + seed)
        for pri in (prior, None):
            gamma, Xi, Pi, loglik = H.posteriors_ref(probs, [(0, T)], A, pri)
            g, x, ll = H.enumerate_paths(probs, A, pri)
            assert np.abs(gamma - g).max() <= 1e-12 and np.abs(Xi - x).max() <= 1e-12 and abs(loglik[0] - ll) <= 1e-12 * max(1.0, abs(ll))
            assert np.abs(Pi - g[0]).max() <= 1e-12


def layout(lengths):
    """The lengths back to back with a clip of no frame after the second, a gap of 5 unowned frames and 3 at the end."""
    table, at = [], 0
    for i, n in enumerate(lengths):
        table.append((at, n))
        at += n
        if i == 1:
            table.append((at, 0))
            at += 5
    return np.array(table, np.int64), at + 3


HOST_CASES = [(C, inputs, kind) for C in (1, 2, 9) for inputs in H.INPUTS for kind in H.TRANSITIONS]


@pytest.mark.parametrize("C,inputs,kind", HOST_CASES)
def test_posteriors_host_equals_the_reference_and_keeps_the_identities(C, inputs, kind):
    rng = np.random.default_rng(100 * C + 10 * H.INPUTS.index(inputs) + H.TRANSITIONS.index(kind))
    table, N = layout([1, 2, 37, 64, 150])
    probs, A = H.make_probs(inputs, N, C, rng), H.make_transitions(kind, C, rng)
    prior = rng.dirichlet(np.ones(C))
    want = H.posteriors_ref(probs, table, A, prior)
    gamma, Xi, Pi, loglik, flags = bouts.posteriors_host(probs, table, A, prior)
    assert flags == 0 and gamma.dtype == np.float64
    assert np.abs(gamma - want[0]).max() <= 1e-11
    assert np.abs(Xi - want[1]).max() <= 1e-10 * max(1.0, want[1].max()) and np.abs(Pi - want[2]).max() <= 1e-11
    assert np.abs(loglik - want[3]).max() <= 1e-10 * max(1.0, np.abs(want[3]).max()) and loglik[2] == 0.0
    owned = np.zeros(N, bool)
    for first, n in table:
        owned[first:first + n] = True
    assert (gamma[~owned] == 0).all() and (~owned).sum() == 8
    for g, x, p in ((gamma, Xi, Pi), want[:3]):
        rows, total, occupancy, first = H.identities(g, x, p, table)
        assert rows <= 1e-12 and total <= 1e-9 and occupancy <= 1e-9 and first <= 1e-12
    # the float32 restatement: the same function, close to it
    g32, x32, p32, l32, _ = bouts.posteriors_host(probs, table, A, prior, dtype=np.float32)
    assert g32.dtype == np.float32 and np.abs(g32 - want[0]).max() <= 1e-4 and np.abs(l32 - want[3]).max() <= 1e-3 * max(1.0, np.abs(want[3]).max())
    # the public entry on CPU inputs
    out = bouts.posteriors(torch.from_numpy(probs), table, A, prior, return_counts=True)
    assert out[0].dtype == torch.float32 and np.array_equal(out[0].numpy(), gamma.astype(np.float32)) and np.array_equal(out[1].numpy(), Xi)
    assert torch.equal(bouts.posteriors(probs, table, A, prior), out[0])


def test_flags_and_emission_prior():
    rng = np.random.default_rng(3)
    probs = H.make_probs("softmax", 40, 3, rng)
    A = bouts.sticky_transitions(3, stay=0.9, as_probs=True)
    bad = probs.copy()
    bad[5, 1], bad[9, 0] = np.nan, -0.5
    fixed = bad.copy()
    fixed[5, 1] = fixed[9, 0] = 0.0
    got, want = bouts.posteriors_host(bad, [(0, 40)], A), bouts.posteriors_host(fixed, [(0, 40)], A)
    assert got[4] == bouts.FLAG_EMISSION and want[4] == 0 and np.array_equal(got[0], want[0])
    assert bouts.posteriors_host(bad, [(10, 30)], A)[4] == 0                        # outside every clip: not looked at
    freq = np.array([0.6, 0.3, 0.1])
    scaled = probs / freq.astype(np.float32)
    scaled = scaled / scaled.sum(axis=1, keepdims=True)
    assert torch.equal(bouts.posteriors(probs, [(0, 40)], A, emission_prior=freq), bouts.posteriors(scaled, [(0, 40)], A))
    # probabilities without a finite sum: no posterior, NaN rows and the second flag
    g, _, _, _, flags = bouts.posteriors_host(np.array([[1.0, 0.0], [np.inf, np.inf]], np.float32), [(0, 2)], np.eye(2))
    assert flags & bouts.FLAG_POSTERIOR and np.isnan(g).any()


def sampled_chain(T=20000, stay=0.95, seed=0):
    """Probabilities 0.7 / 0.15 / 0.15 around the true state of a sticky 3-state chain."""
    rng = np.random.default_rng(seed)
    state = np.zeros(T, np.int64)
    leave, other = rng.random(T) >= stay, rng.integers(1, 3, size=T)
    for t in range(1, T):
        state[t] = (state[t - 1] + other[t]) % 3 if leave[t] else state[t - 1]
    # what the classifier sees is the state through a confusion of 0.7 / 0.15 / 0.15, and it reports that confusion's likelihoods
    seen = np.where(rng.random(T) < 0.7, state, (state + rng.integers(1, 3, size=T)) % 3)
    probs = np.full((T, 3), 0.15, np.float32)
    probs[np.arange(T), seen] = 0.7
    return probs


def test_fit_transitions_on_the_host():
    probs = sampled_chain()
    table = [(0, 12000), (12000, 8000)]
    init = bouts.sticky_transitions(3, stay=0.5, as_probs=True)
    A, prior, rounds = bouts.fit_transitions(probs, table, init=init, iters=30, smoothing=0.0)
    assert A.shape == (3, 3) and A.dtype == np.float32 and prior.shape == (3,) and rounds.shape == (30,) and rounds.dtype == np.float64
    print("fit: diagonal", np.diag(A), "loglik", rounds[0], "->", rounds[-1])
    assert (np.diff(rounds) >= -1e-9 * np.abs(rounds[:-1])).all()
    assert np.abs(np.diag(A) - 0.95).max() <= 0.02
    assert np.abs(A.sum(axis=1) - 1).max() <= 1e-6 and np.allclose(prior, 1 / 3)
    # exactly `iters` rounds, each one posteriors -> rownorm(Xi + smoothing); the prior likewise
    _, Xi, Pi, loglik = bouts.posteriors(probs, table, init, return_counts=True)
    one, pri, first = bouts.fit_transitions(probs, table, init=init, iters=1, smoothing=2.0, fit_prior=True)
    want = (Xi.numpy() + 2.0) / (Xi.numpy() + 2.0).sum(axis=1, keepdims=True)
    assert np.array_equal(one, want.astype(np.float32)) and first[0] == loglik.sum().item() == rounds[0]
    assert np.array_equal(pri, ((Pi.numpy() + 2.0) / (Pi.numpy() + 2.0).sum()).astype(np.float32))
    # the learned matrix goes to the Viterbi decode through log_scores
    labels = bouts.viterbi_labels(probs[:500], [(0, 500)], bouts.log_scores(A))
    assert labels.shape == (500,) and int(labels.min()) >= 0
    default = bouts.fit_transitions(probs[:300], [(0, 300)], iters=2)[0]
    assert np.abs(default.sum(axis=1) - 1).max() <= 1e-6
    for kw in (dict(iters=0), dict(smoothing=-1.0)):
        with pytest.raises(ValueError):
            bouts.fit_transitions(probs[:50], [(0, 50)], **kw)


def test_transition_probs_and_validation():
    S = bouts.sticky_transitions(4, stay=0.9)
    P = bouts.transition_probs(S)
    assert P.dtype == np.float32 and np.abs(P - bouts.sticky_transitions(4, stay=0.9, as_probs=True)).max() <= 2e-3
    assert np.abs(P.sum(axis=1) - 1).max() <= 1e-6 and np.array_equal(bouts.transition_probs(P), P)
    assert np.abs(bouts.log_scores(P) - S).max() <= 1
    assert bouts.transition_probs(np.array([0, -256], np.int32)).tolist() == pytest.approx([2 / 3, 1 / 3])
    assert bouts.sticky_transitions(1, as_probs=True).tolist() == [[1.0]] and bouts.sticky_transitions(3).dtype == np.int32
    probs = np.full((6, 2), 0.5, np.float32)
    good = np.array([[0.9, 0.1], [0.2, 0.8]])
    for A in (np.array([[0.9, 0.0], [0.2, 0.8]]), np.array([[1.1, -0.1], [0.2, 0.8]]), np.array([[np.nan, 0.1], [0.2, 0.8]]),
              np.array([[0.9, 0.1, 0.0], [0.2, 0.8, 0.0]]), np.eye(3), bouts.sticky_transitions(2), np.array([[np.inf, 0.0], [0.2, 0.8]])):
        with pytest.raises(ValueError):
            bouts.posteriors_host(probs, [(0, 6)], A)
        with pytest.raises(ValueError):
            bouts.posteriors(probs, [(0, 6)], A)
    for prior in (np.array([0.5, 0.4]), np.array([1.5, -0.5]), np.array([np.nan, 1.0]), np.ones(3) / 3, np.array([0, 0], np.int32)):
        with pytest.raises(ValueError):
            bouts.posteriors_host(probs, [(0, 6)], good, prior)
    with pytest.raises(ValueError):
        bouts.posteriors_host(probs, [(0, 7)], good)
    with pytest.raises(ValueError):
        bouts.posteriors_host(probs[:, 0], [(0, 6)], good)
    with pytest.raises(ValueError):
        bouts.posteriors(np.zeros((3, 65), np.float32), [(0, 3)], np.eye(65))
    with pytest.raises(ValueError):
        bouts.transition_probs(np.zeros((2, 3)))
    index = type("I", (), dict(n_rows=5, _table=np.array([[0, 5]])))()
    with pytest.raises(ValueError):
        bouts.index_posteriors(index, probs, good)
    assert bouts.index_posteriors(index, probs[:5], good).shape == (5, 2)


def test_cli_rules():
    base = ["--dir", "d", "--model", "m", "--out", "o.csv"]
    _, a = bouts.parse_cli(base)
    assert (a.fit_transitions, a.posteriors, a.save_transitions) == (None, None, None)
    _, a = bouts.parse_cli(base + ["--fit-transitions", "10", "--posteriors", "m_hmm", "--save-transitions", "A.npy", "--write-outputs", "m_viterbi"])
    assert (a.fit_transitions, a.posteriors, a.save_transitions) == (10, "m_hmm", "A.npy")
    for bad in (["--fit-transitions", "5", "--stay", "0.9"], ["--fit-transitions", "5", "--mean-duration", "40"],
                ["--fit-transitions", "5", "--instances", "x.csv"], ["--fit-transitions", "0"], ["--posteriors", "m"],
                ["--posteriors", "x", "--write-outputs", "x"], ["--save-transitions", "A.txt"]):
        with pytest.raises(SystemExit):
            bouts.parse_cli(base + bad)


def test_cli_end_to_end_on_the_host(tmp_path, capsys):
    probs = sampled_chain(T=1500, seed=4)[:, :3]
    pipeline.write_probs_csv(str(tmp_path / "rec_1_net_outputs.csv"), probs[:900], ["rest", "groom", "eat"])
    pipeline.write_probs_csv(str(tmp_path / "rec_2_net_outputs.csv"), probs[900:], ["rest", "groom", "eat"])
    out, saved = tmp_path / "bouts.csv", tmp_path / "A.npy"
    assert bouts.main(["--dir", str(tmp_path), "--model", "net", "--fit-transitions", "10", "--posteriors", "net_hmm", "--out", str(out),
                       "--save-transitions", str(saved), "--device", "cpu"]) == 0
    assert "transitions after 10 rounds" in capsys.readouterr().out
    A = np.load(saved)
    assert A.shape == (3, 3) and A.dtype == np.float32 and (np.diag(A) > 0.8).all()
    files = postprocess.outputs_files(str(tmp_path), "net_hmm")
    assert files == [str(tmp_path / "rec_1_net_hmm_outputs.csv"), str(tmp_path / "rec_2_net_hmm_outputs.csv")]
    header, values, _ = pipeline.read_outputs_csv(files[0])
    want = bouts.posteriors(probs[:900], [(0, 900)], A).numpy()
    assert header == ["rest", "groom", "eat"] and values.shape == (900, 3) and np.abs(values - want).max() <= 1e-4
    assert np.abs(values.sum(axis=1) - 1).max() <= 1e-3 and ((values > 0.05) & (values < 0.95)).any()       # graded, not one-hot
    # a head's consumers read them: the actogram's bins at a threshold that a one-hot file would make meaningless
    bins = postprocess.activity_bins(files, None, None, "groom", 1.0, 1, 0.7)
    assert len(bins) == 900 // 60 + 600 // 60 and 0 < sum(bins) < 1500
    assert out.read_text().splitlines()[0] == "file,start_frame,end_frame,label,confidence"
    # without --fit-transitions the scores of --stay are turned into probabilities
    assert bouts.main(["--dir", str(tmp_path), "--model", "net", "--stay", "0.9", "--posteriors", "net_hmm2", "--out", str(out), "--device", "cpu"]) == 0
    _, again, _ = pipeline.read_outputs_csv(str(tmp_path / "rec_2_net_hmm2_outputs.csv"))
    want = bouts.posteriors(probs[900:], [(0, 600)], bouts.transition_probs(bouts.sticky_transitions(3, stay=0.9))).numpy()
    assert np.abs(again - want).max() <= 1e-4


def test_header_and_bindings():
    header = open(os.path.join(os.path.dirname(B.HERE), "include", "cbas_mi355x_ext.h")).read()
    for name, n_args in (("cbasx_hmm_workspace_bytes", 3), ("cbasx_hmm_posteriors", 15)):
        m = re.search(rf"\b(int|int64_t) {name}\s*\(([^)]*)\)\s*;", header)
        assert m, name
        args = [a.strip() for a in m.group(2).split(",")]
        restype, argtypes = _lib.EXT_SIGNATURES[name]
        assert len(args) == n_args == len(argtypes)
        assert restype.__name__ == {"int": "c_int", "int64_t": "c_long"}[m.group(1)] or restype.__name__ == "c_int64"
        for decl, ctype in zip(args, argtypes):
            want = "c_void_p" if "*" in decl else {"int64_t": "c_long", "int32_t": "c_int"}[decl.split()[0]]
            assert ctype.__name__ in (want, {"c_long": "c_int64", "c_int": "c_int32"}.get(want, want)), (name, decl)
    for name, value in (("MAX_CLASSES", bouts.MAX_CLASSES), ("CHUNK", bouts.HMM_CHUNK), ("FLAG_EMISSION", bouts.FLAG_EMISSION),
                        ("FLAG_POSTERIOR", bouts.FLAG_POSTERIOR), ("FLOOR_LOG2", int(np.log2(bouts.HMM_FLOOR)))):
        m = re.search(rf"#define CBASX_HMM_{name} \(?(-?\d+)u?\)?", header)
        assert m and int(m.group(1)) == value, name
    assert re.search(r"#define CBASX_HMM_ROW_TOL 1e-4f", header) and bouts.HMM_ROW_TOL == 1e-4
    assert "seq_hmm.hip" in B.SOURCES and B.EXTRA_FLAGS["seq_hmm.hip"] == B.NO_PACKED
