"""cbasx_hmm_posteriors (csrc/seq_hmm.hip) and the forward-backward half of cbas_amd/bouts.py on the device, against the float64
definition of tests/hmm_ref.py: clip lengths around the piece size, every class-count path of the kernels, three kinds of input and
of transitions, the bit-for-bit promises, the identities of the definition across the seams, the refusals, ``fit_transitions``
and ``FrameIndex.smooth``.

The accuracy bars are measured per case, not fixed: with e32 the error of the serial float32 restatement
(``bouts.posteriors_host(dtype=np.float32)``) against float64 on the same case, the device passes at ``4 * e32 + 2^-23`` - for
gamma in absolute terms, for Xi relative to its largest entry, for loglik relative to its magnitude.  The device's piecewise order
is another rounding path than the serial one, not a worse one; 2^-23 keeps a case where the restatement lands exact from asking
for exactness.  A wrong seam shows as 1e-2 or more."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_ref as H  # noqa: E402

from cbas_amd import _lib, bouts, h5io, search  # noqa: E402

pytestmark = pytest.mark.gpu
P = bouts.HMM_CHUNK
LENGTHS = [1, 2, P - 1, P, P + 1, 2 * P + 3]
CLASSES = [1, 2, 9, 33, 64]                                    # register widths 2, 2, 16, 64, 64 of the passes
SENTINEL = 77.0


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
def case(C, inputs, kind):
    """``(probs, table, A, prior, float64 reference, float32 restatement)``, computed once per case and left unchanged."""
    rng = np.random.default_rng(1000 * C + 10 * H.INPUTS.index(inputs) + H.TRANSITIONS.index(kind))
    table, N = layout()
    probs, A = H.make_probs(inputs, N, C, rng), H.make_transitions(kind, C, rng)
    prior = rng.dirichlet(np.ones(C)).astype(np.float32)
    prior = (prior / prior.sum()).astype(np.float32)
    ref = H.posteriors_ref(probs, table, A, prior)
    r32 = bouts.posteriors_host(probs, table, A, prior, dtype=np.float32)[:4]
    for x in (probs, table, A, prior) + tuple(ref) + tuple(r32):
        x.setflags(write=False)
    return probs, table, A, prior, ref, r32


def raw(probs, table, A, prior, outputs=None, workspace=None, n_total=None, n_clips=None, C=None, null=()):
    """The raw entry point on numpy inputs: ``(gamma, xi, pi, loglik, flags)`` device tensors.  The keyword arguments override
    what a refusal test wants to get wrong; ``null`` names pointers to pass as NULL."""
    lib, dev = _lib.load(), torch.device("cuda:0")
    p = torch.from_numpy(np.array(probs, np.float32)).to(dev)
    t = torch.from_numpy(np.array(table, np.int64).reshape(-1, 2)).to(dev)
    a = torch.from_numpy(np.array(A, np.float32)).to(dev)
    pr = None if prior is None else torch.from_numpy(np.array(prior, np.float32)).to(dev)
    N, K, Cn = int(p.shape[0]), int(t.shape[0]), int(p.shape[1])
    if outputs is None:
        outputs = (torch.empty((N, Cn), dtype=torch.float32, device=dev), torch.empty((Cn, Cn), dtype=torch.float64, device=dev),
                   torch.empty(Cn, dtype=torch.float64, device=dev), torch.empty(K, dtype=torch.float64, device=dev))
    gamma, xi, pi, loglik = outputs
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    if workspace is None:
        need = int(lib.cbasx_hmm_workspace_bytes(N, K, Cn))
        assert need > 0
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    ptr = {"probs": p.data_ptr(), "table": t.data_ptr(), "trans": a.data_ptr(), "gamma": gamma.data_ptr(), "xi": xi.data_ptr(), "pi": pi.data_ptr(),
           "loglik": loglik.data_ptr(), "flags": flags.data_ptr(), "workspace": workspace.data_ptr()}
    for name in null:
        ptr[name] = None
    with torch.cuda.device(dev):
        _lib.check(lib.cbasx_hmm_posteriors(ptr["probs"], N if n_total is None else n_total, ptr["table"], K if n_clips is None else n_clips,
                                            Cn if C is None else C, ptr["trans"], None if pr is None else pr.data_ptr(), ptr["gamma"], ptr["xi"],
                                            ptr["pi"], ptr["loglik"], ptr["flags"], ptr["workspace"], int(workspace.numel()),
                                            torch.cuda.current_stream(dev).cuda_stream), "cbasx_hmm_posteriors")
    return gamma, xi, pi, loglik, flags


def bars(ref, r32):
    """Per quantity ``(e32, bar)``: gamma absolute, Xi relative to its largest entry, loglik relative to its magnitude."""
    xi_top = max(ref[1].max(), 1e-300)
    ll = np.abs(ref[3])
    with np.errstate(divide="ignore", invalid="ignore"):
        ll_err = np.where(ll > 0, np.abs(r32[3] - ref[3]) / ll, np.where(r32[3] == ref[3], 0.0, np.inf))
    e = {"gamma": np.abs(r32[0].astype(np.float64) - ref[0]).max(), "xi": np.abs(r32[1] - ref[1]).max() / xi_top, "loglik": ll_err.max()}
    return {k: (v, 4 * v + 2.0 ** -23) for k, v in e.items()}


@pytest.mark.parametrize("kind", H.TRANSITIONS)
@pytest.mark.parametrize("inputs", H.INPUTS)
@pytest.mark.parametrize("C", CLASSES)
def test_posteriors_within_the_measured_bars(C, inputs, kind):
    probs, table, A, prior, ref, r32 = case(C, inputs, kind)
    gamma, xi, pi, loglik, flags = raw(probs, table, A, prior)
    g, x, p, ll = (v.cpu().numpy() for v in (gamma, xi, pi, loglik))
    assert int(flags.item()) == 0
    # frames outside every clip are rows of zeros; the clip of no frame has loglik 0
    owned = np.zeros(probs.shape[0], bool)
    for first, n in table:
        owned[first:first + n] = True
    assert (g[~owned] == 0).all() and (~owned).sum() == 8 and ll[2] == 0.0
    # the measured bars
    bar = bars(ref, r32)
    xi_top, mag = max(ref[1].max(), 1e-300), np.abs(ref[3])
    with np.errstate(divide="ignore", invalid="ignore"):
        ll_err = np.where(mag > 0, np.abs(ll - ref[3]) / mag, np.where(ll == ref[3], 0.0, np.inf)).max()
    err = {"gamma": np.abs(g.astype(np.float64) - ref[0]).max(), "xi": np.abs(x - ref[1]).max() / xi_top, "loglik": ll_err}
    print(f"hmm C={C} {inputs} {kind}: " + " ".join(f"{k} e32={bar[k][0]:.3g} device={err[k]:.3g} bar={bar[k][1]:.3g}" for k in err)
          + f" pi={np.abs(p - ref[2]).max():.3g}")
    for k in err:
        assert err[k] <= bar[k][1], (k, err[k], bar[k])
    assert np.abs(p - ref[2]).max() <= len(table) * bar["gamma"][1]               # Pi is a sum of gamma rows, one per clip
    # the identities of the definition, on the device output: the seam check for the step across pieces
    T = int(table[:, 1].sum())
    rows, total, occupancy, first = H.identities(g, x, p, table)
    assert rows <= 1e-5 and total <= 1e-5 * T and occupancy <= 1e-5 * T and first <= 1e-5 * len(table)
    # two calls agree bit for bit, and gamma does not depend on which sums are asked for
    again = raw(probs, table, A, prior)
    assert all(torch.equal(u, v) for u, v in zip(again[:4], (gamma, xi, pi, loglik)))
    spare = (torch.empty_like(gamma), torch.full_like(xi, SENTINEL), torch.full_like(pi, SENTINEL), torch.full_like(loglik, SENTINEL))
    alone = raw(probs, table, A, prior, outputs=spare, null=("xi", "pi", "loglik"))
    assert torch.equal(alone[0], gamma) and all(bool((v == SENTINEL).all()) for v in spare[1:])
    if C > 1:
        none = raw(probs, table, A, None)                                         # no prior: uniform
        want = H.posteriors_ref(probs[:2], [(0, 1)], A, None)
        assert abs(float(none[3][0]) - want[3][0]) <= 1e-5 and not torch.equal(none[0][:1], gamma[:1])


@pytest.mark.parametrize("C,inputs,kind", [(2, "uniform", "positive"), (9, "softmax", "sticky"), (33, "softmax", "positive"), (64, "one_hot", "forbidden")])
def test_a_clip_alone_gives_the_bits_of_the_batch(C, inputs, kind):
    probs, table, A, prior, _, _ = case(C, inputs, kind)
    gamma, _, _, loglik, _ = raw(probs, table, A, prior)
    for c, (first, n) in enumerate(table):
        if n == 0:
            continue
        g, _, pi, ll, _ = raw(probs[first:first + n], [(0, n)], A, prior)          # alone, and at another place
        assert torch.equal(g, gamma[first:first + n]), (c, n)
        assert torch.equal(ll[0], loglik[c]) and torch.equal(pi.to(torch.float32), g[0])


def test_flags():
    probs, table, A, prior, _, _ = case(9, "softmax", "sticky")
    bad = probs.copy()
    bad[table[4, 0] + 7, 3] = np.nan                               # in the clip of P frames
    bad[table[6, 0] + P + 1, 0] = -0.25                            # in the second piece of the longest clip
    bad[table[2, 0] + 2, 1] = np.nan                               # in the gap: owned by no clip, not looked at
    fixed = bad.copy()
    fixed[np.isnan(bad) | (bad < 0)] = 0.0
    got, want = raw(bad, table, A, prior), raw(fixed, table, A, prior)
    assert int(got[4].item()) == bouts.FLAG_EMISSION and int(want[4].item()) == 0
    assert all(torch.equal(u, v) for u, v in zip(got[:4], want[:4]))


def test_refusals_leave_the_outputs_untouched():
    probs, table, A, prior, _, _ = case(9, "softmax", "positive")
    dev = torch.device("cuda:0")
    N, C = probs.shape
    lib = _lib.load()
    need = int(lib.cbasx_hmm_workspace_bytes(N, len(table), C))
    big = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    bad_table_end, bad_table_neg = table.copy(), table.copy()
    bad_table_end[-1, 1] += 4                                   # 3 unowned frames follow the last clip
    bad_table_neg[0, 0] = -1
    row09, negative, nan_A, inf_A, bad_prior = A.copy(), A.copy(), A.copy(), A.copy(), prior.copy()
    row09[4] *= 0.9
    negative[2, 3], negative[2, 4] = -0.01, negative[2, 4] + negative[2, 3] + 0.01          # the row still sums to 1
    nan_A[8, 8] = np.nan
    inf_A[0, 1] = np.inf
    bad_prior[1] += 0.01
    refusals = [
        dict(null=["probs"]), dict(null=["table"]), dict(null=["trans"]), dict(null=["gamma"]), dict(null=["flags"]), dict(null=["workspace"]),
        dict(C=0), dict(C=65), dict(n_total=-1), dict(n_clips=0),
        dict(table=bad_table_end), dict(table=bad_table_neg), dict(A=row09), dict(A=negative), dict(A=nan_A), dict(A=inf_A), dict(prior=bad_prior),
        dict(workspace=big[:need - 1]), dict(workspace=big[1:need + 1]),
    ]
    for r in refusals:
        outputs = (torch.full((N, C), SENTINEL, dtype=torch.float32, device=dev), torch.full((C, C), SENTINEL, dtype=torch.float64, device=dev),
                   torch.full((C,), SENTINEL, dtype=torch.float64, device=dev), torch.full((len(table),), SENTINEL, dtype=torch.float64, device=dev))
        kw = {k: v for k, v in r.items() if k not in ("table", "A", "prior")}
        with pytest.raises(RuntimeError, match="cbasx_hmm_posteriors"):
            raw(probs, r.get("table", table), r.get("A", A), r.get("prior", prior), outputs=outputs, **kw)
        torch.cuda.synchronize()
        assert all(bool((v == SENTINEL).all()) for v in outputs), r.keys()
    for shape in ((-1, 1, 9), (10, 0, 9), (10, 1, 0), (10, 1, 65)):
        assert lib.cbasx_hmm_workspace_bytes(*shape) == -1
    assert lib.cbasx_hmm_workspace_bytes(0, 1, 1) > 0
    # a row within 1e-4 of 1 is taken
    near = A.copy()
    near[4] *= 1 + 5e-5
    assert int(raw(probs, table, near, prior)[4].item()) == 0


def test_python_api_and_fit_transitions_against_the_host():
    dev = torch.device("cuda:0")
    probs, table, A, prior, ref, _ = case(9, "softmax", "sticky")
    p_dev = torch.from_numpy(probs).to(dev)
    want = raw(probs, table, A, prior)
    gamma = bouts.posteriors(p_dev, table, A, prior)
    assert gamma.is_cuda and gamma.dtype == torch.float32 and torch.equal(gamma, want[0])
    out = bouts.posteriors(p_dev, torch.from_numpy(table).to(dev), torch.from_numpy(A).to(dev), torch.from_numpy(prior).to(dev), return_counts=True)
    assert all(torch.equal(u, v) for u, v in zip(out, want[:4]))
    freq = np.linspace(0.05, 0.2, 9)
    scaled = probs / freq.astype(np.float32)
    scaled = scaled / scaled.sum(axis=1, keepdims=True)
    assert (bouts.posteriors(p_dev, table, A, emission_prior=freq) - raw(scaled, table, A, None)[0]).abs().max() <= 1e-5
    with pytest.raises(ValueError):
        bouts.posteriors(p_dev, table, A * 0.5)
    with pytest.raises(RuntimeError, match="cbasx_hmm_posteriors"):
        bouts.posteriors(p_dev, table, torch.from_numpy(A * 0.5).to(dev))           # on the device already: the call's own check
    assert bouts.posteriors(p_dev[:0], [(0, 0)], A).shape == (0, 9)
    # three rounds on the device against three rounds on the host.  An entry of Xi is held to 1e-5 * T by the identities' bar and
    # a row of Xi sums to about T / C, so a round moves an entry of A by at most C * 1e-5; three rounds, three times that
    C, T = 3, 2 * P + 700
    rng = np.random.default_rng(21)
    p3 = H.make_probs("softmax", T, C, rng)
    t3 = np.array([(0, 2 * P + 100), (2 * P + 100, 600)], np.int64)
    init = bouts.sticky_transitions(C, stay=0.6, as_probs=True)
    A_host, pri_host, ll_host = bouts.fit_transitions(p3, t3, init=init, iters=3, smoothing=1.0, fit_prior=True)
    A_dev, pri_dev, ll_dev = bouts.fit_transitions(torch.from_numpy(p3).to(dev), t3, init=init, iters=3, smoothing=1.0, fit_prior=True)
    print("fit: |A_dev - A_host| =", np.abs(A_dev - A_host).max(), "prior", np.abs(pri_dev - pri_host).max(), "loglik", np.abs(ll_dev / ll_host - 1).max())
    assert A_dev.dtype == np.float32 and ll_dev.shape == (3,) and (np.diff(ll_dev) > 0).all()
    assert np.abs(A_dev - A_host).max() <= 3 * C * 1e-5 and np.abs(pri_dev - pri_host).max() <= 3 * C * 1e-5
    assert np.abs(ll_dev / ll_host - 1).max() <= 1e-5


def test_frame_index_smooth(tmp_path):
    rng = np.random.default_rng(5)
    paths = []
    for name, n in (("a_cls.h5", 40), ("b_cls.h5", P + 9)):
        with h5io.ClsWriter(str(tmp_path / name), 32, dtype="f2") as w:
            w.append(rng.standard_normal((n, 32)).astype(np.float16))
        paths.append(str(tmp_path / name))
    index = search.FrameIndex(paths, "cuda:0")
    N, C = index.n_rows, 4
    probs = H.make_probs("softmax", N, C, rng)
    A = bouts.sticky_transitions(C, stay=0.9, as_probs=True)
    gamma, Xi, Pi, loglik = index.smooth(torch.from_numpy(probs).to(index.device), A, return_counts=True)
    ref = H.posteriors_ref(probs, [(0, 40), (40, P + 9)], A)
    assert gamma.is_cuda and tuple(gamma.shape) == (N, C) and loglik.shape == (2,)
    assert np.abs(gamma.cpu().numpy() - ref[0]).max() <= 1e-5 and np.abs(Xi.cpu().numpy() - ref[1]).max() <= 1e-5 * N
    assert abs(float(Pi.sum()) - 2.0) <= 1e-5 and torch.equal(index.smooth(torch.from_numpy(probs).to(index.device), A), gamma)
    with pytest.raises(ValueError):
        index.smooth(torch.from_numpy(probs[:-1]).to(index.device), A)
