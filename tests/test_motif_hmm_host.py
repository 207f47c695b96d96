"""The motif HMM on the host (cbas_amd/motif_hmm.py): the header against the bindings, the properties of EM
through the float64 restatements of rows_hmm_ref.py and ``bouts.posteriors_host``, the module's own host path against them, the
model file and the command line on ``--device cpu``."""
import csv
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rows_hmm_ref as H  # noqa: E402
import rows_kmeans_ref as R  # noqa: E402

from cbas_amd import _lib, bouts, build as B, h5io, motif_hmm as M, motifs, pipeline, postprocess, search as S  # noqa: E402

NAMES = (("cbasx_rows_emissions", 12), ("cbasx_rows_weighted_sums_workspace_bytes", 3), ("cbasx_rows_weighted_sums", 12))


def test_header_bindings_and_build():
    header = open(os.path.join(os.path.dirname(B.HERE), "include", "cbas_mi355x_ext.h")).read()
    for name, n_args in NAMES:
        m = re.search(rf"\b(int|int64_t) {name}\s*\(([^)]*)\)\s*;", header)
        assert m, name
        args = [a.strip() for a in m.group(2).split(",")]
        restype, argtypes = _lib.EXT_SIGNATURES[name]
        assert len(args) == n_args == len(argtypes), name
        assert restype.__name__ in ({"int": "c_int", "int64_t": "c_long"}[m.group(1)], "c_int64")
        for decl, ctype in zip(args, argtypes):
            want = "c_void_p" if "*" in decl else {"int64_t": "c_long", "int32_t": "c_int", "float": "c_float"}[decl.split()[0]]
            assert ctype.__name__ in (want, {"c_long": "c_int64", "c_int": "c_int32"}.get(want, want)), (name, decl)
    for name, value in (("MAX_STATES", M.MAX_STATES), ("MAX_DIM", M.MAX_DIM), ("MAX_PARTS", M.MAX_PARTS), ("PART_ROWS", M.PART_ROWS)):
        m = re.search(rf"#define CBASX_ROWS_HMM_{name} (\d+)", header)
        assert m and int(m.group(1)) == value, name
    assert (H.MAX_PARTS, H.PART_ROWS, H.MAX_C, H.MAX_D, H.MASS_MIN) == (M.MAX_PARTS, M.PART_ROWS, M.MAX_STATES, M.MAX_DIM, M.MASS_MIN)
    assert "rows_hmm.hip" in B.SOURCES and B.EXTRA_FLAGS["rows_hmm.hip"] == B.NO_PACKED
    assert os.path.exists(os.path.join(B.CSRC, "rows_hmm.hip"))
    source = open(os.path.join(B.CSRC, "rows_hmm.hip")).read()
    assert "rows_api.h" in source and "rows_rn.h" in source and "cbas_use_device_of" in source and "atomic" not in source.lower().replace("no atomics", "")
    assert S.FrameIndex.motif_hmm is not None
    # the parts are a function of n_rows alone, at most 256 of a multiple of 64 rows, and cover the rows
    for n in (0, 1, 63, 64, 65, 128, 129, 16384, 16385, 180_000, 2_000_000):
        rpp, parts = H.parts(n)
        assert rpp % 64 == 0 and parts <= 256 and parts * rpp >= n and (parts - 1) * rpp < max(n, 1)
    assert max(H.workspace_bytes(n, 768, 64) for n in (2_000_000, 20_000_000, 1 << 40)) <= 256 * (4 * 64 * 768 + 256)      # no growth with n_rows


PLANT = dict(seed=5, lengths=(300, 1500, 40), D=64, C=4)


@pytest.fixture(scope="module")
def planted():
    x, table, states, dirs = H.planted(**PLANT)
    start = dirs + 0.25 * np.random.default_rng(1).standard_normal(dirs.shape)     # a poor start: the rounds have something to do
    start /= np.linalg.norm(start, axis=1, keepdims=True)
    return x, table, states, dirs, start


def test_likelihood_never_decreases_and_planted_states_are_recovered(planted):
    x, table, states, dirs, start = planted
    C = dirs.shape[0]
    A = bouts.sticky_transitions(C, mean_duration=40, as_probs=True).astype(np.float64)
    out = H.fit(x, table, start, A, kappa=10.0, iters=8, smoothing=0.0, fit_prior=True)
    ll = out["loglik"]
    print("loglik", ll)
    assert ll.shape == (8,) and (np.diff(ll) >= -1e-9 * np.abs(ll[:-1])).all() and ll[-1] > ll[0]
    # the planted directions and states, up to the renumbering
    cos = out["means"] @ dirs.T
    match = cos.argmax(axis=1)
    assert sorted(match.tolist()) == list(range(C)) and cos.max(axis=1).min() > 0.99
    labels = out["gamma"].argmax(axis=1)
    assert np.array_equal(match[labels], states)
    top = np.sort(out["gamma"], axis=1)
    assert (top[:, -1] - top[:, -2]).min() > 0.5
    assert (np.diff(out["occupancy"]) <= 0).all() and abs(out["occupancy"].sum() - x.shape[0]) < 1e-6
    stay = np.diag(out["transitions"])
    assert (stay > 0.95).all() and np.abs(out["transitions"].sum(axis=1) - 1).max() < 1e-12


def test_zero_temperature_is_spherical_kmeans(planted):
    x, table, _, dirs, start = planted
    C = dirs.shape[0]
    uniform = np.full((C, C), 1.0 / C)
    gamma, new, _, _, _ = H.em_round(x, table, start, uniform, np.full(C, 1.0 / C), kappa=2000.0, smoothing=0.0)
    want, _, gap = R.assign(x, start, 1)                           # unit centroids: the largest score is the largest cosine
    clear = gap > 1e-9
    assert clear.mean() > 0.99 and np.array_equal(gamma.argmax(axis=1)[clear], want[clear])
    assert gamma.max(axis=1)[gap > 0.02].min() > 1 - 1e-6          # one-hot but for frames on a boundary
    means = R.update(x, want, start, 1)
    means /= np.linalg.norm(means, axis=1, keepdims=True)
    assert np.abs(new - means).max() < 2e-2 and np.abs(np.linalg.norm(new, axis=1) - 1).max() < 1e-12


def test_update_and_calibration_on_cpu_tensors():
    rng = np.random.default_rng(2)
    C, D = 5, 32
    means = rng.standard_normal((C, D)).astype(np.float32)
    S_, mass = rng.standard_normal((C, D)), rng.uniform(1, 9, C)
    mass[3], S_[1] = 1e-9, 0.0                                     # too little mass, and no direction: both keep their mean
    Xi, Pi, prior = rng.uniform(0, 5, (C, C)), rng.uniform(0, 2, C), np.full(C, 0.2)
    for fit_prior in (False, True):
        want = H.update(means, S_, mass, Xi, Pi, prior, 1.5, fit_prior)
        got = M.em_update(torch.from_numpy(means), torch.from_numpy(S_), torch.from_numpy(mass), torch.from_numpy(Xi), torch.from_numpy(Pi),
                          torch.from_numpy(prior), 1.5, fit_prior)
        assert got[0].dtype == torch.float32 and np.array_equal(got[0].numpy(), want[0].astype(np.float32))
        assert np.allclose(got[1].numpy(), want[1], rtol=0, atol=1e-15) and np.allclose(got[2].numpy(), want[2], rtol=0, atol=1e-15)
        assert np.array_equal(got[0].numpy()[[1, 3]], means[[1, 3]])
    # the median of log(p1 / p2) over ln 9
    p = np.array([[0.6, 0.3, 0.1], [0.5, 0.25, 0.25], [0.8, 0.1, 0.1], [0.2, 0.7, 0.1]], np.float32)
    t = float(M.calibrate_temperature(torch.from_numpy(p)))
    gaps = np.sort(np.log(np.array([2.0, 2.0, 8.0, 3.5])))
    assert abs(t - gaps[1] / np.log(9.0)) < 1e-6                   # torch's median of an even count: the lower of the two
    assert float(M.calibrate_temperature(torch.from_numpy(p), torch.tensor([False, False, True, False]))) == pytest.approx(np.log(8.0) / np.log(9.0), rel=1e-6)
    assert float(M.calibrate_temperature(torch.ones((3, 1)))) == 1.0
    # the host statements are the reference's
    x = rng.standard_normal((50, D)).astype(np.float16)
    x[7] = 0
    logw = rng.standard_normal(C)
    for normalize in (0, 1):
        a, b = M.emissions_host(x, means, 3.0, logw, normalize), H.emissions(x, means, 3.0, logw, normalize)
        assert np.abs(a[0] - b[0]).max() < 1e-14 and np.abs(a[1] - b[1]).max() < 1e-12
        w = rng.uniform(0, 1, (50, C))
        a, b = M.weighted_sums_host(x, w, normalize), H.weighted_sums(x, w, normalize)
        assert np.abs(a[0] - b[0]).max() < 1e-12 and np.abs(a[1] - b[1]).max() < 1e-12
    soft = np.exp(logw - logw.max())
    assert np.abs(H.emissions(x, means, 3.0, logw, 1)[0][7] - soft / soft.sum()).max() < 1e-15      # a zero row: the softmax of logw


def write_files(tmp_path, x, table):
    paths = []
    for i, (first, n) in enumerate(table):
        paths.append(str(tmp_path / f"clip{i}_cls.h5"))
        with h5io.ClsWriter(paths[-1], x.shape[1]) as w:
            w.append(x[first:first + n])
    return paths


def test_fit_on_a_cpu_index_renumbers_consistently_and_round_trips(planted, tmp_path):
    x, table, states, dirs, start = planted
    C, D = dirs.shape
    index = S.FrameIndex(write_files(tmp_path, x, table), "cpu")
    gamma, model = index.motif_hmm(iters=4, temperature=0.1, init=start, smoothing=1.0)
    A0 = bouts.sticky_transitions(C, mean_duration=40, as_probs=True).astype(np.float64)
    want = H.fit(x, table, start.astype(np.float32), A0, kappa=10.0, iters=4, smoothing=1.0)
    assert gamma.shape == (x.shape[0], C) and gamma.dtype == torch.float32 and model.n_states == C and model.dim == D and model.normalize
    assert model.temperature == 0.1 and model.loglik.shape == (4,) and np.abs(model.loglik - want["loglik"]).max() <= 1e-6 * np.abs(want["loglik"]).max()
    assert np.abs(model.means - want["means"]).max() < 1e-5 and np.abs(model.transitions - want["transitions"]).max() < 1e-5
    assert np.abs(gamma.numpy() - want["gamma"]).max() < 1e-4 and np.abs(model.occupancy - want["occupancy"]).max() < 1e-2
    # one permutation, applied to everything: the returned gamma is the E step under the returned parameters
    assert (np.diff(model.occupancy) <= 0).all() and np.allclose(model.prior, 1.0 / C)
    probs = H.emissions(x, model.means, 10.0)[0]
    again = bouts.posteriors_host(probs, table, model.transitions.astype(np.float64) / model.transitions.sum(axis=1, keepdims=True), model.prior.astype(np.float64) / model.prior.sum())[0]
    assert np.abs(again - gamma.numpy()).max() < 1e-5 and np.abs(gamma.numpy().sum(axis=0) - model.occupancy).max() < 1e-2
    match = (model.means @ dirs.T).argmax(axis=1)
    labels = model.labels(index).numpy()
    assert np.array_equal(match[labels], states) and np.array_equal(labels, gamma.numpy().argmax(axis=1))
    # the calibrated temperature is returned, and the default start (a short k-means on the host) finds the same states
    g2, auto = M.fit(index, n_states=C, iters=3)
    probs1 = torch.from_numpy(H.emissions(x, M._initial_means(index, None, C, True), 1.0)[0])
    assert auto.temperature == pytest.approx(float(M.calibrate_temperature(probs1)), rel=1e-6) and 0.005 < auto.temperature < 1.0
    m2 = (auto.means @ dirs.T).argmax(axis=1)
    assert np.array_equal(m2[g2.numpy().argmax(axis=1)], states)
    # save / load; another width is refused, as FrameClusters refuses it
    path = str(tmp_path / "hmm.npz")
    model.save(path)
    loaded = M.MotifHMM.load(path)
    for key in ("means", "transitions", "prior", "occupancy", "loglik"):
        assert getattr(loaded, key).tobytes() == getattr(model, key).tobytes(), key
    assert (loaded.temperature, loaded.dim, loaded.normalize) == (model.temperature, model.dim, model.normalize)
    assert torch.equal(loaded.posteriors(index), gamma) and torch.equal(loaded.emissions(index), model.emissions(index))
    narrow = M.MotifHMM(np.eye(C, 32), model.transitions, model.prior, 0.1, model.occupancy, model.loglik, 32, True)
    for call in (narrow.emissions, narrow.posteriors, narrow.labels):
        with pytest.raises(ValueError, match="width"):
            call(index)
    with pytest.raises(ValueError, match="width"):
        M.fit(index, init=motifs.FrameClusters(np.eye(C, 32), np.zeros(C), np.zeros(1), None, 32, True))
    for kw in (dict(n_states=0), dict(n_states=65), dict(iters=-1), dict(smoothing=-1.0), dict(temperature=0.0), dict(init=np.zeros((C, D))),
               dict(n_states=C, transitions=np.eye(C + 1))):
        with pytest.raises(ValueError):
            M.fit(index, **kw)
    with pytest.raises(ValueError):
        M.MotifHMM(model.means, model.transitions[:2], model.prior, 0.1, model.occupancy, model.loglik, D, True)


def test_cli_on_the_host(planted, tmp_path, capsys):
    x, table, states, dirs, _ = planted
    C = dirs.shape[0]
    paths = write_files(tmp_path, x, table)
    frames, runs_csv, saved = (str(tmp_path / n) for n in ("frames.csv", "runs.csv", "hmm.npz"))
    assert motifs.main(["--files", *paths, "--clusters", str(C), "--hmm", "3", "--out", frames, "--runs", runs_csv, "--min-frames", "2",
                        "--save-hmm", saved, "--write-outputs", "mhmm", "--device", "cpu"]) == 0
    assert "temperature" in capsys.readouterr().out
    model = M.MotifHMM.load(saved)
    with open(frames, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == motifs.HMM_FRAME_COLUMNS and len(rows) == x.shape[0] + 1
    labels = np.array([int(r[2]) for r in rows[1:]])
    match = (model.means @ dirs.T).argmax(axis=1)
    assert np.array_equal(match[labels], states) and min(float(r[3]) for r in rows[1:]) > 0.5
    with open(runs_csv, newline="") as f:
        runs = list(csv.reader(f))
    assert runs[0] == motifs.RUN_COLUMNS and len(runs) - 1 == sum(len(r) for r in motifs.runs_host(labels, table, 1, 2))
    # the graded posteriors, which a head's consumers read
    out = postprocess.outputs_files(str(tmp_path), "mhmm")
    assert len(out) == 3
    names, values, _ = pipeline.read_outputs_csv(out[1])
    assert names == motifs.motif_names(C) and values.shape == (1500, C) and np.abs(values.sum(axis=1) - 1).max() < 1e-3
    assert ((values > 0) & (values < 1)).any()
    # a later recording, segmented by the saved model
    assert motifs.main(["--files", *paths[1:], "--load-hmm", saved, "--out", frames, "--device", "cpu"]) == 0
    with open(frames, newline="") as f:
        assert [int(r[2]) for r in list(csv.reader(f))[1:]] == labels[300:].tolist()
    # the rules of the flags; without --hmm the parse is what it was
    base = ["--files", "a_cls.h5", "--out", "o.csv"]
    _, a = motifs.parse_cli(base + ["--clusters", "4"])
    assert (a.hmm, a.temperature, a.save_hmm, a.load_hmm, a.mean_duration) == (None, None, None, None, 40.0)
    for bad in (["--clusters", "4", "--temperature", "0.1"], ["--clusters", "4", "--save-hmm", "x.npz"], ["--clusters", "4", "--hmm", "-1"],
                ["--clusters", "4", "--hmm", "2", "--temperature", "0"], ["--clusters", "4", "--hmm", "2", "--mean-duration", "1"],
                ["--clusters", "4", "--hmm", "2", "--smooth", "5"], ["--load-hmm", "x.npz", "--clusters", "4"], ["--load-hmm", "x.npz", "--hmm", "2"],
                ["--hmm", "2"]):
        with pytest.raises(SystemExit):
            motifs.parse_cli(base + bad)
