"""The linear probe over resident CLS rows on the GPU (csrc/rows_probe.hip through cbas_rows_probe_fit / _predict, then cbas_amd.probe).

  predict      logits and probabilities against float64 on the very fp16 rows and fp32 weights handed to the device, within the
               derived bounds; a zero row's logits are the bias exactly; the argmax is float64's but for rows within twice the bound
  one step     iters = 1 from given weights: (w0 - w1) L against the float64 gradient, loss[0] and loss[1] against float64 F, with and
               without sample weights and with rows of weight 0 that hold junk
  convergence  80 steps on planted data end inside Nesterov's bound on F - F*
  invariance   bit for bit: two fits, another ld, a slice, NULL weights against ones, logits asked for or not
The bounds are derived in rows_probe_ref.py.  Cases print their largest error / bound (run with -s)."""
import json
import os

import numpy as np
import pytest
import torch

import rows_probe_ref as R
from cbas_amd import _lib, h5io, knn, pipeline, postprocess, probe, search as S, synth

pytestmark = pytest.mark.gpu

TILE, SEGMENT = R.TILE, R.SEGMENT
PAD = np.float16(60000.0)                  # in the columns past D: read into any sum, it shows


def store(x, pad=8):
    """The fp16 rows as a device tensor with `pad` columns of PAD after the D."""
    img = np.full((x.shape[0], x.shape[1] + pad), PAD, np.float16)
    img[:, :x.shape[1]] = x
    return torch.from_numpy(img).cuda()


def dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def fit(rows, D, y, C, l2, iters, omega=None, W0=None, b0=None):
    """cbas_rows_probe_fit on a (M, ld) fp16 device tensor; numpy outputs.  Every output starts as 7.0."""
    lib = _lib.load()
    M = rows.shape[0]
    need = int(lib.cbas_rows_probe_workspace_bytes(M, D, C))
    assert need > 0, lib.cbas_last_error()
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    W, b, loss = torch.full((C, D), 7.0, device="cuda"), torch.full((C,), 7.0, device="cuda"), torch.full((iters + 1,), 7.0, device="cuda")
    yd, od, W0d, b0d = dev(y, np.int32), dev(omega, np.float32), dev(W0, np.float32), dev(b0, np.float32)
    _lib.check(lib.cbas_rows_probe_fit(rows.data_ptr(), M, D, rows.shape[1], yd.data_ptr(), ptr(od), C, float(l2), iters, ptr(W0d), ptr(b0d),
                                       W.data_ptr(), b.data_ptr(), loss.data_ptr(), ws.data_ptr(), need, None), "cbas_rows_probe_fit")
    torch.cuda.synchronize()
    return {"W": W.cpu().numpy(), "b": b.cpu().numpy(), "loss": loss.cpu().numpy()}


def predict(rows, D, W, b, first=0, n=None, want_logits=True):
    lib = _lib.load()
    n = rows.shape[0] - first if n is None else n
    Wd, bd = dev(W, np.float32), dev(b, np.float32)
    C = Wd.shape[0]
    probs = torch.full((n, C), 7.0, device="cuda")
    logits = torch.full((n, C), 7.0, device="cuda") if want_logits else None
    _lib.check(lib.cbas_rows_probe_predict(rows.data_ptr() + first * rows.shape[1] * 2, n, D, rows.shape[1], Wd.data_ptr(), bd.data_ptr(), C,
                                           probs.data_ptr(), ptr(logits), None), "cbas_rows_probe_predict")
    torch.cuda.synchronize()
    return probs.cpu().numpy(), (logits.cpu().numpy() if want_logits else None)


# ---- a. predict against float64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,C,N", [(32, 2, 1), (32, 64, 64), (96, 16, 127), (96, 17, 129), (768, 64, 4097), (1536, 17, 2 * 128 + 3)])
def test_predict(D, C, N):
    rng, x, _ = R.planted(D + 3 * C + N, max(N, C), D, C)
    x = x[:N]
    if N > 1:
        x[N // 2] = 0                                                          # a zero row: u = 0, its logits are the bias
    W = (3.0 * rng.standard_normal((C, D))).astype(np.float32)                 # logits a few units apart
    b = rng.standard_normal(C).astype(np.float32)
    probs, logits = predict(store(x), D, W, b)
    want_p, want_z = R.predict(x, W, b)
    dz, dp = R.logit_bound(x, W, b), R.prob_bound(x, W, b)
    if N > 1:
        assert np.array_equal(logits[N // 2], b) and (dz[N // 2] == 0).all()
        dz[N // 2] = np.finfo(np.float64).tiny                                 # the ratio below: an exact 0 over a positive number
    rz = (np.abs(logits.astype(np.float64) - want_z) / dz).max()
    rp = (np.abs(probs.astype(np.float64) - want_p) / dp).max()
    part = np.partition(want_z, -2, axis=1)
    top = want_z.argmax(axis=1)
    loose = part[:, -1] - part[:, -2] <= 2.0 * dz.max(axis=1)
    print(f"D={D} C={C} N={N}: logit error / bound {rz:.3f}, probability error / bound {rp:.3f}, {int(loose.sum())} rows within the bound of a tie")
    assert rz <= 1.0 and rp <= 1.0
    assert np.array_equal(logits.argmax(axis=1)[~loose], top[~loose])
    assert np.abs(probs.sum(axis=1, dtype=np.float64) - 1.0).max() <= 1e-5 and (probs >= 0).all()


# ---- b. one step ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["none", "given", "zeros"])
@pytest.mark.parametrize("D,C,M", [(32, 2, 2), (96, 17, SEGMENT - 1), (96, 16, SEGMENT + 1), (768, 64, 2 * SEGMENT + 131)])
def test_one_step(D, C, M, weights):
    rng, x, y = R.planted(2 * D + C + M, max(M, C), D, C)
    x, y = x[:M], y[:M]
    l2 = 1e-2
    omega = None
    keep = np.ones(M, bool)
    if weights != "none":
        omega = rng.uniform(0.5, 2.0, M).astype(np.float32)
    if weights == "zeros":
        keep = rng.random(M) > 0.25
        keep[0] = True
        omega[~keep] = 0.0
        x[~keep] = (30000.0 * np.sign(rng.standard_normal((int((~keep).sum()), D)))).astype(np.float16)    # junk in rows of weight 0
    W0 = (0.5 * rng.standard_normal((C, D))).astype(np.float32)
    b0 = (0.5 * rng.standard_normal(C)).astype(np.float32)
    got = fit(store(x), D, y, C, l2, 1, omega, W0, b0)
    # float64 of the fit WITHOUT the rows of weight 0; the bounds over all rows: a row of weight 0 adds exact zeros to every chain
    sub = (x[keep], y[keep], None if omega is None else omega[keep])
    gW, gb = R.gradient(*sub, W0, b0, np.float32(l2))
    bW, bb = R.step_bound(x, y, omega, W0, b0, np.float32(l2), got["W"], got["b"])
    L = 1.0 + float(np.float32(l2))
    rW = (np.abs((W0.astype(np.float64) - got["W"]) * L - gW) / bW).max()
    rb = (np.abs((b0.astype(np.float64) - got["b"]) * L - gb) / bb).max()
    r0 = abs(got["loss"][0] - R.objective(*sub, W0, b0, np.float32(l2))) / R.loss_bound(x, y, omega, W0, b0, np.float32(l2))
    r1 = abs(got["loss"][1] - R.objective(*sub, got["W"], got["b"], np.float32(l2))) / R.loss_bound(x, y, omega, got["W"], got["b"], np.float32(l2))
    print(f"D={D} C={C} M={M} weights={weights}: gradient error / bound {rW:.3f} (bias {rb:.3f}), loss[0] {r0:.3f}, loss[1] {r1:.3f}")
    assert rW <= 1.0 and rb <= 1.0 and r0 <= 1.0 and r1 <= 1.0
    assert np.abs(gW).max() > 10 * bW.max()                                    # the comparison has teeth: the bound is far below the gradient
    if weights == "none":                                                      # NULL weights are ones, bit for bit
        ones = fit(store(x), D, y, C, l2, 1, np.ones(M, np.float32), W0, b0)
        for key in got:
            assert got[key].tobytes() == ones[key].tobytes(), key


# ---- c. convergence ---------------------------------------------------------------------------------------------------------------------
def test_convergence():
    C, D, l2, iters = 16, 96, 1e-2, 80
    _, x, y = R.planted(11, 3 * SEGMENT + 37, D, C)                            # tests/test_rows_probe_host.py: float64 meets the bound here
    omega = R.balanced(y, C)[y].astype(np.float32)
    lam = np.float32(l2)
    got = fit(store(x), D, y, C, l2, iters, omega)
    fstar, _, _ = R.optimum(x, y, omega, lam, C)
    f0 = R.objective(x, y, omega, np.zeros((C, D)), np.zeros(C), lam)
    f = R.objective(x, y, omega, got["W"], got["b"], lam)
    bound = R.theorem_bound(lam, iters, f0, fstar)
    print(f"F(0) = {f0:.6f}, F* = {fstar:.6f}, F(device) - F* = {f - fstar:.3e}, bound {bound:.3e}: gap / bound {(f - fstar) / bound:.4f}")
    assert 0.0 <= f - fstar <= bound
    assert abs(got["loss"][0] - f0) <= R.loss_bound(x, y, omega, np.zeros((C, D)), np.zeros(C), lam)
    assert abs(got["loss"][-1] - f) <= R.loss_bound(x, y, omega, got["W"], got["b"], lam)
    assert got["loss"].shape == (iters + 1,) and np.isfinite(got["loss"]).all() and got["loss"][-1] < got["loss"][0]
    # iters = 0 returns the start and loss[0]
    start = fit(store(x), D, y, C, l2, 0, omega, got["W"], got["b"])
    assert start["W"].tobytes() == got["W"].tobytes() and start["b"].tobytes() == got["b"].tobytes()
    assert start["loss"].tobytes() == got["loss"][-1:].tobytes()


# ---- d. invariance, bit for bit ---------------------------------------------------------------------------------------------------------
def test_invariance():
    D, C, M = 96, 17, 2 * SEGMENT + TILE + 3
    rng, x, y = R.planted(77, M, D, C)
    omega = rng.uniform(0.0, 2.0, M).astype(np.float32)
    rows = store(x)
    a, b = fit(rows, D, y, C, 1e-3, 6, omega), fit(rows, D, y, C, 1e-3, 6, omega)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    wide = fit(store(x, pad=40), D, y, C, 1e-3, 6, omega)
    for key in a:
        assert a[key].tobytes() == wide[key].tobytes(), key
    plain, ones = fit(rows, D, y, C, 1e-3, 6), fit(rows, D, y, C, 1e-3, 6, np.ones(M, np.float32))
    for key in plain:
        assert plain[key].tobytes() == ones[key].tobytes(), key
    assert plain["W"].tobytes() != a["W"].tobytes()
    probs, logits = predict(rows, D, a["W"], a["b"])
    assert predict(rows, D, a["W"], a["b"], want_logits=False)[0].tobytes() == probs.tobytes()
    assert predict(store(x, pad=40), D, a["W"], a["b"])[0].tobytes() == probs.tobytes()
    for first, n in ((0, 1), (5, TILE), (TILE - 3, SEGMENT + 9), (M - 7, 7)):
        part = predict(rows, D, a["W"], a["b"], first=first, n=n)
        assert part[0].tobytes() == probs[first:first + n].tobytes() and part[1].tobytes() == logits[first:first + n].tobytes()


# ---- e. refusals: by return code and a word of the message; none of these calls writes an output ---------------------------------------------
def test_refusals():
    lib = _lib.load()
    names = ("rows", "label", "omega", "w0", "b0", "W", "b", "loss", "ws", "probs", "logits")
    bufs = {name: torch.full((1 << 18,), 7.0, device="cuda") for name in names}
    bufs["label"] = torch.zeros(1 << 18, dtype=torch.int32, device="cuda")
    bufs["omega"].fill_(1.0)
    outputs = ("W", "b", "loss", "probs", "logits")

    def rc_fit(n=100, D=64, ld=64, C=5, l2=1e-3, iters=2, ws_bytes=4 << 18, null=("omega", "w0", "b0"), shift=None):
        p = {name: bufs[name].data_ptr() for name in names}
        for name in null:
            p[name] = None
        if shift:
            p[shift] += 4
        return lib.cbas_rows_probe_fit(p["rows"], n, D, ld, p["label"], p["omega"], C, l2, iters, p["w0"], p["b0"], p["W"], p["b"], p["loss"],
                                       p["ws"], ws_bytes, None)

    def rc_predict(n=100, D=64, ld=64, C=5, null=(), shift=None, **_):
        p = {name: bufs[name].data_ptr() for name in names}
        for name in null:
            p[name] = None
        if shift:
            p[shift] += 4
        return lib.cbas_rows_probe_predict(p["rows"], n, D, ld, p["W"], p["b"], C, p["probs"], p["logits"], None)

    def refused(code, word):
        msg = lib.cbas_last_error().decode()
        assert code == -1 and word in msg, (code, word, msg)           # CBAS_EINVAL
    for rc in (rc_fit, rc_predict):
        refused(rc(C=1), "n_classes")
        refused(rc(C=65), "n_classes")
        refused(rc(D=48), "multiple of 32")
        refused(rc(D=0), "multiple of 32")
        refused(rc(D=1568, ld=1568), "multiple of 32")
        refused(rc(ld=32), "ld =")
        refused(rc(ld=68), "multiple of 8")
        refused(rc(n=-1), "n_")
        refused(rc(shift="rows"), "16-byte aligned")
        refused(rc(shift="W"), "16-byte aligned")
        refused(rc(null=("rows",)), "NULL")
        refused(rc(null=("W",)), "NULL")
        refused(rc(null=("b",)), "NULL")
    refused(rc_fit(n=0), "n_train")
    refused(rc_fit(n=4194305), "n_train")
    refused(rc_fit(iters=-1), "iters")
    for l2 in (0.0, -1.0, float("inf"), float("nan")):
        refused(rc_fit(l2=l2), "l2")
    refused(rc_fit(shift="ws"), "16-byte aligned")
    refused(rc_fit(null=("omega", "b0"), shift="w0"), "16-byte aligned")
    for name in ("label", "loss", "ws"):
        refused(rc_fit(null=("omega", "w0", "b0", name)), "NULL")
    refused(rc_predict(null=("probs",)), "NULL")
    need = int(lib.cbas_rows_probe_workspace_bytes(100, 64, 5))
    assert 0 < need <= 4 << 18
    refused(rc_fit(ws_bytes=need - 1), "workspace")
    for args in ((0, 64, 5), (4194305, 64, 5), (100, 48, 5), (100, 1568, 5), (100, 64, 1), (100, 64, 65)):
        assert lib.cbas_rows_probe_workspace_bytes(*args) == -1
    # O(n_train C) plus one (C, D) block per SEGMENT
    big = int(lib.cbas_rows_probe_workspace_bytes(65536, 768, 64))
    assert big <= 65536 * (8 + 4 * 64) + (4 * 64 * 768 + 264) * (65536 // SEGMENT + 3) + 1024
    assert rc_predict(n=0) == 0                                        # does nothing
    torch.cuda.synchronize()
    for name in outputs + ("ws",):                                     # every buffer is as it was
        assert bool((bufs[name] == 7.0).all()), name
    # the checks on the device: a label out of range, a bad weight, Omega = 0 - only the workspace is written
    rows = np.random.default_rng(1).standard_normal(1 << 15).astype(np.float16)
    bufs["rows"].copy_(torch.from_numpy(np.resize(rows.view(np.float32), 1 << 18)).cuda())
    for bad in (5, -1):
        bufs["label"][37] = bad
        refused(rc_fit(), "label")
        bufs["label"][37] = 0
    for bad in (-1.0, float("inf"), float("nan")):
        bufs["omega"][11] = bad
        refused(rc_fit(null=("w0", "b0")), "sample weight")
        bufs["omega"][11] = 1.0
    bufs["omega"][:100] = 0.0
    refused(rc_fit(null=("w0", "b0")), "Omega")
    bufs["omega"][:100] = 1.0
    torch.cuda.synchronize()
    for name in outputs:
        assert bool((bufs[name] == 7.0).all()), name
    # the neighbours that must be served: an exact workspace, every optional pointer NULL or given
    assert rc_fit(ws_bytes=need) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(bufs["W"][:320]).all()) and bool((bufs["W"][320:] == 7.0).all()) and bool((bufs["b"][5:] == 7.0).all())
    assert bool((bufs["loss"][3:] == 7.0).all()) and bool(torch.isfinite(bufs["loss"][:3]).all())
    bufs["w0"].fill_(0.0)
    bufs["b0"].fill_(0.0)
    assert rc_fit(null=()) == 0 and rc_predict(null=("logits",)) == 0
    torch.cuda.synchronize()
    assert bool((bufs["logits"] == 7.0).all()) and bool((bufs["probs"][500:] == 7.0).all())
    assert abs(float(bufs["probs"][:500].sum()) - 100.0) < 1e-3


# ---- f. the Python layer and the command line --------------------------------------------------------------------------------------------
def test_python_layer(tmp_path):
    C, D, stride, folds, l2, iters = 4, 64, 2, 3, 1e-3, 100
    sizes = (300, 420, 260)
    rows_of, labels_of = R.planted_project(5, sizes, D, C)                     # test_rows_probe_host.py: float64 gets every frame right
    paths = []
    for i, rows in enumerate(rows_of):
        paths.append(os.path.join(str(tmp_path), f"clip{i}_cls.h5"))
        with h5io.ClsWriter(paths[-1], D) as w:
            w.append(rows)
    behaviors = [f"b{c}" for c in range(C)]
    instances = [(p, a, b, behaviors[c]) for p, lab in zip(paths, labels_of) for a, b, c in synth.label_runs(lab)]
    index = S.FrameIndex(paths, "cuda:0")
    bank = knn.LabelBank.from_instances(index, instances, behaviors, stride=stride, group="instance")
    x, y, group = R.project_bank(rows_of, labels_of, stride)
    M, N = len(bank), index.n_rows
    assert N == 980 and M == len(y) and np.array_equal(bank.label.cpu().numpy(), y) and np.array_equal(bank.group.cpu().numpy(), group)
    assert bank.rows.cpu().numpy().tobytes() == x.tobytes()
    # fit_probe and probe_labels against the raw entry points, bit for bit
    fitted = index.linear_probe(bank, l2=l2, iters=iters)
    omega = probe.balanced_weights(y, C)[y]
    direct = fit(bank.rows, D, y, C, l2, iters, omega)
    assert fitted.weights.tobytes() == direct["W"].tobytes() and fitted.bias.tobytes() == direct["b"].tobytes()
    assert fitted.loss.tobytes() == direct["loss"].tobytes() and (fitted.l2, fitted.iters, fitted.dim, fitted.behaviors) == (l2, iters, D, behaviors)
    assert np.array_equal(fitted.class_weights, probe.balanced_weights(y, C))
    probs, logits = index.probe_labels(fitted, return_logits=True)
    want = predict(index.rows, D, direct["W"], direct["b"])
    assert probs.shape == (N, C) and probs.dtype == torch.float32 and probs.is_cuda
    assert probs.cpu().numpy().tobytes() == want[0].tobytes() and logits.cpu().numpy().tobytes() == want[1].tobytes()
    assert index.probe_labels(fitted).cpu().numpy().tobytes() == want[0].tobytes()
    truth = np.concatenate(labels_of)
    assert np.array_equal(want[0].argmax(axis=1), truth)                       # planted, well separated: every frame is right
    plain = probe.fit_probe(index, bank, l2=l2, iters=5, class_weights=None)   # no weights at all: NULL
    assert plain.class_weights is None and plain.weights.tobytes() == fit(bank.rows, D, y, C, l2, 5)["W"].tobytes()
    more = probe.fit_probe(index, bank, l2=l2, iters=3, class_weights=None, init=plain)
    assert more.weights.tobytes() == fit(bank.rows, D, y, C, l2, 3, None, plain.weights, plain.bias)["W"].tobytes()
    # the report: every entry predicted by a probe whose fit gave it weight 0
    report = probe.probe_report(index, bank, folds=folds, l2=l2, iters=iters)
    fold_of = R.deal_folds(group, folds)
    pred = np.full(M, -1, np.int64)
    for f in range(folds):
        hold = fold_of == f
        om = (probe.balanced_weights(y, C, ~hold)[y] * ~hold).astype(np.float32)
        one = fit(bank.rows, D, y, C, l2, iters, om)
        pred[hold] = predict(bank.rows, D, one["W"], one["b"])[0][hold].argmax(axis=1)
    assert report == knn.report_from_predictions(y, pred, behaviors) and set(report) == set(knn.knn_report(index, bank, k=5))
    assert report["accuracy"] == 1.0 and report["weighted avg"]["support"] == M
    # the files, and the probabilities where a head's go
    out = knn.write_outputs(index, probs, behaviors, "probe")
    host = probs.cpu().numpy()
    for path, (first, n) in zip(out, index._table):
        names, _, f32 = pipeline.read_outputs_csv(path)
        assert names == behaviors and f32 is not None and f32.tobytes() == host[first:first + n].tobytes()
    events = postprocess.predictions_to_instances(probs[:300].contiguous(), behaviors, "clip0.mp4")
    assert events == postprocess.predictions_to_instances(host[:300], behaviors, "clip0.mp4") and len(events) > 0
    bins = postprocess.activity_bins_device(probs[:300].contiguous(), 0, 0.5, 2)
    assert int(bins.sum()) == int(((host[:300].argmax(axis=1) == 0) & (host[:300, 0] >= 0.5)).sum())
    with pytest.raises(ValueError, match="width"):
        index.linear_probe(knn.LabelBank(bank.rows, bank.label, bank.group, bank.row_group, bank.store_row, behaviors, 32, "instance"))
    with pytest.raises(ValueError, match="width"):
        index.probe_labels(probe.LinearProbe(np.zeros((C, 32)), np.zeros(C), behaviors, 32, l2, 0, [0.0]))
    # the command line, end to end; --save / --load give the same probabilities bit for bit
    labels_csv, saved, rep = (str(tmp_path / name) for name in ("labels.csv", "cli.npz", "report.json"))
    with open(labels_csv, "w") as f:
        f.write("file,start,end,label\n" + "".join(f"{p},{a},{b},{name}\n" for p, a, b, name in instances))
    assert probe.main(["--files", *paths, "--instances", labels_csv, "--l2", str(l2), "--iters", str(iters), "--stride", str(stride), "--folds",
                       str(folds), "--report", rep, "--save", saved, "--write-outputs", "cli"]) == 0
    with open(rep) as f:
        assert json.load(f) == report
    loaded = probe.LinearProbe.load(saved)
    assert loaded.weights.tobytes() == fitted.weights.tobytes() and loaded.bias.tobytes() == fitted.bias.tobytes()
    first_run = [pipeline.read_outputs_csv(p.replace("_cls.h5", "_cli_outputs.csv"))[2] for p in paths]
    assert np.concatenate(first_run).tobytes() == host.tobytes()
    assert probe.main(["--files", *paths, "--load", saved, "--write-outputs", "again"]) == 0
    for p, before in zip(paths, first_run):
        assert pipeline.read_outputs_csv(p.replace("_cls.h5", "_again_outputs.csv"))[2].tobytes() == before.tobytes()
