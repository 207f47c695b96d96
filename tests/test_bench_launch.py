"""`python bench.py --gpus N` must produce an N-rank run by itself: with N > 1 and no launcher around it,
bench.py starts the ranks as child processes; it never measures one GPU under an N-GPU label."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(argv, env_extra=None, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CBAS_BUILD_DEBUG")}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    return r, lines


def test_more_ranks_than_devices_over_rccl_is_refused_with_a_null_value():
    """Here (no GPU) and on a one-GPU box alike: `--gpus 2` over RCCL cannot run; the single line says so and the exit code is 2."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("two devices visible: the request is satisfiable")
    r, lines = _run(["--gpus", "2", "--steps", "3", "--warmup", "1"], timeout=300)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["value"] is None and rec["n_gpus"] == 2 and rec["ranks_seen"] == 0 and "device(s) are visible" in rec["error"]


@pytest.mark.gpu
def test_gpus_2_starts_two_ranks_by_itself_gloo_rehearsal():
    """CBAS_DIST_BACKEND=gloo python bench.py --gpus 2: two child ranks (sharing this box's GPU - a rehearsal of the control
    flow, not a measurement), ONE line on stdout, n_gpus = ranks_seen = 2, weak scaling: 2 x K x batch frames."""
    r, lines = _run(["--gpus", "2", "--steps", "6", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-gates", "--files", "1",
                     "--clip-frames", "512", "--preroll-seconds", "0.2"], {"CBAS_DIST_BACKEND": "gloo"})
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["ranks_seen"] == 2 and rec["scaling"] == "weak"
    assert rec["value"] and rec["value"] > 0
    assert rec["config"]["frames_per_gpu"] == 6 * 64
    assert abs(rec["value"] - 2 * 6 * 64 / (rec["ms_per_step"] * 6e-3)) < 0.01 * rec["value"]
    assert rec["files_path"]["value"]


@pytest.mark.gpu
def test_default_line_carries_the_contract_fields():
    """--full: one JSON line on stdout with the fields the driver and the judge read: BASELINE.json's metric string verbatim, whole-job
    frames/s, `roofline` (bound, achieved, peak, frac, traffic) from HIP events taken live, `cpu_baseline` (value, cores, kind,
    sample) with the ViT-S cfg1 figure beside ViT-B's, and the label statement next to `value` (fp16 operands: not identical)
    and inside `label_exact` (precision 4, the drop-in's default: identical).  Runs on the PRODUCT library (no debug symbols)."""
    r, lines = _run(["--steps", "12", "--warmup", "2", "--full", "--cpu-frames", "64", "--files", "1", "--clip-frames", "512",
                     "--preroll-seconds", "0.2"], timeout=900)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    assert rec["metric"] == base["metric"] and rec["unit"] == "frames/s" and rec["higher_is_better"] is True
    assert rec["n_gpus"] == 1 and rec["ranks_seen"] == 1 and rec["steps"] == 12 and rec["warmup"] == 2 and rec["scaling"] == "weak"
    assert rec["vs_baseline"] is None and rec["data"] == "synthetic" and rec["dtype"] == "f16"
    assert abs(rec["value"] - 12 * 64 / (rec["ms_per_step"] * 12e-3)) < 0.01 * rec["value"] and rec["value"] > 2000
    rf = rec["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and rf["peak"] == 2500.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and 0.1 < rf["frac"] < 1.0 and "traffic" in rf
    cb = rec["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb
    assert cb["cfg1_vits16"]["value"] > cb["value"]                       # ViT-S/16 (cfg1) beside ViT-B/16
    assert rec["labels_identical"] is False                                # the fp16-operand mode flips near-tie labels ...
    le = rec["label_exact"]
    assert le["precision"] == 4 and le["labels_identical"] is True and le["value"] > 2000      # ... precision 4 does not
    assert rec["gates"]["cls_rel_err_max"] <= 1e-3 and le["gates"]["cls_rel_err_max"] <= 5e-6
    assert rec["value_r3_definition"]["value"] > 0 and rec["hbm_resident"]["bit_identical_to_value_pass"] is True


@pytest.mark.gpu
def test_plain_run_times_the_headline_pass_and_dumps_its_outputs(tmp_path):
    """Without --full: the line's headline fields only (none of the secondary measurements), `steps` timed steps, and
    --dump-outputs writes the timed pass's CLS rows and probabilities - the same bytes from a second run with the same
    arguments, and checked outside bench.py: the CLS rows of the first frames of the seeded clip against the CPU fp32
    oracle (the fp16 mode's bar for fp16 rows), the probabilities against the head run here on the dumped rows."""
    dumps = []
    for i in range(2):
        d = tmp_path / f"out{i}"
        r, lines = _run(["--steps", "6", "--warmup", "2", "--preroll-seconds", "0.2", "--dump-outputs", str(d)], timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        assert len(lines) == 1, lines
        rec = json.loads(lines[0])
        assert rec["steps"] == 6 and rec["warmup"] == 2 and rec["dtype"] == "f16" and rec["higher_is_better"] is True
        assert abs(rec["value"] - 6 * 64 / (rec["ms_per_step"] * 6e-3)) < 0.01 * rec["value"] and rec["value"] > 2000
        for k in ("hbm_resident", "value_r3_definition", "roofline", "files_path", "gates", "label_exact", "cpu_baseline"):
            assert k not in rec, k
        import numpy as np
        cls, probs, idx = (np.load(d / f"{n}.npy") for n in ("cls", "probs", "row_index"))
        assert cls.dtype == np.float32 and probs.dtype == np.float32 and idx.dtype == np.float64
        assert cls.shape == (6 * 64, 768) and probs.shape == (6 * 64, 9) and (idx == np.arange(6 * 64)).all()
        assert np.isfinite(cls).all() and np.allclose(probs.sum(1), 1.0, atol=1e-4)
        dumps.append((cls, probs))
    assert all(np.array_equal(a, b) for a, b in zip(*dumps))
    import torch
    from cbas_amd import config as C, weights as W
    from cbas_amd.head import ClassifierLSTMDeltas
    from oracle import vit_oracle_torch as VT
    cls, probs = dumps[0]
    gen = torch.Generator(device="cuda:0")                 # bench.py's clip: 6 batches of seeded uniform RGB on device 0
    gen.manual_seed(1000)
    clip = torch.randint(0, 256, (6 * 64, 224, 224, 3), dtype=torch.uint8, device="cuda:0", generator=gen)[:4].cpu().numpy()
    cfg = C.VIT_B16
    ref = VT.encode_frames(clip, VT.to_torch(W.synth_encoder_weights(cfg, 1234)), cfg, 4).astype(np.float64)
    rel = np.linalg.norm(cls[:4] - ref, axis=1) / np.linalg.norm(ref, axis=1)
    assert rel.max() < 1e-3 + 5e-4, rel                  # the fp16 mode's bar + the fp16 storage rounding (test_gpu_parity)
    head = ClassifierLSTMDeltas(768, 9, seq_len=31)
    head.load_state_dict(W.synth_head_weights(C.HeadConfig(in_features=768, out_features=9, seq_len=31), 4321))
    head.to("cuda:0")
    p = head.infer_clip(torch.from_numpy(cls.astype(np.float16)).to("cuda:0")).cpu().numpy()
    head.close()
    assert np.abs(p - probs).max() < 1e-3, np.abs(p - probs).max()


def test_dump_outputs_stays_within_its_budget_with_a_fixed_sample(tmp_path, monkeypatch):
    """Above the budget --dump-outputs keeps a seeded sample of rows: the same rows every time, under 64 MB in all."""
    import numpy as np
    # bench.py sets this on import: set it here first, so that monkeypatch restores the caller's state (unset or not) afterwards
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    monkeypatch.syspath_prepend(REPO)
    import bench
    n = 24000
    rng = np.random.default_rng(1)
    rows = [(rng.standard_normal((n // 2, 768), dtype=np.float32), rng.random((n // 2, 9), dtype=np.float32)) for _ in range(2)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), bench.sample_rows(rows))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64e6 and total > 0.9 * bench.DUMP_BYTES
    idx = np.load(tmp_path / "a" / "row_index.npy").astype(np.int64)
    assert len(idx) < n and (np.diff(idx) > 0).all()
    full = np.concatenate([c for c, _ in rows])
    assert np.array_equal(np.load(tmp_path / "a" / "cls.npy"), full[idx])
    for f in ("cls.npy", "probs.npy", "row_index.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    small = [(c[:100], p[:100]) for c, p in rows]
    bench.dump_outputs(str(tmp_path / "c"), bench.sample_rows(small))
    assert np.array_equal(np.load(tmp_path / "c" / "probs.npy"), np.concatenate([p for _, p in small]))
    assert np.array_equal(np.load(tmp_path / "c" / "row_index.npy"), np.arange(200))
