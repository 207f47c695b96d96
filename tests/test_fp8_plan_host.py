"""fp8 plans of the MX-fp8 mode (precision 2), the parts that need no GPU: names and masks, the file stamp per plan, the
refusal of a bundle trained on another plan's rows, and the CPU restatement the GPU tests measure the encoder against."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from cbas_amd import config as C, weights as W, synth


def test_plan_names_and_masks():
    assert C.FP8_PLANS == {"all": 15, "mlp": 12, "mlp_qkv": 13, "up": 4, "down": 8}
    assert C.FP8_PLAN_BITS == {"qkv": 1, "proj": 2, "up": 4, "down": 8}
    assert C.FP8_PLAN_DEFAULT == 15 and C.parse_fp8_plan(None) == 15
    for name, mask in C.FP8_PLANS.items():
        assert C.parse_fp8_plan(name) == mask and C.parse_fp8_plan(mask) == mask and C.parse_fp8_plan(str(mask)) == mask
        assert C.fp8_plan_name(mask) == name
    assert C.parse_fp8_plan(" MLP ") == 12                       # what CBAS_FP8_PLAN may carry
    assert C.parse_fp8_plan("up+down") == 12 and C.parse_fp8_plan("qkv+up+down") == 13 and C.parse_fp8_plan("proj") == 2
    assert C.parse_fp8_plan(0) == 0 and C.fp8_plan_name(0) == "p0" and C.fp8_plan_name(5) == "p5"
    # the mask bits are the header's
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cbas_mi355x.h")).read()
    for macro, bit in (("QKV", 1), ("PROJ", 2), ("UP", 4), ("DOWN", 8), ("ALL", 15)):
        assert f"#define CBAS_FP8_PLAN_{macro}" in hdr
        assert int(hdr.split(f"#define CBAS_FP8_PLAN_{macro}")[1].split()[0]) == bit


@pytest.mark.parametrize("bad", ["", "mlpx", "up,down", "up+", "16", "-1", 16, -1, 1.5, True, "0x4"])
def test_bad_plans_are_refused(bad):
    with pytest.raises(ValueError, match="fp8 plan"):
        C.parse_fp8_plan(bad)


def test_file_stamp_names_the_plan():
    from cbas_amd import pipeline as P
    assert P.fp8_tag(None) == P.fp8_tag("all") == P.fp8_tag(15) == P.FP8_TAG == "mx-fp8"
    assert P.fp8_tag("mlp") == "mx-fp8-mlp" and P.fp8_tag(13) == "mx-fp8-mlp_qkv" and P.fp8_tag("up") == "mx-fp8-up"
    assert P.fp8_tag("down") == "mx-fp8-down" and P.fp8_tag(5) == "mx-fp8-p5"
    P.set_project_stamp("some/encoder")
    try:
        a16 = P.file_attrs(SimpleNamespace(precision=0, fp8_plan=0))
        a_all = P.file_attrs(SimpleNamespace(precision=2, fp8_plan=15))
        a_old = P.file_attrs(SimpleNamespace(precision=2))                    # an object without the property: the default plan
        a_mlp = P.file_attrs(SimpleNamespace(precision=2, fp8_plan=12))
    finally:
        P.set_project_stamp(None)
    assert a16["encoder_model_identifier"] == "some/encoder" and "encoder_precision" not in a16
    assert a_all == a_old and a_all["encoder_model_identifier"] == "some/encoder#mx-fp8" and a_all["encoder_precision"] == "mx-fp8"
    assert a_mlp["encoder_model_identifier"] == "some/encoder#mx-fp8-mlp" and a_mlp["encoder_precision"] == "mx-fp8-mlp"
    assert len({P.fp8_tag(mask) for mask in range(16)}) == 16                 # one stamp per mask
    # without a project only the precision attribute is written
    assert P.file_attrs(SimpleNamespace(precision=2, fp8_plan=4)) == {"encoder_precision": "mx-fp8-up"}


def test_encode_files_refuses_a_bundle_of_another_plan(tmp_path, capsys):
    from cbas_amd import encode_files as E
    from cbas_amd.bundle import load_model_bundle
    assert E.run_stamp("enc", 0) == E.run_stamp("enc", 4, None) == "enc"
    assert E.run_stamp("enc", 2) == E.run_stamp("enc", 2, "all") == "enc#mx-fp8"
    assert E.run_stamp("enc", 2, "mlp") == "enc#mx-fp8-mlp"

    def bundle(trained_on):
        d = tmp_path / trained_on.replace("#", "_")
        d.mkdir(exist_ok=True)
        # a v2 architecture: a bundle that passes the encoder comparison is then refused for THAT reason, before any weight
        # (or GPU) is touched - which tells the two refusals apart
        (d / "model_meta.json").write_text(json.dumps({"encoder_model_identifier": trained_on,
                                                        "head_architecture_version": "ClassifierLegacyLSTM"}))
        return str(d)

    for trained, run, mismatch in [("enc#mx-fp8", E.run_stamp("enc", 2, "mlp"), True),
                                   ("enc#mx-fp8-mlp", E.run_stamp("enc", 2, "all"), True),
                                   ("enc#mx-fp8-mlp", E.run_stamp("enc", 2, "mlp_qkv"), True),
                                   ("enc", E.run_stamp("enc", 2, "up"), True),
                                   ("enc#mx-fp8-mlp", E.run_stamp("enc", 0), True),
                                   ("enc#mx-fp8-mlp", E.run_stamp("enc", 2, 12), False)]:
        assert load_model_bundle(bundle(trained), device="cpu", project_encoder=run) == (None, None)
        out = capsys.readouterr().out
        assert ("Encoder mismatch" in out) == mismatch, (trained, run, out)
        assert ("has architecture" in out) == (not mismatch)


def test_encoder_refuses_a_plan_outside_precision_2():
    from cbas_amd.encoder import DinoEncoder
    cfg = C.NAMED_VIT["tiny"]
    with pytest.raises(ValueError, match="needs precision=2"):           # raised before any device is touched
        DinoEncoder.from_weights(cfg, {}, "cuda", precision=0, fp8_plan="mlp")
    with pytest.raises(ValueError, match="fp8 plan"):
        DinoEncoder.from_weights(cfg, {}, "cuda", precision=2, fp8_plan="mpl")


@pytest.fixture(scope="module")
def tiny():
    cfg = C.NAMED_VIT["tiny"]
    w = W.synth_encoder_weights(cfg, 1234)
    fr = synth.noise_frames(3, 2, 64, 64)
    from oracle import vit_oracle as V
    pixels = np.repeat(V.preprocess_green(fr)[:, None], 3, axis=1)
    return cfg, w, pixels


def test_restatement_plan_15_is_the_mx_oracle_and_plan_0_the_fp32_oracle(tiny):
    from oracle import mx_oracle as MX, vit_oracle as V
    from fp8_plan_restatement import vit_forward_plan
    cfg, w, pixels = tiny
    assert np.array_equal(vit_forward_plan(pixels, w, cfg, 15), MX.vit_forward_mx(pixels, w, cfg))
    assert np.array_equal(vit_forward_plan(pixels, w, cfg, 0), V.vit_forward(pixels, w, cfg))


def test_restatement_plans_differ_and_shrink_the_error(tiny):
    """Every named plan is its own arithmetic (no two give the same rows), and quantising fewer GEMMs moves the CLS rows less:
    the ordering the per-plan table of the GPU test is read against."""
    from fp8_plan_restatement import vit_forward_plan
    cfg, w, pixels = tiny
    ref = vit_forward_plan(pixels, w, cfg, 0)[:, 0].astype(np.float64)
    rows = {n: vit_forward_plan(pixels, w, cfg, m)[:, 0].astype(np.float64) for n, m in C.FP8_PLANS.items()}
    err = {n: float((np.linalg.norm(r - ref, axis=1) / np.linalg.norm(ref, axis=1)).max()) for n, r in rows.items()}
    names = list(rows)
    for i, a in enumerate(names):
        assert np.isfinite(rows[a]).all() and err[a] > 0
        for b in names[i + 1:]:
            assert not np.array_equal(rows[a], rows[b]), (a, b)
    assert max(err["up"], err["down"]) < err["all"], err
