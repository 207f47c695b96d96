"""The shape of a ViT forward's launch schedule (api_enc.hip run_blocks / run_blocks_f32), which bit identity of the rows cannot
pin: a duplicated or additional launch can leave every output untouched.

One block is LayerNorm 1 -> q|k|v -> attention -> o_proj -> LayerNorm 2 -> up -> down, behind one patch GEMM.  The expected launch
counts per profiling category follow from that schedule, for L layers:

* the pruned last layer (the default) splits its q|k|v GEMM in two - k|v of every row, q of the CLS rows - so q|k|v has L + 1
  launches with it and L without; every other GEMM and attention run once per layer either way;
* LayerNorm runs twice per layer.  A precision-2 plan whose q|k|v GEMM is MX-fp8 writes the pruned layer's LayerNorm 1 twice
  (MX-fp8 for k|v of every row, fp16 for the CLS queries): one more.  Under the LayerNorm fold only the row statistics before
  layer 0 and the pruned layer's two CLS-row LayerNorms remain: 3, and 1 without the pruning.
"""
import pytest
import torch

from cbas_amd import config as C, weights as W, synth

pytestmark = pytest.mark.gpu

# the smallest width the LayerNorm fold and MX-fp8 accept
SMALL = C.ViTConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=3, num_attention_heads=4)

CASES = {
    "p0": (SMALL, 0, None, False), "p1": (SMALL, 1, None, False), "p3": (SMALL, 3, None, False), "p4": (SMALL, 4, None, False),
    "p2_all": (SMALL, 2, "all", False), "p2_mlp": (SMALL, 2, "mlp", False),
    "p0_ln_fold": (SMALL, 0, None, True),
    "gated_p0": (C.NAMED_VIT["tiny_gated"], 0, None, False), "gated_p3": (C.NAMED_VIT["tiny_gated"], 3, None, False),
    "gated_p4": (C.NAMED_VIT["tiny_gated"], 4, None, False),
}


def expected_launches(L, prune, fold, f8_qkv):
    if fold:
        layernorm = 3 if prune else 1
    else:
        layernorm = 2 * L + (1 if prune and f8_qkv else 0)
    return {"patch_gemm": 1, "layernorm": layernorm, "qkv_gemm": L + 1 if prune else L, "attention": L, "oproj_gemm": L,
            "up_gemm": L, "down_gemm": L}


@pytest.mark.parametrize("case", list(CASES))
def test_launch_counts_follow_the_schedule(case):
    from cbas_amd.encoder import DinoEncoder
    cfg, precision, plan, fold = CASES[case]
    fr = torch.from_numpy(synth.noise_frames(3, 3, 32, 48)).cuda()
    enc = DinoEncoder.from_weights(cfg, W.synth_encoder_weights(cfg, 1234), "cuda", max_batch=4, max_frame=(32, 48),
                                   precision=precision, fp8_plan=plan)
    try:
        if fold:
            enc.debug_option("ln_fold", 1)
        f8_qkv = bool(enc.fp8_plan & C.FP8_PLAN_BITS["qkv"])
        for prune in (True, False):
            enc.set_prune_last_layer(prune)
            quiet16, quiet32 = enc.encode_u8(fr)
            enc.profile(True)
            prof16, prof32 = enc.encode_u8(fr)
            prof = enc.profile_read()
            enc.profile(False)
            torch.cuda.synchronize()
            got = {name: rec["launches"] for name, rec in prof.items()}
            print(f"[schedule {case} prune={prune}] {got}")
            assert got == expected_launches(cfg.num_hidden_layers, prune, fold, f8_qkv), (case, prune)
            assert torch.equal(prof32, quiet32) and torch.equal(prof16, quiet16), (case, prune)
    finally:
        enc.close()
