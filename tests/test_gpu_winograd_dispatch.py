"""GPU: which launches a vgg_64 eval step takes, in order.  Every parity test passes when a dispatch regression sends a layer down
a slower but correct path; this one does not.  The ordered C entry points ([r[6] for r in KernelTimer.records]: the ordered
form of what KernelTimer.entry_points() counts) of one decoder call followed by one encoder call, after two conditioning frames
and declare_frozen_skips - the set-up of tests/test_gpu_upconv_live.py's rollout test - are compared with literals.

B = 32 is the smallest batch at which every upsampled Winograd layer takes the form (ops.winograd_ok: T % 128 == 0); at B = 4
nothing Winograd runs in the decoder.

The literals were RECORDED, not derived: this file was run on a checkout of the parent commit acd353b ("Upsample + Winograd
conv: drop the 11 transform positions that are zero") on an MI355X, before the launchers in dvg_amd/csrc/winograd.hip and the
call sites in fused.conv3_bn_act were folded (docs/DESIGN_NOTES_winograd_launchers.md).  A change that moves a launch on purpose
records them again and says so."""
import pytest
import torch

from oracle import params
from tests.common import dev

pytestmark = pytest.mark.gpu
B = 32

# the switches the literals hold under (dvg_amd.fused): their defaults
DEFAULTS = {"WINOGRAD": 4, "WINOGRAD_CHAIN": True, "_CHAIN_LEVEL": 3, "UPCONV_WINOGRAD": True, "UPCONV_WINO_LIVE": True,
            "_UPCONV_WINO_MAX": 16, "WINOGRAD_LAYER_OVERRIDE": {}, "LAST_PROJ_FUSED": True, "SKIP_HOIST": True,
            "UPCONV_AS_CONVT": True, "CONV3_WX": True, "FIRST_PAIR": True}

# name -> (ENERGY tile policy, grad mode enabled with every parameter requires_grad_(False))
CASES = {"latency": (False, False), "energy": (True, False), "latency_grad_mode": (False, True)}

EXPECTED = {
    "latency": """
        dvg_stem_up_winograd_input_live dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output dvg_gemm_batched_k16_as
        dvg_winograd_output_input_live dvg_gemm_batched_k16 dvg_winograd_output_input dvg_gemm_batched_k16
        dvg_winograd_output_up_input_live dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output
        dvg_gemm_batched_k16_as dvg_winograd_output_input_live dvg_gemm_batched_k16 dvg_winograd_output_input
        dvg_gemm_batched_k16 dvg_winograd_output dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output
        dvg_convT4x4s2_bn_act_v2 dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output dvg_conv3x3_bn_act_v2
        dvg_convT4x4s2_bn_act_proj dvg_convT_gather dvg_conv3x3_first_pair dvg_winograd_input dvg_gemm_batched_k16
        dvg_winograd_output_input dvg_gemm_batched_k16 dvg_winograd_output_pool_input dvg_gemm_batched_k16
        dvg_winograd_output_input dvg_gemm_batched_k16 dvg_winograd_output_input dvg_gemm_batched_k16
        dvg_winograd_output_pool_input dvg_gemm_batched_k16 dvg_winograd_output_input dvg_gemm_batched_k16
        dvg_winograd_output_input dvg_gemm_batched_k16 dvg_winograd_output dvg_gemm_nt_bias_act
    """.split(),
    "energy": """
        dvg_stem_up_winograd_input_live dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output dvg_gemm_batched_k16_as
        dvg_winograd_output_input_live dvg_gemm_batched_k16 dvg_winograd_output_input dvg_gemm_batched_k16
        dvg_winograd_output_up_input_live dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output
        dvg_gemm_batched_k16_as dvg_winograd_output_input_live dvg_gemm_batched_k16 dvg_winograd_output_input
        dvg_gemm_batched_k16 dvg_winograd_output dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output
        dvg_convT4x4s2_bn_act_v2 dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output dvg_conv3x3_bn_act_wx
        dvg_convT4x4s2_bn_act_proj dvg_convT_gather dvg_conv3x3_first_pair_wx dvg_winograd_input dvg_gemm_batched_k16
        dvg_winograd_output_input dvg_gemm_batched_k16 dvg_winograd_output_pool_input dvg_gemm_batched_k16
        dvg_winograd_output_input dvg_gemm_batched_k16 dvg_winograd_output_input dvg_gemm_batched_k16
        dvg_winograd_output_pool_input dvg_gemm_batched_k16 dvg_winograd_output_input dvg_gemm_batched_k16
        dvg_winograd_output_input dvg_gemm_batched_k16 dvg_winograd_output dvg_gemm_nt_bias_act
    """.split(),
    "latency_grad_mode": """
        dvg_stem_gemm dvg_conv3x3_bn_act_v2 dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output dvg_winograd_input
        dvg_gemm_batched_k16 dvg_winograd_output dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output
        dvg_conv3x3_bn_act_v2 dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output dvg_winograd_input
        dvg_gemm_batched_k16 dvg_winograd_output dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output
        dvg_conv3x3_bn_act_v2 dvg_convT4x4s2_bn_act_v2 dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output
        dvg_conv3x3_bn_act_v2 dvg_convT4x4s2_bn_act_v2 dvg_pixel_proj dvg_convT_gather dvg_conv3x3_first_pair
        dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output dvg_winograd_input dvg_gemm_batched_k16
        dvg_winograd_output dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output dvg_winograd_input
        dvg_gemm_batched_k16 dvg_winograd_output dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output
        dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output dvg_winograd_input dvg_gemm_batched_k16
        dvg_winograd_output dvg_winograd_input dvg_gemm_batched_k16 dvg_winograd_output dvg_gemm_nt_bias_act
    """.split(),
}


def sequence(case):
    """The ordered entry points of one decoder call + one encoder call."""
    from dvg_amd import fused, ops
    from tests.test_gpu_configs import _build
    energy, grad_mode = CASES[case]
    (enc, dec, *_), _ = _build("vgg", 64, 1, B, 8900)
    enc.to(dev()).eval(), dec.to(dev()).eval()
    for p in list(enc.parameters()) + list(dec.parameters()):
        p.requires_grad_(False)
    frames = [params.frames(8910 + i, B, 1, 64).to(dev()) for i in range(2)]
    vec = params.normal(8920, B, 90, scale=0.5).tanh().to(dev())
    fused.clear_skip_hoist_cache()
    ops.clear_skip_proj_cache()
    timer = ops.KernelTimer()
    try:
        with torch.set_grad_enabled(grad_mode), ops.tile_policy(energy):
            for f in frames:
                _, skips = enc(f)
            fused.declare_frozen_skips(skips)
            ops.set_timer(timer)
            try:
                enc(dec([vec, skips]))
            finally:
                ops.set_timer(None)
        torch.cuda.synchronize()
    finally:
        fused.clear_skip_hoist_cache()
        ops.clear_skip_proj_cache()
    return [r[6] for r in timer.records]


@pytest.mark.parametrize("case", list(CASES))
def test_a_vgg_64_eval_step_takes_the_recorded_launches_in_order(case):
    from dvg_amd import _lib, fused
    moved = {k: getattr(fused, k) for k, v in DEFAULTS.items() if getattr(fused, k) != v}
    if moved:
        pytest.skip(f"the sequences were recorded under the default switches; set here: {moved}")
    if _lib.lib().dvg_mfma_mode() != 1:
        pytest.skip("the sequences were recorded with the product library (dvg_mfma_mode() == 1)")
    got = sequence(case)
    print(case, len(got), " ".join(got))
    assert got == EXPECTED[case], [(i, g, e) for i, (g, e) in enumerate(zip(got, EXPECTED[case])) if g != e][:4]
