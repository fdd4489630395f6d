"""CPU suite of precision="fp16": csrc/conv_f16.hip compiled unchanged against the SIMT emulator, through dream_amd.ops / models.
Every entry of the fp16 variant table runs every small shape; the bounds are those of fp16_checks (derived per launch, measured on
the reference end to end)."""
import os

import pytest
import torch

import fp16_checks as fc
from dream_amd import _hip, ops
from emu_util import emulated_hip

NUM_VARIANTS = 8
_FULL = os.environ.get("DREAM_EMU_FULL", "0") == "1"


@pytest.fixture(scope="module")
def emu():
    with emulated_hip() as lib:
        yield lib


def test_variant_table_has_eight_entries(emu):
    assert emu.dream_conv_f16_set_variant(NUM_VARIANTS - 1) == 0
    assert emu.dream_conv_f16_set_variant(NUM_VARIANTS) != 0
    assert emu.dream_conv_f16_set_variant(-1) == 0


@pytest.mark.parametrize("variant", range(NUM_VARIANTS))
def test_conv_f16_variants(emu, variant):
    emu.dream_conv_f16_set_variant(variant)
    try:
        fc.check_conv_f16("cpu", 1, 7, 9, 32, 40, 3, ops.CONV_RELU, seed=variant)
        fc.check_conv_f16("cpu", 2, 12, 20, 64, 7, 3, ops.CONV_OUT_NCHW, x_scale=300.0, w_scale=1e-3, seed=variant)
        fc.check_conv_f16("cpu", 1, 6, 8, 32, 64, 3, ops.CONV_RELU | ops.CONV_UPSAMPLE2X, x_scale=1e-3, w_scale=5.0, seed=variant)
        fc.check_conv_f16("cpu", 2, 9, 11, 64, 48, 1, 0, seed=variant)
        fc.check_conv_f16("cpu", 2, 12, 20, 32, 48, 3, ops.CONV_RELU | ops.CONV_POOL2, seed=variant)
        fc.check_conv_f16("cpu", 1, 13, 9, 64, 32, 3, ops.CONV_RELU | ops.CONV_POOL2, seed=variant)
        fc.check_conv_transpose4x4_f16("cpu", 1, 5, 6, 32, 48, seed=variant)
        fc.check_conv_transpose3x3_f16("cpu", 1, 5, 7, 32, 48, seed=variant)
    finally:
        emu.dream_conv_f16_set_variant(-1)


def test_conv_f16_measured_rule(emu):
    """The rule's own choice (no forced variant) for a shape of each of its branches."""
    fc.check_conv_f16("cpu", 1, 7, 9, 32, 40, 3, ops.CONV_RELU)              # Cout > 32
    fc.check_conv_f16("cpu", 2, 12, 20, 64, 7, 3, ops.CONV_OUT_NCHW)         # Cout <= 32
    fc.check_conv_f16("cpu", 1, 5, 5, 128, 128, 1, 0)                        # tiny grid, >= 128 channels


def test_vgg_q_inference_golden_fp16(emu):
    fc.check_golden_f16("cpu", "vgg_q", (1, 50, 75))


@pytest.mark.skipif(not _FULL, reason="set DREAM_EMU_FULL=1 (minutes under the emulator); the GPU suite runs the structured cases")
def test_hourglass_variant_fp16(emu):
    fc.check_golden_f16("cpu", "vgg_f_ms2_skip", (1, 32, 48))



# ---- what launch_f16 (csrc/conv_f16.hip) and launch_wgrad16 (csrc/wgrad_f16.hip) refuse -----------------------------------------------
# One frame, a 4 x 4 map, 32 -> 32 channels, through ops.call: every case returns before any launch.  The other requirements of the two
# launchers are tripped by fp16_grad_storage_checks.check_dgrad_refusals, fp16_ksplit_checks.check_refused_flags and the three
# check_wgrad_*_zero_repeat_and_flags, or cannot be reached through an entry point.
def _refusal_case():
    B, H, W, C = 1, 4, 4, 32
    hi, _, exp, _ = ops.pack_conv_weight_f16(torch.randn(C, C, 3, 3) * 0.1, 0)
    t = dict(x=torch.ones(B, H, W, C), xh=torch.ones(B, H, W, C + 8, dtype=torch.float16), amax=ops.new_amax("cpu"), w=hi, exp=exp,
             y=torch.zeros(B, H, W, C + 8), ws=torch.zeros(2 * B * H * W * C + 1024 + 9 * 64 * C), dwp=torch.zeros(9, 64, C))
    p = {k: ops.ptr(v) for k, v in t.items()}
    shape = (B, H, W, C, C, _hip.cout_pad(C))
    return t, p, shape


def _conv_f32(p, shape, x="x", amax="amax", residual=None, flags=0, **over):
    b, h, w, cin, cout, pad = (over.get(k, v) for k, v in zip(("B", "H", "W", "Cin", "Cout", "CoutPad"), shape))
    return ("dream_conv2d_f16_nhwc_f32", p.get(x), p.get(amax), p["w"], p["exp"], None, None, p.get(residual), p["y"], None,
            b, h, w, cin, cout, pad, 3, 1, flags, None)


def _conv_f16(p, shape, x, y, flags=0):
    return ("dream_conv2d_f16_nhwc_f16", x, p["w"], p["exp"], None, None, y, None) + shape + (3, 1, flags, None)


def _wgrad(name, p, shape, head, B=None, H=None, W=None, Cdy=None):
    b, h, w, cin, cout, _ = shape
    return (name,) + head + (p["dwp"], None, p["ws"], B or b, H or h, W or w, cin, Cdy or cout, 64, 0, None)


REFUSALS = {
    # launch_f16
    "null amax_in": (lambda p, s: _conv_f32(p, s, amax="none"), "null pointer"),
    "half storage with the ReLU-mask flag": (lambda p, s: _conv_f16(p, s, p["xh"], p["y"], ops.CONV_RELUMASK), "flags|ReLU mask"),
    "half x off 16 bytes": (lambda p, s: _conv_f16(p, s, p["xh"] + 2, p["y"]), "16-byte aligned"),
    "half y off 16 bytes": (lambda p, s: _conv_f16(p, s, p["xh"], p["y"] + 8), "16-byte aligned"),
    "half mask of a half gradient off 4 bytes": (
        lambda p, s: ("dream_conv2d_f16_g16_nhwc_f16", p["xh"], p["w"], p["exp"], p["xh"] + 2, p["y"], None) + s + (3, 1, 0, None),
        "half mask|half-stored data gradient"),
    "Cin no multiple of 32": (lambda p, s: _conv_f32(p, s, Cin=48), "Cin=48 must be a multiple of 32"),
    "CoutPad below Cout": (lambda p, s: _conv_f32(p, s, CoutPad=16), "CoutPad=16"),
    "pool with the NCHW output": (lambda p, s: _conv_f32(p, s, flags=ops.CONV_POOL2 | ops.CONV_OUT_NCHW), "max-pool"),
    "ReLU-mask flag without the mask": (lambda p, s: _conv_f32(p, s, flags=ops.CONV_RELUMASK), "ReLU mask"),
    "more than 1024 slices": (
        lambda p, s: ("dream_conv2d_f16_ksplit_nhwc_f16", p["xh"], p["w"], p["exp"], None, None, p["y"], None, p["ws"], 1025) + s
        + (3, 1, 0, None), "1024 slices"),
    # launch_wgrad16
    "wgrad: null amax_dy": (lambda p, s: _wgrad("dream_conv3x3_wgrad_f16_nhwc_f32", p, s, (p["x"], p["amax"], p["x"], None)), "null pointer"),
    "wgrad: Cdy no multiple of 4": (lambda p, s: _wgrad("dream_conv3x3_wgrad_f16_nhwc_f32", p, s, (p["x"], p["amax"], p["x"], p["amax"]), Cdy=30),
                                    "bad shape"),
    "wgrad: 2^45 elements": (lambda p, s: _wgrad("dream_conv3x3_wgrad_f16_nhwc_f32", p, s, (p["x"], p["amax"], p["x"], p["amax"]),
                                                 B=1 << 20, H=1 << 10, W=1 << 10), "too large"),
    "wgrad: half x off 16 bytes": (lambda p, s: _wgrad("dream_conv3x3_wgrad_f16_x16_nhwc_f32", p, s, (p["xh"] + 2, p["x"], p["amax"])),
                                   "half x must be 16-byte aligned"),
    "wgrad: half dy off 16 bytes": (lambda p, s: _wgrad("dream_conv3x3_wgrad_f16_x16_dy16_nhwc_f32", p, s, (p["xh"], p["xh"] + 2, p["amax"])),
                                    "half dy .*16-byte aligned"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_launch_refusals(emu, what):
    tensors, pointers, shape = _refusal_case()
    make_args, message = REFUSALS[what]
    args = make_args(pointers, shape)
    with pytest.raises(RuntimeError, match="%s failed.*(%s)" % (args[0], message)):
        ops.call(*args)
    assert float(tensors["y"].abs().max()) == 0.0 and float(tensors["dwp"].abs().max()) == 0.0      # nothing was launched
