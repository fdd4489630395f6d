"""CPU suite of precision="fp16": csrc/conv_f16.hip compiled unchanged against the SIMT emulator, through dream_amd.ops / models.
Every entry of the fp16 variant table runs every small shape; the bounds are those of fp16_checks (derived per launch, measured on
the reference end to end)."""
import os

import pytest

import fp16_checks as fc
from dream_amd import ops
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

