"""CPU suite of the ragged training steps (ragged_train_checks): the product's kernels compiled unchanged against the SIMT emulator,
driven by the product's host code through whole training steps at (2, 37, 50), (1, 35, 45), (2, 75, 101) and (2, 33, 47).  The default
suite runs three shipped-architecture fp32 cases (10, 14 and 82 s under the emulator); DREAM_EMU_FULL=1 adds resnet_f, the variants, the
switches, F(4x4) and the fp16 modes, which the GPU suite (test_gpu_ragged_training.py) always runs."""
import os

import pytest

import ragged_train_checks as rc
from emu_util import emulated_hip

_FULL = os.environ.get("DREAM_EMU_FULL", "0") == "1"
_full_only = pytest.mark.skipif(not _FULL, reason="set DREAM_EMU_FULL=1 (minutes under the emulator); the GPU suite runs these on the device")


@pytest.fixture(scope="module")
def emu():
    with emulated_hip() as lib:
        yield lib


@pytest.mark.parametrize("name", rc.EMULATED_ALWAYS)
def test_fp32_step_matches_the_oracle(emu, name):
    rc.check_fp32_step("cpu", name)


@_full_only
@pytest.mark.parametrize("name", [n for n in rc.FP32_CASES if n not in rc.EMULATED_ALWAYS])
def test_fp32_step_matches_the_oracle_every_mode(emu, name):
    rc.check_fp32_step("cpu", name)


@_full_only
@pytest.mark.parametrize("name", rc.REFUSED_VARIANTS)
def test_multi_stage_variants_refuse_the_shape_as_the_reference_does(emu, name):
    rc.check_variant_refused("cpu", name)


@_full_only
@pytest.mark.parametrize("mode", rc.FP16_CASES)
def test_fp16_mode_within_its_own_yardstick(emu, mode):
    rc.check_fp16_step("cpu", mode)
