"""GPU suite (-m gpu) of train_activation_storage="fp16": the half-x weight gradient, the half-mask data gradient, the half-x max-pool
backward and the widening pass through the C ABI on an MI355X, and a vgg_q training step on them, held to the bounds of
fp16_train_storage_checks (bit equality per launch; measured on the CPU reference end to end)."""
import pytest
import torch

import fp16_train_storage_checks as sc
from dream_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
NUM_VARIANTS = 8


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_library():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    _hip.check_symbols()
    with open("/proc/self/maps") as f:
        assert "libdream_hip.so" in f.read(), "the native HIP library is not loaded"
    yield


@pytest.mark.parametrize("shape", sc.WGRAD_CASES, ids=lambda s: "x".join(str(v) for v in s[:5]))
def test_wgrad_half_x(shape):
    sc.check_wgrad_x16(DEV, *shape)


def test_wgrad_half_x_zero_repeat_and_flags():
    sc.check_wgrad_x16_zero_repeat_and_flags(DEV)


@pytest.mark.parametrize("variant", list(range(NUM_VARIANTS)) + [-1])
def test_masked_dgrad_half_mask_variants(variant):
    lib = _hip.lib()
    lib.dream_conv_f16_set_variant(variant)
    try:
        sc.check_dgrad_mask16_shapes(DEV, seed=max(variant, 0))
    finally:
        lib.dream_conv_f16_set_variant(-1)


def test_maxpool_backward_half_x():
    sc.check_pool_bwd_x16(DEV)


def test_widening():
    sc.check_widen(DEV)


def test_training_step_half_storage():
    sc.check_training_step(DEV)


def test_entries_outside_the_run_bit_equal():
    sc.check_entries_outside_the_run_bit_equal(DEV)


def test_training_still_trains():
    sc.check_training_trains(DEV)
