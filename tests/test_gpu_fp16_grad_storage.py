"""GPU suite (-m gpu) of train_gradient_storage="fp16": the three half-gradient forms of the data-gradient conv, the half-dy weight
gradient and the all-half max-pool backward through the C ABI on an MI355X, and a vgg_q training step on them, held to the bounds of
fp16_grad_storage_checks (bit equality per launch; measured on the CPU reference end to end)."""
import pytest
import torch

import fp16_grad_storage_checks as gc
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


@pytest.mark.parametrize("shape", gc.WGRAD_CASES, ids=lambda s: "x".join(str(v) for v in s[:5]))
def test_wgrad_half_dy(shape):
    gc.check_wgrad_dy16(DEV, *shape)


def test_wgrad_half_dy_zero_repeat_and_flags():
    gc.check_wgrad_dy16_zero_repeat_and_flags(DEV)


@pytest.mark.parametrize("variant", list(range(NUM_VARIANTS)) + [-1])
def test_dgrad_forms_variants(variant):
    lib = _hip.lib()
    lib.dream_conv_f16_set_variant(variant)
    try:
        gc.check_dgrad_shapes(DEV, seed=max(variant, 0))
    finally:
        lib.dream_conv_f16_set_variant(-1)


def test_dgrad_refusals():
    gc.check_dgrad_refusals(DEV)


def test_maxpool_backward_all_half():
    gc.check_pool_bwd_dy16(DEV)


def test_training_step_half_gradients():
    gc.check_training_step(DEV)


def test_training_still_trains():
    gc.check_training_trains(DEV)
