"""GPU suite (-m gpu) of train_precision="fp16": the real wgrad_f16 / conv_f16 kernels through the C ABI on an MI355X and a vgg_q
training step on them, held to the bounds of fp16_train_checks (derived per launch; measured on the CPU reference end to end)."""
import pytest
import torch

import fp16_train_checks as tc
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


@pytest.mark.parametrize("shape", tc.WGRAD_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:5]))
def test_wgrad_f16(shape):
    tc.check_wgrad_f16(DEV, *shape)


def test_wgrad_f16_splitk():
    tc.check_wgrad_f16_splitk(DEV)


def test_wgrad_f16_zero_repeat_and_flags():
    tc.check_wgrad_f16_zero_and_repeat(DEV)


@pytest.mark.parametrize("variant", list(range(NUM_VARIANTS)) + [-1])
def test_masked_dgrad_f16_variants(variant):
    lib = _hip.lib()
    lib.dream_conv_f16_set_variant(variant)
    try:
        tc.check_dgrad_f16_shapes(DEV, seed=max(variant, 0))
    finally:
        lib.dream_conv_f16_set_variant(-1)


def test_training_step_fp16():
    tc.check_training_step(DEV)


def test_non_plain_entries_bit_equal():
    tc.check_non_plain_entries_bit_equal(DEV)


def test_rejections():
    tc.check_rejections(DEV)


def test_hip_graph_train_refuses_fp16():
    net = tc.training_network(DEV, "fp16")
    with pytest.raises(ValueError, match="train_precision"):
        net.hip_graph_train = True
    net.model.module.train_precision = "fp32"
    net.hip_graph_train = True
    net.model.module.train_precision = "fp16"
    x = tc.training_case()[1].to(DEV)
    t, _ = tc._target(net, DEV)
    with pytest.raises(ValueError, match="train_precision"):
        net.train([x], t)
    net.hip_graph_train = False


def test_training_still_trains():
    tc.check_training_trains(DEV)
