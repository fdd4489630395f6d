"""GPU suite (-m gpu) of DreamHourglass's train_upsample_precision="fp16": the scaled-x weight gradient with its folding reduce, and the
forward and data-gradient launches as the switch uses them, through the C ABI on an MI355X, held to the bounds of
fp16_upsample_train_checks (derived per launch); then one decoder block, the whole step and twenty optimizer steps against the yardsticks
computed on the CPU reference."""
import pytest
import torch

import fp16_upsample_train_checks as uc
from dream_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
_ids = lambda s: "x".join(str(v) for v in s)      # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_library():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    _hip.check_symbols()
    with open("/proc/self/maps") as f:
        assert "libdream_hip.so" in f.read(), "the native HIP library is not loaded"
    yield


@pytest.mark.parametrize("scales", uc.SCALES, ids=("unit", "x2^-16", "x2^10"))
@pytest.mark.parametrize("shape", uc.SHAPES, ids=_ids)
def test_wgrad(shape, scales):
    _, split = uc.check_wgrad(DEV, shape, *scales)
    assert split == (2 if shape[1] == 5 else 1)          # one 8 x 16 position tile per frame / a single one


def test_zero_gradient_gives_exact_zeros():
    uc.check_wgrad(DEV, uc.SHAPES[1], zero_dz=True)
    uc.check_dgrad(DEV, uc.SHAPES[1], zero_dz=True)


def test_split_weight_gradient_repeats_bit_for_bit():
    uc.check_repeat(DEV)


def test_fold_is_the_adjoint_of_the_collapse():
    uc.check_fold(DEV)


@pytest.mark.parametrize("shape", uc.SHAPES, ids=_ids)
def test_forward(shape):
    uc.check_forward(DEV, shape)


@pytest.mark.parametrize("shape", uc.SHAPES + [uc.SPLIT_SHAPE], ids=_ids)
def test_dgrad(shape):
    uc.check_dgrad(DEV, shape)


@pytest.mark.parametrize("variant", range(uc.NUM_VARIANTS))
def test_dgrad_on_every_tile(variant):
    uc.check_dgrad(DEV, uc.VARIANT_SHAPE, variant=variant)


def test_refusals():
    uc.check_refusals(DEV)


def test_one_block():
    uc.check_block(DEV)


def test_whole_step():
    uc.check_step(DEV)


def test_uncovered_entries_are_bit_equal():
    uc.check_uncovered_entries_bit_equal(DEV)


@pytest.mark.parametrize("optimizer", ("adam", "sgd"))
def test_training_still_trains(optimizer):
    uc.check_training_trains(DEV, optimizer)


def test_default_step_is_untouched_by_a_visit_of_the_mode():
    uc.check_default_untouched(DEV)


def test_hip_graph_train_refuses_the_mode():
    net = uc.training_network(DEV, "fp16")
    net.model.module.train_precision = "fp32"             # (so that the refusal names this switch)
    with pytest.raises(ValueError, match="train_upsample_precision"):
        net.hip_graph_train = True
