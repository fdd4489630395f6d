"""GPU suite (-m gpu) of ResnetSimple's train_decoder_precision="fp16": the convT4 dgrad form, wgrad_convT4_f16_kernel and the kPlain
transposed forward through the C ABI on an MI355X, held to the bounds of fp16_resnet_decoder_checks (derived per launch), then one decoder
stage, the whole step and twenty optimizer steps -- the new switch alone and both training switches -- against the yardsticks computed on
the CPU reference."""
import pytest
import torch

import fp16_resnet_decoder_checks as dc
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


@pytest.mark.parametrize("shape", dc.SHAPES, ids=_ids)
def test_forward_and_statistics(shape):
    dc.check_forward(DEV, shape)


@pytest.mark.parametrize("shape", dc.SHAPES + [dc.SPLIT_SHAPE], ids=_ids)
def test_dgrad(shape):
    dc.check_dgrad(DEV, shape)


@pytest.mark.parametrize("variant", range(dc.NUM_VARIANTS))
def test_dgrad_on_every_tile(variant):
    dc.check_dgrad(DEV, dc.VARIANT_SHAPE, variant=variant)


@pytest.mark.parametrize("shape", dc.SHAPES, ids=_ids)
def test_wgrad(shape):
    _, split = dc.check_wgrad(DEV, shape)
    assert split == (2 if shape[1] == 5 else 1)


def test_zero_gradient_gives_exact_zeros():
    dc.check_dgrad(DEV, dc.SHAPES[1], zero_dz=True)
    dc.check_wgrad(DEV, dc.SHAPES[1], zero_dz=True)


def test_split_weight_gradient_repeats_bit_for_bit():
    dc.check_repeat(DEV)


def test_scales():
    dc.check_scales(DEV)


def test_batched_pack():
    dc.check_batched_pack(DEV)


def test_bias_gradient_of_the_covered_leaf():
    dc.check_bias_gradient(DEV)


def test_later_steps_repack_the_half_planes_in_one_batch():
    """From the second step on the half planes come from the batched pack: a step after an optimizer step equals the step of a network
    whose copies were packed one by one from the same parameters."""
    from dream_amd import data_parallel
    net = dc.network(DEV, "fp16", optimizer="sgd", lr=1e-2)
    ow, oh = net.trained_net_output_resolution()
    x, t = dc.sc.step_case().to(DEV), dc.sc._target((ow, oh)).to(DEV)
    net.train([x], t)
    module = net.model.module
    loss_batched = float(net.train([x], t).item())
    assert module._packs.view().half_table_built
    for group in net.optimizer.param_groups:
        group["lr"] = 0.0
    loss_a = float(net.train([x], t).item())
    data_parallel.reset_weight_caches(module)
    loss_b = float(net.train([x], t).item())
    assert loss_a == loss_b and loss_batched != loss_a


def test_refusals():
    dc.check_refusals(DEV)


def test_one_stage():
    dc.check_stage(DEV)


def test_small_map_stage_stays_fp32():
    dc.check_small_map_stays_fp32(DEV)


@pytest.mark.parametrize("both", (False, True), ids=("decoder", "decoder+gemm"))
def test_whole_step(both):
    dc.check_step(DEV, both)


@pytest.mark.parametrize("both", (False, True), ids=("decoder", "decoder+gemm"))
@pytest.mark.parametrize("optimizer", ("adam", "sgd"))
def test_training_still_trains(optimizer, both):
    dc.check_training_trains(DEV, optimizer, both)


def test_default_step_is_untouched_by_a_visit_of_the_mode():
    """fp32 -> fp16 -> fp32 on one network with lr = 0: the two fp32 steps give the same bits."""
    net = dc.network(DEV, "fp32")
    ow, oh = net.trained_net_output_resolution()
    x, t = dc.sc.step_case().to(DEV), dc.sc._target((ow, oh)).to(DEV)
    grads = lambda: [p.grad.detach().clone() for p in net.model.module.parameters()]      # noqa: E731
    l0 = float(net.train([x], t).item())
    g0 = grads()
    net.model.module.train_decoder_precision = "fp16"
    l1 = float(net.train([x], t).item())
    net.model.module.train_decoder_precision = "fp32"
    l2 = float(net.train([x], t).item())
    assert l0 == l2 and l1 != l0 and all(torch.equal(a, b) for a, b in zip(g0, grads()))


def test_hip_graph_train_refuses_the_mode():
    net = dc.network(DEV, "fp16")
    with pytest.raises(ValueError, match="train_decoder_precision"):
        net.hip_graph_train = True
