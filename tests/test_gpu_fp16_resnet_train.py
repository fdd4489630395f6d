"""GPU suite (-m gpu) of ResnetSimple's train_gemm_precision="fp16": the real gemm1x1_f16 / wgrad1x1_f16 kernels and the amax form of
bn_bwd_apply through the C ABI on an MI355X, held to the bounds of fp16_resnet_train_checks (derived per launch), then one Bottleneck at
a time, the whole step and twenty optimizer steps against the yardsticks of fp16_resnet_step_checks (computed on the CPU reference)."""
import pytest
import torch

import fp16_resnet_step_checks as sc
import fp16_resnet_train_checks as rc
from dream_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_library():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    _hip.check_symbols()
    with open("/proc/self/maps") as f:
        assert "libdream_hip.so" in f.read(), "the native HIP library is not loaded"
    yield


@pytest.mark.parametrize("ks", (0, 1, 2, 4))
@pytest.mark.parametrize("form", rc.GEMM_FORMS)
@pytest.mark.parametrize("shape", rc.GEMM_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_gemm_f16(shape, form, ks):
    if ks and shape[1] % (32 * ks):        # K = 64 four ways: the fp32 entry points' contract (K % (32 ks)), refused before the launch
        with pytest.raises(RuntimeError, match="cannot be split"):
            rc.check_gemm(DEV, shape, form, ks)
    else:
        rc.check_gemm(DEV, shape, form, ks)


def test_gemm_f16_padded_rows():
    rc.check_gemm(DEV, (70, 64, 64), "plain_grad", 0, stride_pad=4)
    rc.check_gemm(DEV, (70, 64, 64), "res", 2, stride_pad=4)


def test_gemm_f16_repeats_bit_for_bit():
    rc.check_gemm_repeat(DEV)


@pytest.mark.parametrize("shape", rc.WGRAD_SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_wgrad_f16(shape):
    split = rc.check_wgrad(DEV, shape)
    assert (split > 1) == (shape[0] == 4112)


def test_scales():
    rc.check_scales(DEV)


def test_bn_bwd_apply_amax():
    rc.check_bn_bwd_apply_amax(DEV)


def test_batched_pack():
    rc.check_batched_pack(DEV)


def test_refusals():
    rc.check_refusals(DEV)


def test_later_steps_repack_in_one_batch():
    """From the second step on the half copies come from the batched pack: the gradients of a step after an optimizer step are those of
    a network whose copies were packed one by one from the same parameters."""
    import fp16_resnet_step_checks as sc2
    from dream_amd import data_parallel
    net = sc2.network(DEV, "fp16", optimizer="sgd", lr=1e-2)
    ow, oh = net.trained_net_output_resolution()
    x, t = sc2.step_case().to(DEV), sc2._target((ow, oh)).to(DEV)
    net.train([x], t)
    module = net.model.module
    loss_batched = float(net.train([x], t).item())
    assert module._packs.view().half_table_built
    g_batched = {n: p.grad.detach().clone() for n, p in module.named_parameters()}
    # the same parameters, every copy packed lazily one by one: a step with lr = 0 from here
    for group in net.optimizer.param_groups:
        group["lr"] = 0.0
    loss_a = float(net.train([x], t).item())
    data_parallel.reset_weight_caches(module)
    loss_b = float(net.train([x], t).item())
    assert loss_a == loss_b
    assert loss_batched != loss_a and all(bool(torch.isfinite(g).all()) for g in g_batched.values())


@pytest.mark.parametrize("block", sc.BLOCKS)
def test_one_bottleneck(block):
    sc.check_block(DEV, block)


def test_whole_step():
    sc.check_step(DEV)


@pytest.mark.parametrize("optimizer", ("adam", "sgd"))
def test_training_still_trains(optimizer):
    sc.check_training_trains(DEV, optimizer)


def test_hip_graph_train_refuses_the_mode():
    net = sc.network(DEV, "fp16")
    with pytest.raises(ValueError, match="train_gemm_precision"):
        net.hip_graph_train = True
