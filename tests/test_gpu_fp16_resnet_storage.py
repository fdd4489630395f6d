"""GPU suite (-m gpu) of ResnetSimple.inference_activation_storage="fp16": the residual form of conv_f16_kernel, the four streaming
kernels and the half-storage walk through the C ABI on an MI355X, held to the bounds of fp16_resnet_storage_checks (derived per
launch; measured on the CPU reference end to end)."""
import pytest
import torch

import cases
import fp16_resnet_step_checks as step
import fp16_resnet_storage_checks as rs
import parity_checks as pc
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


@pytest.mark.parametrize("variant", list(range(rs.NUM_VARIANTS)) + [-1])
def test_residual_form_launches(variant):
    lib = _hip.lib()
    lib.dream_conv_f16_set_variant(variant)
    try:
        rs.check_residual_launches(DEV, seed=max(variant, 0))
    finally:
        lib.dream_conv_f16_set_variant(-1)


def test_residual_saturation_is_finite_and_reported():
    rs.check_residual_saturation(DEV)


def test_residual_refusals():
    rs.check_residual_refusals(DEV)


def test_gathers_and_pool():
    rs.check_gathers_and_pool(DEV)


@pytest.mark.parametrize("variant", list(range(rs.NUM_VARIANTS)) + [-1])
def test_strided_convs_through_the_gather(variant):
    lib = _hip.lib()
    lib.dream_conv_f16_set_variant(variant)
    try:
        rs.check_strided_convs(DEV, seed=max(variant, 0))
    finally:
        lib.dream_conv_f16_set_variant(-1)


def test_one_bottleneck():
    rs.check_bottleneck(DEV)


@pytest.mark.parametrize("case", ["resnet_h", "resnet_f"])
def test_structured_half_storage(case):
    rs.check_structured(DEV, case)


def test_hip_graph_replays_the_half_storage_walk_bit_for_bit():
    net = rs.structured_network(DEV, "resnet_f")
    x = torch.from_numpy(cases.structured_input("resnet_f")[0]).to(DEV)
    with torch.no_grad():
        m0, k0 = net.inference(x)
        peak = net.model.module.half_storage_peak()
        net.hip_graph = True
        for _ in range(3):                                         # capture, then 2 replays
            m1, k1 = net.inference(x)
            assert torch.equal(m0, m1) and torch.equal(k0, k1)
            assert net.model.module.half_storage_peak() == peak
        # flipping the switch must not replay the graph of the other storage
        net.model.module.inference_activation_storage = "fp32"
        m32 = net.inference(x)[0]
        assert len(net._graphs) == 2
        assert torch.equal(m32, rs.structured_network(DEV, "resnet_f", "fp32").inference(x)[0])
    print("resnet_f max|maps(storage fp16) - maps(storage fp32)| %.3g" % float((m32 - m0).abs().max()))


def test_half_storage_peak_covers_the_replicas():
    """gpu_ids = [0, 0]: the frames go to two replicas; the maps are the single device's, the wrapper's half_storage_peak() is the
    maximum over both replicas."""
    from test_gpu_parity import _dp_network
    x = torch.from_numpy(cases.structured_input("resnet_h")[0]).to(DEV)
    weights, _ = rs.fc._structured_weights("resnet_h")
    got = []
    for ids in ([0], [0, 0]):
        net = _dp_network("resnet_h", ids, in_res=(400, 400), weights=weights)
        net.enable_evaluation()
        net.model.module.precision = net.model.module.inference_activation_storage = "fp16"
        with torch.no_grad():
            maps = net.inference(x)[0]
        got.append((maps, net.model.half_storage_peak(), net.model.module.half_storage_peak()))
    rep = net.model._replicas[0]
    assert len(net.model._replicas) == 1 and rep.inference_activation_storage == "fp16"
    assert torch.equal(got[0][0], got[1][0])
    assert got[1][1] == got[0][1] == got[0][2] == max(got[1][2], rep.half_storage_peak())


def test_training_step_ignores_the_switch():
    """precision="fp16" with inference_activation_storage="fp16" are inference modes: a training step with both set is the fp32 step,
    bit for bit."""
    results = []
    for precision in ("fp32", "fp16"):
        net = step.network(DEV, "fp32", precision)
        net.model.module.inference_activation_storage = precision
        ow, oh = net.trained_net_output_resolution()
        loss = float(net.train([pc.to(DEV, step.step_case())], pc.to(DEV, step._target((ow, oh)))).item())
        results.append((loss, [p.grad.detach().clone() for p in net.model.module.parameters()]))
    assert results[0][0] == results[1][0]
    for g32, g16 in zip(results[0][1], results[1][1]):
        assert torch.equal(g32, g16)


def test_value_errors():
    x = torch.from_numpy(cases.structured_input("resnet_f")[0]).to(DEV)
    net = rs.structured_network(DEV, "resnet_f")
    for precision in ("fp32", "fp16x3"):
        net.model.module.precision = precision
        with pytest.raises(ValueError, match="inference_activation_storage.*precision"), torch.no_grad():
            net.inference(x)
    net.model.module.precision, net.model.module.inference_activation_storage = "fp16", "half"
    with pytest.raises(ValueError, match="unknown inference_activation_storage"), torch.no_grad():
        net.inference(x)
    with pytest.raises(RuntimeError, match="no forward with inference_activation_storage"):
        net.model.module.half_storage_peak()
