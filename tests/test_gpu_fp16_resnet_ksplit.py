"""GPU suite (-m gpu) of ResnetSimple.inference_conv_ksplit="auto": the split 4x4 transposed conv and its finishing pass, the split walk,
its hipGraph and its replicas through the C ABI on an MI355X, held to the bounds of fp16_resnet_ksplit_checks (derived per launch;
measured on the CPU reference end to end)."""
import pytest
import torch

import cases
import fp16_resnet_ksplit_checks as rk
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


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("case", rk.CONVT_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_split_transposed_launches(case, relu):
    rk.check_convT_case(DEV, case, relu)


@pytest.mark.parametrize("variant", range(8))
def test_split_transposed_launches_on_every_tile(variant):
    rk.check_convT_tile(DEV, variant)


def test_saturation_is_finite_and_reported():
    rk.check_convT_saturation(DEV)


def test_refusals():
    rk.check_convT_refusals(DEV)


def test_one_bottleneck():
    rk.check_bottleneck(DEV)


def test_one_decoder_stage():
    rk.check_stage(DEV)


@pytest.mark.parametrize("case", ["resnet_h", "resnet_f"])
def test_structured_split_walk(case):
    rk.check_structured(DEV, case)


def test_hip_graph_replays_the_split_walk_bit_for_bit():
    net = rk.ksplit_network(DEV, "resnet_f")
    x = torch.from_numpy(cases.structured_input("resnet_f")[0]).to(DEV)
    with torch.no_grad():
        with rk.kc.launch_names() as names:
            m0, k0 = net.inference(x)
        assert sum(names.count(e) for e in rk.SPLIT_ENTRIES) >= 1
        peak = net.model.module.half_storage_peak()
        net.hip_graph = True
        for _ in range(3):                                         # capture, then 2 replays
            m1, k1 = net.inference(x)
            assert torch.equal(m0, m1) and torch.equal(k0, k1)
            assert net.model.module.half_storage_peak() == peak
        # flipping the switch must not replay the graph of the split walk
        net.model.module.inference_conv_ksplit = "off"
        m_off = net.inference(x)[0]
        assert len(net._graphs) == 2
        assert torch.equal(m_off, rk.ksplit_network(DEV, "resnet_f", "off").inference(x)[0])
    print("resnet_f max|maps(auto) - maps(off)| %.3g" % float((m_off - m0).abs().max()))


def test_split_walk_on_two_replicas():
    """gpu_ids = [0, 0]: the frames go to two replicas, which take the switch from the master; each gives the maps gpu_ids = [0] gives for
    the frames it saw (one frame each: the rule sees b = 1, as on one device asked for one frame), bit for bit; the wrapper's
    half_storage_peak() is the maximum over both replicas."""
    from test_gpu_parity import _dp_network
    x = torch.from_numpy(cases.structured_input("resnet_h")[0]).to(DEV)
    assert int(x.shape[0]) == 2
    weights, _ = rs.fc._structured_weights("resnet_h")
    nets = {}
    for ids in ([0], [0, 0]):
        net = nets[len(ids)] = _dp_network("resnet_h", ids, in_res=(400, 400), weights=weights)
        net.enable_evaluation()
        net.model.module.precision = net.model.module.inference_activation_storage = "fp16"
        net.model.module.inference_conv_ksplit = "auto"
    one, two = nets[1], nets[2]
    with torch.no_grad():
        with rk.kc.launch_names() as names:
            got = two.inference(x)[0]
        peak = two.model.half_storage_peak()
        rep = two.model._replicas[0]
        assert len(two.model._replicas) == 1 and rep.inference_conv_ksplit == "auto"
        assert peak == max(two.model.module.half_storage_peak(), rep.half_storage_peak())
        ref, ref_peaks = [], []
        for i in range(2):
            ref.append(one.inference(x[i:i + 1])[0])
            ref_peaks.append(one.model.half_storage_peak())
    assert sum(names.count(e) for e in rk.SPLIT_ENTRIES) >= 2
    assert torch.equal(got, torch.cat(ref))
    assert peak == max(ref_peaks)


def test_training_step_ignores_the_three_switches():
    """precision="fp16", inference_activation_storage="fp16" and inference_conv_ksplit="auto" are inference modes: a training step with
    all three set is the fp32 step, bit for bit."""
    results = []
    for precision in ("fp32", "fp16"):
        net = step.network(DEV, "fp32", precision)
        net.model.module.inference_activation_storage = precision
        net.model.module.inference_conv_ksplit = "auto" if precision == "fp16" else "off"
        ow, oh = net.trained_net_output_resolution()
        loss = float(net.train([pc.to(DEV, step.step_case())], pc.to(DEV, step._target((ow, oh)))).item())
        results.append((loss, [p.grad.detach().clone() for p in net.model.module.parameters()]))
    assert results[0][0] == results[1][0]
    for g32, g16 in zip(results[0][1], results[1][1]):
        assert torch.equal(g32, g16)


def test_value_errors():
    x = torch.from_numpy(cases.structured_input("resnet_f")[0]).to(DEV)
    net = rk.ksplit_network(DEV, "resnet_f")
    for precision, storage in (("fp32", "fp32"), ("fp16", "fp32")):
        net.model.module.precision, net.model.module.inference_activation_storage = precision, storage
        with pytest.raises(ValueError, match="inference_conv_ksplit.*precision.*inference_activation_storage"), torch.no_grad():
            net.inference(x)
    net.model.module.precision = net.model.module.inference_activation_storage = "fp16"
    net.model.module.inference_conv_ksplit = "on"
    with pytest.raises(ValueError, match="unknown inference_conv_ksplit"), torch.no_grad():
        net.inference(x)
    with pytest.raises(ValueError, match="conv_ksplit='auto' is not supported"):
        net.model.module.conv_ksplit = "auto"
