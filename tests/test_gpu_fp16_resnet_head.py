"""GPU suite (-m gpu) of ResnetSimple.inference_head_fusion="on": the fused last stage + head entry, the walk, its memory, its hipGraph
and its replicas through the C ABI on an MI355X.  What is compared bit for bit and the bounds: fp16_resnet_head_checks."""
import pytest
import torch

import fp16_resnet_head_checks as rh
import fp16_resnet_step_checks as step
import fp16_resnet_storage_checks as rs
import parity_checks as pc
from dream_amd import _hip, models

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_library():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    _hip.check_symbols()
    with open("/proc/self/maps") as f:
        assert "libdream_hip.so" in f.read(), "the native HIP library is not loaded"
    yield


# ---- per launch -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("case", rh.LAUNCH_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_fused_launch_is_the_two_launches_bit_for_bit(case, relu):
    rh.check_launch(DEV, *case, relu=relu, seed=case[1])


def test_fused_launch_on_the_decoder_shape():
    """The shape the walk runs it on (resnet_h, one 400 x 400 frame): 104 x 104 x 256 -> 7 maps of 208 x 208, 85 tiles a phase."""
    rh.check_launch(DEV, 1, 104, 104, 256, 7, seed=9, w_scale=0.1)


def test_saturation_is_finite_and_reported():
    rh.check_saturation(DEV)


def test_refusals():
    rh.check_refusals(DEV)


def test_symbols_resolve():
    lib = _hip.lib()
    assert lib.dream_conv_transpose4x4s2_head_f16_applies(256, 256, 17) == 1 and lib.dream_conv_transpose4x4s2_head_f16_applies(256, 256, 33) == 0
    assert rh.FUSED in _hip.check_symbols()


# ---- the walk -------------------------------------------------------------------------------------------------------------------------
def test_decoder_walk_on_is_off_bit_for_bit():
    rh.check_decoder_walk(DEV, 17, True, hw=(3, 2))


@pytest.mark.parametrize("case", ["resnet_f", "resnet_h"])
def test_walk_on_is_off_bit_for_bit(case):
    names = rh.check_walk_identity(DEV, case)
    assert names.count(rh.FUSED) == 1


@pytest.mark.parametrize("case", ["resnet_f", "resnet_h"])
def test_structured_fused_walk(case):
    rh.check_structured(DEV, case)


@pytest.mark.parametrize("case", ["resnet_f", "resnet_h"])
def test_walk_with_ksplit_at_one_frame(case):
    """inference_conv_ksplit="auto" at one frame: equal again, whichever branch the rule picks for the last stage (the trace says which);
    with two slices forced the fusion yields and the walk is the split walk."""
    rh.check_walk_identity(DEV, case, ksplit="auto", frames=1)
    with rh.forced_ksplit(2):
        names = rh.check_walk_identity(DEV, case, ksplit="auto", frames=1)
    assert rh.FUSED not in names and rh.SPLIT_STAGE in names


def test_33_keypoints_fall_back_to_the_unfused_launches():
    rh.check_fallback(DEV)


def test_the_last_stage_output_is_never_allocated():
    """resnet_f at its structured input, after a warm-up call (so that the packed weights exist): T = the bytes of the last stage's half
    output.  "off" allocates it: the call's transient peak is >= T by construction.  "on" must stay below T: from tensor sizes the
    next-largest transient is about 0.3 T (fourth stage in + out; the stem's im2col + output)."""
    x = rh.structured_x(DEV, "resnet_f")
    peaks = {}
    for fusion in ("off", "on"):
        net = rh.head_network(DEV, "resnet_f", fusion)
        with torch.no_grad():
            maps = net.inference(x)[0]
            torch.cuda.synchronize()
            del maps
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            maps = net.inference(x)[0]
            torch.cuda.synchronize()
            peaks[fusion] = torch.cuda.max_memory_allocated() - base
        b, _, ho, wo = (int(v) for v in maps.shape)
        del net, maps
    T = b * ho * wo * rh.CMID * 2
    print("resnet_f %s: last stage output T = %d bytes; transient peak of one inference() call: off %d (%.2f T), on %d (%.2f T)"
          % (tuple(x.shape), T, peaks["off"], peaks["off"] / T, peaks["on"], peaks["on"] / T))
    assert peaks["off"] >= T
    assert peaks["on"] < T


def test_hip_graph_replays_the_fused_walk_bit_for_bit():
    net = rh.head_network(DEV, "resnet_f", "on")
    x = rh.structured_x(DEV, "resnet_f")
    with torch.no_grad():
        m0, k0, peak, names = rh.run_walk(net, x)
        assert names.count(rh.FUSED) == 1
        net.hip_graph = True
        for _ in range(3):                                         # capture, then 2 replays
            m1, k1 = net.inference(x)
            assert torch.equal(m0, m1) and torch.equal(k0, k1)
            assert net.model.module.half_storage_peak() == peak
        # flipping the switch must not replay the graph of the fused walk
        net.model.module.inference_head_fusion = "off"
        m_off = net.inference(x)[0]
        assert len(net._graphs) == 2
        assert torch.equal(m_off, m0)


def test_fused_walk_on_two_replicas():
    """gpu_ids = [0, 0]: the replica takes the switch from the master; each gives the maps gpu_ids = [0] gives for the frame it saw."""
    from test_gpu_parity import _dp_network
    x = rh.structured_x(DEV, "resnet_h")
    assert int(x.shape[0]) == 2
    weights, _ = rs.fc._structured_weights("resnet_h")
    nets = {}
    for ids in ([0], [0, 0]):
        net = nets[len(ids)] = _dp_network("resnet_h", ids, in_res=(400, 400), weights=weights)
        net.enable_evaluation()
        net.model.module.precision = net.model.module.inference_activation_storage = "fp16"
        net.model.module.inference_head_fusion = "on"
    one, two = nets[1], nets[2]
    with torch.no_grad():
        with rh.kc.launch_names() as names:
            got = two.inference(x)[0]
        peak = two.model.half_storage_peak()
        rep = two.model._replicas[0]
        assert len(two.model._replicas) == 1 and rep.inference_head_fusion == "on"
        ref, ref_peaks = [], []
        for i in range(2):
            ref.append(one.inference(x[i:i + 1])[0])
            ref_peaks.append(one.model.half_storage_peak())
    assert names.count(rh.FUSED) == 2
    assert torch.equal(got, torch.cat(ref)) and peak == max(ref_peaks)


def test_training_step_ignores_the_switch():
    """A training step with precision="fp16", half storage and the fused head set is the fp32 step, bit for bit."""
    results = []
    for precision in ("fp32", "fp16"):
        net = step.network(DEV, "fp32", precision)
        net.model.module.inference_activation_storage = precision
        net.model.module.inference_head_fusion = "on" if precision == "fp16" else "off"
        ow, oh = net.trained_net_output_resolution()
        loss = float(net.train([pc.to(DEV, step.step_case())], pc.to(DEV, step._target((ow, oh)))).item())
        results.append((loss, [p.grad.detach().clone() for p in net.model.module.parameters()]))
    assert results[0][0] == results[1][0]
    for g32, g16 in zip(results[0][1], results[1][1]):
        assert torch.equal(g32, g16)


def test_value_errors():
    x = rh.structured_x(DEV, "resnet_f")
    net = rh.head_network(DEV, "resnet_f", "on")
    for precision, storage in (("fp32", "fp32"), ("fp16", "fp32")):
        net.model.module.precision, net.model.module.inference_activation_storage = precision, storage
        with pytest.raises(ValueError, match="inference_head_fusion.*precision.*inference_activation_storage"), torch.no_grad():
            net.inference(x)
    net.model.module.precision = net.model.module.inference_activation_storage = "fp16"
    net.model.module.inference_head_fusion = "auto"
    with pytest.raises(ValueError, match="unknown inference_head_fusion"), torch.no_grad():
        net.inference(x)
    with pytest.raises(ValueError, match="inference_head_fusion='on' is not supported"):
        models.DreamHourglass(7).inference_head_fusion = "on"
