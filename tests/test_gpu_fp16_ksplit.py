"""GPU suite (-m gpu) of conv_ksplit="auto": the split kernel and its finishing pass through the C ABI on an MI355X, held to the bounds
of fp16_ksplit_checks (derived per launch; the half-storage oracle, measured on the CPU reference, end to end)."""
import pytest
import torch

import cases
import fp16_ksplit_checks as kc
import parity_checks as pc
from dream_amd import _hip, ops
from oracle import models as om

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_library():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    _hip.check_symbols()
    with open("/proc/self/maps") as f:
        assert "libdream_hip.so" in f.read(), "the native HIP library is not loaded"
    yield


@pytest.mark.parametrize("ksize", [1, 3])
@pytest.mark.parametrize("case", kc.LAUNCH_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_split_launches(case, ksize):
    kc.check_case(DEV, case, ksize)


@pytest.mark.parametrize("variant", [0, 1, 3])
def test_split_launches_on_the_tiles_of_the_deep_layers(variant):
    """The tiles the rule picks from 128 output channels on (128 x 128, 64 x 128; 256 x 64 for the deep launches), forced; more than
    one workgroup in every grid dimension."""
    lib = _hip.lib()
    lib.dream_conv_f16_set_variant(variant)
    try:
        for S in (2, 5, 16):
            kc.check_conv(DEV, 2, 25, 27, 128, 256, 3, S, seed=variant)
    finally:
        lib.dream_conv_f16_set_variant(-1)


@pytest.mark.parametrize("variant", range(8))
def test_split_launches_on_every_tile(variant):
    kc.check_tile(DEV, variant)


@pytest.mark.parametrize("ksize", [1, 3])
@pytest.mark.parametrize("case", kc.LAUNCH_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_saturation_is_finite_and_reported(case, ksize):
    kc.check_saturation(DEV, case, ksize)


@pytest.mark.parametrize("case", kc.LAUNCH_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_refused_flags(case):
    kc.check_refused_flags(DEV, case)


@pytest.mark.parametrize("case,ksize", [(kc.LAUNCH_CASES[2], 1), (kc.LAUNCH_CASES[2], 3), (kc.LAUNCH_CASES[0], 1), (kc.LAUNCH_CASES[3], 3)],
                         ids=lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v))
def test_slices_past_the_stages_are_zero(case, ksize):
    """2 x 13 x 13 x 32 -> 34 with ksize 1 is one stage: three slices asked of the entry point leave two empty."""
    kc.check_empty_slices(DEV, case, ksize)


@pytest.mark.parametrize("case", ["vgg_q", "vgg_q_400"])
def test_structured_split(case):
    kc.check_structured(DEV, case)


def test_hip_graph_replays_the_split_walk_bit_for_bit():
    """Two input shapes, so two captured graphs; either one replayed equals its eager walk, maps, keypoints and peak."""
    net = kc.ksplit_network(DEV, "vgg_q")
    xa = torch.from_numpy(cases.structured_input("vgg_q")[0]).to(DEV)            # (2, 200, 200)
    xb = (xa[:1, :, :96, :128] * 3.0).contiguous()
    with torch.no_grad():
        eager = []
        for x in (xa, xb):
            with kc.launch_names() as names:
                m, k = net.inference(x)
            assert names.count(kc.SPLIT_ENTRY) >= 1
            eager.append((m, k, net.model.module.half_storage_peak()))
        net.hip_graph = True
        for i in (0, 1, 0, 0, 1, 0):                                             # capture a, capture b, then replays of either
            m, k = net.inference((xa, xb)[i])
            assert torch.equal(m, eager[i][0]) and torch.equal(k, eager[i][1])
            assert net.model.module.half_storage_peak() == eager[i][2]
        assert len(net._graphs) == 2
        net.model.module.conv_ksplit = "off"                                     # the switch is part of the cache key: a third graph
        m_off, _ = net.inference(xa)
        assert len(net._graphs) == 3
        m_ref = kc.ksplit_network(DEV, "vgg_q", "off").inference(xa)[0]
    assert torch.equal(m_off, m_ref)


def test_off_is_the_parents_launch_list_and_bits():
    """conv_ksplit="off" reaches no split entry point, and a walk in which the rule splits nothing is the unsplit walk bit for bit."""
    x = torch.from_numpy(cases.structured_input("vgg_q")[0]).to(DEV)
    with torch.no_grad():
        with kc.launch_names() as off_names:
            m_off = kc.ksplit_network(DEV, "vgg_q", "off").inference(x)[0]
        with kc.forced_ksplit(1), kc.launch_names() as one_names:
            m_one = kc.ksplit_network(DEV, "vgg_q").inference(x)[0]
    assert kc.SPLIT_ENTRY not in off_names and one_names == off_names
    assert torch.equal(m_one, m_off)


def test_replicas_follow_the_switch():
    """gpu_ids = [0, 0]: the replica takes the switch from the master; the frames of both give the maps of one device."""
    from test_gpu_parity import _dp_network
    x = torch.from_numpy(cases.structured_input("vgg_q")[0]).to(DEV)
    weights, _ = kc.fc._structured_weights("vgg_q")
    net = _dp_network("vgg_q", [0, 0], in_res=(200, 200), weights=weights)
    net.enable_evaluation()
    net.model.module.precision = net.model.module.activation_storage = "fp16"
    net.model.module.conv_ksplit = "auto"
    with torch.no_grad():
        got = net.inference(x)[0]
    assert len(net.model._replicas) == 1 and net.model._replicas[0].conv_ksplit == "auto"
    with torch.no_grad():
        ref = torch.cat([kc.ksplit_network(DEV, "vgg_q").inference(x[i:i + 1])[0] for i in range(2)])
    assert torch.equal(got, ref)                                                # (one frame each: the rule sees b = 1)


def test_training_step_ignores_conv_ksplit():
    """A training step with the three inference switches set is the fp32 step, bit for bit."""
    b, h, w = 2, 64, 96
    wts = om.recipe_weights(om.build_model("vgg_q", 7).state_dict(), cases.TRAIN_FINAL_KEYS, cases.TRAIN_FINAL_SCALE)
    x = torch.from_numpy(cases.image_batch(b, h, w, seed=7)).to(DEV)
    results = []
    for precision, ksplit in (("fp32", "off"), ("fp16", "auto")):
        net = pc.build_network("vgg_q", DEV, weights=wts, optimizer="adam", lr=cases.TRAIN_LR["adam"], in_res=(w, h))
        net.model.module.precision = net.model.module.activation_storage = precision
        net.model.module.conv_ksplit = ksplit
        net.enable_training()
        ow, oh = net.trained_net_output_resolution()
        t = torch.from_numpy(cases.target_batch(b, 7, (ow, oh), in_wh=(w, h), seed=7)).to(DEV)
        loss = net.train([x], t).item()
        results.append((loss, [p.detach().clone() for p in net.model.parameters()]))
    assert results[0][0] == results[1][0]
    for p32, p16 in zip(results[0][1], results[1][1]):
        assert torch.equal(p32, p16)


def test_value_errors():
    x = torch.from_numpy(cases.structured_input("vgg_q")[0]).to(DEV)
    net = kc.ksplit_network(DEV, "vgg_q")
    for precision, storage in (("fp32", "fp32"), ("fp16", "fp32")):
        net.model.module.precision, net.model.module.activation_storage = precision, storage
        with pytest.raises(ValueError, match="conv_ksplit.*precision.*activation_storage"), torch.no_grad():
            net.inference(x)
    net.model.module.precision = net.model.module.activation_storage = "fp16"
    net.model.module.conv_ksplit = "on"
    with pytest.raises(ValueError, match="unknown conv_ksplit"), torch.no_grad():
        net.inference(x)
    for arch in ("vgg_ms2", "resnet_h"):
        other = pc.build_network(arch, DEV).model.module
        with pytest.raises(ValueError, match="conv_ksplit='auto' is not supported"):
            other.conv_ksplit = "auto"
