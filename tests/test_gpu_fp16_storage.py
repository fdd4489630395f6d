"""GPU suite (-m gpu) of activation_storage="fp16": the half-storage kernels through the C ABI on an MI355X, held to the bounds of
fp16_storage_checks (derived per launch; measured on the CPU reference end to end)."""
import pytest
import torch

import cases
import fp16_storage_checks as sc
import parity_checks as pc
from dream_amd import _hip, ops
from oracle import models as om

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


@pytest.mark.parametrize("variant", list(range(NUM_VARIANTS)) + [-1])
def test_half_storage_launches(variant):
    lib = _hip.lib()
    lib.dream_conv_f16_set_variant(variant)
    try:
        sc.check_launches(DEV, seed=max(variant, 0), large=True)
    finally:
        lib.dream_conv_f16_set_variant(-1)


def test_half_storage_transposed4x4():
    sc.check_conv_transpose(DEV, 4, 1, 5, 6, 32, 48)
    sc.check_conv_transpose(DEV, 4, 2, 13, 13, 512, 256)


def test_saturation_is_finite_and_reported():
    sc.check_saturation(DEV)


def test_first_conv_maxpool_add():
    sc.check_first_conv(DEV)
    sc.check_maxpool(DEV)
    sc.check_add(DEV)


@pytest.mark.parametrize("case", ["vgg_q", "vgg_q_400", "vgg_f", "vgg_f_recipe"])
def test_structured_half_storage(case):
    sc.check_structured(DEV, case)


def test_skip_variant_half_storage():
    sc.check_golden(DEV, "vgg_f_skip", (1, 48, 64))


def _fp32_storage_peak(net, x):
    """max|value| over the tensors the precision="fp16" walk stores between its convs, from the amax scalars of its own launches."""
    seen, wrapped = [], ("conv3x3_first_amax", "conv2d_f16", "conv_transpose4x4s2_f16", "conv_transpose3x3s2_f16", "add")
    with pytest.MonkeyPatch.context() as mp:
        for name in wrapped:
            def spy(*a, _fn=getattr(ops, name), **k):
                out = _fn(*a, **k)
                seen.append(out[1])
                return out
            mp.setattr(ops, name, spy)
        with torch.no_grad():
            net.inference(x)
    return max(sc.fc._amax_value(a) for a in seen if a is not None)


def test_half_storage_peak_is_the_walks_maximum():
    x = torch.from_numpy(cases.structured_input("vgg_q")[0]).to(DEV)
    net = sc.structured_network(DEV, "vgg_q")
    with torch.no_grad():
        net.inference(x)
    peak = net.model.module.half_storage_peak()
    want = _fp32_storage_peak(sc.structured_network(DEV, "vgg_q", "fp32"), x)
    print("half_storage_peak %.6g, fp32-storage walk %.6g" % (peak, want))
    assert abs(peak - want) <= 1e-3 * want


def test_hip_graph_replays_the_half_storage_walk_bit_for_bit():
    net = sc.structured_network(DEV, "vgg_q")
    x = torch.from_numpy(cases.structured_input("vgg_q")[0]).to(DEV)
    with torch.no_grad():
        m0, k0 = net.inference(x)
        peak = net.model.module.half_storage_peak()
        net.hip_graph = True
        for _ in range(3):                                         # capture, then 2 replays
            m1, k1 = net.inference(x)
            assert torch.equal(m0, m1) and torch.equal(k0, k1)
            assert net.model.module.half_storage_peak() == peak
        m32 = sc.structured_network(DEV, "vgg_q", "fp32").inference(x)[0]
    assert not torch.equal(m32, m0)                                # (and the graph really held the half-storage launches)


def test_half_storage_peak_follows_the_replayed_graph():
    """Two input shapes, so two captured graphs: after both exist, a replay of the FIRST must leave the first forward's peak to read
    (one persistent scalar per module, zeroed in place -- not a tensor of whichever capture came last)."""
    net = sc.structured_network(DEV, "vgg_q")
    xa = torch.from_numpy(cases.structured_input("vgg_q")[0]).to(DEV)            # (2, 200, 200)
    xb = (xa[:1, :, :96, :128] * 3.0).contiguous()
    with torch.no_grad():
        peaks = []
        for x in (xa, xb):
            net.inference(x)
            peaks.append(net.model.module.half_storage_peak())
        assert peaks[0] != peaks[1]
        net.hip_graph = True
        for x, want in ((xa, peaks[0]), (xb, peaks[1]), (xa, peaks[0]), (xa, peaks[0]), (xb, peaks[1]), (xa, peaks[0])):
            net.inference(x)
            assert net.model.module.half_storage_peak() == want
    assert len(net._graphs) == 2


def test_half_storage_peak_covers_the_replicas():
    """gpu_ids = [0, 0]: the frames go to two replicas; the wrapper's half_storage_peak() is the maximum over both, whichever holds it."""
    from test_gpu_parity import _dp_network
    x = torch.from_numpy(cases.structured_input("vgg_q")[0]).to(DEV)
    weights, _ = sc.fc._structured_weights("vgg_q")
    for order in (x, x.flip(0).contiguous()):
        got = []
        for ids in ([0], [0, 0]):
            net = _dp_network("vgg_q", ids, in_res=(200, 200), weights=weights)
            net.enable_evaluation()
            net.model.module.precision = net.model.module.activation_storage = "fp16"
            with torch.no_grad():
                maps = net.inference(order)[0]
            got.append((maps, net.model.half_storage_peak(), net.model.module.half_storage_peak()))
        assert len(net.model._replicas) == 1 and torch.equal(got[0][0], got[1][0])
        assert got[1][1] == got[0][1] == got[0][2] and got[1][2] <= got[1][1]


def test_training_step_ignores_activation_storage():
    """precision="fp16" with activation_storage="fp16" are inference modes: a training step with both set is the fp32 step, bit for bit."""
    b, h, w = 2, 64, 96
    wts = om.recipe_weights(om.build_model("vgg_q", 7).state_dict(), cases.TRAIN_FINAL_KEYS, cases.TRAIN_FINAL_SCALE)
    x = torch.from_numpy(cases.image_batch(b, h, w, seed=7)).to(DEV)
    results = []
    for precision in ("fp32", "fp16"):
        net = pc.build_network("vgg_q", DEV, weights=wts, optimizer="adam", lr=cases.TRAIN_LR["adam"], in_res=(w, h))
        net.model.module.precision = net.model.module.activation_storage = precision
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
    net = sc.structured_network(DEV, "vgg_q")
    for precision in ("fp32", "fp16x3"):
        net.model.module.precision = precision
        with pytest.raises(ValueError, match="activation_storage.*precision"), torch.no_grad():
            net.inference(x)
    net.model.module.precision, net.model.module.activation_storage = "fp16", "half"
    with pytest.raises(ValueError, match="unknown activation_storage"), torch.no_grad():
        net.inference(x)
    for arch in ("vgg_ms2", "resnet_h"):
        other = pc.build_network(arch, DEV).model.module
        with pytest.raises(ValueError, match="activation_storage='fp16' is not supported"):
            other.activation_storage = "fp16"
