"""GPU suite (-m gpu) of precision="fp16": the real conv_f16 kernels through the C ABI on an MI355X, held to the bounds of
fp16_checks (derived per launch; measured on the CPU reference end to end)."""
import pytest
import torch

import cases
import fp16_checks as fc
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
def test_conv_f16_variants(variant):
    lib = _hip.lib()
    lib.dream_conv_f16_set_variant(variant)
    try:
        s = max(variant, 0)
        fc.check_conv_f16(DEV, 1, 7, 9, 32, 40, 3, ops.CONV_RELU, seed=s)
        fc.check_conv_f16(DEV, 2, 12, 20, 64, 7, 3, ops.CONV_OUT_NCHW, x_scale=300.0, w_scale=1e-3, seed=s)
        fc.check_conv_f16(DEV, 1, 6, 8, 32, 64, 3, ops.CONV_RELU | ops.CONV_UPSAMPLE2X, x_scale=1e-3, w_scale=5.0, seed=s)
        fc.check_conv_f16(DEV, 2, 9, 11, 64, 48, 1, 0, seed=s)
        fc.check_conv_f16(DEV, 2, 12, 20, 32, 48, 3, ops.CONV_RELU | ops.CONV_POOL2, seed=s)
        fc.check_conv_f16(DEV, 1, 13, 9, 64, 32, 3, ops.CONV_RELU | ops.CONV_POOL2, seed=s)
        fc.check_conv_transpose4x4_f16(DEV, 1, 5, 6, 32, 48, seed=s)
        fc.check_conv_transpose3x3_f16(DEV, 1, 5, 7, 32, 48, seed=s)
        fc.check_conv_f16(DEV, 2, 33, 47, 64, 96, 3, ops.CONV_RELU, seed=s)          # several tiles, ragged edges
        fc.check_conv_f16(DEV, 2, 25, 25, 512, 128, 1, 0, seed=s)                    # 16 channel chunks of one tap
    finally:
        lib.dream_conv_f16_set_variant(-1)


def test_conv_transpose4x4_f16_deep_and_wide():
    fc.check_conv_transpose4x4_f16(DEV, 2, 13, 13, 2048, 256)      # the deepest accumulation: 4 taps x 2048 channels
    fc.check_conv_transpose4x4_f16(DEV, 1, 52, 52, 256, 256)


@pytest.mark.parametrize("case", sorted(cases.STRUCTURED_CASES))
def test_structured_fp16(case):
    fc.check_structured_f16(DEV, case)


def test_hip_graph_replays_the_fp16_walk_bit_for_bit():
    net = fc.structured_network(DEV, "vgg_q")                      # (2, 200, 200)
    x = torch.from_numpy(cases.structured_input("vgg_q")[0]).to(DEV)
    with torch.no_grad():
        m0, k0 = net.inference(x)
        net.hip_graph = True
        for _ in range(2):                                         # capture, then replay
            m1, k1 = net.inference(x)
            assert torch.equal(m0, m1) and torch.equal(k0, k1)
    net32 = fc.structured_network(DEV, "vgg_q", precision="fp32")
    with torch.no_grad():
        assert not torch.equal(net32.inference(x)[0], m0)          # (and the graph really held the fp16 launches)


def test_training_step_ignores_fp16():
    """precision="fp16" is an inference mode: a training step with it set is the fp32 step, bit for bit."""
    b, h, w = 2, 64, 96
    wts = om.recipe_weights(om.build_model("vgg_q", 7).state_dict(), cases.TRAIN_FINAL_KEYS, cases.TRAIN_FINAL_SCALE)
    x = torch.from_numpy(cases.image_batch(b, h, w, seed=7)).to(DEV)
    results = []
    for precision in ("fp32", "fp16"):
        net = pc.build_network("vgg_q", DEV, weights=wts, optimizer="adam", lr=cases.TRAIN_LR["adam"], in_res=(w, h))
        net.model.module.precision = precision
        net.enable_training()
        ow, oh = net.trained_net_output_resolution()
        t = torch.from_numpy(cases.target_batch(b, 7, (ow, oh), in_wh=(w, h), seed=7)).to(DEV)
        loss = net.train([x], t).item()
        results.append((loss, [p.detach().clone() for p in net.model.parameters()]))
    assert results[0][0] == results[1][0]
    for p32, p16 in zip(results[0][1], results[1][1]):
        assert torch.equal(p32, p16)
