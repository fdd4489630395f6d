"""CPU suite of train_gradient_storage="fp16": the GRAD16 forms of csrc/conv_f16.hip, the half-dy kernel of csrc/wgrad_f16.hip and the
all-half max-pool backward of csrc/elementwise.hip compiled unchanged against the SIMT emulator, through dream_amd.ops / models; the
launch list of such a training step and the host's refusals without any kernel (meta device); the sanity of the reference the
end-to-end bound is measured on.  Bounds: see fp16_grad_storage_checks."""
import collections
import os
import warnings

import pytest
import torch

import fp16_grad_storage_checks as gc
import fp16_train_checks as tc
import launch_trace as lt
from dream_amd import data_parallel, models, ops
from emu_util import emulated_hip

NUM_VARIANTS = 8
_FULL = os.environ.get("DREAM_EMU_FULL", "0") == "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    with emulated_hip() as lib:
        yield lib


@pytest.mark.parametrize("shape", gc.WGRAD_CASES, ids=lambda s: "x".join(str(v) for v in s[:5]))
def test_wgrad_half_dy(emu, shape):
    gc.check_wgrad_dy16("cpu", *shape)


def test_wgrad_half_dy_zero_repeat_and_flags(emu):
    gc.check_wgrad_dy16_zero_repeat_and_flags("cpu")


@pytest.mark.parametrize("variant", list(range(NUM_VARIANTS)) + [-1])
def test_dgrad_forms_variants(emu, variant):
    emu.dream_conv_f16_set_variant(variant)
    try:
        gc.check_dgrad_shapes("cpu", seed=max(variant, 0))
    finally:
        emu.dream_conv_f16_set_variant(-1)


def test_dgrad_refusals(emu):
    gc.check_dgrad_refusals("cpu")


def test_maxpool_backward_all_half(emu):
    gc.check_pool_bwd_dy16("cpu")


def test_reference_sanity():
    gc.check_reference_sanity((24, 16))          # the belief maps of a 96 x 64 input: (W, H) / 4


@pytest.mark.skipif(not _FULL, reason="set DREAM_EMU_FULL=1 (minutes under the emulator); the GPU suite runs the training step")
def test_training_step_half_gradients(emu):
    gc.check_training_step("cpu")


# ---- host behaviour: no kernel runs (meta device) ------------------------------------------------------------------------------
def _net(**variant):
    with pytest.MonkeyPatch.context() as env, warnings.catch_warnings():
        env.setenv("DREAM_VGG19_WEIGHTS", os.path.join(ROOT, "tests", "golden", "no-such-weights.pth"))
        warnings.simplefilter("ignore")
        return models.DreamHourglass(7, internalize_spatial_softmax=False, **variant).to("meta")


def _trace(net, mp, shape=(4, 64, 96)):
    data_parallel.reset_weight_caches(net)
    rec = lt.Recorder()
    rec.install(mp, ops)
    b, h, w = shape
    params = [p.detach() for p in net.plan_parameters()]
    out, saved = net.run_forward(torch.empty((b, 3, h, w), device="meta"), params, True)
    split = len(rec.launches)
    grads = net.run_backward(saved, torch.empty(out.shape, device="meta"))
    assert [tuple(g.shape) for g in grads] == [tuple(p.shape) for p in params]
    keep = lambda seq: [l for l in seq if not lt.is_pack(l)]      # noqa: E731
    return keep(rec.launches[:split]), keep(rec.launches[split:]), saved


def _name(launch):
    return launch.split(" ", 1)[0]


def _count(seq, name):
    return sum(1 for l in seq if _name(l) == name)


ENTRY, INTERIOR, EXIT = "dream_conv2d_f16_g16_entry_nhwc_f16", "dream_conv2d_f16_g16_nhwc_f16", "dream_conv2d_f16_g16_exit_nhwc_f32"
WGRAD_DY16 = "dream_conv3x3_wgrad_f16_x16_dy16_nhwc_f32"
POOL_DY16 = ("dream_maxpool2_bwd_x16_dy16_nhwc_f16", "dream_maxpool2_relu_bwd_x16_dy16_nhwc_f16")
NEW = (ENTRY, INTERIOR, EXIT, WGRAD_DY16) + POOL_DY16
# what the new launches replace in the run (compared by count, not by argument)
REPLACED = ("dream_conv3x3_wgrad_f16_x16_nhwc_f32", "dream_conv2d_f16_mask16_nhwc_f32", "dream_conv2d_f16_nhwc_f32")


def test_launch_trace_of_a_half_gradient_training_step(monkeypatch):
    net = _net()
    net.train_precision = net.train_activation_storage = net.train_gradient_storage = "fp16"
    fwd, bwd, saved = _trace(net, monkeypatch)
    net.train_gradient_storage = "fp32"
    fwd2, bwd2, saved2 = _trace(net, monkeypatch)
    layers = net.plan_layers()
    half = net._half_storage_plan()
    readers = sorted(saved.half_in)
    pools = [li for li, (kind, _, _) in enumerate(layers) if kind == "pool" and li in half]
    R = len(readers)
    assert R >= 14 and len(pools) == 4 and saved2.half_in == saved.half_in
    assert saved.grad16 == {li for li in half if li != 0} == net._half_gradient_plan() and not saved2.grad16
    assert fwd == fwd2                                               # the forward is the two-switch forward, launch for launch
    # weight gradients: the boundary conv keeps today's x16 (its dy is fp32), every other reader takes the half dy
    assert _count(bwd, WGRAD_DY16) == R - 1 and _count(bwd, "dream_conv3x3_wgrad_f16_x16_nhwc_f32") == 1
    assert _count(bwd2, "dream_conv3x3_wgrad_f16_x16_nhwc_f32") == R
    # data gradients: one entry, one exit, R - 2 interior launches; nothing of the two-switch forms is left in the run
    assert (_count(bwd, ENTRY), _count(bwd, EXIT), _count(bwd, INTERIOR)) == (1, 1, R - 2)
    assert _count(bwd, "dream_conv2d_f16_mask16_nhwc_f32") == 0 and _count(bwd2, "dream_conv2d_f16_mask16_nhwc_f32") == R - len(pools)
    # pools: four all-half backwards, no x16 one
    assert sum(_count(bwd, n) for n in POOL_DY16) == len(pools)
    assert _count(bwd, "dream_maxpool2_bwd_x16_nhwc_f32") + _count(bwd, "dream_maxpool2_relu_bwd_x16_nhwc_f32") == 0
    assert _count(bwd, "dream_maxpool2_bwd_nhwc_f32") + _count(bwd, "dream_maxpool2_relu_bwd_nhwc_f32") == 0
    # absmax: one pass over the loss gradient, none inside the run, fewer in all (behind every pool the two-switch step takes one)
    names = [_name(l) for l in bwd]
    first, last = names.index(ENTRY), names.index(EXIT)
    assert first < last and "dream_absmax_f32" not in names[first:last + 1]
    assert all(n in NEW or n.startswith("dream_unpack") for n in names[first:last + 1]), names[first:last + 1]
    assert _count(bwd, "dream_absmax_f32") == _count(bwd2, "dream_absmax_f32") + 1 - len(pools) < _count(bwd2, "dream_absmax_f32")
    assert names[0] == "dream_absmax_f32" and bwd[0] == "dream_absmax_f32 %d" % (4 * 7 * 16 * 24)
    # every conv-type launch outside the run is, arguments included, that of the two-switch trace
    outside = lambda seq: collections.Counter(l for l in seq if "conv" in _name(l) and "unpack" not in _name(l)      # noqa: E731
                                              and _name(l) not in NEW + REPLACED)
    assert outside(fwd + bwd) == outside(fwd2 + bwd2)
    run = lambda seq: collections.Counter(l for l in seq if _name(l) in REPLACED)      # noqa: E731
    gone = run(fwd2 + bwd2) - run(fwd + bwd)
    # what went: R - 1 weight gradients, R - 4 masked and 4 unmasked fp32 data gradients
    assert not (run(fwd + bwd) - run(fwd2 + bwd2)) and sum(gone.values()) == (R - 1) + R, sorted(gone.elements())
    # the default is untouched: with train_gradient_storage="fp32" no new entry point appears in a training or an inference trace
    assert not [l for l in fwd2 + bwd2 if _name(l) in NEW]
    rec = lt.Recorder()
    rec.install(monkeypatch, ops)
    net.train_gradient_storage = "fp16"                              # inference ignores the switch
    net.run_forward(torch.empty((2, 3, 64, 96), device="meta"), [p.detach() for p in net.plan_parameters()], False)
    assert rec.launches and not [l for l in rec.launches if _name(l) in NEW]
    assert [tuple(t.shape) for pair in saved for t in pair] == [tuple(t.shape) for pair in saved2 for t in pair]


def test_the_rule_on_other_plans():
    plain = _net()
    assert len(plain._half_gradient_plan()) == 18                   # conv1_2 .. conv5_3 and the four pools
    assert 0 not in plain._half_gradient_plan()
    assert not _net(n_image_input_channels=10)._half_gradient_plan()  # a "wide" first conv starts no run


def test_half_gradient_peak_before_the_first_backward():
    with pytest.raises(RuntimeError, match="half_gradient_peak"):
        _net().half_gradient_peak()


def test_value_errors_and_refusing_properties(monkeypatch):
    net = _net()
    net.train_gradient_storage = "fp16"
    with pytest.raises(ValueError, match="train_gradient_storage=\"fp16\" needs"):
        _trace(net, monkeypatch, (1, 32, 32))
    net.train_precision = "fp16"                                     # still no half activations
    with pytest.raises(ValueError, match="train_gradient_storage=\"fp16\" needs"):
        _trace(net, monkeypatch, (1, 32, 32))
    net.train_activation_storage, net.train_gradient_storage = "fp16", "bf16"
    with pytest.raises(ValueError, match="unknown train_gradient_storage"):
        _trace(net, monkeypatch, (1, 32, 32))
    with pytest.MonkeyPatch.context() as env, warnings.catch_warnings():
        env.setenv("DREAM_VGG19_WEIGHTS", os.path.join(ROOT, "tests", "golden", "no-such-weights.pth"))
        warnings.simplefilter("ignore")
        multi = models.DreamHourglassMultiStage(7, internalize_spatial_softmax=False, n_stages=2)
        resnet = models.ResnetSimple(7, pretrained=False)
    for other in (multi, resnet):
        assert other.train_gradient_storage == "fp32"
        other.train_gradient_storage = "fp32"
        with pytest.raises(ValueError, match="train_gradient_storage='fp16' is not supported"):
            other.train_gradient_storage = "fp16"
    assert tc.TRAIN_SHAPE == (2, 64, 96)
