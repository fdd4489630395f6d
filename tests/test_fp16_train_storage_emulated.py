"""CPU suite of train_activation_storage="fp16": the half-x kernel of csrc/wgrad_f16.hip, the half-mask epilogue of csrc/conv_f16.hip, the
half-x max-pool backward and the widening pass of csrc/elementwise.hip compiled unchanged against the SIMT emulator, through
dream_amd.ops / models; the launch list of such a training step and the host's refusals without any kernel (meta device).  Bounds: see
fp16_train_storage_checks."""
import collections
import os
import warnings

import pytest
import torch

import fp16_train_checks as tc
import fp16_train_storage_checks as sc
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


@pytest.mark.parametrize("shape", sc.WGRAD_CASES, ids=lambda s: "x".join(str(v) for v in s[:5]))
def test_wgrad_half_x(emu, shape):
    sc.check_wgrad_x16("cpu", *shape)


def test_wgrad_half_x_zero_repeat_and_flags(emu):
    sc.check_wgrad_x16_zero_repeat_and_flags("cpu")


@pytest.mark.parametrize("variant", list(range(NUM_VARIANTS)) + [-1])
def test_masked_dgrad_half_mask_variants(emu, variant):
    emu.dream_conv_f16_set_variant(variant)
    try:
        sc.check_dgrad_mask16_shapes("cpu", seed=max(variant, 0))
    finally:
        emu.dream_conv_f16_set_variant(-1)


def test_maxpool_backward_half_x(emu):
    sc.check_pool_bwd_x16("cpu")


def test_widening(emu):
    sc.check_widen("cpu")


@pytest.mark.skipif(not _FULL, reason="set DREAM_EMU_FULL=1 (minutes under the emulator); the GPU suite runs the training step")
def test_training_step_half_storage(emu):
    sc.check_training_step("cpu")
    sc.check_entries_outside_the_run_bit_equal("cpu")


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


NEW_OR_HALF = ("dream_conv3x3_first_nchw_f16", "dream_conv2d_f16_nhwc_f16", "dream_maxpool2_nhwc_f16", "dream_widen_f16_f32",
               "dream_conv3x3_wgrad_f16_x16_nhwc_f32", "dream_conv2d_f16_mask16_nhwc_f32", "dream_maxpool2_bwd_x16_nhwc_f32",
               "dream_maxpool2_relu_bwd_x16_nhwc_f32")


def test_launch_trace_of_a_half_stored_training_step(monkeypatch):
    net = _net()
    net.train_precision = net.train_activation_storage = "fp16"
    fwd, bwd, saved = _trace(net, monkeypatch)
    net.train_activation_storage = "fp32"
    fwd16, bwd16, saved16 = _trace(net, monkeypatch)
    layers = net.plan_layers()
    half = net._half_storage_plan()
    readers = sorted(saved.half_in)                                  # the plain convs with a half input
    pools = [li for li, (kind, _, _) in enumerate(layers) if kind == "pool" and li in half]
    assert len(readers) >= 14 and len(pools) == 4
    assert readers == [li for li in range(1, len(layers)) if layers[li][1] is not None and li - 1 in half]
    assert all(tc.is_plain(*layers[li], int(saved[li][0].shape[3])) for li in readers)
    # which tensors are half: the outputs of the run, nothing else; the boundary conv's saved output is the widened tensor
    for li, (inp, out) in enumerate(saved):
        assert (out.dtype == torch.float16) == (li in half), li
        assert (inp.dtype == torch.float16) == (li - 1 in half), li
    boundary = [li for li in readers if li not in half]
    assert len(boundary) == 1 and saved[boundary[0]][1].dtype == torch.float32
    # forward: the first conv, one half-storage launch per reader, the half pools, exactly one widening launch
    assert _name(fwd[0]) == "dream_conv3x3_first_nchw_f16" and _count(fwd, "dream_conv3x3_first_nchw_f16") == 1
    assert _count(fwd, "dream_conv2d_f16_nhwc_f16") == len(readers)
    assert _count(fwd, "dream_maxpool2_nhwc_f16") == len(pools) and _count(fwd, "dream_maxpool2_nhwc_f32") == 0
    assert _count(fwd + bwd, "dream_widen_f16_f32") == 1
    assert fwd.index(next(l for l in fwd if _name(l) == "dream_widen_f16_f32")) == 1 + len(readers) + len(pools)
    # backward: one half-x weight gradient and one half-mask (or, behind a pool, unmasked) data gradient per reader
    n_plain = _count(bwd16, "dream_conv3x3_wgrad_f16_nhwc_f32")
    assert _count(bwd, "dream_conv3x3_wgrad_f16_x16_nhwc_f32") == len(readers)
    assert _count(bwd, "dream_conv3x3_wgrad_f16_nhwc_f32") == n_plain - len(readers)       # none with an fp32 x for them
    assert _count(bwd, "dream_conv2d_f16_mask16_nhwc_f32") == len(readers) - len(pools)
    assert _count(bwd, "dream_maxpool2_relu_bwd_x16_nhwc_f32") == len(pools)
    assert _count(bwd, "dream_maxpool2_bwd_nhwc_f32") + _count(bwd, "dream_maxpool2_relu_bwd_nhwc_f32") == 0
    assert _count(bwd, "dream_relu_bwd_f32") == _count(bwd16, "dream_relu_bwd_f32")
    # every entry outside the run: its conv-type launches, arguments included, are those of the train_precision="fp16" trace
    outside = lambda seq: collections.Counter(l for l in seq if "conv" in _name(l) and "unpack" not in _name(l)      # noqa: E731
                                              and _name(l) not in NEW_OR_HALF)
    now, was = outside(fwd + bwd), outside(fwd16 + bwd16)
    assert not (now - was), sorted((now - was).elements())
    # what went: per reader its forward, weight gradient and masked data gradient (behind a pool the data gradient carries no mask --
    # the pool's backward does -- and is the same launch in both traces), and the first conv's forward
    gone = was - now
    assert sum(gone.values()) == 3 * len(readers) - len(pools) + 1, sorted(gone.elements())
    assert {_name(l) for l in gone} == {"dream_conv2d_f16_nhwc_f32", "dream_conv3x3_wgrad_f16_nhwc_f32", "dream_conv3x3_first_nchw_f32"}
    # the default is untouched: with train_activation_storage="fp32" no new or half-storage launch appears
    assert not [l for l in fwd16 + bwd16 if _name(l) in NEW_OR_HALF]


def test_the_rule_on_other_plans():
    plain = _net()
    assert len(plain._half_storage_plan()) == 19                    # conv1_1 .. conv5_3 and the four pools
    skip = _net(skip_connections=True, deconv_decoder=True)
    half = skip._half_storage_plan()
    first_source = min(skip._skip_sources)
    assert half == set(range(first_source)) and half                # the run ends at the first skip source
    assert not _net(n_image_input_channels=10)._half_storage_plan()  # a "wide" first conv starts none


def test_inference_and_default_ignore_the_switch(monkeypatch):
    net = _net()
    rec = lt.Recorder()
    rec.install(monkeypatch, ops)
    x = torch.empty((2, 3, 64, 96), device="meta")
    params = [p.detach() for p in net.plan_parameters()]
    net.run_forward(x, params, False)
    default, rec.launches = [l for l in rec.launches if not lt.is_pack(l)], []
    net.train_activation_storage = "fp16"                            # (train_precision is "fp32": a training forward would raise)
    net.run_forward(x, params, False)
    assert [l for l in rec.launches if not lt.is_pack(l)] == default and default


def test_value_errors(monkeypatch):
    net = _net()
    net.train_activation_storage = "fp16"
    with pytest.raises(ValueError, match="train_activation_storage.*train_precision"):
        _trace(net, monkeypatch, (1, 32, 32))
    net.train_precision, net.train_activation_storage = "fp16", "bf16"
    with pytest.raises(ValueError, match="unknown train_activation_storage"):
        _trace(net, monkeypatch, (1, 32, 32))
    with pytest.MonkeyPatch.context() as env, warnings.catch_warnings():
        env.setenv("DREAM_VGG19_WEIGHTS", os.path.join(ROOT, "tests", "golden", "no-such-weights.pth"))
        warnings.simplefilter("ignore")
        multi = models.DreamHourglassMultiStage(7, internalize_spatial_softmax=False, n_stages=2)
        resnet = models.ResnetSimple(7, pretrained=False)
    for other in (multi, resnet):
        assert other.train_activation_storage == "fp32"
        other.train_activation_storage = "fp32"
        with pytest.raises(ValueError, match="train_activation_storage='fp16' is not supported"):
            other.train_activation_storage = "fp16"
