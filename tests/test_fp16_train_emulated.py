"""CPU suite of train_precision="fp16": csrc/wgrad_f16.hip and the ReLU-mask epilogue of csrc/conv_f16.hip compiled unchanged against
the SIMT emulator, through dream_amd.ops / models; the launch list of a training step without any kernel (meta device).  The bounds
are those of fp16_train_checks (derived per launch, measured on the reference end to end)."""
import collections
import os
import warnings

import pytest
import torch

import fp16_train_checks as tc
import launch_trace as lt
from dream_amd import data_parallel, models, ops
from emu_util import emulated_hip

NUM_VARIANTS = 8
_FULL = os.environ.get("DREAM_EMU_FULL", "0") == "1"


@pytest.fixture(scope="module")
def emu():
    with emulated_hip() as lib:
        yield lib


@pytest.mark.parametrize("shape", tc.WGRAD_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:5]))
def test_wgrad_f16(emu, shape):
    tc.check_wgrad_f16("cpu", *shape)


def test_wgrad_f16_splitk(emu):
    tc.check_wgrad_f16_splitk("cpu")


def test_wgrad_f16_zero_repeat_and_flags(emu):
    tc.check_wgrad_f16_zero_and_repeat("cpu")


@pytest.mark.parametrize("variant", range(NUM_VARIANTS))
def test_masked_dgrad_f16_variants(emu, variant):
    emu.dream_conv_f16_set_variant(variant)
    try:
        tc.check_dgrad_f16_shapes("cpu", seed=variant)
    finally:
        emu.dream_conv_f16_set_variant(-1)


def test_masked_dgrad_f16_measured_rule(emu):
    tc.check_dgrad_f16_shapes("cpu")


def test_rejections(emu):
    tc.check_rejections("cpu")


@pytest.mark.skipif(not _FULL, reason="set DREAM_EMU_FULL=1 (minutes under the emulator); the GPU suite runs the training step")
def test_training_step_fp16(emu):
    tc.check_training_step("cpu")
    tc.check_non_plain_entries_bit_equal("cpu")


# ---- launch trace: which entry points a vgg_q training step calls (no kernel runs: meta device) ---------------------------------------
HALF_ONLY = ("dream_conv3x3_wgrad_f16_nhwc_f32", "dream_conv2d_f16_nhwc_f32")
WGRAD_FP32 = ("dream_conv3x3_wgrad_nhwc_f32", "dream_conv3x3_wgrad_winograd_bias_nhwc_f32", "dream_conv3x3_wgrad_winograd_nhwc_f32")


def _trace(train_precision, mp, shape=(4, 64, 96), precision="fp32"):
    with pytest.MonkeyPatch.context() as env:
        env.setenv("DREAM_VGG19_WEIGHTS", os.path.join(os.path.dirname(__file__), "golden", "no-such-weights.pth"))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            net = models.DreamHourglass(7, internalize_spatial_softmax=False).to("meta")
    net.train_precision, net.precision = train_precision, precision
    data_parallel.reset_weight_caches(net)
    rec = lt.Recorder()
    rec.install(mp, ops)
    b, h, w = shape
    x = torch.empty((b, 3, h, w), device="meta")
    params = [p.detach() for p in net.plan_parameters()]
    out, saved = net.run_forward(x, params, True)
    grads = net.run_backward(saved, torch.empty(out.shape, device="meta"))
    assert [tuple(g.shape) for g in grads] == [tuple(p.shape) for p in params]
    return net, [l for l in rec.launches if not lt.is_pack(l)], saved


def _name(launch):
    return launch.split(" ", 1)[0]


def test_launch_trace_of_a_half_precision_training_step(monkeypatch):
    net, seq16, saved = _trace("fp16", monkeypatch)
    _, seq32, _ = _trace("fp32", monkeypatch)
    layers = net.plan_layers()
    plain = [li for li, (kind, mod, flags) in enumerate(layers) if mod is not None and tc.is_plain(kind, mod, flags, int(saved[li][0].shape[3]))]
    others = [li for li, (kind, mod, flags) in enumerate(layers) if mod is not None and li not in plain]
    assert len(plain) >= 15 and len(others) >= 4         # vgg_q: conv1_1, two upsample convs, the K-channel output conv
    count = lambda seq, name: sum(1 for l in seq if _name(l) == name)      # noqa: E731
    # one half-precision weight gradient per plain conv, its forward and its data gradient on conv2d_f16
    assert count(seq16, "dream_conv3x3_wgrad_f16_nhwc_f32") == len(plain)
    assert count(seq16, "dream_conv2d_f16_nhwc_f32") == 2 * len(plain)
    assert count(seq32, "dream_conv3x3_wgrad_f16_nhwc_f32") == 0 and count(seq32, "dream_conv2d_f16_nhwc_f32") == 0
    # the fp32 weight-gradient launches that remain are those of the non-plain 3x3 convs behind the first ("first" has its own kernel)
    n_fp32_wgrad = sum(count(seq16, n) for n in WGRAD_FP32)
    assert n_fp32_wgrad == len(others) - 1, (n_fp32_wgrad, len(others))
    assert sum(count(seq32, n) for n in WGRAD_FP32) == len(plain) + len(others) - 1
    # every non-plain entry has exactly the launches of the default trace: each conv-type launch that is left (arguments included) is one
    # of the default trace, and what the default trace has beyond them are the three fp32 launches (forward, data gradient, weight
    # gradient) of each plain conv.  (Element-wise passes differ by design: no pool is folded into a half-precision conv.)
    heavy = lambda seq: collections.Counter(l for l in seq if "conv" in _name(l) and "unpack" not in _name(l) and _name(l) not in HALF_ONLY)      # noqa: E731
    h16, h32 = heavy(seq16), heavy(seq32)
    assert not (h16 - h32), sorted((h16 - h32).elements())
    assert sum((h32 - h16).values()) == 3 * len(plain), sorted((h32 - h16).elements())
    # the first conv, the upsample convs and the output conv: their launches, arguments included, are the default's
    for name in ("dream_conv3x3_first_nchw_f32", "dream_conv3x3_first_wgrad_f32", "dream_conv_transpose4x4s2_nhwc_f32",
                 "dream_conv_transpose4x4s2_winograd_nhwc_f32", "dream_conv_transpose4x4s2_winograd4_nhwc_f32", "dream_upsample2_bwd_nhwc_f32",
                 "dream_nchw_to_nhwc_pad_f32"):
        assert [l for l in seq16 if _name(l) == name] == [l for l in seq32 if _name(l) == name], name


def test_default_launch_trace_is_untouched_by_inference_precision(monkeypatch):
    """precision="fp16" with the default train_precision: the training launch list is the fp32 one."""
    _, seq32, _ = _trace("fp32", monkeypatch)
    _, seq, _ = _trace("fp32", monkeypatch, precision="fp16")
    assert seq == seq32 and not any("f16" in _name(l) for l in seq)
