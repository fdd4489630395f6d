"""CPU suite of conv_ksplit="auto": the split kernel and its finishing pass (csrc/conv_f16.hip KSPLIT) compiled unchanged against the
SIMT emulator, through dream_amd.ops / models; the rule (a host computation of the product library) and the host behaviour on the
``meta`` device.  Bounds: see fp16_ksplit_checks (derived per launch; the half-storage oracle end to end)."""
import pytest
import torch

import fp16_ksplit_checks as kc
import fp16_storage_checks as sc
import launch_trace as lt
from dream_amd import _hip, ops
from emu_util import emulated_hip
from test_fp16_storage_emulated import _meta_net, _trace

VGG = {"vgg_q": {}, "vgg_f": dict(deconv_decoder=True)}
PLAIN_ENTRY = "dream_conv2d_f16_nhwc_f16"


@pytest.fixture(scope="module")
def emu():
    with emulated_hip() as lib:
        yield lib


@pytest.mark.parametrize("ksize", [1, 3])
@pytest.mark.parametrize("case", kc.LAUNCH_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_split_launches(emu, case, ksize):
    kc.check_case("cpu", case, ksize)


@pytest.mark.parametrize("variant", [0, 3])
def test_split_launches_on_the_128_channel_tiles(emu, variant):
    """The 128 x 128 and 64 x 128 tiles (what the rule picks from 128 output channels on), forced on a 128-channel launch."""
    emu.dream_conv_f16_set_variant(variant)
    try:
        for S in (2, 5):
            kc.check_conv("cpu", 1, 11, 13, 64, 128, 3, S, seed=variant)
    finally:
        emu.dream_conv_f16_set_variant(-1)


@pytest.mark.parametrize("variant", range(8))
def test_split_launches_on_every_tile(emu, variant):
    kc.check_tile("cpu", variant)


@pytest.mark.parametrize("ksize", [1, 3])
@pytest.mark.parametrize("case", kc.LAUNCH_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_saturation_is_finite_and_reported(emu, case, ksize):
    kc.check_saturation("cpu", case, ksize)


@pytest.mark.parametrize("case", kc.LAUNCH_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_refused_flags(emu, case):
    kc.check_refused_flags("cpu", case)


@pytest.mark.parametrize("case,ksize", [(kc.LAUNCH_CASES[2], 1), (kc.LAUNCH_CASES[2], 3), (kc.LAUNCH_CASES[0], 1)],
                         ids=lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v))
def test_slices_past_the_stages_are_zero(emu, case, ksize):
    """2 x 13 x 13 x 32 -> 34 with ksize 1 is one stage: three slices asked of the entry point leave two empty."""
    kc.check_empty_slices("cpu", case, ksize)


def test_vgg_q_golden_split(emu):
    """The smallest end-to-end case: one 50 x 75 frame, every splittable launch split by the rule; held to the half-storage oracle
    exactly as the unsplit walk is (fp16_storage_checks.check_golden)."""
    seen = []
    build = sc.pc.build_network

    def build_split(*a, **k):
        net = build(*a, **k)
        net.model.module.conv_ksplit = "auto"
        seen.append(net)
        return net

    with pytest.MonkeyPatch.context() as mp, kc.launch_names() as names:
        mp.setattr(sc.pc, "build_network", build_split)
        sc.check_golden("cpu", "vgg_q", (1, 50, 75), with_fp32=False)
    assert len(seen) == 1 and seen[0].model.module.conv_ksplit == "auto"
    assert names.count(kc.SPLIT_ENTRY) >= 1, "no launch of this walk was split: the test shows nothing"


# ---- the rule: the product library's host function, no device ------------------------------------------------------------------
def _conv_launches(net, shape, monkeypatch):
    """(name, b, h, w, cin, cout, ksize, flags) of every plain / split half-storage conv launch of one inference walk on ``meta``."""
    rec = lt.Recorder()
    rec.install(monkeypatch, ops)
    b, h, w = shape
    net.run_forward(torch.empty((b, 3, h, w), device="meta"), [p.detach() for p in net.plan_parameters()], False)
    out = []
    for l in rec.launches:
        name, *args = l.split(" ")
        if name in (PLAIN_ENTRY, kc.SPLIT_ENTRY):
            a = [int(v) for v in args][-9:]                # b h w cin cout coutpad ksize stride flags (the split entry: S in front)
            out.append((name, a[0], a[1], a[2], a[3], a[4], a[6], a[8]))
    return out, [l for l in rec.launches if not lt.is_pack(l)]


@pytest.mark.parametrize("arch", sorted(VGG))
def test_rule_splits_nothing_at_128_frames(arch, monkeypatch):
    net = _meta_net(**VGG[arch])
    net.precision = net.activation_storage = "fp16"
    convs, off = _conv_launches(net, (128, 400, 400), monkeypatch)
    assert len(convs) >= 10
    for _, b, h, w, cin, cout, k, flags in convs:
        assert ops.conv2d_f16_ksplit(b, h, w, cin, cout, k, flags) == 1, (b, h, w, cin, cout, k, flags)
    net.conv_ksplit = "auto"
    _, auto = _conv_launches(net, (128, 400, 400), monkeypatch)
    assert auto == off


def test_rule_splits_the_deep_layers_of_one_frame():
    for hw in (25, 50):
        assert ops.conv2d_f16_ksplit(1, hw, hw, 512, 512, 3, ops.CONV_RELU) > 1, hw
    assert ops.conv2d_f16_ksplit(1, 400, 400, 64, 64, 3, ops.CONV_RELU) == 1
    assert ops.conv2d_f16_ksplit(1, 25, 25, 512, 512, 3, ops.CONV_RELU | ops.CONV_POOL2) == 1
    assert int(_hip.lib().dream_conv2d_f16_ksplit_workspace(1, 7, 9, 34, 3)) == 3 * 2144 * 4      # slices of round_up(2142, 8) floats


@pytest.mark.parametrize("arch", sorted(VGG))
def test_rule_is_monotone_in_the_batch(arch, monkeypatch):
    net = _meta_net(**VGG[arch])
    net.precision = net.activation_storage = "fp16"
    convs, _ = _conv_launches(net, (1, 400, 400), monkeypatch)
    shapes = sorted({(h, w, cin, cout, k) for _, _, h, w, cin, cout, k, flags in convs if not flags & ~ops.CONV_RELU})
    assert len(shapes) >= 4
    kc.check_rule_monotone(shapes + [(13, 13, 32, 34, 1), (16, 16, 512, 64, 3), (100, 100, 256, 256, 3), (7, 9, 96, 40, 3)])


# ---- host behaviour: no kernel runs (meta device) ------------------------------------------------------------------------------
def test_one_frame_walk_splits_and_off_is_the_parents_walk(monkeypatch):
    net = _meta_net()
    net.precision = net.activation_storage = "fp16"
    _, off = _conv_launches(net, (1, 400, 400), monkeypatch)
    net.conv_ksplit = "auto"
    convs, auto = _conv_launches(net, (1, 400, 400), monkeypatch)
    net.conv_ksplit = "off"
    _, off_again = _conv_launches(net, (1, 400, 400), monkeypatch)
    assert off_again == off and not [l for l in off if l.startswith(kc.SPLIT_ENTRY)]
    split = [c for c in convs if c[0] == kc.SPLIT_ENTRY]
    assert split and len(auto) == len(off)
    for name, b, h, w, cin, cout, k, flags in convs:
        s = ops.conv2d_f16_ksplit(b, h, w, cin, cout, k, flags)
        assert (name == kc.SPLIT_ENTRY) == (s > 1), (name, s)
        assert name == PLAIN_ENTRY or not flags & (ops.CONV_POOL2 | ops.CONV_UPSAMPLE2X | ops.CONV_OUT_NCHW)
    # everything that is not a split conv is the launch it was, in place
    for a, o in zip(auto, off):
        assert a == o or (a.startswith(kc.SPLIT_ENTRY) and o.startswith(PLAIN_ENTRY + " ")), (a, o)


def test_training_ignores_the_switch(monkeypatch):
    net = _meta_net()
    _, train_off, _ = _trace(net, (1, 64, 96), monkeypatch, save=True)
    net.conv_ksplit = "auto"                             # (precision / activation_storage still "fp32": a training forward does not look)
    _, train_auto, _ = _trace(net, (1, 64, 96), monkeypatch, save=True)
    assert train_auto == train_off


def test_value_errors(monkeypatch):
    import os
    import warnings
    from dream_amd import models
    net = _meta_net()
    assert net.conv_ksplit == "off"
    net.conv_ksplit = "auto"
    for precision, storage in (("fp32", "fp32"), ("fp16x3", "fp32"), ("fp16", "fp32")):
        net.precision, net.activation_storage = precision, storage
        with pytest.raises(ValueError, match="conv_ksplit.*precision.*activation_storage"):
            _trace(net, (1, 32, 32), monkeypatch)
    net.precision = net.activation_storage = "fp16"
    net.conv_ksplit = "on"
    with pytest.raises(ValueError, match="unknown conv_ksplit"):
        _trace(net, (1, 32, 32), monkeypatch)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with pytest.MonkeyPatch.context() as mp, warnings.catch_warnings():
        mp.setenv("DREAM_VGG19_WEIGHTS", os.path.join(root, "tests", "golden", "no-such-weights.pth"))
        warnings.simplefilter("ignore")
        multi = models.DreamHourglassMultiStage(7, internalize_spatial_softmax=False, n_stages=2)
        resnet = models.ResnetSimple(7, pretrained=False)
    for other in (multi, resnet):
        assert other.conv_ksplit == "off"
        other.conv_ksplit = "off"
        with pytest.raises(ValueError, match="conv_ksplit='auto' is not supported"):
            other.conv_ksplit = "auto"


def test_replica_settings_carry_the_switch():
    from dream_amd import data_parallel
    net = _meta_net()
    off = data_parallel._settings(net)
    net.conv_ksplit = "auto"
    assert data_parallel._settings(net) != off and "auto" in data_parallel._settings(net)
