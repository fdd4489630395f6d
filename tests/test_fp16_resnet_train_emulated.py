"""CPU suite of ResnetSimple's train_gemm_precision="fp16": csrc/gemm1x1_f16.hip and the amax form of bn_bwd_apply compiled unchanged against
the SIMT emulator (bounds: fp16_resnet_train_checks); the launch list of a training step without any kernel (meta device); the switch."""
import collections
import json

import pytest
import torch

import fp16_resnet_train_checks as rc
import launch_trace as lt
import test_resnet_launch_trace as rt
from dream_amd import models
from emu_util import emulated_hip


@pytest.fixture(scope="module")
def emu():
    with emulated_hip() as lib:
        yield lib


@pytest.mark.parametrize("ks", (1, 2, 4))
@pytest.mark.parametrize("form", rc.GEMM_FORMS)
@pytest.mark.parametrize("shape", rc.GEMM_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_gemm_f16(emu, shape, form, ks):
    if shape[1] % (32 * ks):               # K = 64 four ways: the fp32 entry points' contract (K % (32 ks)), refused before the launch
        with pytest.raises(RuntimeError, match="cannot be split"):
            rc.check_gemm("cpu", shape, form, ks)
    else:
        rc.check_gemm("cpu", shape, form, ks)


def test_gemm_f16_padded_rows_and_split_by_shape(emu):
    rc.check_gemm("cpu", (70, 64, 64), "plain_grad", 0, stride_pad=4)
    rc.check_gemm("cpu", (70, 64, 64), "res", 2, stride_pad=4)


def test_gemm_f16_repeats_bit_for_bit(emu):
    rc.check_gemm_repeat("cpu")


@pytest.mark.parametrize("shape", rc.WGRAD_SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_wgrad_f16(emu, shape):
    split = rc.check_wgrad("cpu", shape)
    assert (split > 1) == (shape[0] == 4112)         # the workspace query: the long one is split over positions, the short ones are not


def test_scales(emu):
    rc.check_scales("cpu")


def test_bn_bwd_apply_amax(emu):
    rc.check_bn_bwd_apply_amax("cpu")


def test_batched_pack(emu):
    rc.check_batched_pack("cpu")


def test_refusals(emu):
    rc.check_refusals("cpu")


# ---- the launch list (meta device, no kernel: the harness of test_resnet_launch_trace.py) ---------------------------------------------
TWINS = {"dream_conv1x1_bnstats_f16_nhwc_f32": "dream_conv1x1_bnstats_nhwc_f32",
         "dream_conv1x1_bwd_bnmask_f16_nhwc_f32": "dream_conv1x1_bwd_bnmask_nhwc_f32",
         "dream_conv1x1_f16_nhwc_f32": "dream_conv1x1_nhwc_f32",
         "dream_conv1x1_wgrad_f16_nhwc_f32": "dream_conv1x1_wgrad_*_nhwc_f32",
         "dream_bn_bwd_apply_amax_nhwc_f32": "dream_bn_bwd_apply_nhwc_f32"}


def _as_fp32(launch):
    """An f16 launch written as the fp32 launch it replaces (same scalar arguments; the plain GEMM's twin carries flags = 0); the two
    fp32 weight-gradient entry points differ by a pointer only, which a trace does not hold."""
    name, _, args = launch.partition(" ")
    if name in ("dream_conv1x1_wgrad_nhwc_f32", "dream_conv1x1_wgrad_pre_nhwc_f32"):
        name = "dream_conv1x1_wgrad_*_nhwc_f32"
    if name in TWINS:
        name, args = TWINS[name], args + (" 0" if name == "dream_conv1x1_f16_nhwc_f32" else "")
    return (name + " " + args).strip()


def _trace(case_name, mp, train_gemm_precision):
    case = rt.CASES[case_name]                            # (run_case sets every switch: the value goes through the case's options)
    return rt.run_case(dict(case, opts=dict(case["opts"], train_gemm_precision=train_gemm_precision)), mp)


@pytest.mark.parametrize("case_name", ["h-16x400x400-training", "f-2x70x93-training", "h-128x400x400-training"])
def test_launch_list(case_name, monkeypatch):
    with open(rt.FIXTURE) as f:
        want = lt.decode(json.load(f), case_name)
    explicit = _trace(case_name, monkeypatch, "fp32")
    assert explicit["seq"] == want["seq"]                              # "fp32" set explicitly: the default trace
    got = _trace(case_name, monkeypatch, "fp16")
    seq16, seq32 = got["seq"], want["seq"]
    name = lambda l: l.split(" ", 1)[0]                                # noqa: E731
    # launch for launch: every f16 launch stands where its fp32 twin stood, with its arguments; everything else is identical
    assert [_as_fp32(l) for l in seq16] == [_as_fp32(l) for l in seq32], lt.first_difference(seq32, seq16)
    n16 = collections.Counter(name(l) for l in seq16)
    n32 = collections.Counter(name(l) for l in seq32)
    assert not any("absmax" in n for n in n16)
    # covered: the 70 bias-free 1x1 convs of the Bottlenecks + the stride-2 3x3 convs that run on their patch rows (one im2col3s2 launch
    # each in the forward): each with one forward, one amax-publishing BatchNorm backward and one data gradient
    blocks = list(rt._net(rt.CASES[case_name]["net"])._trunk())
    convs_1x1 = sum(2 + hasattr(blk, "downsample") for _, blk in blocks)
    assert convs_1x1 == 70
    covered = n16["dream_conv1x1_bnstats_f16_nhwc_f32"]
    assert covered == convs_1x1 + n32["dream_im2col3s2_nhwc_f32"]
    assert n16["dream_bn_bwd_apply_amax_nhwc_f32"] == covered
    assert n16["dream_conv1x1_bwd_bnmask_f16_nhwc_f32"] + n16["dream_conv1x1_f16_nhwc_f32"] == covered
    # not covered, and still there: the stem's GEMM and its statistics, the head (loader form, masked data gradient, weight gradient),
    # the transposed convs' small-map GEMM (DREAM_CONV_NO_KSPLIT)
    assert n16["dream_conv1x1_bnstats_nhwc_f32"] == n32["dream_conv1x1_bnstats_nhwc_f32"] - covered
    assert n16["dream_conv1x1_pre_nhwc_f32"] == n32["dream_conv1x1_pre_nhwc_f32"]
    # the weight gradients on the GEMM kernel (arguments: M, Cin, Cout, Cdy): half exactly from 256 x 128 channel pairs on -- below, the
    # covered units of layer1 keep the fp32 launch (ops.conv1x1_wgrad_f16_pays: measured slower), and so do the stem's and the head's
    n_half = 0
    for l32, l16 in zip(seq32, seq16):
        if name(l32) in ("dream_conv1x1_wgrad_nhwc_f32", "dream_conv1x1_wgrad_pre_nhwc_f32"):
            _, cin, cout, _ = (int(v) for v in l32.split(" ")[1:])
            assert (name(l16) == "dream_conv1x1_wgrad_f16_nhwc_f32") == (cin * cout >= 32768), (l32, l16)
            assert name(l16) in ("dream_conv1x1_wgrad_f16_nhwc_f32", name(l32))
            n_half += name(l16) != name(l32)
    assert n_half >= 60
    assert [l for l in seq16 if name(l) == "dream_conv1x1_nhwc_f32"] == [l for l in seq32 if l.endswith(" 128") and name(l) == "dream_conv1x1_nhwc_f32"]
    assert n16["dream_bn_bwd_apply_nhwc_f32"] == n32["dream_bn_bwd_apply_nhwc_f32"] - covered
    for other in ("dream_conv3x3_winograd_bnstats_nhwc_f32", "dream_conv3x3_winograd_bwd_bnmask_nhwc_f32", "dream_bn_stats_nhwc_f32",
                  "dream_bn_bwd_stats_nhwc_f32", "dream_maxpool3s2_idx_nhwc_f32", "dream_conv2d_nhwc_f32"):
        assert [l for l in seq16 if name(l) == other] == [l for l in seq32 if name(l) == other], other
    # the packed copies: half ones for the covered convs (both directions), the fp32 ones of everything else unchanged
    packs16 = collections.Counter(l.split(" ", 1)[0] for l in got["packs"])
    assert packs16["dream_pack_conv1x1_weight_f16"] == 2 * covered


def test_inference_precision_leaves_the_training_step_alone(monkeypatch):
    """precision="fp16" is an inference switch: the training launch list with it is the default one."""
    case = dict(rt.CASES["h-2x70x93-training"], opts=dict(precision="fp16"))
    with open(rt.FIXTURE) as f:
        want = lt.decode(json.load(f), "h-2x70x93-training")
    assert rt.run_case(case, monkeypatch)["seq"] == want["seq"]


# ---- the switch ---------------------------------------------------------------------------------------------------------------------------
def _meta_net():
    return models.ResnetSimple(7, pretrained=False).to("meta")


def _forward(net, training, mp):
    rec = lt.Recorder()
    rec.install(mp, rt.ops)
    net.train(training)
    x = torch.empty((2, 3, 64, 64), device="meta")
    with torch.no_grad():
        return net.run_forward_train(x) if training else net.run_forward(x)


def test_switch_is_an_instance_attribute(monkeypatch):
    a, b = _meta_net(), _meta_net()
    assert a.train_gemm_precision == "fp32"
    a.train_gemm_precision = "fp16"
    assert a.train_gemm_precision == "fp16" and b.train_gemm_precision == "fp32"
    _forward(a, True, monkeypatch)
    _forward(a, False, monkeypatch)                       # inference ignores a known value


@pytest.mark.parametrize("training", (True, False))
def test_unknown_value_raises_in_both_passes(training, monkeypatch):
    net = _meta_net()
    net.train_gemm_precision = "bf16"
    with pytest.raises(ValueError, match="unknown train_gemm_precision 'bf16'"):
        _forward(net, training, monkeypatch)


@pytest.mark.parametrize("switch", (dict(bn_fusion=False), dict(conv1x1_algorithm="direct")))
def test_fp16_needs_the_fused_gemm_path(switch, monkeypatch):
    net = _meta_net()
    net.train_gemm_precision = "fp16"
    for k, v in switch.items():
        setattr(net, k, v)
    with pytest.raises(ValueError, match="train_gemm_precision=\"fp16\" needs bn_fusion"):
        _forward(net, True, monkeypatch)
    net.train_gemm_precision = "fp32"
    _forward(net, True, monkeypatch)                      # the fp32 step runs with either switch


def test_hip_graph_train_refuses_the_mode():
    import parity_checks as pc
    net = pc.build_network("resnet_h", "cpu")
    net.model.module.train_gemm_precision = "fp16"
    with pytest.raises(ValueError, match="hip_graph_train does not replay train_gemm_precision='fp16'"):
        net.hip_graph_train = True
    net.model.module.train_gemm_precision = "fp32"


def test_other_switches_still_refuse():
    net = _meta_net()
    for name in ("train_precision", "activation_storage", "train_activation_storage", "train_gradient_storage"):   # (train_precision: the hourglass's switch, fixed here)
        with pytest.raises(ValueError):
            setattr(net, name, "fp16")


# ---- the yardsticks of the GPU suite, recomputed on the CPU reference; one Bottleneck under the emulator -------------------------------
import fp16_resnet_step_checks as sc  # noqa: E402


@pytest.mark.parametrize("block", sc.BLOCKS)
def test_block_yardstick_is_a_rounding_distance(block):
    E = sc.block_yardstick(block)
    assert set(E) >= {"conv1.weight", "conv2.weight", "conv3.weight", "bn1.weight", "bn3.bias", "dx"}
    assert 5e-3 < max(E.values()) < 5e-2, E              # (measured: 1.1e-2 .. 3.6e-2, worst tensor per block)


def test_step_yardstick_conditions_exactly_the_last_decoder_tensors():
    E, move = sc.step_yardstick((32, 32))
    assert sorted(n for n, e in E.items() if e <= 0.05) == sorted(sc.CONDITIONED)
    assert min(e for n, e in E.items() if n not in sc.CONDITIONED) >= 0.19
    assert 1e-4 < move < 1e-2


@pytest.mark.parametrize("optimizer", ("adam", "sgd"))
def test_training_gap_constants_hold(optimizer):
    gap, plain, rounded = sc.rounded_training_gap(optimizer, (32, 32))
    assert rounded[-1] < 0.5 * rounded[0] and plain[-1] < 0.5 * plain[0]
    assert sc.TRAIN_GAP[optimizer] / 2 <= gap <= 1.25 * sc.TRAIN_GAP[optimizer], (gap, sc.TRAIN_GAP[optimizer])


def test_one_bottleneck_emulated(emu):
    sc.check_block("cpu", "layer1.0")
