"""CPU suite of ResnetSimple.inference_conv_ksplit="auto": the split 4x4 transposed conv (four ksplit-form launches and
convT4_f16_ksplit_finish_kernel, csrc/conv_f16.hip) compiled unchanged against the SIMT emulator, through dream_amd.ops / models; the
rule ResnetSimple asks (a host computation of the product library) and the host behaviour on the ``meta`` device.  Bounds: see
fp16_resnet_ksplit_checks (derived per launch; the half-storage oracle end to end)."""
import os

import pytest
import torch

import fp16_resnet_ksplit_checks as rk
import parity_checks as pc
from dream_amd import data_parallel, models, ops
from emu_util import emulated_hip
from oracle import models as om
from test_fp16_resnet_storage_emulated import NETWORKS, _trace
from test_fp16_resnet_storage_emulated import _meta_net as _storage_meta_net

_FULL = os.environ.get("DREAM_EMU_FULL", "0") == "1"


@pytest.fixture(scope="module")
def emu():
    with emulated_hip() as lib:
        yield lib


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    """The meta networks are shared with the other suites of this process: none of them leaves here with the switch on."""
    yield
    for name in NETWORKS:
        _storage_meta_net(name).inference_conv_ksplit = "off"


def _meta_net(name, ksplit="off"):
    net = _storage_meta_net(name)
    net.precision = net.inference_activation_storage = "fp16"
    net.inference_conv_ksplit = ksplit
    return net


# ---- the split transposed conv, per launch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("case", rk.CONVT_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_split_transposed_launches(emu, case, relu):
    rk.check_convT_case("cpu", case, relu)


@pytest.mark.parametrize("variant", range(8))
def test_split_transposed_launches_on_every_tile(emu, variant):
    rk.check_convT_tile("cpu", variant)


def test_saturation_is_finite_and_reported(emu):
    rk.check_convT_saturation("cpu")


def test_refusals(emu):
    rk.check_convT_refusals("cpu")


def test_one_bottleneck(emu):
    rk.check_bottleneck("cpu")


def test_one_decoder_stage(emu):
    rk.check_stage("cpu")


@pytest.mark.skipif(not _FULL, reason="set DREAM_EMU_FULL=1 (minutes under the emulator); the GPU suite runs the structured cases")
@pytest.mark.parametrize("case", ["resnet_h", "resnet_f"])
def test_structured_split_walk(emu, case):
    rk.check_structured("cpu", case)


# ---- the rule: the product library's host functions, no device -----------------------------------------------------------------------
def _covered_shapes(monkeypatch):
    shapes = set()
    for name in sorted(NETWORKS):
        convs, _ = rk.covered_launches(_meta_net(name), (1, 400, 400), monkeypatch)
        # covered: a conv of the trunk (the stem is the first plain launch, the head the NCHW one) and every decoder stage
        shapes |= {(h, w, cin, cout, k) for _, _, h, w, cin, cout, k, flags in convs[1:] if not flags & ops.CONV_OUT_NCHW}
    return sorted(shapes)


def test_rule_properties_on_every_covered_shape(monkeypatch):
    shapes = _covered_shapes(monkeypatch)
    assert len(shapes) >= 20 and sum(1 for s in shapes if s[4] == 0) == 5, shapes
    rk.check_rule_properties(shapes + [(7, 9, 96, 40, 3), (13, 13, 64, 64, 0), (4, 5, 512, 32, 0)])


def test_rule_is_one_for_a_one_stage_launch():
    assert ops.conv2d_f16_ksplit_resnet(1, 13, 13, 32, 64, 1, ops.CONV_RELU) == 1
    with rk.forced_ksplit(4):
        assert ops.conv2d_f16_ksplit_resnet(1, 13, 13, 32, 64, 1, ops.CONV_RELU) == 1
        assert ops.conv_transpose4x4s2_f16_ksplit(1, 13, 13, 32, 64) == 4                      # (a phase of 32 channels: 4 stages)


def test_rule_splits_the_deep_half_of_one_frame():
    """The launches the mode exists for: the first decoder stage and layer4's contractions at one frame; nothing at a full map."""
    assert ops.conv_transpose4x4s2_f16_ksplit(1, 13, 13, 2048, 256) > 1
    assert ops.conv2d_f16_ksplit_resnet(1, 13, 13, 512, 512, 3, ops.CONV_RELU) > 1
    assert ops.conv2d_f16_ksplit_resnet(1, 13, 13, 4608, 512, 1, ops.CONV_RELU) > 1
    assert ops.conv2d_f16_ksplit_resnet(128, 100, 100, 64, 64, 3, ops.CONV_RELU) == 1
    assert ops.conv_transpose4x4s2_f16_ksplit(128, 104, 104, 256, 256) == 1


def test_the_hourglass_rule_answers_what_it_answered():
    for args, s in rk.HOURGLASS_RULE:
        assert ops.conv2d_f16_ksplit(*args) == s, (args, s)


# ---- host behaviour: no kernel runs (meta device) ------------------------------------------------------------------------------------
def test_switch_is_an_instance_attribute_with_a_default():
    a, b = models.ResnetSimple(pretrained=False), _storage_meta_net("h")
    assert a.inference_conv_ksplit == "off" and "inference_conv_ksplit" in a.__dict__
    assert not hasattr(models.ResnetSimple, "inference_conv_ksplit")
    a.inference_conv_ksplit = "auto"
    assert b.inference_conv_ksplit == "off"


def test_value_errors(monkeypatch):
    net = _storage_meta_net("h")
    net.inference_conv_ksplit = "auto"
    for precision, storage in (("fp32", "fp32"), ("fp16x3", "fp32"), ("fp16", "fp32")):
        net.precision, net.inference_activation_storage = precision, storage
        with pytest.raises(ValueError, match="inference_conv_ksplit.*precision.*inference_activation_storage"):
            _trace(net, (1, 64, 64), monkeypatch)
        _trace(net.train(), (2, 64, 96), monkeypatch, training=True)                 # (a training pass does not look at the needs)
        net.eval()
    net.precision = net.inference_activation_storage = "fp16"
    net.inference_conv_ksplit = "on"
    for training in (False, True):
        with pytest.raises(ValueError, match="unknown inference_conv_ksplit"):
            _trace(net.train(training), (2, 64, 96), monkeypatch, training=training)
    net.eval()
    # the hourglass's name stays what it was on this class: fixed, refusing
    assert net.conv_ksplit == "off"
    net.conv_ksplit = "off"
    with pytest.raises(ValueError, match="conv_ksplit='auto' is not supported"):
        net.conv_ksplit = "auto"


def test_training_ignores_the_switch(monkeypatch):
    net = _storage_meta_net("h")
    _, train_off, _ = _trace(net.train(), (2, 64, 96), monkeypatch, training=True)
    net = _meta_net("h", "auto")
    _, train_auto, _ = _trace(net.train(), (2, 64, 96), monkeypatch, training=True)
    net.eval()
    assert train_auto == train_off
    assert not [l for l in train_auto if l.split(" ", 1)[0] in rk.SPLIT_ENTRIES]


def test_replica_settings_carry_the_switch():
    net = models.ResnetSimple(pretrained=False)
    off = data_parallel._settings(net)
    net.inference_conv_ksplit = "auto"
    assert data_parallel._settings(net) != off and "auto" in data_parallel._settings(net)


def test_replicas_follow_the_switch(emu, monkeypatch):
    """Two emulated devices: a replica made before the switch moved takes the master's value at the next _sync_replicas."""
    monkeypatch.setenv("DREAM_DP_EMULATED_DEVICES", "2")
    wts = om.recipe_weights(om.build_model("resnet_h", 7).state_dict())
    net = pc.build_network("resnet_h", "cpu", weights=wts, in_res=(32, 32))
    net.enable_evaluation()
    dp = net.model
    dp._ensure_replicas(2)
    rep = dp._replicas[0]
    assert rep is not dp.module and rep.inference_conv_ksplit == "off"
    dp.module.precision = dp.module.inference_activation_storage = "fp16"
    dp.module.inference_conv_ksplit = "auto"
    dp._sync_replicas(2)
    assert rep.inference_conv_ksplit == "auto"
    dp.module.inference_conv_ksplit = "off"
    dp._sync_replicas(2)
    assert rep.inference_conv_ksplit == "off"
