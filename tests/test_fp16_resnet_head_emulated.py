"""CPU suite of ResnetSimple.inference_head_fusion="on": convT4_head_f16_kernel (csrc/conv_head_f16.hip: the act16 main loop with the
head's GEMM as its epilogue) compiled unchanged against the SIMT emulator, through dream_amd.ops / models; the host behaviour on the
``meta`` device.  Bounds and what is compared bit for bit: see fp16_resnet_head_checks."""
import pytest
import torch

import fp16_resnet_head_checks as rh
import parity_checks as pc
from dream_amd import _hip, data_parallel, models
from emu_util import emulated_hip
from oracle import models as om
from test_fp16_resnet_storage_emulated import NETWORKS, _trace
from test_fp16_resnet_storage_emulated import _meta_net as _storage_meta_net


@pytest.fixture(scope="module")
def emu():
    with emulated_hip() as lib:
        yield lib


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    """The meta networks are shared with the other suites of this process: none of them leaves here with the switch on."""
    yield
    for name in NETWORKS:
        _storage_meta_net(name).inference_head_fusion = "off"
        _storage_meta_net(name).inference_conv_ksplit = "off"


# ---- the fused entry, per launch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("case", rh.LAUNCH_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_fused_launch_is_the_two_launches_bit_for_bit(emu, case, relu):
    rh.check_launch("cpu", *case, relu=relu, seed=case[1])


def test_the_unfused_variant_does_not_matter(emu):
    """The stage launch of the pair on every tile of the variant table: the fused entry equals each (the order of a pixel's stages does
    not depend on the tile)."""
    for variant in (0, 1, 3, 4):
        emu.dream_conv_f16_set_variant(variant)
        try:
            rh.check_launch("cpu", 1, 9, 6, 32, 5, seed=variant)
        finally:
            emu.dream_conv_f16_set_variant(-1)


def test_saturation_is_finite_and_reported(emu):
    rh.check_saturation("cpu")


def test_refusals(emu):
    rh.check_refusals("cpu")


def test_symbols_resolve(emu):
    for name in (rh.FUSED, "dream_conv_transpose4x4s2_head_f16_applies"):
        assert name in _hip._SIGNATURES and name in _hip.header_functions()
        assert getattr(emu, name) is not None
    assert emu.dream_conv_transpose4x4s2_head_f16_applies(256, 256, 17) == 1
    assert emu.dream_conv_transpose4x4s2_head_f16_applies(256, 256, 0) == 0
    assert emu.dream_conv_transpose4x4s2_head_f16_applies(0, 256, 7) == 0


# ---- the walk: the decoder at the smallest input it allows ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,full", [(7, False), (17, True)], ids=["resnet_h", "resnet_f"])
def test_decoder_walk_on_is_off_bit_for_bit(emu, k, full):
    rh.check_decoder_walk("cpu", k, full)


def test_33_keypoints_run_the_unfused_launches(emu):
    names = rh.check_decoder_walk("cpu", 33, False, seed=2)
    assert rh.FUSED not in names


# ---- host behaviour: no kernel runs (meta device) ------------------------------------------------------------------------------------
def _meta_net(name, fusion="on"):
    net = _storage_meta_net(name)
    net.precision = net.inference_activation_storage = "fp16"
    net.inference_head_fusion = fusion
    return net


def test_switch_is_an_instance_attribute_with_a_default():
    a, b = models.ResnetSimple(pretrained=False), _storage_meta_net("h")
    assert a.inference_head_fusion == "off" and "inference_head_fusion" in a.__dict__
    assert not hasattr(models.ResnetSimple, "inference_head_fusion")
    a.inference_head_fusion = "on"
    assert b.inference_head_fusion == "off"


def test_value_errors(monkeypatch):
    net = _storage_meta_net("h")
    net.inference_head_fusion = "on"
    for precision, storage in (("fp32", "fp32"), ("fp16x3", "fp32"), ("fp16", "fp32")):
        net.precision, net.inference_activation_storage = precision, storage
        with pytest.raises(ValueError, match="inference_head_fusion.*precision.*inference_activation_storage"):
            _trace(net, (1, 64, 64), monkeypatch)
        _trace(net.train(), (2, 64, 96), monkeypatch, training=True)                 # (a training pass does not look at the needs)
        net.eval()
    net.precision = net.inference_activation_storage = "fp16"
    net.inference_head_fusion = "auto"
    for training in (False, True):
        with pytest.raises(ValueError, match="unknown inference_head_fusion"):
            _trace(net.train(training), (2, 64, 96), monkeypatch, training=training)
    net.eval()


def test_the_hourglasses_refuse_the_switch():
    for net in (models.DreamHourglass(7), models.DreamHourglassMultiStage(7, n_stages=2)):
        assert net.inference_head_fusion == "off"
        net.inference_head_fusion = "off"
        with pytest.raises(ValueError, match="inference_head_fusion='on' is not supported"):
            net.inference_head_fusion = "on"


def test_training_ignores_the_switch(monkeypatch):
    net = _storage_meta_net("h")
    _, train_off, _ = _trace(net.train(), (2, 64, 96), monkeypatch, training=True)
    net = _meta_net("h", "on")
    _, train_on, _ = _trace(net.train(), (2, 64, 96), monkeypatch, training=True)
    net.eval()
    assert train_on == train_off
    assert not [l for l in train_on if l.split(" ", 1)[0] == rh.FUSED]


def test_the_fused_launch_gets_the_peak_and_writes_the_maps(monkeypatch):
    net = _meta_net("f", "on")
    out, launches, tensors = _trace(net, (2, 70, 93), monkeypatch)
    assert launches[-1].split(" ", 1)[0] == rh.FUSED and out.dtype == torch.float32
    acts = [t for t in tensors[-1] if t.dim() == 4 and int(t.shape[0]) == 2]
    assert [t.dtype for t in acts] == [torch.float16, torch.float32] and acts[-1] is out
    assert any(t is net._storage_peak._last for t in tensors[-1])
    # no half tensor of the last stage's output shape was handed to any launch
    b, k, ho, wo = (int(v) for v in out.shape)
    assert not [t for ts in tensors for t in ts if tuple(t.shape) == (b, ho, wo, 256)]


def test_replica_settings_and_graph_key_carry_the_switch():
    net = models.ResnetSimple(pretrained=False)
    off = data_parallel._settings(net)
    net.inference_head_fusion = "on"
    assert data_parallel._settings(net) != off and "on" in data_parallel._settings(net)


def test_replicas_follow_the_switch(emu, monkeypatch):
    """Two emulated devices: a replica made before the switch moved takes the master's value at the next _sync_replicas."""
    monkeypatch.setenv("DREAM_DP_EMULATED_DEVICES", "2")
    wts = om.recipe_weights(om.build_model("resnet_h", 7).state_dict())
    net = pc.build_network("resnet_h", "cpu", weights=wts, in_res=(32, 32))
    net.enable_evaluation()
    dp = net.model
    dp._ensure_replicas(2)
    rep = dp._replicas[0]
    assert rep is not dp.module and rep.inference_head_fusion == "off"
    dp.module.precision = dp.module.inference_activation_storage = "fp16"
    dp.module.inference_head_fusion = "on"
    dp._sync_replicas(2)
    assert rep.inference_head_fusion == "on"
    dp.module.inference_head_fusion = "off"
    dp._sync_replicas(2)
    assert rep.inference_head_fusion == "off"
