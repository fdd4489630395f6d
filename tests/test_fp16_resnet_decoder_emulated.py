"""CPU suite of ResnetSimple's train_decoder_precision="fp16": the convT4 dgrad form of csrc/conv_f16.hip and wgrad_convT4_f16_kernel of
csrc/wgrad_f16.hip compiled unchanged against the SIMT emulator (bounds: fp16_resnet_decoder_checks); the switch on the host; the
yardsticks of the GPU suite recomputed on the CPU reference."""
import pytest
import torch

import fp16_resnet_decoder_checks as dc
import launch_trace as lt
from dream_amd import models, ops
from emu_util import emulated_hip

_ids = lambda s: "x".join(str(v) for v in s)      # noqa: E731


@pytest.fixture(scope="module")
def emu():
    with emulated_hip() as lib:
        yield lib


@pytest.mark.parametrize("shape", dc.SHAPES, ids=_ids)
def test_forward_and_statistics(emu, shape):
    dc.check_forward("cpu", shape)


@pytest.mark.parametrize("shape", dc.SHAPES + [dc.SPLIT_SHAPE], ids=_ids)
def test_dgrad(emu, shape):
    dc.check_dgrad("cpu", shape)


@pytest.mark.parametrize("variant", range(dc.NUM_VARIANTS))
def test_dgrad_on_every_tile(emu, variant):
    dc.check_dgrad("cpu", dc.VARIANT_SHAPE, variant=variant)


@pytest.mark.parametrize("shape", dc.SHAPES, ids=_ids)
def test_wgrad(emu, shape):
    _, split = dc.check_wgrad("cpu", shape)
    assert split == (2 if shape[1] == 5 else 1)          # two 8 x 16 position tiles (one per frame) / a single one


def test_zero_gradient_gives_exact_zeros(emu):
    dc.check_dgrad("cpu", dc.SHAPES[1], zero_dz=True)
    dc.check_wgrad("cpu", dc.SHAPES[1], zero_dz=True)


def test_split_weight_gradient_repeats_bit_for_bit(emu):
    dc.check_repeat("cpu")


def test_scales(emu):
    dc.check_scales("cpu")


def test_batched_pack(emu):
    dc.check_batched_pack("cpu")


def test_bias_gradient_of_the_covered_leaf(emu):
    dc.check_bias_gradient("cpu")


def test_refusals(emu):
    dc.check_refusals("cpu")


def test_one_stage_emulated(emu):
    dc.check_stage("cpu")


def test_small_map_stage_stays_fp32(emu):
    dc.check_small_map_stays_fp32("cpu")


# ---- the switch ---------------------------------------------------------------------------------------------------------------------------
def _meta_net():
    return models.ResnetSimple(7, pretrained=False).to("meta")


def _forward(net, training, mp):
    rec = lt.Recorder()
    rec.install(mp, ops)
    net.train(training)
    x = torch.empty((2, 3, 64, 64), device="meta")
    with torch.no_grad():
        return net.run_forward_train(x) if training else net.run_forward(x)


def test_switch_is_an_instance_attribute(monkeypatch):
    a, b = _meta_net(), _meta_net()
    assert a.train_decoder_precision == "fp32"
    a.train_decoder_precision = "fp16"
    assert a.train_decoder_precision == "fp16" and b.train_decoder_precision == "fp32"
    _forward(a, True, monkeypatch)
    _forward(a, False, monkeypatch)                       # inference ignores a known value


@pytest.mark.parametrize("training", (True, False))
def test_unknown_value_raises_in_both_passes(training, monkeypatch):
    net = _meta_net()
    net.train_decoder_precision = "bf16"
    with pytest.raises(ValueError, match="unknown train_decoder_precision 'bf16'"):
        _forward(net, training, monkeypatch)


def test_fp16_needs_bn_fusion(monkeypatch):
    net = _meta_net()
    net.train_decoder_precision, net.bn_fusion = "fp16", False
    with pytest.raises(ValueError, match="train_decoder_precision=\"fp16\" needs bn_fusion"):
        _forward(net, True, monkeypatch)
    net.train_decoder_precision = "fp32"
    _forward(net, True, monkeypatch)


def test_independent_of_train_gemm_precision(monkeypatch):
    net = _meta_net()
    net.train_decoder_precision, net.train_gemm_precision = "fp16", "fp16"
    walk = net._resolve_switches(True)
    assert walk.dec16 and walk.train16
    net.train_gemm_precision = "fp32"
    walk = net._resolve_switches(True)
    assert walk.dec16 and not walk.train16
    net.train_gemm_precision = "fp16"
    net.CONVT_GEMM_MAX_PIXELS = 0                         # (2 x 64 x 64: every stage would otherwise be a small-map GEMM)
    _, tape = _forward(net, True, monkeypatch)
    assert [r["f16"] for r in tape if r["kind"] == "convT"] == [True] * 4
    assert any(r["kind"] == "conv" and r["f16"] for r in tape)
    with pytest.raises(ValueError):                       # train_precision stays the hourglass's switch, refused here
        net.train_precision = "fp16"


@pytest.mark.parametrize("cls", (models.DreamHourglass, models.DreamHourglassMultiStage))
def test_hourglass_classes_refuse_the_mode(cls):
    switch = cls.__dict__["train_decoder_precision"]         # a _FixedSwitch of the class itself: no instance state is read
    assert type(switch) is models._FixedSwitch and switch.value == "fp32"
    obj = cls.__new__(cls)
    assert obj.train_decoder_precision == "fp32"
    obj.train_decoder_precision = "fp32"
    with pytest.raises(ValueError, match="train_decoder_precision='fp16' is not supported"):
        obj.train_decoder_precision = "fp16"


def test_hip_graph_train_refuses_the_mode():
    import parity_checks as pc
    net = pc.build_network("resnet_h", "cpu")
    net.model.module.train_decoder_precision = "fp16"
    with pytest.raises(ValueError, match="hip_graph_train does not replay train_decoder_precision='fp16'"):
        net.hip_graph_train = True
    net.model.single_device_graphs = True                 # ... and where the environment switched the graphs on
    net.model.module.train()
    with pytest.raises(ValueError, match="train_decoder_precision"):
        net.model(torch.zeros(1, 3, 64, 64))
    net.model.single_device_graphs = False
    net.model.module.train_decoder_precision = "fp32"
    net.hip_graph_train = False


def test_replicas_follow_the_switch(emu, monkeypatch):
    """Two emulated devices, training mode: a replica made before the switch moved takes the master's value at the next _sync_replicas,
    in both directions."""
    import parity_checks as pc
    monkeypatch.setenv("DREAM_DP_EMULATED_DEVICES", "2")
    net = pc.build_network("resnet_h", "cpu", weights=dc.sc._weights(), in_res=(32, 32))
    net.enable_training()
    dp = net.model
    dp._ensure_replicas(2)
    rep = dp._replicas[0]
    assert rep is not dp.module and rep.training and rep.train_decoder_precision == "fp32"
    dp.module.train_decoder_precision = "fp16"
    dp._sync_replicas(2)
    assert rep.train_decoder_precision == "fp16" and rep._resolve_switches(True).dec16
    dp.module.train_decoder_precision = "fp32"
    dp._sync_replicas(2)
    assert rep.train_decoder_precision == "fp32" and not rep._resolve_switches(True).dec16


# ---- the yardsticks of the GPU suite, recomputed on the CPU reference -----------------------------------------------------------------
def test_stage_yardstick_is_a_rounding_distance():
    E = dc.stage_yardstick()
    assert set(E) == {"dx", "dW", "dbias", "dgamma", "dbeta"}
    assert all(1e-5 < e < 0.1 for k, e in E.items() if k != "dbias") and E["dbias"] > 0, E      # (dbias: noise around an exact zero)


@pytest.mark.parametrize("both", (False, True))
def test_step_yardstick_conditions_the_last_decoder_tensors(both):
    E, move = dc.step_yardstick((32, 32), both)
    assert move > 0 and all(0 < E[n] < 0.1 for n in dc.sc.CONDITIONED), (move, {n: E[n] for n in dc.sc.CONDITIONED})


@pytest.mark.parametrize("both", (False, True))
@pytest.mark.parametrize("optimizer", ("adam", "sgd"))
def test_training_gap_constants_hold(optimizer, both):
    gap = dc.rounded_training_gap(optimizer, (32, 32), both)
    want = dc.TRAIN_GAP[optimizer, both]
    assert want / 2 <= gap <= 1.25 * want, (gap, want)
