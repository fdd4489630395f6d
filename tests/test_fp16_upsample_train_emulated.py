"""CPU suite of DreamHourglass's train_upsample_precision="fp16": wgrad_convT4_f16_xs_kernel and the folding reduce of csrc/wgrad_f16.hip,
and the forward / data-gradient forms of csrc/conv_f16.hip as the switch launches them, compiled unchanged against the SIMT emulator
(bounds: fp16_upsample_train_checks); the switch on the host; the yardsticks of the GPU suite recomputed on the CPU reference."""
import os

import pytest
import torch

import fp16_upsample_train_checks as uc
import launch_trace as lt
from dream_amd import models, ops
from emu_util import emulated_hip

_FULL = os.environ.get("DREAM_EMU_FULL", "0") == "1"
_ids = lambda s: "x".join(str(v) for v in s)      # noqa: E731


@pytest.fixture(scope="module")
def emu():
    with emulated_hip() as lib:
        yield lib


@pytest.mark.parametrize("scales", uc.SCALES, ids=("unit", "x2^-16", "x2^10"))
@pytest.mark.parametrize("shape", uc.SHAPES, ids=_ids)
def test_wgrad(emu, shape, scales):
    _, split = uc.check_wgrad("cpu", shape, *scales)
    assert split == (2 if shape[1] == 5 else 1)


def test_zero_gradient_gives_exact_zeros(emu):
    uc.check_wgrad("cpu", uc.SHAPES[1], zero_dz=True)
    uc.check_dgrad("cpu", uc.SHAPES[1], zero_dz=True)


def test_split_weight_gradient_repeats_bit_for_bit(emu):
    uc.check_repeat("cpu")


def test_fold_is_the_adjoint_of_the_collapse(emu):
    uc.check_fold("cpu")


@pytest.mark.parametrize("shape", uc.SHAPES, ids=_ids)
def test_forward(emu, shape):
    uc.check_forward("cpu", shape)


@pytest.mark.parametrize("shape", uc.SHAPES + [uc.SPLIT_SHAPE], ids=_ids)
def test_dgrad(emu, shape):
    uc.check_dgrad("cpu", shape)


@pytest.mark.parametrize("variant", range(uc.NUM_VARIANTS))
def test_dgrad_on_every_tile(emu, variant):
    uc.check_dgrad("cpu", uc.VARIANT_SHAPE, variant=variant)


def test_refusals(emu):
    uc.check_refusals("cpu")


def test_one_block_emulated(emu):
    uc.check_block("cpu")


@pytest.mark.skipif(not _FULL, reason="set DREAM_EMU_FULL=1 (minutes under the emulator); the GPU suite runs the training step")
def test_whole_step_emulated(emu):
    uc.check_step("cpu")
    uc.check_uncovered_entries_bit_equal("cpu")
    uc.check_default_untouched("cpu")


# ---- the switch ---------------------------------------------------------------------------------------------------------------------------
def _meta_net(cls=models.DreamHourglass, **kw):
    return cls(7, **kw).to("meta")


def _forward(net, training, mp):
    rec = lt.Recorder()
    rec.install(mp, ops)
    net.train(training)
    x = torch.empty((2, 3, 64, 96), device="meta")
    with torch.no_grad():
        return net.run_forward(x, [p.detach() for p in net.plan_parameters()], training)


def test_switch_is_an_instance_attribute(monkeypatch):
    a, b = _meta_net(), _meta_net()
    assert a.train_upsample_precision == "fp32"
    a.train_upsample_precision = a.train_precision = "fp16"
    assert a.train_upsample_precision == "fp16" and b.train_upsample_precision == "fp32"
    assert a._resolve_switches(True).ups16 and not b._resolve_switches(True).ups16
    _, saved = _forward(a, True, monkeypatch)
    layers = a.plan_layers()
    covered = [li for li, (kind, mod, flags) in enumerate(layers) if uc.is_covered(kind, mod, flags)]
    assert len(covered) == 2 and all(li in saved.half and saved.half[li] is not None for li in covered)
    assert not a._resolve_switches(False).ups16
    _forward(a, False, monkeypatch)                       # inference ignores a known value


def test_unknown_value_raises_in_the_training_pass(monkeypatch):
    net = _meta_net()
    net.train_upsample_precision = "bf16"
    with pytest.raises(ValueError, match="unknown train_upsample_precision 'bf16'"):
        _forward(net, True, monkeypatch)


def test_fp16_needs_train_precision(monkeypatch):
    net = _meta_net()
    net.train_upsample_precision = "fp16"
    with pytest.raises(ValueError, match="train_upsample_precision=\"fp16\" needs train_precision=\"fp16\""):
        _forward(net, True, monkeypatch)
    net.train_precision = "fp16"
    _forward(net, True, monkeypatch)


def test_multi_stage_forwards_the_switch():
    net = models.DreamHourglassMultiStage(7, internalize_spatial_softmax=False, n_stages=2).to("meta")
    assert net.train_upsample_precision == "fp32"
    net.train_upsample_precision = "fp16"
    assert [st.train_upsample_precision for st in net.stages()] == ["fp16", "fp16"] and net.train_upsample_precision == "fp16"


def test_resnet_refuses_the_mode():
    switch = models.ResnetSimple.__dict__["train_upsample_precision"]
    assert type(switch) is models._FixedSwitch and switch.value == "fp32"
    obj = models.ResnetSimple.__new__(models.ResnetSimple)
    assert obj.train_upsample_precision == "fp32"
    obj.train_upsample_precision = "fp32"
    with pytest.raises(ValueError, match="train_upsample_precision='fp16' is not supported"):
        obj.train_upsample_precision = "fp16"


def test_hip_graph_train_refuses_the_mode():
    import parity_checks as pc
    net = pc.build_network("vgg_q", "cpu")
    net.model.module.train_upsample_precision = "fp16"
    with pytest.raises(ValueError, match="hip_graph_train does not replay train_upsample_precision='fp16'"):
        net.hip_graph_train = True
    net.model.single_device_graphs = True                 # ... and where the environment switched the graphs on
    net.model.module.train()
    with pytest.raises(ValueError, match="train_upsample_precision"):
        net.model(torch.zeros(1, 3, 64, 64))
    net.model.single_device_graphs = False
    net.model.module.train_upsample_precision = "fp32"
    net.hip_graph_train = False


def test_replicas_follow_the_switch(emu, monkeypatch):
    """Two emulated devices, training mode: a replica made before the switch moved takes the master's value at the next _sync_replicas,
    in both directions."""
    import parity_checks as pc
    monkeypatch.setenv("DREAM_DP_EMULATED_DEVICES", "2")
    net = pc.build_network("vgg_q", "cpu", in_res=(32, 32))
    net.enable_training()
    dp = net.model
    dp._ensure_replicas(2)
    rep = dp._replicas[0]
    assert rep is not dp.module and rep.training and rep.train_upsample_precision == "fp32"
    dp.module.train_precision = dp.module.train_upsample_precision = "fp16"
    dp._sync_replicas(2)
    assert rep.train_upsample_precision == "fp16" and rep._resolve_switches(True).ups16
    dp.module.train_upsample_precision = "fp32"
    dp._sync_replicas(2)
    assert rep.train_upsample_precision == "fp32" and not rep._resolve_switches(True).ups16


# ---- the yardsticks of the GPU suite, recomputed on the CPU reference -----------------------------------------------------------------
def test_block_yardstick_is_a_rounding_distance():
    E = uc.block_yardstick()
    assert set(E) == {"dx", "dW", "dbias"}
    assert all(1e-5 < e < 0.1 for e in E.values()), E


def test_step_yardstick_is_a_rounding_distance():
    E, ncov = uc.rounded_training_oracle((24, 16))
    assert ncov == 2 and all(1e-5 < e < 0.1 for e in E.values()), E


@pytest.mark.parametrize("optimizer", ("adam", "sgd"))
def test_training_gap_constants_hold(optimizer):
    gap = uc.rounded_training_gap(optimizer, (24, 16))
    want = uc.TRAIN_GAP[optimizer]
    assert want / 2 <= gap <= 1.25 * want, (gap, want)
