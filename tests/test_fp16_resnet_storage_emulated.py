"""CPU suite of ResnetSimple.inference_activation_storage="fp16": the residual form of conv_f16_kernel and the four streaming kernels
compiled unchanged against the SIMT emulator, through dream_amd.ops / models; the host behaviour on the ``meta`` device.  Bounds: see
fp16_resnet_storage_checks (derived per launch, measured on the reference end to end)."""
import os

import pytest
import torch

import fp16_resnet_storage_checks as rs
import launch_trace as lt
import parity_checks as pc
from dream_amd import data_parallel, models, ops
from emu_util import emulated_hip
from oracle import models as om

_FULL = os.environ.get("DREAM_EMU_FULL", "0") == "1"


@pytest.fixture(scope="module")
def emu():
    with emulated_hip() as lib:
        yield lib


@pytest.mark.parametrize("variant", list(range(rs.NUM_VARIANTS)) + [-1])
def test_residual_form_launches(emu, variant):
    emu.dream_conv_f16_set_variant(variant)
    try:
        rs.check_residual_launches("cpu", seed=max(variant, 0))
    finally:
        emu.dream_conv_f16_set_variant(-1)


def test_residual_saturation_is_finite_and_reported(emu):
    rs.check_residual_saturation("cpu")


def test_residual_refusals(emu):
    rs.check_residual_refusals("cpu")


def test_gathers_and_pool(emu):
    rs.check_gathers_and_pool("cpu")


@pytest.mark.parametrize("variant", [0, 3, -1])
def test_strided_convs_through_the_gather(emu, variant):
    emu.dream_conv_f16_set_variant(variant)
    try:
        rs.check_strided_convs("cpu", seed=max(variant, 0))
    finally:
        emu.dream_conv_f16_set_variant(-1)


def test_one_bottleneck(emu):
    rs.check_bottleneck("cpu")


@pytest.mark.skipif(not _FULL, reason="set DREAM_EMU_FULL=1 (minutes under the emulator); the GPU suite runs the structured cases")
@pytest.mark.parametrize("case", ["resnet_h", "resnet_f"])
def test_structured_half_storage(emu, case):
    rs.check_structured("cpu", case)


def test_the_yardstick_is_a_rounding_distance():
    """E of the half-storage oracle is the distance half rounding of 108 stored tensors puts between the maps and the golden: a hook
    wired to nothing would give the fp32 reference's ~1e-6."""
    orc = rs.stored_oracle("resnet_f")
    print("half-storage oracle resnet_f: E %.3g, P %.3g px, %d of %d maps left out" % (orc["E"], orc["P"], int((~orc["held"]).sum()), orc["held"].size))
    assert 5e-4 < orc["E"] < 3e-3, orc["E"]
    assert int((~orc["held"]).sum()) <= 2


# ---- host behaviour: no kernel runs (meta device) ------------------------------------------------------------------------------
class _Recorder(lt.Recorder):
    """lt.Recorder that also keeps, per launch, the tensors whose pointers were handed over."""

    def __init__(self):
        super().__init__()
        self.tensors, self._pending = [], []

    def call(self, name, *args):
        super().call(name, *args)
        self.tensors.append(self._pending)
        self._pending = []

    def ptr(self, t):
        if t is not None:
            self._pending.append(t)
        return lt.Recorder.ptr(t)


NETWORKS = {"h": dict(n_keypoints=7, full=False), "f": dict(n_keypoints=17, full=True)}
_nets = {}


def _meta_net(name):
    if name not in _nets:
        _nets[name] = models.ResnetSimple(pretrained=False, **NETWORKS[name]).to("meta")
    net = _nets[name]
    net.precision, net.train_gemm_precision, net.inference_activation_storage = "fp32", "fp32", "fp32"
    data_parallel.reset_weight_caches(net)
    return net.eval()


def _trace(net, shape, monkeypatch, training=False):
    rec = _Recorder()
    rec.install(monkeypatch, ops)
    b, h, w = shape
    x = torch.empty((b, 3, h, w), device="meta")
    with torch.no_grad():
        out = net.run_forward_train(x)[0] if training else net.run_forward(x)
    keep = [i for i, l in enumerate(rec.launches) if not lt.is_pack(l)]
    return out, [rec.launches[i] for i in keep], [rec.tensors[i] for i in keep]


HALF_ENTRY_POINTS = {"dream_conv2d_f16_nhwc_f16", "dream_conv2d_f16_res16_nhwc_f16", "dream_conv_transpose4x4s2_f16_nhwc_f16",
                     "dream_maxpool3s2_nhwc_f16", "dream_subsample2_nhwc_f16", "dream_im2col3s2_nhwc_f16"}


@pytest.mark.parametrize("name,shape", [("h", (3, 400, 400)), ("f", (2, 70, 93))])
def test_every_launch_between_the_ends_is_half_storage(name, shape, monkeypatch):
    net = _meta_net(name)
    net.precision, net.inference_activation_storage = "fp16", "fp16"
    out, launches, tensors = _trace(net, shape, monkeypatch)
    names = [l.split(" ", 1)[0] for l in launches]
    assert out.dtype == torch.float32
    assert tuple(out.shape) == (shape[0], NETWORKS[name]["n_keypoints"]) + tuple(net.output_resolution((shape[2], shape[1])))[::-1]
    names = [n for n in names if n != "dream_bn_fold_f32"]                    # (the lazy BatchNorm folds: parameters, not activations)
    tensors = [ts for l, ts in zip(launches, tensors) if not l.startswith("dream_bn_fold_f32")]
    assert names[0] == "dream_im2col_nchw_f16" and names[-1] == "dream_conv2d_f16_nhwc_f16"
    assert set(names[1:]) <= HALF_ENTRY_POINTS, sorted(set(names[1:]) - HALF_ENTRY_POINTS)
    assert names.count("dream_conv2d_f16_res16_nhwc_f16") == 33 and names.count("dream_subsample2_nhwc_f16") == 3
    assert names.count("dream_im2col3s2_nhwc_f16") == 3 and names.count("dream_maxpool3s2_nhwc_f16") == 1
    assert names.count("dream_conv_transpose4x4s2_f16_nhwc_f16") == (5 if NETWORKS[name]["full"] else 4)
    assert names.count("dream_conv2d_f16_nhwc_f16") == 1 + 33 * 2 + 4 + 1        # stem, conv1 / conv2, downsample, head
    acts = [[t for t in ts if t.dim() == 4 and int(t.shape[0]) == shape[0]] for ts in tensors]
    assert [t.dtype for t in acts[0]] == [torch.float32, torch.float16]                                  # image in, half rows out
    assert [t.dtype for t in acts[-1]] == [torch.float16, torch.float32]                                 # half in, belief maps out
    for n, ts in zip(names[1:-1], acts[1:-1]):
        assert len(ts) >= 2 and all(t.dtype == torch.float16 for t in ts), n
    # every half-writing launch is handed the module's one peak scalar (the gathers and the pool round nothing)
    peak = net._storage_peak._last
    for n, ts in zip(names[:-1], tensors[:-1]):
        if n not in ("dream_maxpool3s2_nhwc_f16", "dream_subsample2_nhwc_f16", "dream_im2col3s2_nhwc_f16"):
            assert any(t is peak for t in ts), n
    assert not any(t is peak for t in tensors[-1])


@pytest.mark.parametrize("precision", ["fp32", "fp16", "fp16x3"])
def test_fp32_storage_is_the_launch_list_of_the_attribute_never_set(precision, monkeypatch):
    if "never set" not in _nets:                                      # (no caller ever assigns the attribute on this one)
        _nets["never set"] = models.ResnetSimple(pretrained=False, **NETWORKS["h"]).to("meta").eval()
    fresh = _nets["never set"]
    fresh.precision = precision
    data_parallel.reset_weight_caches(fresh)
    _, never_set, _ = _trace(fresh, (2, 70, 93), monkeypatch)
    net = _meta_net("h")
    net.precision, net.inference_activation_storage = precision, "fp32"
    _, fp32, _ = _trace(net, (2, 70, 93), monkeypatch)
    assert fp32 == never_set and len(fp32) > 100
    new = (HALF_ENTRY_POINTS | {"dream_im2col_nchw_f16"}) - {"dream_conv2d_f16_nhwc_f16", "dream_conv_transpose4x4s2_f16_nhwc_f16"}
    assert not [l for l in fp32 if l.split(" ", 1)[0] in new]


def test_switch_is_an_instance_attribute_with_a_default():
    a, b = models.ResnetSimple(pretrained=False), _meta_net("h")
    assert a.inference_activation_storage == "fp32" and "inference_activation_storage" in a.__dict__
    assert not hasattr(models.ResnetSimple, "inference_activation_storage")
    a.inference_activation_storage = "fp16"
    assert b.inference_activation_storage == "fp32"
    with pytest.raises(RuntimeError, match="no forward with inference_activation_storage"):
        a.half_storage_peak()


def test_value_errors(monkeypatch):
    net = _meta_net("h")
    for precision in ("fp32", "fp16x3"):
        net.precision, net.inference_activation_storage = precision, "fp16"
        with pytest.raises(ValueError, match="inference_activation_storage.*precision"):
            _trace(net, (1, 64, 64), monkeypatch)
    net.precision, net.inference_activation_storage = "fp16", "bf16"
    for training in (False, True):
        with pytest.raises(ValueError, match="unknown inference_activation_storage"):
            _trace(net, (1, 64, 64), monkeypatch, training=training)
    # the hourglass's name stays what it was on this class: fixed, refusing
    assert net.activation_storage == "fp32"
    net.activation_storage = "fp32"
    with pytest.raises(ValueError, match="activation_storage='fp16' is not supported"):
        net.activation_storage = "fp16"


def test_training_ignores_the_switch(monkeypatch):
    net = _meta_net("h")
    net.precision = "fp16"
    _, train32, _ = _trace(net.train(), (2, 64, 96), monkeypatch, training=True)
    net = _meta_net("h")
    net.precision, net.inference_activation_storage = "fp16", "fp16"
    _, train16, _ = _trace(net.train(), (2, 64, 96), monkeypatch, training=True)
    net.eval()
    assert train16 == train32
    assert not [l for l in train16 if l.split(" ", 1)[0] in HALF_ENTRY_POINTS]


def test_graph_keys_follow_the_switch():
    net = models.ResnetSimple(pretrained=False)
    before = data_parallel._settings(net)
    net.inference_activation_storage = "fp16"
    assert data_parallel._settings(net) != before


def test_replicas_follow_the_switch(emu, monkeypatch):
    """Two emulated devices: a replica made before the switch moved takes the master's value at the next _sync_replicas.  (No forward
    runs here -- ResNet-101 takes a minute under the emulator; the GPU suite runs the replicas and compares maps and peaks.)"""
    monkeypatch.setenv("DREAM_DP_EMULATED_DEVICES", "2")
    wts = om.recipe_weights(om.build_model("resnet_h", 7).state_dict())
    net = pc.build_network("resnet_h", "cpu", weights=wts, in_res=(32, 32))
    net.enable_evaluation()
    dp = net.model
    dp._ensure_replicas(2)
    rep = dp._replicas[0]
    assert rep is not dp.module and rep.inference_activation_storage == "fp32" and rep._storage_peak is not dp.module._storage_peak
    dp.module.precision = dp.module.inference_activation_storage = "fp16"
    dp._sync_replicas(2)
    assert rep.inference_activation_storage == "fp16" and rep.precision == "fp16"
    dp.module.inference_activation_storage = "fp32"
    dp._sync_replicas(2)
    assert rep.inference_activation_storage == "fp32"
