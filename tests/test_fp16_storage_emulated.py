"""CPU suite of activation_storage="fp16": the half-storage kernels (csrc/conv_f16.hip ACT16, conv_first.hip, elementwise.hip) compiled
unchanged against the SIMT emulator, through dream_amd.ops / models; the host behaviour on the ``meta`` device.  Bounds: see
fp16_storage_checks (derived per launch, measured on the reference end to end)."""
import os
import warnings

import pytest
import torch

import fp16_storage_checks as sc
import launch_trace as lt
from dream_amd import models, ops
from emu_util import emulated_hip

NUM_VARIANTS = 8
_FULL = os.environ.get("DREAM_EMU_FULL", "0") == "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    with emulated_hip() as lib:
        yield lib


@pytest.mark.parametrize("variant", list(range(NUM_VARIANTS)) + [-1])
def test_half_storage_launches(emu, variant):
    emu.dream_conv_f16_set_variant(variant)
    try:
        sc.check_launches("cpu", seed=max(variant, 0))
    finally:
        emu.dream_conv_f16_set_variant(-1)


def test_half_storage_transposed4x4(emu):
    sc.check_conv_transpose("cpu", 4, 1, 5, 6, 32, 48)


def test_saturation_is_finite_and_reported(emu):
    sc.check_saturation("cpu")


def test_first_conv_maxpool_add(emu):
    sc.check_first_conv("cpu")
    sc.check_maxpool("cpu")
    sc.check_add("cpu")


def test_wrappers_refuse_other_dtypes(emu):
    x = torch.zeros(1, 4, 4, 32)
    with pytest.raises(RuntimeError, match="expected float16"):
        ops.maxpool2_f16(x)
    with pytest.raises(RuntimeError, match="expected float16"):
        ops.add_f16(x.half(), x)
    with pytest.raises(RuntimeError, match="expected float32"):
        ops.maxpool2(x.half())


def test_vgg_q_golden_half_storage(emu):
    sc.check_golden("cpu", "vgg_q", (1, 50, 75), with_fp32=False)


@pytest.mark.skipif(not _FULL, reason="set DREAM_EMU_FULL=1 (minutes under the emulator); the GPU suite runs these on the device")
def test_skip_variant_half_storage(emu):
    sc.check_golden("cpu", "vgg_f_skip", (1, 48, 64))


@pytest.mark.skipif(not _FULL, reason="set DREAM_EMU_FULL=1 (minutes under the emulator); the GPU suite runs the structured cases")
@pytest.mark.parametrize("case", ["vgg_q", "vgg_f"])
def test_structured_half_storage(emu, case):
    sc.check_structured("cpu", case)


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


def _meta_net(**variant):
    with pytest.MonkeyPatch.context() as mp, warnings.catch_warnings():
        mp.setenv("DREAM_VGG19_WEIGHTS", os.path.join(ROOT, "tests", "golden", "no-such-weights.pth"))
        warnings.simplefilter("ignore")
        net = models.DreamHourglass(7, internalize_spatial_softmax=False, **variant)
    return net.to("meta")


def _trace(net, shape, monkeypatch, save=False):
    rec = _Recorder()
    rec.install(monkeypatch, ops)
    b, h, w = shape
    out, _ = net.run_forward(torch.empty((b, 3, h, w), device="meta"), [p.detach() for p in net.plan_parameters()], save)
    keep = [i for i, l in enumerate(rec.launches) if not lt.is_pack(l)]
    return out, [rec.launches[i].split(" ", 1)[0] for i in keep], [rec.tensors[i] for i in keep]


HALF_ENTRY_POINTS = {"dream_conv2d_f16_nhwc_f16", "dream_conv_transpose4x4s2_f16_nhwc_f16", "dream_conv_transpose3x3s2_f16_nhwc_f16",
                     "dream_maxpool2_nhwc_f16", "dream_add_f16"}


@pytest.mark.parametrize("variant,shape", [({}, (3, 400, 400)), (dict(deconv_decoder=True, skip_connections=True), (3, 96, 128))])
def test_every_launch_between_the_ends_is_half_storage(variant, shape, monkeypatch):
    net = _meta_net(**variant)
    net.precision, net.activation_storage = "fp16", "fp16"
    out, names, tensors = _trace(net, shape, monkeypatch)
    assert out.dtype == torch.float32 and out.shape[:2] == (shape[0], 7)
    assert names[0] == "dream_conv3x3_first_nchw_f16" and names[-1] == "dream_conv2d_f16_nhwc_f16"
    assert set(names[1:]) <= HALF_ENTRY_POINTS, sorted(set(names[1:]) - HALF_ENTRY_POINTS)
    if variant:
        assert "dream_add_f16" in names and "dream_conv_transpose3x3s2_f16_nhwc_f16" in names and "dream_maxpool2_nhwc_f16" in names
    else:
        assert names.count("dream_conv_transpose4x4s2_f16_nhwc_f16") == 2 and names.count("dream_maxpool2_nhwc_f16") == 2
    acts = [[t for t in ts if t.dim() == 4 and int(t.shape[0]) == shape[0]] for ts in tensors]          # (weight planes: 9 / 4 x 4 first)
    assert [t.dtype for t in acts[0]] == [torch.float32, torch.float16]                                  # image in, half out
    assert [t.dtype for t in acts[-1]] == [torch.float16, torch.float32]                                 # half in, belief maps out
    for name, ts in zip(names[1:-1], acts[1:-1]):
        assert len(ts) >= 2 and all(t.dtype == torch.float16 for t in ts), name


def test_default_and_training_launch_no_half_storage(monkeypatch):
    net = _meta_net()
    net.precision = "fp16"
    _, default, _ = _trace(net, (2, 64, 96), monkeypatch)
    net.activation_storage = "fp16"
    _, train16, _ = _trace(net, (2, 64, 96), monkeypatch, save=True)
    net.precision = net.activation_storage = "fp32"
    _, train32, _ = _trace(net, (2, 64, 96), monkeypatch, save=True)
    assert not [n for n in default + train16 if n in HALF_ENTRY_POINTS or n == "dream_conv3x3_first_nchw_f16"]
    assert train16 == train32


def test_value_errors(monkeypatch):
    net = _meta_net()
    for precision in ("fp32", "fp16x3"):
        net.precision, net.activation_storage = precision, "fp16"
        with pytest.raises(ValueError, match="activation_storage.*precision"):
            _trace(net, (1, 32, 32), monkeypatch)
    net.precision, net.activation_storage = "fp16", "bf16"
    with pytest.raises(ValueError, match="unknown activation_storage"):
        _trace(net, (1, 32, 32), monkeypatch)
    with pytest.MonkeyPatch.context() as mp, warnings.catch_warnings():
        mp.setenv("DREAM_VGG19_WEIGHTS", os.path.join(ROOT, "tests", "golden", "no-such-weights.pth"))
        warnings.simplefilter("ignore")
        multi = models.DreamHourglassMultiStage(7, internalize_spatial_softmax=False, n_stages=2)
        resnet = models.ResnetSimple(7, pretrained=False)
    for other in (multi, resnet):
        assert other.activation_storage == "fp32"
        other.activation_storage = "fp32"
        with pytest.raises(ValueError, match="activation_storage='fp16' is not supported"):
            other.activation_storage = "fp16"
