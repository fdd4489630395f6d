"""GPU suite of the ragged training steps (ragged_train_checks): whole training steps on the MI355X at resolutions that no pool and no
stride divides -- the fp32 step of every shipped architecture, of the runnable variant and of every plan switch against the oracle with
the launches asserted, two Adam steps twice, hipGraph replay against eager, and the fp16 training modes within their own 3 E_p."""
import pytest
import torch

import ragged_train_checks as rc
from dream_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_library():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    _hip.check_symbols()
    with open("/proc/self/maps") as f:
        assert "libdream_hip.so" in f.read(), "the native HIP library is not loaded"
    yield


def _ids(value):
    return "x".join(str(v) for v in value) if isinstance(value, tuple) else str(value)


@pytest.mark.parametrize("name", sorted(rc.FP32_CASES))
def test_fp32_step_matches_the_oracle(name):
    rc.check_fp32_step(DEV, name)


@pytest.mark.parametrize("name", rc.REFUSED_VARIANTS)
def test_multi_stage_variants_refuse_the_shape_as_the_reference_does(name):
    rc.check_variant_refused(DEV, name)


@pytest.mark.parametrize("arch,shape", [("resnet_h", rc.RESNET_H_SHAPE), ("vgg_q_skip", rc.HOURGLASS_SHAPES[0])], ids=_ids)
def test_two_adam_steps_are_deterministic(arch, shape):
    rc.check_deterministic(DEV, arch, shape)


@pytest.mark.parametrize("arch,shape,split", [("resnet_h", rc.RESNET_H_SHAPE, 0), ("resnet_h", rc.RESNET_H_SHAPE, 7),
                                              ("vgg_q", rc.HOURGLASS_SHAPES[0], 0)], ids=_ids)
def test_graph_replay_equals_eager(arch, shape, split):
    rc.check_graph_replay(DEV, arch, shape, split)


@pytest.mark.parametrize("mode", rc.FP16_CASES)
def test_fp16_mode_within_its_own_yardstick(mode):
    rc.check_fp16_step(DEV, mode)
