"""GPU suite: the launches of train_upsample_precision="fp16" inside the poisoned arenas of the guard-band harness (guard_band_checks), under
both alignments -- the new weight-gradient entry point, split and unsplit, with its folding reduce, and the data-gradient / forward launches
as the mode calls them: no store outside an output or workspace, no over-read that reaches the arithmetic, no element left unwritten."""
import pytest
import torch

import fp16_upsample_train_checks as uc
import guard_band_checks as gb
from dream_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = {
    "wgrad_unsplit": lambda dev: uc.check_wgrad(dev, uc.SHAPES[2]),
    "wgrad_two_tiles": lambda dev: uc.check_wgrad(dev, uc.SHAPES[1], 2.0 ** -16, 1e-6),
    "wgrad_split": lambda dev: uc.check_wgrad(dev, uc.SPLIT_SHAPE),
    "fold": uc.check_fold,
    "dgrad": lambda dev: uc.check_dgrad(dev, uc.SHAPES[1]),
    "forward": lambda dev: uc.check_forward(dev, uc.SHAPES[1]),
}


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_library():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    _hip.check_symbols()
    with open("/proc/self/maps") as f:
        assert "libdream_hip.so" in f.read(), "the native HIP library is not loaded"
    yield


def run_guarded(dev, name, skew):
    with gb.guarded(dev, skew) as arena:
        try:
            CASES[name](dev)
        except AssertionError as err:
            found = arena.violations()
            if found:
                raise AssertionError("%s\nand guard bands touched:\n  %s" % (err, "\n  ".join(found))) from err
            raise
        arena.assert_intact()
        return len(arena.blocks)


@pytest.mark.parametrize("skew", gb.SKEWS, ids=lambda s: "skew%d" % s)
@pytest.mark.parametrize("name", sorted(CASES))
def test_guarded(name, skew):
    assert run_guarded(DEV, name, skew) > 0
