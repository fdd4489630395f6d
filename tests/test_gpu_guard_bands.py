"""GPU suite of the guard-band harness (tests/guard_band_checks.py): its self-tests on device memory (plain torch, no kernel), and every
entry of its case table -- an existing check of a kernel family on the real libdream_hip.so -- inside poisoned arenas under both
alignments: no store outside an output or workspace, no over-read that reaches the arithmetic, no element left unwritten."""
import pytest
import torch

import guard_band_checks as gb
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


@pytest.mark.parametrize("selfcheck", gb.SELFCHECKS, ids=lambda f: f.__name__)
def test_harness(selfcheck):
    selfcheck(DEV)


@pytest.mark.parametrize("skew", gb.SKEWS, ids=lambda s: "skew%d" % s)
@pytest.mark.parametrize("name", gb.CASE_IDS)
def test_guarded(name, skew):
    assert gb.run_case(DEV, name, skew) > 0
