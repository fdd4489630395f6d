"""CPU suite of the guard-band harness (tests/guard_band_checks.py): its self-tests, and every entry of its case table -- an existing check
of a kernel family, compiled unchanged against the SIMT emulator -- inside poisoned arenas under both alignments."""
import pytest

import guard_band_checks as gb
from emu_util import emulated_hip


@pytest.fixture(scope="module")
def emu():
    with emulated_hip() as lib:
        yield lib


@pytest.mark.parametrize("selfcheck", gb.SELFCHECKS, ids=lambda f: f.__name__)
def test_harness(selfcheck):
    selfcheck("cpu")


@pytest.mark.parametrize("skew", gb.SKEWS, ids=lambda s: "skew%d" % s)
@pytest.mark.parametrize("name", gb.CASE_IDS)
def test_guarded(emu, name, skew):
    assert gb.run_case("cpu", name, skew) > 0
