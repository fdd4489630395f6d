"""GPU suite (the real library through the C ABI) for the front of the VGG encoder: the first conv with dwordx4 stores and persistent
workgroups, the narrow workgroup shape of the F(4x4,3x3) kernel on its paired weight layout, and that layout itself."""
import itertools

import pytest

import front_conv_checks as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("mode", fc.NARROW_MODES)
@pytest.mark.parametrize("size", fc.NARROW_SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_narrow_winograd4(size, mode):
    """Every (size, mode) at every input depth and both row counts."""
    for seed, (cin, cout) in enumerate(itertools.product(fc.NARROW_CIN, fc.NARROW_COUT)):
        fc.check_narrow_winograd4(DEV, size, cin, cout, mode, seed=seed)


@pytest.mark.parametrize("cout,cin,mode", [(48, 16, 0), (64, 32, 0), (64, 64, 0), (7, 16, 0), (64, 48, 1), (128, 16, 1)])
def test_narrow_pack_layout(cout, cin, mode):
    fc.check_narrow_pack_layout(DEV, cout, cin, mode, seed=cout + cin)


def test_narrow_pack_batched_equals_lazy():
    fc.check_narrow_pack_batched_equals_lazy(DEV)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("size", fc.FIRST_SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_first_conv(size, relu):
    for seed, (cin, cout) in enumerate(itertools.product(fc.FIRST_CIN, fc.FIRST_COUT)):
        fc.check_first_conv(DEV, size, cin, cout, relu, seed=seed)
