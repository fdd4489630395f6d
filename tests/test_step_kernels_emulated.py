"""CPU suite of the training-step kernels: the fused losses, Adam / SGD, SoftArgmax and the glue kernels of csrc/elementwise.hip and
csrc/softargmax.hip compiled unchanged against the SIMT emulator, held to the float64 references and rounding budgets of step_checks."""
import pytest

import step_checks as sc
from emu_util import emulated_hip


@pytest.fixture(scope="module")
def emu():
    with emulated_hip() as lib:
        yield lib


VIEW_IDS = {False: "aligned", True: "view"}


@pytest.mark.parametrize("kind", ["mse", "huber"])
@pytest.mark.parametrize("n", sc.LOSS_SIZES)
def test_loss_against_float64(emu, kind, n):
    sc.check_loss("cpu", kind, n)


@pytest.mark.parametrize("kind", ["mse", "huber"])
def test_loss_on_a_stacked_output_and_an_expanded_target(emu, kind):
    sc.check_loss_stacked_target("cpu", kind)


@pytest.mark.parametrize("kind", ["mse", "huber"])
def test_loss_modules_hand_autograd_the_kernel_gradient(emu, kind):
    sc.check_loss_module("cpu", kind)


@pytest.mark.parametrize("view", [False, True], ids=VIEW_IDS.get)
@pytest.mark.parametrize("n", sc.LOSS_SIZES)
def test_adam_kernel_sizes(emu, n, view):
    hyper = sc.ADAM_HYPER[sc.LOSS_SIZES.index(n) % len(sc.ADAM_HYPER)]
    for p_init in ("zero", "randn"):
        sc.check_adam_kernel("cpu", n, view=view, hyper=hyper, p_init=p_init)


@pytest.mark.parametrize("mode", ["classes", "random"])
@pytest.mark.parametrize("hyper", sc.ADAM_HYPER, ids=lambda h: "lr%g-b%g-%g-eps%g" % h)
def test_adam_kernel_hyper_parameters(emu, hyper, mode):
    for view in (False, True):
        for p_init in ("zero", "randn"):
            sc.check_adam_kernel("cpu", 1003, view=view, hyper=hyper, p_init=p_init, mode=mode, seed=1)


@pytest.mark.parametrize("view", [False, True], ids=VIEW_IDS.get)
def test_adam_kernel_zero_gradient_moves_nothing(emu, view):
    for n in (3, 1003):
        sc.check_adam_zero_gradient("cpu", n, view=view)


@pytest.mark.parametrize("view", [False, True], ids=VIEW_IDS.get)
@pytest.mark.parametrize("n", sc.LOSS_SIZES)
def test_sgd_kernel_sizes(emu, n, view):
    sc.check_sgd_kernel("cpu", n, view=view)


@pytest.mark.parametrize("case", sc.OPT_CASES)
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_optimizers_against_torch_optim(emu, kind, case):
    sc.check_optimizer("cpu", kind, case)


@pytest.mark.parametrize("size_mult", [1.0, 2.5])
@pytest.mark.parametrize("hw", sc.SOFTARGMAX_MAPS, ids=lambda s: "%dx%d" % s)
def test_softargmax_distinct_betas(emu, hw, size_mult):
    sc.check_softargmax_distinct_betas("cpu", hw, size_mult)


def test_softargmax_large_values_stay_finite(emu):
    sc.check_softargmax_large_values("cpu")


def test_softargmax_constant_map(emu):
    sc.check_softargmax_constant_map("cpu")


@pytest.mark.parametrize("n", [1, 3, 1003, 2097153])
def test_add(emu, n):
    sc.check_add("cpu", n)


def test_float4_kernels_refuse_misaligned_pointers(emu):
    sc.check_alignment_contract("cpu")


@pytest.mark.parametrize("up", [1, 2, 4])
@pytest.mark.parametrize("k,cpad", [(7, 16), (7, 32), (17, 32)])
def test_stage_input_and_its_backward(emu, k, cpad, up):
    sc.check_stage_input("cpu", up, k, cpad)


def test_stage_input_refuses_narrow_padding(emu):
    sc.check_stage_input_refuses_narrow_padding("cpu")


@pytest.mark.parametrize("n", [1, 3, 1003, 1030])
def test_relu_bwd(emu, n):
    sc.check_relu_bwd("cpu", n)


@pytest.mark.parametrize("shape", [(2, 6, 10, 8), (1, 2, 2, 4)], ids=lambda s: "x".join(str(v) for v in s))
def test_upsample2_bwd(emu, shape):
    sc.check_upsample2_bwd("cpu", shape)


@pytest.mark.parametrize("hw", sorted(sc.LAYOUT_HW))
@pytest.mark.parametrize("c", sc.LAYOUT_C)
def test_layout_conversions(emu, c, hw):
    sc.check_layout("cpu", c, hw)


def test_multi_copy(emu):
    sc.check_multi_copy("cpu")
