"""GPU suite (-m gpu) of the training-step kernels: the fused losses, Adam / SGD, SoftArgmax and the glue kernels of
csrc/elementwise.hip and csrc/softargmax.hip on an MI355X, held to the float64 references and rounding budgets of step_checks."""
import pytest
import torch

import step_checks as sc
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


VIEW_IDS = {False: "aligned", True: "view"}


@pytest.mark.parametrize("kind", ["mse", "huber"])
@pytest.mark.parametrize("n", sc.LOSS_SIZES)
def test_loss_against_float64(kind, n):
    sc.check_loss(DEV, kind, n)


@pytest.mark.parametrize("kind", ["mse", "huber"])
def test_loss_on_a_stacked_output_and_an_expanded_target(kind):
    sc.check_loss_stacked_target(DEV, kind)


@pytest.mark.parametrize("kind", ["mse", "huber"])
def test_loss_modules_hand_autograd_the_kernel_gradient(kind):
    sc.check_loss_module(DEV, kind)


@pytest.mark.parametrize("view", [False, True], ids=VIEW_IDS.get)
@pytest.mark.parametrize("n", sc.LOSS_SIZES)
def test_adam_kernel_sizes(n, view):
    hyper = sc.ADAM_HYPER[sc.LOSS_SIZES.index(n) % len(sc.ADAM_HYPER)]
    for p_init in ("zero", "randn"):
        sc.check_adam_kernel(DEV, n, view=view, hyper=hyper, p_init=p_init)


@pytest.mark.parametrize("mode", ["classes", "random"])
@pytest.mark.parametrize("hyper", sc.ADAM_HYPER, ids=lambda h: "lr%g-b%g-%g-eps%g" % h)
def test_adam_kernel_hyper_parameters(hyper, mode):
    for view in (False, True):
        for p_init in ("zero", "randn"):
            sc.check_adam_kernel(DEV, 1003, view=view, hyper=hyper, p_init=p_init, mode=mode, seed=1)


@pytest.mark.parametrize("view", [False, True], ids=VIEW_IDS.get)
def test_adam_kernel_zero_gradient_moves_nothing(view):
    for n in (3, 1003):
        sc.check_adam_zero_gradient(DEV, n, view=view)


@pytest.mark.parametrize("view", [False, True], ids=VIEW_IDS.get)
@pytest.mark.parametrize("n", sc.LOSS_SIZES)
def test_sgd_kernel_sizes(n, view):
    sc.check_sgd_kernel(DEV, n, view=view)


@pytest.mark.parametrize("case", sc.OPT_CASES)
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_optimizers_against_torch_optim(kind, case):
    sc.check_optimizer(DEV, kind, case)


@pytest.mark.parametrize("size_mult", [1.0, 2.5])
@pytest.mark.parametrize("hw", sc.SOFTARGMAX_MAPS, ids=lambda s: "%dx%d" % s)
def test_softargmax_distinct_betas(hw, size_mult):
    sc.check_softargmax_distinct_betas(DEV, hw, size_mult)


def test_softargmax_large_values_stay_finite():
    sc.check_softargmax_large_values(DEV)


def test_softargmax_constant_map():
    sc.check_softargmax_constant_map(DEV)


@pytest.mark.parametrize("n", [1, 3, 1003, 2097153])
def test_add(n):
    sc.check_add(DEV, n)


def test_float4_kernels_refuse_misaligned_pointers():
    sc.check_alignment_contract(DEV)


@pytest.mark.parametrize("up", [1, 2, 4])
@pytest.mark.parametrize("k,cpad", [(7, 16), (7, 32), (17, 32)])
def test_stage_input_and_its_backward(k, cpad, up):
    sc.check_stage_input(DEV, up, k, cpad)


def test_stage_input_refuses_narrow_padding():
    sc.check_stage_input_refuses_narrow_padding(DEV)


@pytest.mark.parametrize("n", [1, 3, 1003, 1030])
def test_relu_bwd(n):
    sc.check_relu_bwd(DEV, n)


@pytest.mark.parametrize("shape", [(2, 6, 10, 8), (1, 2, 2, 4)], ids=lambda s: "x".join(str(v) for v in s))
def test_upsample2_bwd(shape):
    sc.check_upsample2_bwd(DEV, shape)


@pytest.mark.parametrize("hw", sorted(sc.LAYOUT_HW))
@pytest.mark.parametrize("c", sc.LAYOUT_C)
def test_layout_conversions(c, hw):
    sc.check_layout(DEV, c, hw)


def test_multi_copy():
    sc.check_multi_copy(DEV)
