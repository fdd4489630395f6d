"""Checks of train_activation_storage="fp16" (the half-x kernel of csrc/wgrad_f16.hip, the half-mask epilogue of csrc/conv_f16.hip, the
half-x max-pool backward and the widening pass of csrc/elementwise.hip, the host wiring of DreamHourglass), shared by the emulator
suite (test_fp16_train_storage_emulated.py) and the GPU suite (test_gpu_fp16_train_storage.py).

Per launch nothing is new arithmetic, so the first check is bit equality with the existing launch on the widened tensor.  For the
weight gradient that needs HALF-EXACT inputs (half_exact(): x.half() with magnitudes below 2^-14 set to 0): a normal half or zero
with max|x| < 2^14 times the power of two 2^ex of the fp32-x kernel is again exactly a half, so both kernels multiply the same
operand, and 2^-ex afterwards is exact.  Independently the launch is held to the bounds of fp16_train_checks: 5e-6 of max|ref|
against the fp64 gradient of (x_half, q(dy)) (fp32 accumulation only), and the fp64 gradient of the unrounded dy must lie more than
5e-5 away (1.9e-4 .. 3.9e-4 on these shapes with a half-exact x).

End to end the bound is measured on the reference, by stored_training_oracle(): oracle.models vgg_q with fp16_train_checks._RoundedConv
on the plain convs and a saturating round-to-half (straight-through backward) on the output of exactly the modules whose output the
rule stores as half (the ReLU behind conv1_1 .. conv5_3; a max-pool of halfs is a half), in float32 and in float64.  E_p = the larger
relative L2 distance of its gradients to the plain reference, per parameter; the device's |g - g32|_2 / |g32|_2 is held to 3 E_p
(3x: the project's margin for another draw of the same rounding noise).

Twenty Adam steps (check_training_trains): the decrease of the loss must be at least (1 - 3 rho) of the fp32 run's, rho = the gap of the
final losses of the rounded-storage oracle and the plain oracle over the same twenty steps (CPU, float32), relative to the plain
oracle's decrease, floored at fp16_train_checks.LOSS_GAP_MEASURED / (the device's fp32 decrease): the gap the project recorded for
train_precision="fp16" itself."""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

import cases
import fp16_train_checks as tc
import parity_checks as pc
from dream_amd import ops
from fp16_checks import _amax_value, q
from oracle import models as om

WGRAD_CASES = list(tc.WGRAD_SHAPES) + [tc.SPLITK_ONE, tc.SPLITK_MANY]
POOL_SHAPES = [(2, 6, 8, 64), (1, 7, 9, 32), (1, 2, 2, 8)]         # NHWC; odd sides; one window


def half_exact(x):
    """x.half() with everything below the smallest normal half set to 0 -> (half tensor, number of values zeroed)."""
    h = x.half()
    small = (h != 0) & (h.abs().float() < 2.0 ** -14)
    h[small] = 0
    return h, int(small.sum())


# ---- weight gradient -------------------------------------------------------------------------------------------------------------
def run_wgrad_x16(dev, xh, dy, flags=0):
    cout, cin = int(dy.shape[1]), int(xh.shape[1])
    gd = pc.to(dev, pc._nhwc(dy))
    dw, db = ops.conv3x3_wgrad_f16_x16(pc.to(dev, pc._nhwc(xh)), gd, ops.absmax(gd), cout, cin, flags)
    return dw.cpu(), db.cpu()


def check_wgrad_x16(dev, B, H, W, Cin, Cout, x_scale=1.0, g_scale=1.0, seed=0):
    x, dy = tc.wgrad_inputs(B, H, W, Cin, Cout, x_scale, g_scale, seed)
    xh, zeroed = half_exact(x)
    xf = xh.float()
    assert zeroed <= 2 and float(xf.abs().max()) < 2.0 ** 14 and torch.equal(q(xf), xf)      # the scaled fp32-storage operand IS xh
    dw, db = run_wgrad_x16(dev, xh, dy)
    old_dw, old_db = tc.run_wgrad(dev, xf, dy)
    ref, ref_unrounded = tc.wgrad_reference(xf, q(dy)), tc.wgrad_reference(xf, dy)
    scale = float(ref.abs().max())
    err = float((dw.double() - ref).abs().max()) / scale
    away = float((ref_unrounded - ref).abs().max()) / scale
    ref_b = dy.double().sum((0, 2, 3))
    berr = float((db.double() - ref_b).abs().max()) / float(ref_b.abs().max())
    print("half-x wgrad %s: err %.3g of max|ref|, unrounded dy %.3g away, bias err %.3g, %d subnormals zeroed"
          % ((B, H, W, Cin, Cout), err, away, berr, zeroed))
    assert tuple(dw.shape) == (Cout, Cin, 3, 3) and tuple(db.shape) == (Cout,)
    assert torch.equal(dw, old_dw) and torch.equal(db, old_db)
    assert err <= 5e-6, (err,)
    assert away > 5e-5, (away,)
    assert berr <= 5e-6, (berr,)


def check_wgrad_x16_zero_repeat_and_flags(dev):
    x, dy = tc.wgrad_inputs(2, 12, 20, 64, 96, seed=3)
    xh, _ = half_exact(x)
    dw, db = run_wgrad_x16(dev, xh, torch.zeros_like(dy))
    assert torch.equal(dw, torch.zeros_like(dw)) and torch.equal(db, torch.zeros_like(db))
    a, b = run_wgrad_x16(dev, xh, dy), run_wgrad_x16(dev, xh, dy)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    try:
        run_wgrad_x16(dev, xh, dy, flags=ops.CONV_UPSAMPLE2X)
    except RuntimeError as e:
        assert "flags" in str(e)
    else:
        raise AssertionError("a non-zero flags argument must be refused")
    try:
        ops.conv3x3_wgrad_f16_x16(pc.to(dev, pc._nhwc(xh.float())), pc.to(dev, pc._nhwc(dy)), None, 96, 64)
    except RuntimeError as e:
        assert "float16" in str(e)
    else:
        raise AssertionError("an fp32 x must be refused")


# ---- masked data gradient ---------------------------------------------------------------------------------------------------------
def check_dgrad_mask16(dev, B, H, W, Cout, Cin, seed=0):
    """conv2d_f16_mask16 with mask.half() against conv2d_f16(relu_mask=mask_half.float()): y and amax bit for bit."""
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(B, Cout, H, W, generator=g)
    dy[0, 0, 0, 0] = 40.0
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1
    mask = torch.randn(B, Cin, H, W, generator=g).relu()
    mask[0, :, 0, 0] = 0.0
    mask[0, 0, 1, 1] = 2e-8                                         # > 0 in fp32, rounds to 0 as a half: the HALF decides
    mh = pc._nhwc(mask.half())
    p16 = ops.pack_conv_weight_f16(pc.to(dev, w), 1)
    gd = pc.to(dev, pc._nhwc(dy))
    amax_in = ops.absmax(gd)
    y, amax = ops.conv2d_f16_mask16(gd, amax_in, p16, p16[3], 3, pc.to(dev, mh))
    y_old, amax_old = ops.conv2d_f16(gd, amax_in, p16, p16[3], 3, relu_mask=pc.to(dev, mh.float()))
    got = y.cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, H, W, Cin)
    assert torch.equal(got, y_old.cpu()) and _amax_value(amax) == _amax_value(amax_old)
    assert bool((got[mh <= 0] == 0).all()) and bool((got[mh > 0] != 0).any()) and float(got[0, 1, 1, 0]) == 0.0
    assert _amax_value(amax) == float(got.abs().max())


def check_dgrad_mask16_shapes(dev, seed=0):
    check_dgrad_mask16(dev, 1, 7, 9, 64, 32, seed=seed)
    check_dgrad_mask16(dev, 2, 12, 20, 32, 64, seed=seed)


# ---- max-pool backward, widening -------------------------------------------------------------------------------------------------
def check_pool_bwd_x16(dev):
    g = torch.Generator().manual_seed(5)
    for shape in POOL_SHAPES:
        b, h, w, c = shape
        xh = torch.randn(shape, generator=g).relu().half()          # exact zeros: all-zero windows and ties at 0
        xh[0, 0, 1, :] = xh[0, 0, 0, :]                             # ties at a positive maximum: the first in scan order wins
        xh[0, 1, 0, : c // 2] = xh[0, 0, 0, : c // 2]
        dy = torch.randn(b, h // 2, w // 2, c, generator=g)
        for relu in (False, True):
            dx = ops.maxpool2_bwd_x16(pc.to(dev, dy), pc.to(dev, xh), relu=relu).cpu()
            want = ops.maxpool2_bwd(pc.to(dev, dy), pc.to(dev, xh.float()), relu=relu).cpu()
            assert dx.dtype == torch.float32 and torch.equal(dx, want), (shape, relu)
            assert bool((dx[:, 2 * (h // 2):] == 0).all()) and bool((dx[:, :, 2 * (w // 2):] == 0).all())
        ties = int(((xh[:, 0:2 * (h // 2):2, 0:2 * (w // 2):2] == xh[:, 0:2 * (h // 2):2, 1:2 * (w // 2):2])).sum())
        assert ties > 0, shape


def check_widen(dev):
    g = torch.Generator().manual_seed(9)
    for n in (8 * 300 + 5, 3, 4096):
        xh = (torch.randn(n, generator=g) * 100).half()
        xh[0], xh[1], xh[2] = 65504.0, -65504.0, 2.0 ** -24       # the largest halfs, the smallest subnormal
        if n > 8:
            xh[3], xh[-1] = -(2.0 ** -15), 6e-8                     # subnormals, one of them in the tail
        out = ops.widen_f16(pc.to(dev, xh)).cpu()
        assert out.dtype == torch.float32 and torch.equal(out, xh.float()), n


# ---- end to end ------------------------------------------------------------------------------------------------------------------
class _StoreHalf(torch.autograd.Function):
    """half(clamp(v, +-65504)) in v's dtype; straight-through backward."""

    @staticmethod
    def forward(ctx, v):
        return v.clamp(-65504.0, 65504.0).half().to(v.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def stored_conv_count():
    """How many conv outputs the rule stores as half for vgg_q (counted on the product's plan, no device needed)."""
    import os
    import warnings
    from dream_amd import models
    old = os.environ.get("DREAM_VGG19_WEIGHTS")
    os.environ["DREAM_VGG19_WEIGHTS"] = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "no-such-weights.pth")
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = models.DreamHourglass(7, internalize_spatial_softmax=False)
    finally:
        if old is None:
            del os.environ["DREAM_VGG19_WEIGHTS"]
        else:
            os.environ["DREAM_VGG19_WEIGHTS"] = old
    half = m._half_storage_plan()
    return sum(1 for li in half if m.plan_layers()[li][1] is not None)


def _oracle_model(weights, dtype, mode):
    """oracle vgg_q; mode "plain" | "stored" (rounded products on the plain convs + half-stored outputs of the run)."""
    model = om.build_model("vgg_q", 7)
    model.load_state_dict(weights)
    model = model.to(dtype).train()
    if mode == "stored":
        for mod in tc._plain_reference_convs(model):
            mod.forward = (lambda m: lambda inp: tc._RoundedConv.apply(inp, m.weight, m.bias))(mod)
        encoder = [model.layer_0_1_down, model.layer_0_2_down, model.layer_0_3_down, model.layer_0_4_down, model.layer_0_5_down]
        relus = [m for seq in encoder for m in seq if isinstance(m, nn.ReLU)]
        n = stored_conv_count()
        assert 14 <= n < len(relus)
        for m in relus[:n]:                                        # the ReLU behind conv1_1 .. conv5_3: the stored tensor
            m.register_forward_hook(lambda mod, inp, out: _StoreHalf.apply(out))
    return model


def _oracle_target(out_wh, shape=tc.TRAIN_SHAPE):
    b, h, w = shape
    return torch.from_numpy(cases.target_batch(b, 7, out_wh, in_wh=(w, h), seed=7))


def stored_training_oracle(out_wh, shape=tc.TRAIN_SHAPE):
    """{parameter name: E_p}; computed once per process and shape."""
    return _stored_training_oracle(out_wh, shape)


@functools.lru_cache(maxsize=None)
def _stored_training_oracle(out_wh, shape):
    wts, x = tc.training_case(shape)
    t = _oracle_target(out_wh, shape)
    E = {}
    for dtype in (torch.float32, torch.float64):
        grads = {}
        for mode in ("plain", "stored"):
            model = _oracle_model(wts, dtype, mode)
            F.mse_loss(model(x.to(dtype))[0], t.to(dtype)).backward()
            grads[mode] = {n: p.grad.double() for n, p in model.named_parameters()}
        for n in grads["plain"]:
            r = float((grads["stored"][n] - grads["plain"][n]).norm() / grads["plain"][n].norm())
            E[n] = max(E.get(n, 0.0), r)
    return E


@functools.lru_cache(maxsize=None)
def oracle_loss_gap(out_wh, steps=20):
    """rho before its floor: |final loss (stored) - final loss (plain)| / (first - final loss (plain)) after ``steps`` Adam steps of
    the oracle on the fixed batch (float32, CPU), and the two loss lists."""
    wts, x = tc.training_case()
    t = _oracle_target(out_wh)
    runs = {}
    for mode in ("plain", "stored"):
        model = _oracle_model(wts, torch.float32, mode)
        opt = torch.optim.Adam(model.parameters(), lr=cases.TRAIN_LR["adam"])
        runs[mode] = []
        for _ in range(steps):
            opt.zero_grad()
            loss = F.mse_loss(model(x)[0], t)
            loss.backward()
            opt.step()
            runs[mode].append(float(loss.detach()))
    rho = abs(runs["stored"][-1] - runs["plain"][-1]) / (runs["plain"][0] - runs["plain"][-1])
    return rho, runs


def training_network(dev, storage="fp16", train_precision="fp16", optimizer="sgd", lr=0.0, shape=tc.TRAIN_SHAPE):
    net = tc.training_network(dev, train_precision, optimizer=optimizer, lr=lr, shape=shape)
    net.model.module.train_activation_storage = storage
    return net


def step_gradients(dev, storage, train_precision="fp16", shape=tc.TRAIN_SHAPE):
    net = training_network(dev, storage, train_precision, shape=shape)
    _, x = tc.training_case(shape)
    t, out_wh = tc._target(net, dev, shape)
    loss = float(net.train([pc.to(dev, x)], t).item())
    grads = {n: p.grad.detach().cpu().clone() for n, p in net.model.module.named_parameters()}
    return grads, loss, out_wh, net


def check_training_step(dev, shape=tc.TRAIN_SHAPE):
    """One vgg_q step at ``shape`` (2 x 64 x 96) with both switches "fp16" against the fp32 step of the same build, every parameter
    to 3 E_p."""
    g32, loss32, out_wh, _ = step_gradients(dev, "fp32", "fp32", shape=shape)
    g16, loss16, _, _ = step_gradients(dev, "fp32", "fp16", shape=shape)      # fp16 products, fp32 storage
    gs, loss_s, _, net = step_gradients(dev, "fp16", "fp16", shape=shape)
    E = stored_training_oracle(out_wh, shape)
    m = net.model.module
    peak = m.half_storage_peak()
    assert 0.0 < peak < 65504.0 and peak == peak, peak
    names = {id(p): n for n, p in m.named_parameters()}
    layers = m.plan_layers()
    half = m._half_storage_plan()
    run_w = {names[id(layers[li][1].weight)] for li in range(1, len(layers)) if layers[li][1] is not None and li - 1 in half}
    assert len(run_w) >= 14, len(run_w)
    worst = dist = 0.0
    for n in sorted(g32):
        ref = g32[n].double()
        r = float((gs[n].double() - ref).norm() / ref.norm())
        d = float((gs[n].double() - g16[n].double()).norm() / g16[n].double().norm())
        print("half-stored training %-40s r_p %.3g  E_p %.3g  distance to the fp32-storage fp16 step %.3g" % (n, r, E[n], d))
        worst, dist = max(worst, r / E[n]), max(dist, d)
        assert r <= 3 * E[n], (n, r, E[n])
        if n in run_w:
            assert not torch.equal(gs[n], g16[n]), n                          # (the half-x weight gradient really ran on other values)
    print("half-stored training: losses %.9g (fp32) %.9g (fp16) %.9g (fp16, half storage), peak %.6g, worst r_p / E_p %.3g, "
          "largest distance to the fp32-storage fp16 step %.3g" % (loss32, loss16, loss_s, peak, worst, dist))
    # a second step (lr = 0: same parameters) gives the same bits
    _, x = tc.training_case(shape)
    t, _ = tc._target(net, dev, shape)
    loss_again = float(net.train([pc.to(dev, x)], t).item())
    assert loss_again == loss_s
    for n, p in m.named_parameters():
        assert torch.equal(p.grad.detach().cpu(), gs[n]), n


def check_entries_outside_the_run_bit_equal(dev):
    """Every plan entry that neither reads nor writes a half tensor gives, on the input the half-storage forward gave it, the output of
    the train_precision="fp16" walk with fp32 storage, bit for bit; the first conv stores half(clamp()) of its fp32 output."""
    net = training_network(dev, "fp16")
    _, x = tc.training_case()
    m = net.model.module
    params = [p.detach() for p in m.plan_parameters()]
    layers = m.plan_layers()
    with torch.no_grad():
        out_s, saved_s = m.run_forward(pc.to(dev, x), params, True)
        m.train_activation_storage = "fp32"
        out_f, saved_f = m.run_forward(pc.to(dev, x), params, True)
        assert not saved_f.half_in and all(t is None or t.dtype == torch.float32 for pair in saved_f for t in pair)
        assert torch.equal(saved_s[0][1].float(), saved_f[0][1].clamp(-65504.0, 65504.0).half().float())
        checked = inside = 0
        for li, (kind, mod, flags) in enumerate(layers):
            inp, out = saved_s[li]
            if li == 0 or torch.float16 in (inp.dtype, out.dtype):
                inside += 1
                assert (li in saved_s.half_in) == (mod is not None and li > 0 and inp.dtype == torch.float16)
                continue
            if kind == "pool":
                assert torch.equal(ops.maxpool2(inp), out), li
            elif tc.is_plain(kind, mod, flags, int(inp.shape[3])):
                w, bias = params[m._param_slot[li]], params[m._param_slot[li] + 1]
                again, _ = m._conv_half("f16", kind, mod, inp, ops.absmax(inp), w, bias, flags)
                assert torch.equal(again, out), li
            else:
                w, bias = params[m._param_slot[li]], params[m._param_slot[li] + 1]
                again, _ = m._conv_fp32(kind, mod, inp, None, w, bias, flags)
                assert torch.equal(again, out), li
            checked += 1
    assert checked >= 6 and inside >= 19, (checked, inside)
    assert out_s.dtype == torch.float32 and not torch.equal(out_s, out_f)


def check_training_trains(dev, steps=20):
    _, x = tc.training_case()
    runs = {}
    for name, tp, storage in (("fp32", "fp32", "fp32"), ("half", "fp16", "fp16")):
        net = training_network(dev, storage, tp, optimizer="adam", lr=cases.TRAIN_LR["adam"])
        t, out_wh = tc._target(net, dev)
        xd = pc.to(dev, x)
        runs[name] = [float(net.train([xd], t).item()) for _ in range(steps)]
    dec32, dec = runs["fp32"][0] - runs["fp32"][-1], runs["half"][0] - runs["half"][-1]
    rho_ref, oracle = oracle_loss_gap(out_wh, steps)
    rho = max(rho_ref, tc.LOSS_GAP_MEASURED / dec32)
    print("half-stored training, %d Adam steps: fp32 %.9g -> %.9g, half storage %.9g -> %.9g (%.6g of the fp32 decrease); oracle plain "
          "%.9g -> %.9g, stored %.9g -> %.9g: rho %.3g (floor %.3g)"
          % (steps, runs["fp32"][0], runs["fp32"][-1], runs["half"][0], runs["half"][-1], dec / dec32, oracle["plain"][0],
             oracle["plain"][-1], oracle["stored"][0], oracle["stored"][-1], rho_ref, tc.LOSS_GAP_MEASURED / dec32))
    assert runs["half"][-1] < runs["half"][0]
    assert dec32 > 0 and dec >= (1 - 3 * rho) * dec32, (dec, dec32, rho)
    return runs
