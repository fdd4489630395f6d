"""Checks of train_gradient_storage="fp16" (the GRAD16 forms of csrc/conv_f16.hip, the half-dy kernel of csrc/wgrad_f16.hip, the all-half
max-pool backward of csrc/elementwise.hip, the host wiring of DreamHourglass), shared by the emulator suite
(test_fp16_grad_storage_emulated.py) and the GPU suite (test_gpu_fp16_grad_storage.py).

A stored gradient is half(clamp(g * 2^e_g, +-65504)), e_g = 9 - exponent(amax of the loss gradient) (grad_exponent(): 0 for a zero
scalar, clamped to +-100).  Per launch nothing is new arithmetic, so every check is bit equality with an existing launch on the widened
tensor: the gradients are HALF-EXACT (fp16_train_storage_checks.half_exact: normal halfs or zero, max < 2^14), so today's fp32-input
kernel multiplies the same operand up to a power of two, and the power of two that is taken out afterwards is exact.  Independently the
half-dy weight gradient is held to 5e-6 of max|ref| against the fp64 gradient of the stored operands (fp32 accumulation only, as in
fp16_train_checks).

End to end the bound is measured on the reference, by grad_stored_training_oracle(): fp16_train_storage_checks' "stored" oracle with a
tensor hook on the input of every reader of the half run but the first that replaces the gradient g by
half(clamp(g * 2^e_g)) * 2^-e_g, e_g from the amax of the loss gradient of that very backward, in float32 and in float64.  E_p = the
larger relative L2 distance of its gradients to the plain reference; the device's |g - g32|_2 / |g32|_2 is held to 3 E_p (3x: the
project's margin for another draw of the same rounding noise).  Twenty Adam steps: the decrease of the loss must be at
least (1 - 3 rho) of the fp32 run's, rho = the extended oracle's final-loss gap over its plain run's decrease, floored at
fp16_train_checks.LOSS_GAP_MEASURED / (the device's fp32 decrease), as for train_activation_storage."""
import functools
import math

import torch
import torch.nn.functional as F

import cases
import fp16_train_checks as tc
import fp16_train_storage_checks as sc
import parity_checks as pc
from dream_amd import ops
from fp16_checks import _amax_value

WGRAD_CASES = sc.WGRAD_CASES
DGRAD_SHAPES = [(1, 7, 9, 64, 32), (2, 12, 20, 32, 64)]            # (B, H, W, Cout, Cin)
POOL_SHAPES = sc.POOL_SHAPES


def grad_exponent(amax):
    """e_g of csrc/half_scale.h for the float ``amax``."""
    if amax == 0.0:
        return 0
    return max(-100, min(100, 9 - (math.frexp(amax)[1] - 1)))


def scalar(dev, value):
    """A device amax scalar holding the bit pattern of the float ``value``."""
    return pc.to(dev, torch.tensor([value], dtype=torch.float32).view(torch.int32))


def sat_half(t):
    return t.clamp(-65504.0, 65504.0).half()


def _half_exact(t):
    h, zeroed = sc.half_exact(t)
    assert float(h.float().abs().max()) < 2.0 ** 14 and zeroed <= max(2, t.numel() // 2000), zeroed
    return h


# ---- weight gradient -------------------------------------------------------------------------------------------------------------
def run_wgrad_dy16(dev, xh, dyh, g_scalar, flags=0):
    cout, cin = int(dyh.shape[1]), int(xh.shape[1])
    dw, db = ops.conv3x3_wgrad_f16_x16_dy16(pc.to(dev, pc._nhwc(xh)), pc.to(dev, pc._nhwc(dyh)), scalar(dev, g_scalar), cout, cin, flags)
    return dw.cpu(), db.cpu()


def check_wgrad_dy16(dev, B, H, W, Cin, Cout, x_scale=1.0, g_scale=1.0, seed=0):
    """The stored dy is half-exact at unit scale; ``g_scale`` moves the loss-gradient scalar, and with it e_g."""
    x, dy = tc.wgrad_inputs(B, H, W, Cin, Cout, x_scale, 1.0, seed)
    xh, dyh = _half_exact(x), _half_exact(dy)
    g_scalar = 30.0 * g_scale
    eg = grad_exponent(g_scalar)
    dw, db = run_wgrad_dy16(dev, xh, dyh, g_scalar)
    old_dw, old_db = sc.run_wgrad_x16(dev, xh, dyh.float())
    ref = tc.wgrad_reference(xh.float(), dyh.float()) * 2.0 ** -eg
    scale = float(ref.abs().max())
    err = float((dw.double() - ref).abs().max()) / scale
    print("half-dy wgrad %s: e_g %d, err %.3g of max|ref|" % ((B, H, W, Cin, Cout), eg, err))
    assert tuple(dw.shape) == (Cout, Cin, 3, 3) and tuple(db.shape) == (Cout,)
    assert torch.equal(dw, old_dw * 2.0 ** -eg) and torch.equal(db, old_db * 2.0 ** -eg)
    assert bool((dw != 0).any()) and bool((db != 0).any())
    assert err <= 5e-6, (err,)


def check_wgrad_dy16_zero_repeat_and_flags(dev):
    x, dy = tc.wgrad_inputs(2, 12, 20, 64, 96, seed=3)
    xh, dyh = _half_exact(x), _half_exact(dy)
    dw, db = run_wgrad_dy16(dev, xh, torch.zeros_like(dyh), 0.25)
    assert torch.equal(dw, torch.zeros_like(dw)) and torch.equal(db, torch.zeros_like(db))
    a, b = run_wgrad_dy16(dev, xh, dyh, 0.25), run_wgrad_dy16(dev, xh, dyh, 0.25)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # a zero loss-gradient scalar: e_g = 0, the x16 result itself
    z, old = run_wgrad_dy16(dev, xh, dyh, 0.0), sc.run_wgrad_x16(dev, xh, dyh.float())
    assert torch.equal(z[0], old[0]) and torch.equal(z[1], old[1]) and bool(torch.isfinite(z[0]).all())
    try:
        run_wgrad_dy16(dev, xh, dyh, 0.25, flags=ops.CONV_UPSAMPLE2X)
    except RuntimeError as e:
        assert "flags" in str(e)
    else:
        raise AssertionError("a non-zero flags argument must be refused")
    try:
        ops.conv3x3_wgrad_f16_x16_dy16(pc.to(dev, pc._nhwc(xh)), pc.to(dev, pc._nhwc(dyh.float())), scalar(dev, 0.25), 96, 64)
    except RuntimeError as e:
        assert "float16" in str(e)
    else:
        raise AssertionError("an fp32 dy must be refused")


# ---- data gradients --------------------------------------------------------------------------------------------------------------
def _dgrad_case(dev, B, H, W, Cout, Cin, seed, g_mul=1.0):
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(B, Cout, H, W, generator=g) * g_mul
    dy[0, 0, 0, 0] = 40.0 * g_mul
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1
    mask = torch.randn(B, Cin, H, W, generator=g).relu()
    mask[0, :, 0, 0] = 0.0
    mask[0, 0, 1, 1] = 2e-8                                         # > 0 in fp32, rounds to 0 as a half: the HALF decides
    mh = pc.to(dev, pc._nhwc(mask.half()))
    p16 = ops.pack_conv_weight_f16(pc.to(dev, w), 1)
    return pc._nhwc(dy), p16, mh


def check_dgrad_interior_and_exit(dev, B, H, W, Cout, Cin, seed=0, g_scalar=3e-3):
    dy, p16, mh = _dgrad_case(dev, B, H, W, Cout, Cin, seed)
    gh = pc.to(dev, _half_exact(dy))
    wide = gh.float()
    amax_in = ops.absmax(wide)
    eg = grad_exponent(g_scalar)
    y32, amax32 = ops.conv2d_f16_mask16(wide, amax_in, p16, p16[3], 3, mh)
    y32u, _ = ops.conv2d_f16(wide, amax_in, p16, p16[3], 3)
    zero = (mh <= 0).cpu()
    # interior, masked: the mask16 launch's value, saturated and rounded; the peak is the largest stored value before that
    peak = ops.new_amax(gh.device)
    y = ops.conv2d_f16_g16(gh, p16, p16[3], 3, relu_mask=mh, peak=peak)
    assert y.dtype == torch.float16 and tuple(y.shape) == (B, H, W, Cin)
    assert torch.equal(y.cpu(), sat_half(y32.cpu())) and bool((y.cpu()[zero] == 0).all()) and bool((y != 0).any())
    assert _amax_value(peak) == float(y32.abs().max()) == _amax_value(amax32)
    # interior, unmasked (behind a pool): the half-storage inference launch, bit for bit, and the fp32 launch's value
    peak_u, peak_a = ops.new_amax(gh.device), ops.new_amax(gh.device)
    yu = ops.conv2d_f16_g16(gh, p16, p16[3], 3, peak=peak_u)
    assert torch.equal(yu.cpu(), sat_half(y32u.cpu()))
    assert torch.equal(yu.cpu(), ops.conv2d_f16_act16(gh, p16, p16[3], 3, peak=peak_a).cpu()) and _amax_value(peak_u) == _amax_value(peak_a)
    # exit: fp32, times 2^-e_g, amax after the mask
    for scalar_value in (g_scalar, 0.0):
        ye, amax_e = ops.conv2d_f16_g16_exit(gh, p16, p16[3], 3, scalar(dev, scalar_value), mh)
        want = y32.cpu() * 2.0 ** -grad_exponent(scalar_value)
        assert ye.dtype == torch.float32 and torch.equal(ye.cpu(), want) and bool((ye.cpu()[zero] == 0).all())
        assert _amax_value(amax_e) == float(want.abs().max()) and bool(torch.isfinite(ye).all())
    assert eg != 0
    # a repeated launch gives the same bits
    assert torch.equal(ops.conv2d_f16_g16(gh, p16, p16[3], 3, relu_mask=mh).cpu(), y.cpu())


def check_dgrad_entry(dev, B, H, W, Cout, Cin, seed=0):
    """fp32 g in (scaled by its own amax, any values), half out times 2^e_g: against conv2d_f16_mask16 / conv2d_f16 for the same g and
    amax.  The scalars: an ordinary one, one that saturates (the result is finite, the peak tells), zero (e_g = 0)."""
    dy, p16, mh = _dgrad_case(dev, B, H, W, Cout, Cin, seed, g_mul=1e-3)
    gd = pc.to(dev, dy)
    amax_in = ops.absmax(gd)
    y32, _ = ops.conv2d_f16_mask16(gd, amax_in, p16, p16[3], 3, mh)
    y32u, _ = ops.conv2d_f16(gd, amax_in, p16, p16[3], 3)
    top = float(y32.abs().max())
    for what, g_scalar in (("plain", 0.02), ("saturating", top * 2.0 ** -20), ("zero", 0.0)):
        eg = grad_exponent(g_scalar)
        for mask, ref in ((mh, y32), (None, y32u)):
            scaled = ref.cpu() * 2.0 ** eg
            peak = ops.new_amax(gd.device)
            y = ops.conv2d_f16_g16_entry(gd, amax_in, p16, p16[3], 3, scalar(dev, g_scalar), relu_mask=mask, peak=peak)
            assert y.dtype == torch.float16 and tuple(y.shape) == (B, H, W, Cin)
            assert bool(torch.isfinite(y).all()) and torch.equal(y.cpu(), sat_half(scaled)), (what, mask is None)
            assert _amax_value(peak) == float(scaled.abs().max()), (what, _amax_value(peak), float(scaled.abs().max()))
            if mask is not None:
                assert bool((y.cpu()[(mh <= 0).cpu()] == 0).all())
        print("entry dgrad %s, %s scalar: e_g %d, peak %.6g" % ((B, H, W, Cout, Cin), what, eg, _amax_value(peak)))
        assert (_amax_value(peak) >= 65504.0) == (what == "saturating")
        assert (eg == 0) == (what == "zero")
    zeros = ops.conv2d_f16_g16_entry(torch.zeros_like(gd), ops.absmax(torch.zeros_like(gd)), p16, p16[3], 3, scalar(dev, 0.02), relu_mask=mh)
    assert torch.equal(zeros.cpu(), torch.zeros_like(zeros.cpu()))


def check_dgrad_shapes(dev, seed=0):
    for shape in DGRAD_SHAPES:
        check_dgrad_interior_and_exit(dev, *shape, seed=seed)
        check_dgrad_entry(dev, *shape, seed=seed)


def check_dgrad_refusals(dev):
    dy, p16, mh = _dgrad_case(dev, 1, 7, 9, 64, 32, 0)
    gh = pc.to(dev, _half_exact(dy))
    for launch in (lambda: ops.conv2d_f16_g16(gh, p16, p16[3], 3, relu_mask=mh, flags=ops.CONV_RELU),
                   lambda: ops.conv2d_f16_g16_exit(gh, p16, p16[3], 3, scalar(dev, 1.0), mh, flags=ops.CONV_RELU),
                   lambda: ops.conv2d_f16_g16_entry(gh.float(), ops.absmax(gh.float()), p16, p16[3], 3, scalar(dev, 1.0), flags=ops.CONV_RELU)):
        try:
            launch()
        except RuntimeError as e:
            assert "flags" in str(e)
        else:
            raise AssertionError("non-zero flags must be refused")
    try:
        ops.conv2d_f16_g16(gh.float(), p16, p16[3], 3, relu_mask=mh)
    except RuntimeError as e:
        assert "float16" in str(e)
    else:
        raise AssertionError("an fp32 gradient must be refused by the interior form")


# ---- max-pool backward -----------------------------------------------------------------------------------------------------------
def check_pool_bwd_dy16(dev):
    g = torch.Generator().manual_seed(5)
    for shape in POOL_SHAPES:
        b, h, w, c = shape
        xh = torch.randn(shape, generator=g).relu().half()
        xh[0, 0, 1, :] = xh[0, 0, 0, :]                             # ties at a positive maximum: the first in scan order wins
        xh[0, 1, 0, : c // 2] = xh[0, 0, 0, : c // 2]
        dyh = (torch.randn(b, h // 2, w // 2, c, generator=g) * 100).half()
        dyh[0, 0, 0, 0], dyh[0, 0, 0, 1] = 65504.0, 2.0 ** -24       # the largest half, the smallest subnormal: copied as they are
        for relu in (False, True):
            dx = ops.maxpool2_bwd_x16_dy16(pc.to(dev, dyh), pc.to(dev, xh), relu=relu).cpu()
            want = ops.maxpool2_bwd_x16(pc.to(dev, dyh.float()), pc.to(dev, xh), relu=relu).cpu()
            assert dx.dtype == torch.float16 and torch.equal(dx.float(), want) and torch.equal(dx, want.half()), (shape, relu)
            assert bool((dx[:, 2 * (h // 2):] == 0).all()) and bool((dx[:, :, 2 * (w // 2):] == 0).all())
            assert bool((dx != 0).any())


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _grad_stored_model(weights, dtype, record):
    """4.8e's "stored" oracle plus the half-stored gradients: a hook on the input of every reader of the run but the first."""
    model = sc._oracle_model(weights, dtype, "stored")
    readers = tc._plain_reference_convs(model)[:sc.stored_conv_count()]        # conv1_2 .. the boundary conv

    def store(g):
        s = 2.0 ** record["e_g"]
        scaled = g * s
        record["peak"] = max(record.get("peak", 0.0), float(scaled.abs().max()))
        return scaled.clamp(-65504.0, 65504.0).half().to(g.dtype) / s

    for mod in readers[1:]:
        mod.register_forward_pre_hook(lambda m, inp: inp[0].register_hook(store) and None)
    return model


def _loss_with_scale(model, x, t, record):
    out = model(x)[0]
    out.register_hook(lambda g: record.__setitem__("e_g", grad_exponent(float(g.abs().max()))))
    return F.mse_loss(out, t)


def grad_stored_training_oracle(out_wh, shape=tc.TRAIN_SHAPE):
    """({parameter name: E_p}, peak = the largest |g * 2^e_g| any hook stored); computed once per process and shape."""
    return _grad_stored_training_oracle(out_wh, shape)


@functools.lru_cache(maxsize=None)
def _grad_stored_training_oracle(out_wh, shape):
    wts, x = tc.training_case(shape)
    t = sc._oracle_target(out_wh, shape)
    E, peak = {}, 0.0
    for dtype in (torch.float32, torch.float64):
        plain = sc._oracle_model(wts, dtype, "plain")
        F.mse_loss(plain(x.to(dtype))[0], t.to(dtype)).backward()
        record = {}
        model = _grad_stored_model(wts, dtype, record)
        _loss_with_scale(model, x.to(dtype), t.to(dtype), record).backward()
        peak = max(peak, record["peak"])
        ref = {n: p.grad.double() for n, p in plain.named_parameters()}
        for n, p in model.named_parameters():
            E[n] = max(E.get(n, 0.0), float((p.grad.double() - ref[n]).norm() / ref[n].norm()))
    return E, peak


def check_reference_sanity(out_wh):
    """The extended oracle adds next to nothing to 4.8e's: E_p within 1.05x, the stored values stay 2^4 below saturation."""
    E, peak = grad_stored_training_oracle(out_wh, tc.TRAIN_SHAPE)        # (the cache keys of check_training_step at the default shape)
    E0 = sc.stored_training_oracle(out_wh, tc.TRAIN_SHAPE)
    worst = max(E[n] / E0[n] for n in E0)
    print("half-gradient oracle: worst E_p / E_p(stored activations) %.5f, peak 2^%.2f" % (worst, math.log2(peak)))
    assert set(E) == set(E0) and worst <= 1.05, worst
    assert 0.0 < peak < 2.0 ** 12, peak


@functools.lru_cache(maxsize=None)
def oracle_loss_gap(out_wh, steps=20):
    """rho before its floor, as fp16_train_storage_checks.oracle_loss_gap, for the extended oracle."""
    wts, x = tc.training_case()
    t = sc._oracle_target(out_wh)
    runs = {}
    for mode in ("plain", "grad-stored"):
        record = {}
        model = sc._oracle_model(wts, torch.float32, "plain") if mode == "plain" else _grad_stored_model(wts, torch.float32, record)
        opt = torch.optim.Adam(model.parameters(), lr=cases.TRAIN_LR["adam"])
        runs[mode] = []
        for _ in range(steps):
            opt.zero_grad()
            loss = _loss_with_scale(model, x, t, record)
            loss.backward()
            opt.step()
            runs[mode].append(float(loss.detach()))
    rho = abs(runs["grad-stored"][-1] - runs["plain"][-1]) / (runs["plain"][0] - runs["plain"][-1])
    return rho, runs


def training_network(dev, gradient_storage="fp16", storage="fp16", train_precision="fp16", optimizer="sgd", lr=0.0, shape=tc.TRAIN_SHAPE):
    net = sc.training_network(dev, storage, train_precision, optimizer=optimizer, lr=lr, shape=shape)
    net.model.module.train_gradient_storage = gradient_storage
    return net


def step_gradients(dev, gradient_storage, storage="fp16", train_precision="fp16", shape=tc.TRAIN_SHAPE):
    net = training_network(dev, gradient_storage, storage, train_precision, shape=shape)
    _, x = tc.training_case(shape)
    t, out_wh = tc._target(net, dev, shape)
    loss = float(net.train([pc.to(dev, x)], t).item())
    grads = {n: p.grad.detach().cpu().clone() for n, p in net.model.module.named_parameters()}
    return grads, loss, out_wh, net


def check_training_step(dev, shape=tc.TRAIN_SHAPE):
    """One vgg_q step at ``shape`` (2 x 64 x 96) with the three switches "fp16" against the fp32 step of the same build, every parameter
    to 3 E_p.

    Measured (r_p / E_p worst, distance to the two-switch step): see DESIGN.md 4.8g."""
    g32, loss32, out_wh, _ = step_gradients(dev, "fp32", "fp32", "fp32", shape=shape)
    g2, loss2, _, _ = step_gradients(dev, "fp32", shape=shape)               # the two-switch step: half activations, fp32 gradients
    gs, loss_s, _, net = step_gradients(dev, "fp16", shape=shape)
    E, _ = grad_stored_training_oracle(out_wh, shape)
    m = net.model.module
    peak = m.half_gradient_peak()
    assert 0.0 < peak < 65504.0 and peak == peak, peak
    names = {id(p): n for n, p in m.named_parameters()}
    layers = m.plan_layers()
    grad16 = m._half_gradient_plan()
    assert len(grad16) == 18, len(grad16)                                     # conv1_2 .. conv5_3 and the four pools
    run_w = {names[id(layers[li][1].weight)] for li in grad16 if layers[li][1] is not None}      # x16 + dy16 weight gradients
    above = {names[id(p)] for li in range(max(grad16) + 1, len(layers)) if layers[li][1] is not None
             for p in (layers[li][1].weight, layers[li][1].bias)}                                 # boundary conv, decoder, heads
    assert len(run_w) == 14 and len(above) >= 12, (len(run_w), len(above))
    worst = dist = 0.0
    for n in sorted(g32):
        ref = g32[n].double()
        r = float((gs[n].double() - ref).norm() / ref.norm())
        d = float((gs[n].double() - g2[n].double()).norm() / g2[n].double().norm())
        print("half-gradient training %-40s r_p %.3g  E_p %.3g  distance to the two-switch step %.3g" % (n, r, E[n], d))
        worst, dist = max(worst, r / E[n]), max(dist, d)
        assert r <= 3 * E[n], (n, r, E[n])
        if n in run_w:
            assert not torch.equal(gs[n], g32[n]), n
        if n in above:
            assert torch.equal(gs[n], g2[n]), n                               # nothing above the run moves
    # The half path really ran: a weight gradient of the run may well keep the two-switch step's bits (that step rounds the same g to
    # half while staging it; the reference leaves 31 of 46 gradients unchanged), but a bias gradient now sums the STORED halfs
    run_b = {n[:-len("weight")] + "bias" for n in run_w}
    moved = sorted(n for n in run_b if not torch.equal(gs[n], g2[n]))
    print("half-gradient training: %d of %d bias gradients of the run differ from the two-switch step's" % (len(moved), len(run_b)))
    assert moved
    print("half-gradient training: losses %.9g (fp32) %.9g (two switches) %.9g (three), peak %.6g = 2^%.2f, worst r_p / E_p %.3g, "
          "largest distance to the two-switch step %.3g" % (loss32, loss2, loss_s, peak, math.log2(peak), worst, dist))
    assert loss_s == loss2                                                    # the forward is the two-switch forward
    # a second step (lr = 0: same parameters) gives the same bits: no state is carried from step to step
    _, x = tc.training_case(shape)
    t, _ = tc._target(net, dev, shape)
    assert float(net.train([pc.to(dev, x)], t).item()) == loss_s
    for n, p in m.named_parameters():
        assert torch.equal(p.grad.detach().cpu(), gs[n]), n
    assert m.half_gradient_peak() == peak


def check_training_trains(dev, steps=20):
    _, x = tc.training_case()
    runs = {}
    for name, switches in (("fp32", ("fp32", "fp32", "fp32")), ("half", ("fp16", "fp16", "fp16"))):
        net = training_network(dev, *switches, optimizer="adam", lr=cases.TRAIN_LR["adam"])
        t, out_wh = tc._target(net, dev)
        xd = pc.to(dev, x)
        runs[name] = [float(net.train([xd], t).item()) for _ in range(steps)]
    dec32, dec = runs["fp32"][0] - runs["fp32"][-1], runs["half"][0] - runs["half"][-1]
    rho_ref, oracle = oracle_loss_gap(out_wh, steps)
    rho = max(rho_ref, tc.LOSS_GAP_MEASURED / dec32)
    print("half-gradient training, %d Adam steps: fp32 %.9g -> %.9g, half gradients %.9g -> %.9g (%.6g of the fp32 decrease); oracle "
          "plain %.9g -> %.9g, gradients stored %.9g -> %.9g: rho %.3g (floor %.3g); peak of the last step %.6g"
          % (steps, runs["fp32"][0], runs["fp32"][-1], runs["half"][0], runs["half"][-1], dec / dec32, oracle["plain"][0],
             oracle["plain"][-1], oracle["grad-stored"][0], oracle["grad-stored"][-1], rho_ref, tc.LOSS_GAP_MEASURED / dec32,
             net.model.module.half_gradient_peak()))
    assert runs["half"][-1] < runs["half"][0]
    assert dec32 > 0 and dec >= (1 - 3 * rho) * dec32, (dec, dec32, rho)
    assert net.model.module.half_gradient_peak() < 65504.0
    return runs
