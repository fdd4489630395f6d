"""Checks of train_precision="fp16" (csrc/wgrad_f16.hip, the ReLU-mask epilogue of csrc/conv_f16.hip, the host wiring of
DreamHourglass), shared by the emulator suite (test_fp16_train_emulated.py) and the GPU suite (test_gpu_fp16_train.py).

Per launch the bounds are derived, as in fp16_checks: the kernel computes the gradient of the ROUNDED operands q(x), q(dy) (q(dy), q(w)
for the data gradient) -- a product of two halfs is exact in fp32 --, so against the fp64 gradient of those it may differ by the fp32
accumulation only (5e-6 of max|ref|; measured on the CPU with torch's fp32 accumulation for these inputs: at most 4.2e-7).  The fp64
gradient of the UNROUNDED operands must lie more than 5e-5 away (measured 2.3e-4 .. 3.7e-4), or the launch under test did not round.

End to end the bound is measured on the reference, by rounded_training_oracle(): oracle.models with q() applied to the operands of the
forward, data-gradient and weight-gradient products of exactly the plain convs (3x3 stride 1, not behind an upsample, not the K-channel
output, cin % 32 == cout % 32 == 0), run in float32 and in float64.  Per parameter r_p = |g - g_plain|_2 / |g_plain|_2 against the
plain reference of the same dtype, E_p = the larger r_p of the two runs; the device's |g16 - g32|_2 / |g32|_2 is held to 3 E_p.

Twenty Adam steps on one fixed 2 x 64 x 96 batch (check_training_trains): the fp16 run's final loss is below its first, and the gap
between the final losses of the fp16 and the fp32 run, |L16 - L32|, is held to three times LOSS_GAP_MEASURED, the value of the first
MI355X run: 5.4054e-06 (fp32 0.0507833 -> 0.00509373, fp16 0.0507714 -> 0.00508833: 1.2e-4 of the fp32 run's own decrease)."""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

import cases
import parity_checks as pc
from dream_amd import ops
from fp16_checks import _amax_value, q
from oracle import models as om

# |final loss (fp16) - final loss (fp32)| after twenty Adam steps on the fixed batch of check_training_trains, first MI355X run:
# fp32 0.0507832654 -> 0.00509373285, fp16 0.0507714003 -> 0.00508832745; the gap is 1.2e-4 of the fp32 run's own decrease
LOSS_GAP_MEASURED = 5.4054e-06

WGRAD_SHAPES = [
    # (B, H, W, Cin, Cout, x_scale, g_scale)
    (1, 7, 9, 32, 32, 1.0, 1.0),            # one partial tile, odd sides
    (2, 12, 20, 64, 96, 1.0, 1e-4),         # two images, more row blocks than column blocks
    (3, 9, 11, 64, 64, 300.0, 1e-6),
    (2, 16, 24, 128, 64, 1.0, 1.0),         # several channel chunks
]
SPLITK_ONE = (1, 8, 16, 32, 32, 1.0, 1.0)   # one position tile: nothing to split
SPLITK_MANY = (4, 32, 32, 32, 32, 1.0, 1.0)


def wgrad_inputs(B, H, W, Cin, Cout, x_scale=1.0, g_scale=1.0, seed=0):
    """x = relu(randn) with an outlier at one corner, dy = randn with half of it zeroed and an outlier at the opposite corner (the two
    outliers meet under no tap: their exact product would set max|ref| and hide the rounding)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g).relu() * x_scale
    x[0, 0, 0, 0] = 40 * x_scale
    dy = torch.randn(B, Cout, H, W, generator=g) * g_scale
    dy = dy * (torch.rand(B, Cout, H, W, generator=g) < 0.5)
    dy[B - 1, Cout - 1, H - 1, W - 1] = 30 * g_scale
    assert B > 1 or (H > 2 and W > 2)
    return x, dy


def wgrad_reference(x, dy):
    """fp64 weight gradient of a 3x3 stride-1 pad-1 conv [Cout,Cin,3,3]."""
    w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, padding=1).backward(dy.double())
    return w.grad


def run_wgrad(dev, x, dy, flags=0):
    cout, cin = int(dy.shape[1]), int(x.shape[1])
    xd, gd = pc.to(dev, pc._nhwc(x)), pc.to(dev, pc._nhwc(dy))
    dw, db = ops.conv3x3_wgrad_f16(xd, ops.absmax(xd), gd, ops.absmax(gd), cout, cin, flags)
    return dw.cpu(), db.cpu()


def check_wgrad_f16(dev, B, H, W, Cin, Cout, x_scale=1.0, g_scale=1.0, seed=0):
    x, dy = wgrad_inputs(B, H, W, Cin, Cout, x_scale, g_scale, seed)
    dw, db = run_wgrad(dev, x, dy)
    ref, ref_unrounded = wgrad_reference(q(x), q(dy)), wgrad_reference(x, dy)
    scale = float(ref.abs().max())
    err = float((dw.double() - ref).abs().max()) / scale
    away = float((ref_unrounded - ref).abs().max()) / scale
    ref_b = dy.double().sum((0, 2, 3))
    berr = float((db.double() - ref_b).abs().max()) / float(ref_b.abs().max())
    print("fp16 wgrad %s: err %.3g of max|ref|, unrounded operands %.3g away, bias err %.3g" % ((B, H, W, Cin, Cout), err, away, berr))
    assert tuple(dw.shape) == (Cout, Cin, 3, 3) and tuple(db.shape) == (Cout,)
    assert err <= 5e-6, (err,)
    assert away > 5e-5, (away,)                   # (so a kernel that does not round its operands cannot pass the line above)
    assert berr <= 5e-6, (berr,)                  # the bias gradient sums the unrounded dy
    return err


def check_wgrad_f16_splitk(dev):
    """The split-count query answers 1 for a single position tile and >= 2 for a shape with many; both reduce paths are right."""
    for shape, many in ((SPLITK_ONE, False), (SPLITK_MANY, True)):
        b, h, w, cin, cout = shape[:5]
        sk = ops.conv3x3_wgrad_f16_splitk(b, h, w, cin, cout)
        assert (sk >= 2) if many else (sk == 1), (shape, sk)
        check_wgrad_f16(dev, *shape)


def check_wgrad_f16_zero_and_repeat(dev):
    x, dy = wgrad_inputs(2, 12, 20, 64, 96, seed=3)
    dw, db = run_wgrad(dev, x, torch.zeros_like(dy))
    assert torch.equal(dw, torch.zeros_like(dw)) and torch.equal(db, torch.zeros_like(db))     # exactly zero, no NaN
    a, b = run_wgrad(dev, x, dy), run_wgrad(dev, x, dy)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                                 # fixed-order reduction: same bits
    try:
        run_wgrad(dev, x, dy, flags=ops.CONV_UPSAMPLE2X)
    except RuntimeError as e:
        assert "flags" in str(e)
    else:
        raise AssertionError("a non-zero flags argument must be refused")


def check_dgrad_f16(dev, B, H, W, Cout, Cin, seed=0):
    """conv2d_f16 with relu_mask and the mode-1 packed plane (dy with Cout channels -> dx with Cin) against
    conv_transpose2d(q(dy), q(w), padding=1) * (mask > 0) in fp64; the published amax is max|y| after the mask."""
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(B, Cout, H, W, generator=g)
    dy[0, 0, 0, 0] = 40.0
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1
    mask = torch.randn(B, Cin, H, W, generator=g).relu()           # about half zeros, exactly 0
    mask[0, :, 0, 0] = 0.0

    def reference(gv, wv):
        return F.conv_transpose2d(gv.double(), wv.double(), padding=1) * (mask > 0)

    p16 = ops.pack_conv_weight_f16(pc.to(dev, w), 1)
    gd = pc.to(dev, pc._nhwc(dy))
    y, amax = ops.conv2d_f16(gd, ops.absmax(gd), p16, p16[3], 3, relu_mask=pc.to(dev, pc._nhwc(mask)))
    got = y.cpu().permute(0, 3, 1, 2)
    ref, ref_unrounded = reference(q(dy), q(w)), reference(dy, w)
    scale = float(ref.abs().max())
    err = float((got.double() - ref).abs().max()) / scale
    away = float((ref_unrounded - ref).abs().max()) / scale
    print("fp16 masked dgrad %s: err %.3g of max|ref|, unrounded operands %.3g away" % ((B, H, W, Cout, Cin), err, away))
    assert p16[3] == Cin and tuple(got.shape) == (B, Cin, H, W)
    assert err <= 5e-6, (err,)
    assert away > 5e-5, (away,)
    assert bool((got[mask <= 0] == 0).all()) and bool((got[mask > 0] != 0).any())
    assert abs(_amax_value(amax) - float(got.abs().max())) <= 1e-6 * scale
    return err


def check_dgrad_f16_shapes(dev, seed=0):
    check_dgrad_f16(dev, 1, 7, 9, 64, 32, seed=seed)
    check_dgrad_f16(dev, 2, 12, 20, 32, 64, seed=seed)


# ---- the layer rule --------------------------------------------------------------------------------------------------------------
def is_plain(kind, mod, flags, in_channels=None):
    """The rule of train_precision="fp16" for one plan entry (``in_channels``: channels the entry's input carries, None: cin)."""
    if kind != "conv" or flags & (ops.CONV_UPSAMPLE2X | ops.CONV_OUT_NCHW):
        return False
    cout, cin = int(mod.weight.shape[0]), int(mod.weight.shape[1])
    return (in_channels is None or in_channels == cin) and cin % 32 == 0 and cout % 32 == 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------
class _RoundedConv(torch.autograd.Function):
    """A 3x3 stride-1 pad-1 conv whose three products (forward, data gradient, weight gradient) see q() of their operands; the bias
    gradient sums the unrounded dy."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return F.conv2d(q(x), q(w), b, padding=1)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gq = q(g)
        dx = F.conv_transpose2d(gq, q(w), padding=1)
        dw = torch.nn.grad.conv2d_weight(q(x), w.shape, gq, padding=1)
        return dx, dw, g.sum((0, 2, 3))


def _plain_reference_convs(model):
    """The reference's Conv2d modules that the rule covers: 3x3, channels multiples of 32, not directly behind an nn.Upsample."""
    out, prev = [], None
    for mod in model.modules():
        if len(list(mod.children())):
            continue
        if (isinstance(mod, nn.Conv2d) and tuple(mod.kernel_size) == (3, 3) and mod.in_channels % 32 == 0 and mod.out_channels % 32 == 0
                and not isinstance(prev, nn.Upsample)):
            out.append(mod)
        prev = mod
    return out


def _reference_grads(weights, x, target, dtype, rounded):
    model = om.build_model("vgg_q", 7)
    model.load_state_dict(weights)
    model = model.to(dtype).train()
    plain = _plain_reference_convs(model)
    if rounded:
        for mod in plain:
            mod.forward = (lambda m: lambda inp: _RoundedConv.apply(inp, m.weight, m.bias))(mod)
    loss = F.mse_loss(model(x.to(dtype))[0], target.to(dtype))
    loss.backward()
    return {n: p.grad.double() for n, p in model.named_parameters()}, len(plain)


TRAIN_SHAPE = (2, 64, 96)


def training_case(shape=TRAIN_SHAPE):
    """(weights, input batch) of the training checks at ``shape`` = (B, H, W); computed once per process and shape."""
    return _training_case(tuple(shape))


@functools.lru_cache(maxsize=None)
def _training_case(shape):
    b, h, w = shape
    wts = om.recipe_weights(om.build_model("vgg_q", 7).state_dict(), cases.TRAIN_FINAL_KEYS, cases.TRAIN_FINAL_SCALE)
    x = torch.from_numpy(cases.image_batch(b, h, w, seed=7))
    return wts, x


def rounded_training_oracle(out_wh, shape=TRAIN_SHAPE):
    """{parameter name: E_p}, and the number of plain convs the reference has; computed once per process and shape."""
    return _rounded_training_oracle(out_wh, shape)


@functools.lru_cache(maxsize=None)
def _rounded_training_oracle(out_wh, shape):
    wts, x = training_case(shape)
    b, h, w = shape
    t = torch.from_numpy(cases.target_batch(b, 7, out_wh, in_wh=(w, h), seed=7))
    E, nplain = {}, 0
    for dtype in (torch.float32, torch.float64):
        plain, _ = _reference_grads(wts, x, t, dtype, rounded=False)
        rounded, nplain = _reference_grads(wts, x, t, dtype, rounded=True)
        for n in plain:
            r = float((rounded[n] - plain[n]).norm() / plain[n].norm())
            E[n] = max(E.get(n, 0.0), r)
    return E, nplain


def training_network(dev, train_precision="fp32", precision="fp32", optimizer="sgd", lr=0.0, shape=TRAIN_SHAPE):
    wts, _ = training_case(shape)
    b, h, w = shape
    net = pc.build_network("vgg_q", dev, weights=wts, optimizer=optimizer, lr=lr, in_res=(w, h))
    net.model.module.precision = precision
    net.model.module.train_precision = train_precision
    net.enable_training()
    return net


def _target(net, dev, shape=TRAIN_SHAPE):
    b, h, w = shape
    ow, oh = net.trained_net_output_resolution()
    return pc.to(dev, torch.from_numpy(cases.target_batch(b, 7, (ow, oh), in_wh=(w, h), seed=7))), (ow, oh)


def step_gradients(dev, train_precision="fp32", precision="fp32", shape=TRAIN_SHAPE):
    """{parameter name: gradient} of one training step (SGD with lr = 0: the parameters stay, .grad is read), and the loss."""
    net = training_network(dev, train_precision, precision, shape=shape)
    _, x = training_case(shape)
    t, out_wh = _target(net, dev, shape)
    loss = float(net.train([pc.to(dev, x)], t).item())
    grads = {n: p.grad.detach().cpu().clone() for n, p in net.model.module.named_parameters()}
    return grads, loss, out_wh, net


def check_training_step(dev, shape=TRAIN_SHAPE):
    """One vgg_q training step at ``shape`` (2 x 64 x 96) with train_precision="fp16" against the fp32 step of the same build."""
    g32, loss32, out_wh, net = step_gradients(dev, "fp32", shape=shape)
    g16, loss16, _, _ = step_gradients(dev, "fp16", shape=shape)
    E, nplain_ref = rounded_training_oracle(out_wh, shape)
    module = net.model.module
    names = {id(p): n for n, p in module.named_parameters()}
    plain_w = {names[id(mod.weight)] for kind, mod, flags in module.plan_layers() if mod is not None and is_plain(kind, mod, flags)}
    assert len(plain_w) == nplain_ref and len(plain_w) > 10, (len(plain_w), nplain_ref)
    worst = 0.0
    for n in sorted(g32):
        r = float((g16[n].double() - g32[n].double()).norm() / g32[n].double().norm())
        print("fp16 training %-40s r_p %.3g  E_p %.3g" % (n, r, E[n]))
        worst = max(worst, r / E[n])
        assert r <= 3 * E[n], (n, r, E[n])
        if n in plain_w:
            assert not torch.equal(g16[n], g32[n]), n          # (the half-precision weight gradient really ran)
    print("fp16 training: losses %.9g (fp32) %.9g (fp16), worst r_p / E_p %.3g" % (loss32, loss16, worst))
    # precision="fp16" alone stays an inference mode: the fp32 step bit for bit
    g_inf, loss_inf, _, _ = step_gradients(dev, "fp32", precision="fp16", shape=shape)
    assert loss_inf == loss32
    for n in g32:
        assert torch.equal(g_inf[n], g32[n]), n


def check_non_plain_entries_bit_equal(dev):
    """Every non-plain plan entry gives the fp32 path's output, bit for bit, when both are given the same input: the saved
    (input, output) pairs of a train_precision="fp16" forward, re-run entry by entry on a train_precision="fp32" module."""
    net = training_network(dev, "fp16")
    _, x = training_case()
    m = net.model.module
    params = [p.detach() for p in m.plan_parameters()]
    with torch.no_grad():
        out16, saved16 = m.run_forward(pc.to(dev, x), params, True)
        m.train_precision = "fp32"
        out32, saved32 = m.run_forward(pc.to(dev, x), params, True)
        layers = m.plan_layers()
        checked = differs = 0
        for li, (kind, mod, flags) in enumerate(layers):
            inp, out = saved16[li]
            if kind == "pool":                                     # the fp32 walk's launch for a pool entry, on the same input
                assert torch.equal(ops.maxpool2(inp), out), (li, kind)
                checked += 1
            if mod is None or kind in ("first", "wide"):
                continue
            w, bias = params[m._param_slot[li]], params[m._param_slot[li] + 1]
            again, _ = m._conv_fp32(kind, mod, inp, None, w, bias, flags)
            if is_plain(kind, mod, flags, int(inp.shape[3])):
                differs += int(not torch.equal(again, out))
            else:
                assert torch.equal(again, out), (li, kind)
                checked += 1
    assert checked >= 3 and differs >= 10, (checked, differs)
    assert torch.equal(saved16[0][1], saved32[0][1])                 # the first conv: same input, same launch
    assert not torch.equal(out16, out32)


def check_rejections(dev):
    from dream_amd import models
    net = training_network(dev, "fp32")
    _, x = training_case()
    t, _ = _target(net, dev)
    net.model.module.train_precision = "bf16"
    try:
        net.train([pc.to(dev, x)], t)
    except ValueError as e:
        assert "train_precision" in str(e)
    else:
        raise AssertionError("train_precision='bf16' must raise")
    net.model.module.train_precision = "fp32"
    resnet = models.ResnetSimple(7, pretrained=False)
    assert resnet.train_precision == "fp32"
    resnet.train_precision = "fp32"
    try:
        resnet.train_precision = "fp16"
    except ValueError:
        pass
    else:
        raise AssertionError("ResnetSimple must refuse train_precision='fp16'")

def check_training_trains(dev, steps=20):
    """Twenty Adam steps on one fixed batch in both precisions -> (first, final) losses per precision; the fp16 run's loss falls,
    and its final loss is within 3 x LOSS_GAP_MEASURED of the fp32 run's."""
    _, x = training_case()
    runs = {}
    for tp in ("fp32", "fp16"):
        net = training_network(dev, tp, optimizer="adam", lr=cases.TRAIN_LR["adam"])
        t, _ = _target(net, dev)
        xd = pc.to(dev, x)
        runs[tp] = [float(net.train([xd], t).item()) for _ in range(steps)]
    gap = abs(runs["fp16"][-1] - runs["fp32"][-1])
    print("fp16 training, %d Adam steps: fp32 %.9g -> %.9g, fp16 %.9g -> %.9g, gap of the final losses %.6g (%.3g of the fp32 decrease)"
          % (steps, runs["fp32"][0], runs["fp32"][-1], runs["fp16"][0], runs["fp16"][-1], gap,
             gap / max(runs["fp32"][0] - runs["fp32"][-1], 1e-30)))
    assert runs["fp16"][-1] < runs["fp16"][0]
    assert gap <= 3 * LOSS_GAP_MEASURED, (gap, LOSS_GAP_MEASURED)
    return runs
