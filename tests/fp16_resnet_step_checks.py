"""ResnetSimple with train_gemm_precision="fp16", above the single launch: one Bottleneck at a time, the whole step, twenty optimizer steps.

The end-to-end gradient distance that holds the hourglass does not work here: through 33 Bottlenecks with batch statistics the trunk
gradients of a reference whose 1x1 products see rounded operands are decorrelated from the plain reference's (relative distance ~1), so a
bound of three times that distance would pass anything.  What IS conditioned, and is held here:

* one Bottleneck on a given input and incoming gradient: E = the larger of the float32 / float64 relative distances, per tensor, between
  the CPU reference block with q() on the products of its covered convs and the plain block (computed here, milliseconds); the device's
  fp16 block against its own fp32 block is held to 3 E per tensor (the project's standing margin);
* the whole step: the loss, and the gradients of the last decoder BatchNorm and the head (the four tensors with E_p <= 0.05);
* training: the gap between the final losses of a rounded and a plain run of twenty steps, over the plain run's decrease.

q(): an activation operand as half(clamp(x)), a gradient / weight operand as half(t 2^e) 2^-e with e from the tensor's amax
(fp16_resnet_train_checks).  Covered convs: the 1x1 convs of a Bottleneck (conv1, conv3, downsample) and its stride-2 3x3 conv, which
runs on its patch rows over the 1x1 GEMM at these sizes (the stride-1 3x3 convs are Winograd convs: fp32, bit-equal).
"""
import copy
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

import cases
import parity_checks as pc
from fp16_resnet_train_checks import q_act, q_scaled
from dream_amd import models, ops
from oracle import models as om

BLOCKS = ["layer1.0", "layer2.0", "layer3.1", "layer3.22", "layer4.0", "layer4.2"]
BLOCK_HW = {"layer1.0": 16, "layer2.0": 16, "layer3.1": 5, "layer3.22": 5, "layer4.0": 5, "layer4.2": 3}
STEP_SHAPE = (2, 64, 64)
CONDITIONED = ("upsample.10.weight", "upsample.10.bias", "upsample.12.weight", "upsample.12.bias")
# measured on the CPU reference by rounded_training_gaps() (rounded against plain, twenty steps on the fixed batch): the gap of the final
# losses over the plain run's decrease; the CPU suite recomputes them and asserts that they hold
TRAIN_STEPS = 20
TRAIN_LR = {"adam": 1e-4, "sgd": 1e-2}
TRAIN_GAP = {"adam": 1.16e-2, "sgd": 0.40e-2}      # (losses 1.2864 -> 0.3474 plain / 0.3365 rounded; 1.2864 -> 0.4436 / 0.4469)


class _RoundedConv(torch.autograd.Function):
    """A bias-free conv whose three products see q() of their operands, in the dtype of the run."""

    @staticmethod
    def forward(ctx, x, w, stride, padding):
        ctx.save_for_backward(x, w)
        ctx.geom = (stride, padding)
        return F.conv2d(q_act(x).to(x.dtype), q_scaled(w).to(x.dtype), None, stride, padding)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        stride, padding = ctx.geom
        gq, wq, xq = q_scaled(g).to(g.dtype), q_scaled(w).to(g.dtype), q_act(x).to(g.dtype)
        dx = torch.nn.grad.conv2d_input(x.shape, wq, gq, stride, padding)
        dw = torch.nn.grad.conv2d_weight(xq, w.shape, gq, stride, padding)
        return dx, dw, None, None


def covered_reference_convs(module):
    """The reference's Conv2d modules inside Bottlenecks that the rule covers at the sizes used here."""
    out = []
    for mod in module.modules():
        if isinstance(mod, nn.Conv2d) and mod.bias is None and (tuple(mod.kernel_size) == (1, 1) or
                                                                  (tuple(mod.kernel_size) == (3, 3) and tuple(mod.stride) == (2, 2))):
            out.append(mod)
    return out


def _round_convs(module):
    for mod in covered_reference_convs(module):
        mod.forward = (lambda m: lambda inp: _RoundedConv.apply(inp, m.weight, m.stride, m.padding))(mod)


@functools.lru_cache(maxsize=None)
def _weights():
    return om.recipe_weights(om.build_model("resnet_h", 7).state_dict())


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---- one Bottleneck -----------------------------------------------------------------------------------------------------------------
def block_case(name):
    layer, index = name.split(".")
    ref = om.build_model("resnet_h", 7)
    ref.load_state_dict(_weights())
    blk = getattr(ref, layer)[int(index)]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    hw = BLOCK_HW[name]
    x = torch.randn(2, blk.conv1.in_channels, hw, hw, generator=g).clamp_min(0.0)
    y = blk.train()(x)
    return blk, x, 1e-4 * torch.randn(y.shape, generator=g)


def reference_block_grads(blk, x, gy, dtype, rounded):
    blk = copy.deepcopy(blk).to(dtype).train()
    if rounded:
        _round_convs(blk)
    xin = x.detach().clone().to(dtype).requires_grad_()
    blk(xin).backward(gy.to(dtype))
    out = {n: p.grad for n, p in blk.named_parameters()}
    out["dx"] = xin.grad
    return out


def block_yardstick(name):
    blk, x, gy = block_case(name)
    E = {}
    for dtype in (torch.float32, torch.float64):
        plain = reference_block_grads(blk, x, gy, dtype, False)
        rounded = reference_block_grads(blk, x, gy, dtype, True)
        for k in plain:
            E[k] = max(E.get(k, 0.0), _rel(rounded[k], plain[k]))
    return E


def device_block(net, name, x, gy, train_gemm_precision):
    """One Bottleneck of ``net`` (a dream_amd ResnetSimple in training mode) as run_forward_train / _bwd_block run it, on a given input and
    incoming gradient -> ({parameter name | "dx": gradient}, the 3x3 conv's (input, output))."""
    blk = dict(net._trunk())[name]
    net.train_gemm_precision = train_gemm_precision
    half = net._resolve_switches(True).train16
    net._packs.restart_pools()
    tape = []
    y = ops.nchw_to_nhwc(x)
    ds, idt = None, y
    if hasattr(blk, "downsample"):
        ds = net._unit(tape, name + ".ds", y, blk.downsample[0], blk.downsample[1], relu=False, src=None, train16=half)
        idt = ds["y"]
    r1 = net._unit(tape, name + ".1", y, blk.conv1, blk.bn1, relu=True, src=None, train16=half)
    r2 = net._unit(tape, name + ".2", r1["y"], blk.conv2, blk.bn2, relu=True, src=r1, materialize=False, train16=half)
    assert net._gemm1x1(blk.conv3, r2["z"])
    r3 = net._unit(tape, name + ".3", r2["z"], blk.conv3, blk.bn3, relu=True, residual=idt, src=r2, pre=True, train16=half)
    rec = dict(kind="block", name=name, ds=ds, u1=r1, u2=r2, u3=r3, src=None)
    bw = dict(grads=models._GradDict(None), side=None, reducer=None, grad_out=None)
    dx = net._bwd_block(rec, ops.nchw_to_nhwc(gy), bw)
    out = {n: bw["grads"][p].detach().cpu().clone() for n, p in blk.named_parameters()}
    out["dx"] = ops.nhwc_to_nchw(dx).cpu()
    covered = [net._half_unit(r) for r in (r1, r2, r3) + ((ds,) if ds is not None else ())]
    return out, (r1["y"].cpu(), r2["z"].cpu()), covered


@functools.lru_cache(maxsize=None)
def _device_resnet(dev):
    net = models.ResnetSimple(7, pretrained=False)
    net.load_state_dict(_weights())
    return (net.to(dev) if dev != "cpu" else net).train()


def check_block(dev, name):
    E = block_yardstick(name)
    print("%s: E per tensor %s" % (name, {k: "%.3g" % v for k, v in E.items()}))
    assert 1e-3 < max(E.values()) < 0.1                       # the yardstick is a rounding distance, neither nothing nor everything
    net = _device_resnet(dev)
    _, x, gy = block_case(name)
    g32, (a32, z32), cov32 = device_block(net, name, pc.to(dev, x), pc.to(dev, gy), "fp32")
    g16, (a16, z16), cov16 = device_block(net, name, pc.to(dev, x), pc.to(dev, gy), "fp16")
    net.train_gemm_precision = "fp32"
    stride2 = tuple(dict(net._trunk())[name].conv2.stride) == (2, 2)
    assert not any(cov32) and cov16 == [True, stride2, True] + ([True] if len(cov16) == 4 else [])
    for k in E:
        d = _rel(g16[k], g32[k])
        print("  %-22s device fp16 against fp32 %.3g   (3 E = %.3g)" % (k, d, 3 * E[k]))
        assert bool(torch.isfinite(g16[k]).all()) and d <= 3 * E[k], (name, k, d, E[k])
        if k.endswith("weight") and g16[k].dim() == 4 and g16[k].shape[-1] == 1:
            assert not torch.equal(g16[k], g32[k]), (name, k)          # every 1x1 weight gradient comes from the half product
    if not stride2:
        # the Winograd 3x3 conv is not covered: on the fp32 block's own input its launch is the fp32 launch, bit for bit (its input in
        # the fp16 block differs, so the conv is run again on the fp32 block's input with the switch on)
        blk = dict(net._trunk())[name]
        again = net._unit([], name + ".2", pc.to(dev, a32), blk.conv2, blk.bn2, relu=True, src=None, materialize=False, train16=True)["z"].cpu()
        assert torch.equal(again, z32), name


# ---- the whole step -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_case(shape=STEP_SHAPE):
    b, h, w = shape
    return torch.from_numpy(cases.image_batch(b, h, w, seed=7))


def _target(out_wh, shape=STEP_SHAPE):
    b, h, w = shape
    return torch.from_numpy(cases.target_batch(b, 7, out_wh, in_wh=(w, h), seed=7))


def _reference_model(dtype, rounded):
    model = om.build_model("resnet_h", 7)
    model.load_state_dict(_weights())
    model = model.to(dtype).train()
    if rounded:
        _round_convs(model)
    return model


def step_yardstick(out_wh, shape=STEP_SHAPE):
    """-> ({parameter: E_p}, the rounded reference's relative move of the loss): the larger of float32 / float64; once per shape."""
    return _step_yardstick(out_wh, shape)


@functools.lru_cache(maxsize=None)
def _step_yardstick(out_wh, shape):
    E, move = {}, 0.0
    for dtype in (torch.float32, torch.float64):
        res = []
        for rounded in (False, True):
            model = _reference_model(dtype, rounded)
            loss = F.mse_loss(model(step_case(shape).to(dtype))[0], _target(out_wh, shape).to(dtype))
            loss.backward()
            res.append((float(loss), {n: p.grad.double() for n, p in model.named_parameters()}))
        (l0, g0), (l1, g1) = res
        move = max(move, abs(l1 - l0) / abs(l0))
        for n in g0:
            E[n] = max(E.get(n, 0.0), _rel(g1[n], g0[n]))
    return E, move


def network(dev, train_gemm_precision="fp32", precision="fp32", optimizer="sgd", lr=0.0, shape=STEP_SHAPE):
    b, h, w = shape
    net = pc.build_network("resnet_h", dev, weights=_weights(), optimizer=optimizer, lr=lr, in_res=(w, h))
    net.model.module.precision = precision
    net.model.module.train_gemm_precision = train_gemm_precision
    net.enable_training()
    return net


def _device_step(dev, train_gemm_precision, precision="fp32", shape=STEP_SHAPE):
    net = network(dev, train_gemm_precision, precision, shape=shape)
    ow, oh = net.trained_net_output_resolution()
    loss = float(net.train([pc.to(dev, step_case(shape))], pc.to(dev, _target((ow, oh), shape))).item())
    return loss, {n: p.grad.detach().cpu().clone() for n, p in net.model.module.named_parameters()}, (ow, oh)


def check_step(dev, shape=STEP_SHAPE, conditioned=CONDITIONED):
    """``conditioned``: the tensors whose E_p the yardstick puts at or below 0.05 at ``shape`` (asserted: the selection is the rule's, on
    the reference, at every shape)."""
    l32, g32, out_wh = _device_step(dev, "fp32", shape=shape)
    l16, g16, _ = _device_step(dev, "fp16", shape=shape)
    lp, gp, _ = _device_step(dev, "fp32", precision="fp16", shape=shape)
    assert lp == l32 and all(torch.equal(gp[n], g32[n]) for n in g32)      # precision is an inference switch: the fp32 step, bit for bit
    E, move = step_yardstick(out_wh, shape)
    small = sorted(n for n, e in E.items() if e <= 0.05)
    print("loss fp32 %.9g fp16 %.9g (relative %.3g; the rounded reference moves %.3g); E_p <= 0.05: %s"
          % (l32, l16, abs(l16 - l32) / l32, move, {n: "%.3g" % E[n] for n in small}))
    assert small == sorted(conditioned), small
    assert abs(l16 - l32) <= 3 * move * abs(l32)
    for n in g32:
        assert bool(torch.isfinite(g16[n]).all()), n
    worst = 0.0
    for n in conditioned:
        d = _rel(g16[n], g32[n])
        worst = max(worst, d / E[n])
        print("  %-20s device fp16 against fp32 %.3g   (3 E_p = %.3g)" % (n, d, 3 * E[n]))
        assert d <= 3 * E[n], (n, d, E[n])
    print("  worst r_p / E_p %.3g" % worst)
    assert not torch.equal(g16["layer3.1.conv1.weight"], g32["layer3.1.conv1.weight"])


# ---- training still trains --------------------------------------------------------------------------------------------------------
def _reference_run(optimizer, rounded, out_wh, steps=TRAIN_STEPS):
    model = _reference_model(torch.float32, rounded)
    opt = (torch.optim.Adam if optimizer == "adam" else torch.optim.SGD)(model.parameters(), lr=TRAIN_LR[optimizer])
    x, t, losses = step_case(), _target(out_wh), []
    for _ in range(steps):
        opt.zero_grad()
        loss = F.mse_loss(model(x)[0], t)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return losses


def rounded_training_gap(optimizer, out_wh):
    """The CPU reference's gap between the final losses of the rounded and the plain run over the plain run's decrease."""
    plain, rounded = _reference_run(optimizer, False, out_wh), _reference_run(optimizer, True, out_wh)
    return abs(rounded[-1] - plain[-1]) / (plain[0] - plain[-1]), plain, rounded


def check_training_trains(dev, optimizer):
    runs = {}
    for tp in ("fp32", "fp16"):
        net = network(dev, tp, optimizer=optimizer, lr=TRAIN_LR[optimizer])
        ow, oh = net.trained_net_output_resolution()
        x, t = pc.to(dev, step_case()), pc.to(dev, _target((ow, oh)))
        runs[tp] = [float(net.train([x], t).item()) for _ in range(TRAIN_STEPS)]
    gap = abs(runs["fp16"][-1] - runs["fp32"][-1]) / (runs["fp32"][0] - runs["fp32"][-1])
    print("%s, %d steps: fp32 %.6g -> %.6g, fp16 %.6g -> %.6g, gap over the fp32 decrease %.3g (3 x measured = %.3g)"
          % (optimizer, TRAIN_STEPS, runs["fp32"][0], runs["fp32"][-1], runs["fp16"][0], runs["fp16"][-1], gap, 3 * TRAIN_GAP[optimizer]))
    assert runs["fp16"][-1] < runs["fp16"][0]
    assert gap <= 3 * TRAIN_GAP[optimizer], (gap, TRAIN_GAP[optimizer])
