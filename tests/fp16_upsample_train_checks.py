"""What the CPU suite (kernels under the SIMT emulator) and the GPU suite share for DreamHourglass's train_upsample_precision="fp16"
(DESIGN.md 4.8o): the convs behind nn.Upsample(2) as the equivalent ConvTranspose2d(k4,s2,p1) on the fp16 matrix cores -- forward
ops.conv_transpose4x4s2_f16 on the "ups_f16" pack, data gradient ops.conv_transpose4x4s2_dgrad_f16 on the "ups_f16b" plane, weight
gradient ops.upsample_conv3x3_wgrad_f16 (wgrad_convT4_f16_xs_kernel + the folding reduce of csrc/wgrad_f16.hip).

Per launch (the project's bounds, 4.8c / 4.8n): against the fp64 result of the ROUNDED operands a launch may differ by the fp32
accumulation, 5e-6 of max|ref|; the fp64 result of the UNROUNDED operands has to lie more than 5e-5 of that maximum away.  The weight
gradient's reference is the 3x3 form -- the gradient of a 3x3 conv on the nearest-upsampled q(x) against q(dz) --, which shares nothing
with the 4x4 path.  The operands the device rounds: x and dz, each scaled by its own amax, and the COLLAPSED 4x4 weight.

One block, whole step, twenty optimizer steps: E / E_p / the gaps are distances on the CPU reference between a run that rounds exactly
those operands (the upsample conv restated as conv_transpose2d with the collapsed weight) and one that does not, train_precision="fp16"
(the plain convs rounded, fp16_train_checks) in both; the device's switch on against off is held to three times that."""
import contextlib
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

import cases
import fp16_train_checks as tc
import parity_checks as pc
from fp16_resnet_decoder_checks import NUM_VARIANTS
from fp16_resnet_train_checks import ACC_BOUND, ROUNDING_GAP, q_act, q_scaled, scale_exponent, _amax_of, _assert_close, _gen
from dream_amd import ops
from oracle import models as om

# (B, H, W, Cin, Cout) of the low-resolution x [B,H,W,Cin]; dz is [B,2H,2W,Cout].  5 x 7: odd, ragged 8 x 16 position tiles, every border
# tap, one position tile per frame (split 2); 1 x 1: a single tile (split 1), every tap but four falls outside
SHAPES = [(2, 5, 7, 32, 32), (2, 5, 7, 64, 96), (1, 1, 1, 32, 96), (1, 1, 1, 64, 32)]
SPLIT_SHAPE = (2, 9, 17, 32, 32)                 # 8 position tiles
VARIANT_SHAPE = (2, 5, 7, 64, 96)
SCALES = [(1.0, 3e-4), (2.0 ** -16, 1e-6), (2.0 ** 10, 1e-6)]          # (x_scale, g_scale)
BLOCK = "upsample_0_4"
BLOCK_SHAPE = (2, 4, 6)                          # the block's input at a 2 x 64 x 96 batch: 64 / 16 x 96 / 16, 512 channels
TRAIN_STEPS = 20
# measured on the CPU reference by rounded_training_gap() (upsample convs rounded against not, the plain convs rounded in both, twenty
# steps on the fixed batch): the gap of the final losses over the unrounded run's decrease; the CPU suite recomputes them
TRAIN_GAP = {"adam": 3.31e-4, "sgd": 1.93e-2}

_K = torch.tensor([[0., 0., 1.], [0., 1., 1.], [1., 1., 0.], [1., 0., 0.]])      # [ky][r] = 1 where ky in K(r): K(0)={2,3}, K(1)={1,2}, K(2)={0,1}


def collapse(w):
    """Conv2d weight [Cout,Cin,3,3] behind a nearest x2 upsample -> the equivalent ConvTranspose2d(k4,s2,p1) weight [Cin,Cout,4,4]."""
    k = _K.to(w.dtype)
    return torch.einsum("yr,oirc,xc->ioyx", k, w, k).contiguous()


def fold(g4):
    """Its adjoint: a gradient [Cin,Cout,4,4] -> [Cout,Cin,3,3]."""
    k = _K.to(g4.dtype)
    return torch.einsum("yr,ioyx,xc->oirc", k, g4, k).contiguous()


def _operands(shape, x_scale=1.0, g_scale=3e-4, seed=0, zero_dz=False):
    b, h, w, cin, cout = shape
    g = _gen(seed + 1000 * h + cin + cout)
    x = torch.randn(b, cin, h, w, generator=g) * 1.5 * x_scale               # signed: upsample_0_3.4 reads a conv without a ReLU
    dz = torch.zeros(b, cout, 2 * h, 2 * w) if zero_dz else torch.randn(b, cout, 2 * h, 2 * w, generator=g) * g_scale
    w3 = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
    return x, dz, w3


def _nhwc(dev, t):
    return pc.to(dev, t.permute(0, 2, 3, 1).contiguous())


def _nchw(t):
    return t.cpu().permute(0, 3, 1, 2).contiguous()


def device_collapse(dev, w3):
    """The collapsed weight as the device's kernel sums it (fp32): the plane both half packs round."""
    return ops.upsample_conv_weight(pc.to(dev, w3)).cpu()


def ref_wgrad3(xq, dzq, wshape):
    """fp64 weight gradient of a 3x3 pad-1 conv on the nearest-upsampled x against dz."""
    up = F.interpolate(xq.double(), scale_factor=2, mode="nearest")
    return torch.nn.grad.conv2d_weight(up, wshape, dzq.double(), padding=1)


def run_wgrad(dev, x, dz):
    cout, cin = int(dz.shape[1]), int(x.shape[1])
    dw, db = ops.upsample_conv3x3_wgrad_f16(_nhwc(dev, x), _amax_of(dev, x), _nhwc(dev, dz), _amax_of(dev, dz), cout, cin)
    return dw.cpu(), db.cpu()


def check_wgrad(dev, shape, x_scale=1.0, g_scale=3e-4, zero_dz=False):
    """One launch pair of the new entry point -> (dW, split)."""
    b, h, w, cin, cout = shape
    x, dz, w3 = _operands(shape, x_scale, g_scale, zero_dz=zero_dz)
    split = ops.upsample_conv3x3_wgrad_f16_splitk(b, h, w, cin, cout)
    dw, db = run_wgrad(dev, x, dz)
    assert tuple(dw.shape) == (cout, cin, 3, 3) and tuple(db.shape) == (cout,)
    if zero_dz:
        assert float(dw.abs().max()) == 0.0 and float(db.abs().max()) == 0.0
        return dw, split
    what = "upsample wgrad %s x_scale %g split %d" % (shape, x_scale, split)
    ref = ref_wgrad3(q_scaled(x), q_scaled(dz), w3.shape)
    _assert_close(dw, ref, ref_wgrad3(x, dz, w3.shape), what)
    if x_scale < 1e-3:
        # the e_x = 0 form (x rounded unscaled, clamped) lands in the half subnormals here: its reference is NOT what the launch computed
        clamped = ref_wgrad3(q_act(x), q_scaled(dz), w3.shape)
        off = float((dw.double() - clamped).abs().max()) / float(clamped.abs().max())
        print("%s: the unscaled clamped rounding lies %.3g away" % (what, off))
        assert off > ACC_BOUND, off
    bref = dz.double().sum((0, 2, 3))
    assert float((db.double() - bref).abs().max()) <= 1e-6 * float(dz.abs().sum((0, 2, 3)).max())
    return dw, split


def check_repeat(dev):
    a, split = check_wgrad(dev, SPLIT_SHAPE)
    b, _ = check_wgrad(dev, SPLIT_SHAPE)
    assert split > 1, split
    assert torch.equal(a, b)


def check_fold(dev):
    """<collapse(W), G> == <W, fold(G)> on small integers (exact in fp32): the existing collapse kernel against the new reduce on a
    one-slice workspace; and both against their restatements here."""
    g = _gen(5)
    cout, cin, rows_pad = 32, 32, 64
    w3 = torch.randint(-4, 5, (cout, cin, 3, 3), generator=g).float()
    g4 = torch.randint(-4, 5, (cin, cout, 4, 4), generator=g).float()
    wt = device_collapse(dev, w3)
    part = torch.full((1, 16, rows_pad, cout), 77.0)                     # (the padded rows are never read)
    part[0, :, :cin] = g4.permute(2, 3, 0, 1).reshape(16, cin, cout)
    dw3 = ops.upsample_conv3x3_wgrad_f16_fold(pc.to(dev, part), None, None, cout, cin).cpu()
    assert torch.equal(wt, collapse(w3)) and torch.equal(dw3, fold(g4))
    assert float((wt.double() * g4.double()).sum()) == float((w3.double() * dw3.double()).sum())
    # two slices are summed, the scales applied once each
    two = pc.to(dev, torch.cat([part, part]))
    ax, ag = pc.to(dev, torch.tensor([3.0]).view(torch.int32)), pc.to(dev, torch.tensor([0.01]).view(torch.int32))
    scaled = ops.upsample_conv3x3_wgrad_f16_fold(two, ax, ag, cout, cin).cpu()
    e = scale_exponent(torch.tensor([3.0])) + scale_exponent(torch.tensor([0.01]))
    assert torch.equal(scaled, 2 * dw3 * 2.0 ** -e)


def check_forward(dev, shape, x_scale=1.0):
    """The forward launch as the switch uses it: the plain transposed form on the "ups_f16" pack, bias and ReLU, amax in and out."""
    b, h, w, cin, cout = shape
    x, _, w3 = _operands(shape, x_scale)
    bias = torch.randn(cout, generator=_gen(7)) * 0.1 * x_scale
    wt = device_collapse(dev, w3)
    pk4 = ops.pack_convT4x4_weight_f16(ops.upsample_conv_weight(pc.to(dev, w3)))
    assert int(pk4[2].cpu()) == scale_exponent(wt)
    y, amax = ops.conv_transpose4x4s2_f16(_nhwc(dev, x), _amax_of(dev, x), pk4, pk4[3], None, pc.to(dev, bias), ops.CONV_RELU, direct_taps=36)
    yc = _nchw(y)
    bd = bias.double().reshape(1, -1, 1, 1)
    ref = F.relu(F.conv_transpose2d(q_scaled(x), q_scaled(wt), None, 2, 1) + bd)
    _assert_close(yc, ref, F.relu(F.conv_transpose2d(x.double(), wt.double(), None, 2, 1) + bd), "upsample forward %s x_scale %g" % (shape, x_scale))
    assert abs(tc._amax_value(amax) - float(yc.abs().max())) <= 1e-6 * float(ref.abs().max())
    return yc


def check_dgrad(dev, shape, variant=-1, g_scale=3e-4, zero_dz=False):
    """The data-gradient launch as the switch uses it: the convT4 dgrad form on the 16-slice plane of the collapsed weight -> dx."""
    b, h, w, cin, cout = shape
    _, dz, w3 = _operands(shape, g_scale=g_scale, zero_dz=zero_dz)
    wt = device_collapse(dev, w3)
    p16 = ops.pack_upsample_conv_dgrad_weight_f16(pc.to(dev, w3))
    assert int(p16[0].shape[0]) == 16 and int(p16[0].shape[2]) == cout and int(p16[2].cpu()) == scale_exponent(wt)
    ops.call("dream_conv_f16_set_variant", variant)
    try:
        dx = _nchw(ops.conv_transpose4x4s2_dgrad_f16(_nhwc(dev, dz), _amax_of(dev, dz), p16, cin))
    finally:
        ops.call("dream_conv_f16_set_variant", -1)
    assert tuple(dx.shape) == (b, cin, h, w)
    if zero_dz:
        assert float(dx.abs().max()) == 0.0
        return dx
    _assert_close(dx, F.conv2d(q_scaled(dz), q_scaled(wt), None, 2, 1), F.conv2d(dz.double(), wt.double(), None, 2, 1),
                  "upsample dgrad %s variant %d" % (shape, variant))
    return dx


def check_refusals(dev):
    """Cin % 32, odd Ho / Wo, a misaligned pointer, non-zero flags, a null pointer: refused by the entry point before any launch."""
    t = pc.to(dev, torch.zeros(4 * 4 * 64 * 16 + 64))
    i = pc.to(dev, torch.zeros(1, dtype=torch.int32))
    p, s = ops.ptr, ops.stream()

    def refused(*args):
        try:
            ops.call("dream_upsample_conv3x3_wgrad_f16_nhwc_f32", *args)
        except RuntimeError as e:
            return str(e)
        raise AssertionError("%r was accepted" % (args,))

    #                         x     ax    dz    ag    dw    ws    B  Ho Wo Cin Cdz flags
    assert "flags" in refused(p(t), p(i), p(t), p(i), p(t), p(t), 1, 4, 4, 64, 64, 2, s)
    assert "even" in refused(p(t), p(i), p(t), p(i), p(t), p(t), 1, 3, 4, 64, 64, 0, s)
    assert "even" in refused(p(t), p(i), p(t), p(i), p(t), p(t), 1, 4, 5, 64, 64, 0, s)
    assert "Cin % 32" in refused(p(t), p(i), p(t), p(i), p(t), p(t), 1, 4, 4, 48, 64, 0, s)
    assert "Cdz % 4" in refused(p(t), p(i), p(t), p(i), p(t), p(t), 1, 4, 4, 64, 30, 0, s)
    assert "null" in refused(p(t), None, p(t), p(i), p(t), p(t), 1, 4, 4, 64, 64, 0, s)
    assert "null" in refused(p(t), p(i), p(t), None, p(t), p(t), 1, 4, 4, 64, 64, 0, s)
    assert "aligned" in refused(p(t[1:]), p(i), p(t), p(i), p(t), p(t), 1, 4, 4, 64, 64, 0, s)
    assert "aligned" in refused(p(t), p(i), p(t[2:]), p(i), p(t), p(t), 1, 4, 4, 64, 64, 0, s)
    assert "aligned" in refused(p(t), p(i), p(t), p(i), p(t[1:]), p(t), 1, 4, 4, 64, 64, 0, s)
    assert ops.upsample_conv3x3_wgrad_f16_splitk(1, 2, 2, 48, 64) == 0 and ops.upsample_conv3x3_wgrad_f16_splitk(1, 2, 2, 64, 64) == 1


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def is_covered(kind, mod, flags, in_channels=None):
    """The rule of train_upsample_precision="fp16" for one plan entry, restated."""
    if kind != "conv" or not flags & ops.CONV_UPSAMPLE2X or flags & ops.CONV_OUT_NCHW:
        return False
    cout, cin = int(mod.weight.shape[0]), int(mod.weight.shape[1])
    return (in_channels is None or in_channels == cin) and cin % 32 == 0 and cout % 32 == 0


# ---- the CPU reference with the upsample convs rounded --------------------------------------------------------------------------------------
class _RoundedUpsConv(torch.autograd.Function):
    """The Conv2d behind nn.Upsample(2), given the UPSAMPLED input, restated as conv_transpose2d of the low-resolution input with the collapsed
    weight; its three products see q() of exactly the operands the device rounds (x, dz, the collapsed weight); the bias gradient is the
    plain sum.  The gradient with respect to the upsampled input is placed at the even positions: nn.Upsample's backward sums it through."""

    @staticmethod
    def forward(ctx, u, w, b):
        x = u[:, :, ::2, ::2]
        ctx.save_for_backward(x, w)
        return F.conv_transpose2d(tc.q(x), tc.q(collapse(w)), b, 2, 1)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gq, wq = tc.q(g), tc.q(collapse(w))
        dx = F.conv2d(gq, wq, None, 2, 1)
        du = dx.new_zeros(dx.shape[0], dx.shape[1], 2 * dx.shape[2], 2 * dx.shape[3])
        du[:, :, ::2, ::2] = dx
        dwt = torch.nn.grad.conv2d_weight(gq, wq.shape, tc.q(x), 2, 1)
        return du, fold(dwt), g.sum((0, 2, 3))


def _upsample_reference_convs(model):
    """The reference's Conv2d modules directly behind an nn.Upsample with channels the rule takes."""
    out, prev = [], None
    for mod in model.modules():
        if len(list(mod.children())):
            continue
        if (isinstance(mod, nn.Conv2d) and isinstance(prev, nn.Upsample) and tuple(mod.kernel_size) == (3, 3)
                and mod.in_channels % 32 == 0 and mod.out_channels % 32 == 0):
            out.append(mod)
        prev = mod
    return out


def _reference_model(dtype, ups):
    """vgg_q with the recipe weights, the plain convs rounded (train_precision="fp16"), the upsample convs too where ``ups``."""
    wts, _ = tc.training_case()
    model = om.build_model("vgg_q", 7)
    model.load_state_dict(wts)
    model = model.to(dtype).train()
    for mod in tc._plain_reference_convs(model):
        mod.forward = (lambda m: lambda inp: tc._RoundedConv.apply(inp, m.weight, m.bias))(mod)
    covered = _upsample_reference_convs(model)
    if ups:
        for mod in covered:
            mod.forward = (lambda m: lambda inp: _RoundedUpsConv.apply(inp, m.weight, m.bias))(mod)
    return model, len(covered)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _cpu_target(out_wh, shape=tc.TRAIN_SHAPE):
    b, h, w = shape
    return torch.from_numpy(cases.target_batch(b, 7, out_wh, in_wh=(w, h), seed=7))


@functools.lru_cache(maxsize=None)
def rounded_training_oracle(out_wh):
    """fp16_train_checks.rounded_training_oracle extended to round the upsample convs too -> ({parameter: E_p}, covered convs): E_p the
    distance between the reference with the upsample convs rounded and the one without, the plain convs rounded in both; the larger of
    float32 / float64."""
    _, x = tc.training_case()
    t = _cpu_target(out_wh)
    E, ncov = {}, 0
    for dtype in (torch.float32, torch.float64):
        res = []
        for ups in (False, True):
            model, ncov = _reference_model(dtype, ups)
            F.mse_loss(model(x.to(dtype))[0], t.to(dtype)).backward()
            res.append({n: p.grad.double() for n, p in model.named_parameters()})
        for n in res[0]:
            E[n] = max(E.get(n, 0.0), _rel(res[1][n], res[0][n]))
    return E, ncov


def rounded_training_gap(optimizer, out_wh):
    """The CPU reference's gap between the final losses with and without the rounded upsample convs, over the latter's decrease."""
    _, x = tc.training_case()
    t = _cpu_target(out_wh)
    runs = []
    for ups in (False, True):
        model, _ = _reference_model(torch.float32, ups)
        opt = (torch.optim.Adam if optimizer == "adam" else torch.optim.SGD)(model.parameters(), lr=cases.TRAIN_LR[optimizer])
        losses = []
        for _ in range(TRAIN_STEPS):
            opt.zero_grad()
            loss = F.mse_loss(model(x)[0], t)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        runs.append(losses)
    plain, rounded = runs
    return abs(rounded[-1] - plain[-1]) / (plain[0] - plain[-1])


# ---- one decoder block -----------------------------------------------------------------------------------------------------------------------
def block_case():
    """(weights of upsample_0_4: w4, b4, w6, b6; x [B,512,4,6]; gy [B,256,8,12])."""
    wts, _ = tc.training_case()
    g = _gen(43)
    b, h, w = BLOCK_SHAPE
    w4 = wts[BLOCK + ".4.weight"]
    x = torch.randn(b, int(w4.shape[1]), h, w, generator=g).clamp_min(0.0)             # conv5_4's output: behind a ReLU
    gy = 1e-4 * torch.randn(b, int(wts[BLOCK + ".6.weight"].shape[0]), 2 * h, 2 * w, generator=g)
    return [wts[BLOCK + k] for k in (".4.weight", ".4.bias", ".6.weight", ".6.bias")], x, gy


def reference_block_grads(dtype, ups):
    """upsample -> conv .4 -> ReLU -> conv .6 on the CPU reference -> dx, dW, dbias of conv .4.  (Conv .6 ends the walk of _only_block and
    writes the NCHW output there: not a plain conv, fp32 in both arms.)"""
    (w4, b4, w6, b6), x, gy = block_case()
    w4, b4, w6, b6 = (t.detach().clone().to(dtype).requires_grad_() for t in (w4, b4, w6, b6))
    xin = x.detach().clone().to(dtype).requires_grad_()
    u = F.interpolate(xin, scale_factor=2, mode="nearest")
    z = _RoundedUpsConv.apply(u, w4, b4) if ups else F.conv2d(u, w4, b4, padding=1)
    F.conv2d(F.relu(z), w6, b6, padding=1).backward(gy.to(dtype))
    return dict(dx=xin.grad, dW=w4.grad, dbias=b4.grad)


@functools.lru_cache(maxsize=None)
def block_yardstick():
    E = {}
    for dtype in (torch.float32, torch.float64):
        plain, rounded = reference_block_grads(dtype, False), reference_block_grads(dtype, True)
        for k in plain:
            E[k] = max(E.get(k, 0.0), _rel(rounded[k], plain[k]))
    return E


@contextlib.contextmanager
def _only_block(m):
    """``m`` (a DreamHourglass) walks the two entries of BLOCK only, on an NHWC input of the block's channels; the second one writes the NCHW
    output, where run_backward takes the loss gradient in."""
    saved = (m._plan, m._skip_sources, m._param_slot, m._check_input)
    keep = [li for li, e in enumerate(m._plan) if e[1] == BLOCK]
    m._plan = [saved[0][li] for li in keep]
    m._plan[-1] = m._plan[-1][:3] + (m._plan[-1][3] | ops.CONV_OUT_NCHW,)
    m._skip_sources = set()
    m._param_slot = {k: 2 * k for k in range(len(keep))}
    m._check_input = lambda x, x_is_nhwc: None
    try:
        yield
    finally:
        m._plan, m._skip_sources, m._param_slot, m._check_input = saved


def device_block(m, x, gy, mode):
    """The block as run_forward / run_backward walk it (train_precision="fp16") -> (gradients of conv .4, was it covered).  dx is what the
    entry's data-gradient launch returned: the walk drops it after the last entry."""
    got = {}

    def keeping(fn):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            got["dx"] = out
            return out
        return wrapped

    m.train_precision, m.train_upsample_precision = "fp16", mode
    ups_conv, dgrad16 = m._ups_conv, ops.conv_transpose4x4s2_dgrad_f16
    m._ups_conv = lambda mod, direction, t, *a, **k: (keeping(ups_conv) if direction else ups_conv)(mod, direction, t, *a, **k)
    ops.conv_transpose4x4s2_dgrad_f16 = keeping(dgrad16)
    try:
        with _only_block(m), torch.no_grad():
            params = [p.detach() for p in m.plan_parameters()]
            y, saved = m.run_forward(ops.nchw_to_nhwc(x), params, True, x_is_nhwc=True)
            grads = m.run_backward(saved, gy.contiguous())
            covered = 0 in saved.half and bool(m._plan[0][3] & ops.CONV_UPSAMPLE2X)
    finally:
        ops.conv_transpose4x4s2_dgrad_f16 = dgrad16
        del m._ups_conv
        m.train_precision = m.train_upsample_precision = "fp32"
    return dict(dx=ops.nhwc_to_nchw(got["dx"]).cpu(), dW=grads[0].cpu().clone(), dbias=grads[1].cpu().clone()), covered


def check_block(dev):
    E = block_yardstick()
    print("%s: E per tensor %s" % (BLOCK, {k: "%.3g" % v for k, v in E.items()}))
    net = tc.training_network(dev, "fp16")
    m = net.model.module
    _, x, gy = block_case()
    gyd, xd = pc.to(dev, gy), pc.to(dev, x)
    off, cov_off = device_block(m, xd, gyd, "fp32")
    on, cov_on = device_block(m, xd, gyd, "fp16")
    again, _ = device_block(m, xd, gyd, "fp32")
    assert cov_on and not cov_off
    assert all(torch.equal(again[k], off[k]) for k in off)                  # the switch leaves nothing behind
    for k in E:
        d = _rel(on[k], off[k])
        print("  %-6s device on against off %.3g   (3 E = %.3g)" % (k, d, 3 * E[k]))
        assert bool(torch.isfinite(on[k]).all()) and d <= 3 * E[k], (k, d, E[k])
    assert not torch.equal(on["dW"], off["dW"]) and not torch.equal(on["dx"], off["dx"])


# ---- the whole step, twenty optimizer steps ---------------------------------------------------------------------------------------------------
def training_network(dev, mode, optimizer="sgd", lr=0.0):
    net = tc.training_network(dev, "fp16", optimizer=optimizer, lr=lr)
    net.model.module.train_upsample_precision = mode
    return net


def _device_step(dev, mode):
    net = training_network(dev, mode)
    _, x = tc.training_case()
    t, out_wh = tc._target(net, dev)
    loss = float(net.train([pc.to(dev, x)], t).item())
    return loss, {n: p.grad.detach().cpu().clone() for n, p in net.model.module.named_parameters()}, out_wh, net


def check_step(dev):
    l_off, g_off, out_wh, net = _device_step(dev, "fp32")
    l_on, g_on, _, _ = _device_step(dev, "fp16")
    E, ncov = rounded_training_oracle(out_wh)
    m = net.model.module
    names = {id(p): n for n, p in m.named_parameters()}
    covered = {names[id(mod.weight)] for kind, mod, flags in m.plan_layers() if mod is not None and is_covered(kind, mod, flags)}
    assert covered == {"upsample_0_4.4.weight", "upsample_0_3.4.weight"} and ncov == 2, (covered, ncov)
    worst = 0.0
    for n in sorted(g_off):
        r = _rel(g_on[n], g_off[n])
        print("upsample fp16 step %-40s r_p %.3g  E_p %.3g" % (n, r, E[n]))
        worst = max(worst, r / E[n])
        assert bool(torch.isfinite(g_on[n]).all()) and r <= 3 * E[n], (n, r, E[n])
    print("upsample fp16 step: losses %.9g (off) %.9g (on), worst r_p / E_p %.3g" % (l_off, l_on, worst))
    for n in covered:
        assert not torch.equal(g_on[n], g_off[n]), n


def check_uncovered_entries_bit_equal(dev):
    """Every entry the rule does not cover gives the off arm's output, bit for bit, given the same input: the saved (input, output) pairs of
    a forward with the switch on, re-run entry by entry with the switch off."""
    net = training_network(dev, "fp16")
    _, x = tc.training_case()
    m = net.model.module
    params = [p.detach() for p in m.plan_parameters()]
    with torch.no_grad():
        _, saved = m.run_forward(pc.to(dev, x), params, True)
        layers = m.plan_layers()
        checked = differs = 0
        for li, (kind, mod, flags) in enumerate(layers):
            inp, out = saved[li]
            if mod is None or kind in ("first", "wide"):
                continue
            w, bias = params[m._param_slot[li]], params[m._param_slot[li] + 1]
            if is_covered(kind, mod, flags, int(inp.shape[3])):
                again, _ = m._conv_fp32(kind, mod, inp, None, w, bias, flags)
                differs += int(not torch.equal(again, out))
                assert li in saved.half and saved.half[li] is not None
            elif tc.is_plain(kind, mod, flags, int(inp.shape[3])):
                again, _ = m._conv_half("f16", kind, mod, inp, saved.half[li], w, bias, flags)
                assert torch.equal(again, out), (li, kind)
                checked += 1
            else:
                again, _ = m._conv_fp32(kind, mod, inp, None, w, bias, flags)
                assert torch.equal(again, out), (li, kind)
                checked += 1
    assert differs == 2 and checked >= 12, (checked, differs)


def check_training_trains(dev, optimizer):
    _, x = tc.training_case()
    runs = {}
    for mode in ("fp32", "fp16"):
        net = training_network(dev, mode, optimizer=optimizer, lr=cases.TRAIN_LR[optimizer])
        t, _ = tc._target(net, dev)
        xd = pc.to(dev, x)
        runs[mode] = [float(net.train([xd], t).item()) for _ in range(TRAIN_STEPS)]
    ref_gap = TRAIN_GAP[optimizer]
    gap = abs(runs["fp16"][-1] - runs["fp32"][-1]) / (runs["fp32"][0] - runs["fp32"][-1])
    print("%s, %d steps: off %.9g -> %.9g, on %.9g -> %.9g, gap over the decrease %.3g (reference %.3g, 3 x = %.3g)"
          % (optimizer, TRAIN_STEPS, runs["fp32"][0], runs["fp32"][-1], runs["fp16"][0], runs["fp16"][-1], gap, ref_gap, 3 * ref_gap))
    assert ref_gap > 0 and runs["fp16"][-1] < runs["fp16"][0]
    assert gap <= 3 * ref_gap, (gap, ref_gap)


def check_default_untouched(dev):
    """fp32 -> fp16 -> fp32 of the switch on one network with lr = 0: the first and third steps give the same bits, the middle one differs."""
    net = training_network(dev, "fp32")
    _, x = tc.training_case()
    t, _ = tc._target(net, dev)
    xd = pc.to(dev, x)
    grads = lambda: [p.grad.detach().clone() for p in net.model.module.parameters()]      # noqa: E731
    l0 = float(net.train([xd], t).item())
    g0 = grads()
    net.model.module.train_upsample_precision = "fp16"
    l1 = float(net.train([xd], t).item())
    g1 = grads()
    net.model.module.train_upsample_precision = "fp32"
    l2 = float(net.train([xd], t).item())
    assert l0 == l2 and all(torch.equal(a, b) for a, b in zip(g0, grads()))
    assert l1 != l0 and any(not torch.equal(a, b) for a, b in zip(g0, g1))
