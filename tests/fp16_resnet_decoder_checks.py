"""What the CPU suite (kernels under the SIMT emulator) and the GPU suite share for ResnetSimple's train_decoder_precision="fp16"
(the convT4 dgrad form of csrc/conv_f16.hip, wgrad_convT4_f16_kernel of csrc/wgrad_f16.hip, the saturating plain transposed forward).

Per launch: against the fp64 result of the ROUNDED operands -- q_act / q_scaled of fp16_resnet_train_checks
-- a launch may differ by the fp32-accumulation bound, 5e-6 of max|ref|; the fp64 result of the UNROUNDED operands has to lie more than
5e-5 of that maximum away, so a launch that does not round cannot pass.

One decoder stage (ConvTranspose2d -> BatchNorm -> ReLU, forward and backward): E = the larger of the float32 / float64 relative
distances, per gradient tensor, between the CPU reference stage with q() on exactly the three covered products and the plain stage; the
device's stage with the switch on against the switch off is held to 3 E (fp16_resnet_step_checks.check_block's yardstick).

Whole step and twenty optimizer steps: the harness of fp16_resnet_step_checks (network, step_case).  At its 2 x 64 x 64 batch every decoder
stage would take the small-map GEMM form, which the rule leaves in fp32; both arms therefore run with CONVT_GEMM_MAX_PIXELS = 0 (the
instance attribute behind DREAM_CONVT_GEMM_MAX_PIXELS), so that all four stages are transposed convs and are covered.
"""
import copy
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

import fp16_resnet_step_checks as sc
import parity_checks as pc
from fp16_resnet_train_checks import ACC_BOUND, ROUNDING_GAP, q_act, q_scaled, scale_exponent, _amax_of, _assert_close, _bn, _ctr, _gen
from dream_amd import models, ops

# (B, H, W, Cin, Cout) of x [B,H,W,Cin]; dz is [B,2H,2W,Cout].  5 x 7: odd input, ragged tiles, every border tap, two position tiles for
# the weight gradient (split 2); 1 x 1: every tap but four falls outside; one and several 32- / 64-channel blocks on either side
SHAPES = [(2, 5, 7, 32, 32), (2, 5, 7, 64, 96), (1, 1, 1, 32, 96), (1, 1, 1, 64, 32)]
SPLIT_SHAPE = (2, 9, 17, 32, 32)                 # 8 position tiles of 8 x 16 on 4 workgroups per slice: split 8
VARIANT_SHAPE = (2, 5, 7, 64, 96)
NUM_VARIANTS = 8                                 # the tile table of csrc/conv_f16.hip (dream_conv_f16_set_variant)
STAGE = "upsample.3"                             # 256 -> 256, the shape of three of the four (five) decoder stages
STAGE_SHAPE = (2, 5, 7)
# measured on the CPU reference by rounded_training_gap() (decoder rounded against not, twenty steps on the fixed batch; ``both``: the 1x1
# GEMMs rounded in either run): the gap of the final losses over the decrease; the CPU suite recomputes them and asserts that they hold
TRAIN_GAP = {("adam", False): 0.50e-2, ("sgd", False): 1.38e-2, ("adam", True): 2.14e-2, ("sgd", True): 0.76e-2}


def _operands(shape, seed=0, zero_dz=False):
    b, h, w, cin, cout = shape
    g = _gen(seed + 1000 * h + cin + cout)
    x = torch.randn(b, cin, h, w, generator=g).abs() * 1.5                  # a ReLU output
    dz = torch.zeros(b, cout, 2 * h, 2 * w) if zero_dz else torch.randn(b, cout, 2 * h, 2 * w, generator=g) * 3e-4
    wt = torch.randn(cin, cout, 4, 4, generator=g) * 0.05
    return x, dz, wt


def _nhwc(dev, t):
    return pc.to(dev, t.permute(0, 2, 3, 1).contiguous())


def _nchw(t):
    return t.cpu().permute(0, 3, 1, 2).contiguous()


def ref_dgrad(dz, wt):
    return F.conv2d(dz, wt, None, 2, 1)


def ref_wgrad(x, dz, wt_shape):
    return torch.nn.grad.conv2d_weight(dz, wt_shape, x, 2, 1)


def check_forward(dev, shape):
    """The covered forward (the saturating plain phases, e_x = 0 with a clamp, bias as shift) and the unchanged statistics pass over the z it wrote."""
    b, h, w, cin, cout = shape
    x, _, wt = _operands(shape)
    g = _gen(7)
    bias = torch.randn(cout, generator=g) * 0.1
    p16 = ops.pack_convT4x4_weight_f16(pc.to(dev, wt))
    assert int(p16[2].cpu()) == scale_exponent(wt)
    z = ops.conv_transpose4x4s2_f16_sat(_nhwc(dev, x), p16, cout, None, pc.to(dev, bias), 0)
    zc = _nchw(z)
    bd = bias.double().reshape(1, -1, 1, 1)
    _assert_close(zc, F.conv_transpose2d(q_act(x), q_scaled(wt), None, 2, 1) + bd, F.conv_transpose2d(x.double(), wt.double(), None, 2, 1) + bd,
                  "forward %s" % (shape,))
    bn = _bn(cout, g)
    ab, mean, invstd = ops.bn_stats(z, bn.to(dev) if dev != "cpu" else bn, _ctr(dev))
    zd = zc.double().permute(1, 0, 2, 3).reshape(cout, -1)
    mu, var = zd.mean(1), zd.var(1, unbiased=False)
    istd = 1.0 / torch.sqrt(var + bn.eps)
    assert float((mean.cpu().double() - mu).abs().max()) <= 1e-5 * max(1.0, float(mu.abs().max()))
    assert float((invstd.cpu().double() / istd - 1.0).abs().max()) <= 1e-5
    return zc


def check_dgrad(dev, shape, variant=-1, zero_dz=False):
    """One launch of the convT4 dgrad form -> dx (NCHW, for repeat checks)."""
    b, h, w, cin, cout = shape
    x, dz, wt = _operands(shape, zero_dz=zero_dz)
    p16 = ops.pack_convT4x4_dgrad_weight_f16(pc.to(dev, wt))
    assert tuple(p16[0].shape)[0] == 16 and int(p16[0].shape[2]) == cout and int(p16[2].cpu()) == scale_exponent(wt)
    ops.call("dream_conv_f16_set_variant", variant)
    try:
        dx = _nchw(ops.conv_transpose4x4s2_dgrad_f16(_nhwc(dev, dz), _amax_of(dev, dz), p16, cin))
    finally:
        ops.call("dream_conv_f16_set_variant", -1)
    assert tuple(dx.shape) == (b, cin, h, w)
    if zero_dz:
        assert float(dx.abs().max()) == 0.0
        return dx
    _assert_close(dx, ref_dgrad(q_scaled(dz), q_scaled(wt)), ref_dgrad(dz.double(), wt.double()), "dgrad %s variant %d" % (shape, variant))
    return dx


def check_wgrad(dev, shape, zero_dz=False):
    """One launch of wgrad_convT4_f16_kernel + its fixed-order reduce -> (dW, split)."""
    b, h, w, cin, cout = shape
    x, dz, wt = _operands(shape, zero_dz=zero_dz)
    split = ops.convT4x4_wgrad_f16_splitk(b, h, w, cin, cout)
    dw = ops.convT4x4_wgrad_f16(_nhwc(dev, x), _nhwc(dev, dz), _amax_of(dev, dz)).cpu()
    assert tuple(dw.shape) == (cin, cout, 4, 4)
    if zero_dz:
        assert float(dw.abs().max()) == 0.0
        return dw, split
    _assert_close(dw, ref_wgrad(q_act(x), q_scaled(dz), wt.shape), ref_wgrad(x.double(), dz.double(), wt.shape), "wgrad %s split %d" % (shape, split))
    return dw, split


def check_repeat(dev):
    """Two runs give the same bits (no floating-point atomics: the split is summed in slice order)."""
    a, split = check_wgrad(dev, SPLIT_SHAPE)
    b, _ = check_wgrad(dev, SPLIT_SHAPE)
    assert split > 1, split
    assert torch.equal(a, b)
    assert torch.equal(check_dgrad(dev, SHAPES[1]), check_dgrad(dev, SHAPES[1]))


def check_scales(dev):
    """Powers of two travel exactly through e_g; an outlier activation saturates to 65504 in the weight gradient AND in the forward, and
    both stay finite and within the bound of the clamped reference."""
    shape = SHAPES[0]
    b, h, w, cin, cout = shape
    x, dz, wt = _operands(shape)
    p16 = ops.pack_convT4x4_dgrad_weight_f16(pc.to(dev, wt))
    dgrad = lambda t: ops.conv_transpose4x4s2_dgrad_f16(_nhwc(dev, t), _amax_of(dev, t), p16, cin).cpu()          # noqa: E731
    wgrad = lambda xx, t: ops.convT4x4_wgrad_f16(_nhwc(dev, xx), _nhwc(dev, t), _amax_of(dev, t)).cpu()           # noqa: E731
    d1, w1 = dgrad(dz), wgrad(x, dz)
    for s in (2.0 ** -20, 2.0 ** 10):
        assert torch.equal(dgrad(dz * s) / s, d1) and torch.equal(wgrad(x, dz * s) / s, w1), s
    xa = x.clone()
    xa[0, 3, 2, 4] = 1e6
    dw = wgrad(xa, dz)
    ref = ref_wgrad(q_act(xa), q_scaled(dz), wt.shape)
    assert bool(torch.isfinite(dw).all()) and float(q_act(xa).max()) == 65504.0
    assert float((dw.double() - ref).abs().max()) <= ACC_BOUND * float(ref.abs().max())


    # ... and through the forward: the same outlier, the same clamp
    pf = ops.pack_convT4x4_weight_f16(pc.to(dev, wt))
    z = _nchw(ops.conv_transpose4x4s2_f16_sat(_nhwc(dev, xa), pf, cout))
    zref = F.conv_transpose2d(q_act(xa), q_scaled(wt), None, 2, 1)
    assert bool(torch.isfinite(z).all()) and float(zref.abs().max()) > 1e3
    assert float((z.double() - zref).abs().max()) <= ACC_BOUND * float(zref.abs().max())


def check_batched_pack(dev):
    """The half planes of the decoder by the batched pack (modes 2 / 3): the one-tensor packers' halfs and exponents, bit for bit (a zero
    weight and a channel count that is padded included)."""
    g = _gen(3)
    ws = [pc.to(dev, w) for w in (torch.randn(64, 32, 4, 4, generator=g) * 0.1, torch.randn(32, 96, 4, 4, generator=g) * 3.0,
                                   torch.zeros(32, 32, 4, 4))]
    entries = []
    for w in ws:
        for mode, pack in ((2, ops.pack_convT4x4_weight_f16), (3, ops.pack_convT4x4_dgrad_weight_f16)):
            want = pack(w)
            entries.append((w, (torch.full_like(want[0], 7.0), None, torch.full_like(want[2], 99), want[3]), mode, want))
    table, scratch = ops.pack16_job_table([e[:3] for e in entries], ws[0].device)
    scratch.fill_(12345)                                                # stale: the launch zeroes the words first
    ops.pack_conv1x1_weights_f16_batched(table, scratch, workgroups_per_job=3)
    for w, got, mode, want in entries:
        assert torch.equal(got[0], want[0]) and int(got[2].cpu()) == int(want[2].cpu()) == scale_exponent(w.cpu()), (tuple(w.shape), mode)


def check_bias_gradient(dev):
    """The weight-gradient leaf of a covered record hands over dbias = the fp32 channel sum of dz, sliced to the bias (no BatchNorm here)."""
    net = sc._device_resnet(dev)
    m, bn = next((m, bn) for name, m, bn in net._decoder() if name == STAGE)
    g = _gen(11)
    b, h, w = STAGE_SHAPE
    x = pc.to(dev, torch.randn(b, h, w, int(m.weight.shape[0]), generator=g).clamp_min(0.0))
    dz = torch.randn(b, 2 * h, 2 * w, int(m.weight.shape[1]), generator=g) * 1e-3
    rec = dict(kind="convT", name=STAGE, conv=m, x=x, f16=True, dz_amax=_amax_of(dev, dz))
    bw = dict(grads=models._GradDict(None), side=None, reducer=None, grad_out=None)
    net._wgrad(rec, pc.to(dev, dz), bw)
    db = bw["grads"][m.bias].cpu()
    ref = dz.double().sum((0, 1, 2))
    assert tuple(db.shape) == tuple(m.bias.shape)
    assert float((db.double() - ref).abs().max()) <= 1e-6 * float(dz.abs().sum((0, 1, 2)).max())
    assert net._wgrad_form(rec, pc.to(dev, dz))[0] == "convT_f16"


def check_refusals(dev):
    """Cin % 32, odd output dimensions, misaligned pointers, flags, null pointers: refused by the entry points before any launch."""
    t = pc.to(dev, torch.zeros(4 * 4 * 64 + 64))
    h16 = pc.to(dev, torch.zeros(16 * 128 * 64 + 64, dtype=torch.float16))
    i = pc.to(dev, torch.zeros(1, dtype=torch.int32))
    p, s = ops.ptr, ops.stream()

    def refused(name, *args):
        try:
            ops.call(name, *args)
        except RuntimeError as e:
            return str(e)
        raise AssertionError("%s%r was accepted" % (name, args))

    dg, wg = "dream_conv_transpose4x4s2_dgrad_f16_nhwc_f32", "dream_convT4x4_wgrad_f16_nhwc_f32"
    #                     dz    amax  w       exp   dx    B  Ho Wo Cdz Cdx pad  flags
    assert "flags" in refused(dg, p(t), p(i), p(h16), p(i), p(t), 1, 4, 4, 64, 64, 128, 1, s)
    assert "even" in refused(dg, p(t), p(i), p(h16), p(i), p(t), 1, 3, 4, 64, 64, 128, 0, s)
    assert "even" in refused(dg, p(t), p(i), p(h16), p(i), p(t), 1, 4, 5, 64, 64, 128, 0, s)
    assert "multiple of 32" in refused(dg, p(t), p(i), p(h16), p(i), p(t), 1, 4, 4, 48, 64, 128, 0, s)
    assert "aligned" in refused(dg, p(t[1:]), p(i), p(h16), p(i), p(t), 1, 4, 4, 64, 64, 128, 0, s)
    assert "aligned" in refused(dg, p(t), p(i), p(h16[1:]), p(i), p(t), 1, 4, 4, 64, 64, 128, 0, s)
    assert "aligned" in refused(dg, p(t), p(i), None, p(i), p(t), 1, 4, 4, 64, 64, 128, 0, s)
    assert "null" in refused(dg, p(t), None, p(h16), p(i), p(t), 1, 4, 4, 64, 64, 128, 0, s)
    assert "CoutPad" in refused(dg, p(t), p(i), p(h16), p(i), p(t), 1, 4, 4, 64, 64, 96, 0, s)
    #                     x     dz    amax  dw    ws    B  Ho Wo Cin Cdz pad flags
    assert "flags" in refused(wg, p(t), p(t), p(i), p(t), p(t), 1, 4, 4, 64, 64, 64, 2, s)
    assert "even" in refused(wg, p(t), p(t), p(i), p(t), p(t), 1, 4, 3, 64, 64, 64, 0, s)
    assert "Cin % 32" in refused(wg, p(t), p(t), p(i), p(t), p(t), 1, 4, 4, 48, 64, 64, 0, s)
    assert "Cdz % 4" in refused(wg, p(t), p(t), p(i), p(t), p(t), 1, 4, 4, 64, 30, 64, 0, s)
    assert "pad % 64" in refused(wg, p(t), p(t), p(i), p(t), p(t), 1, 4, 4, 64, 64, 32, 0, s)
    assert "null" in refused(wg, p(t), p(t), None, p(t), p(t), 1, 4, 4, 64, 64, 64, 0, s)
    assert "aligned" in refused(wg, p(t[1:]), p(t), p(i), p(t), p(t), 1, 4, 4, 64, 64, 64, 0, s)
    assert "aligned" in refused(wg, p(t), p(t[2:]), p(i), p(t), p(t), 1, 4, 4, 64, 64, 64, 0, s)
    assert ops.convT4x4_wgrad_f16_splitk(1, 2, 2, 48, 64) == 0
    assert not ops.convT4x4_f16_train_applies(48, 64, 4, 4) and not ops.convT4x4_f16_train_applies(64, 48, 4, 4)
    assert not ops.convT4x4_f16_train_applies(64, 64, 5, 4) and ops.convT4x4_f16_train_applies(64, 64, 4, 4)


# ---- one decoder stage ----------------------------------------------------------------------------------------------------------------
class _RoundedConvT(torch.autograd.Function):
    """ConvTranspose2d(k4,s2,p1) whose three products see q() of their operands, in the dtype of the run; the bias gradient is the plain sum."""

    @staticmethod
    def forward(ctx, x, w, bias):
        ctx.save_for_backward(x, w)
        return F.conv_transpose2d(q_act(x).to(x.dtype), q_scaled(w).to(x.dtype), bias, 2, 1)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gq, wq, xq = q_scaled(g).to(g.dtype), q_scaled(w).to(g.dtype), q_act(x).to(g.dtype)
        return F.conv2d(gq, wq, None, 2, 1), torch.nn.grad.conv2d_weight(gq, w.shape, xq, 2, 1), g.sum((0, 2, 3))


def stage_case():
    ref = sc.om.build_model("resnet_h", 7)
    ref.load_state_dict(sc._weights())
    mods = dict(ref.upsample.named_children())
    i = int(STAGE.split(".")[1])
    convt, bn = mods[str(i)], mods[str(i + 1)]
    g = _gen(41)
    b, h, w = STAGE_SHAPE
    x = torch.randn(b, convt.in_channels, h, w, generator=g).clamp_min(0.0)
    gy = 1e-4 * torch.randn(b, convt.out_channels, 2 * h, 2 * w, generator=g)
    return convt, bn, x, gy


def reference_stage_grads(convt, bn, x, gy, dtype, rounded):
    convt, bn = copy.deepcopy(convt).to(dtype), copy.deepcopy(bn).to(dtype).train()
    xin = x.detach().clone().to(dtype).requires_grad_()
    z = _RoundedConvT.apply(xin, convt.weight, convt.bias) if rounded else convt(xin)
    F.relu(bn(z)).backward(gy.to(dtype))
    return dict(dx=xin.grad, dW=convt.weight.grad, dbias=convt.bias.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad)


@functools.lru_cache(maxsize=None)
def stage_yardstick():
    convt, bn, x, gy = stage_case()
    E = {}
    for dtype in (torch.float32, torch.float64):
        plain = reference_stage_grads(convt, bn, x, gy, dtype, False)
        rounded = reference_stage_grads(convt, bn, x, gy, dtype, True)
        for k in plain:
            E[k] = max(E.get(k, 0.0), sc._rel(rounded[k], plain[k]))
    return E


def device_stage(net, x, gy, mode):
    """The stage of ``net`` (a dream_amd ResnetSimple in training mode) as run_forward_train / _bwd_convT run it -> (gradients, covered)."""
    m, bn = next((m, bn) for name, m, bn in net._decoder() if name == STAGE)
    net.train_decoder_precision = mode
    try:
        walk = net._resolve_switches(True)
        net._packs.restart_pools()
        tape = []
        rec = net._stage(tape, STAGE, m, bn, ops.nchw_to_nhwc(x), None, walk.dec16)
        bw = dict(grads=models._GradDict(None), side=None, reducer=None, grad_out=None)
        dx = net._bwd_convT(rec, ops.nchw_to_nhwc(gy), bw)
    finally:
        net.train_decoder_precision = "fp32"
    out = dict(dx=ops.nhwc_to_nchw(dx).cpu(), dW=bw["grads"][m.weight].cpu().clone(), dbias=bw["grads"][m.bias].cpu().clone(),
               dgamma=bw["grads"][bn.weight].cpu().clone(), dbeta=bw["grads"][bn.bias].cpu().clone())
    return out, net._half_decoder(rec)


def check_stage(dev):
    E = stage_yardstick()
    print("%s: E per tensor %s" % (STAGE, {k: "%.3g" % v for k, v in E.items()}))
    # (dbias: the BatchNorm behind the conv removes a per-channel constant, so the exact bias gradient is zero and both runs hold rounding
    # noise -- its E is of order one; the other four are rounding distances)
    assert all(e > 0 for e in E.values()) and max(e for k, e in E.items() if k != "dbias") < 0.1
    net = sc._device_resnet(dev)
    saved = net.CONVT_GEMM_MAX_PIXELS
    net.CONVT_GEMM_MAX_PIXELS = 0                    # (70 input pixels: the small-map GEMM form would take the stage, in fp32)
    try:
        _, _, x, gy = stage_case()
        g32, cov32 = device_stage(net, pc.to(dev, x), pc.to(dev, gy), "fp32")
        g16, cov16 = device_stage(net, pc.to(dev, x), pc.to(dev, gy), "fp16")
        again, _ = device_stage(net, pc.to(dev, x), pc.to(dev, gy), "fp32")
    finally:
        net.CONVT_GEMM_MAX_PIXELS = saved
    assert cov16 and not cov32
    assert all(torch.equal(again[k], g32[k]) for k in g32)          # the switch leaves nothing behind
    for k in E:
        d = sc._rel(g16[k], g32[k])
        print("  %-8s device fp16 against fp32 %.3g   (3 E = %.3g)" % (k, d, 3 * E[k]))
        assert bool(torch.isfinite(g16[k]).all()) and d <= 3 * E[k], (k, d, E[k])
    assert not torch.equal(g16["dW"], g32["dW"]) and not torch.equal(g16["dx"], g32["dx"])


def check_small_map_stays_fp32(dev):
    """A stage whose forward takes the small-map GEMM form is not covered: its gradients are the fp32 stage's, bit for bit."""
    net = sc._device_resnet(dev)
    _, _, x, gy = stage_case()
    g32, _ = device_stage(net, pc.to(dev, x), pc.to(dev, gy), "fp32")
    g16, cov16 = device_stage(net, pc.to(dev, x), pc.to(dev, gy), "fp16")
    assert not cov16 and all(torch.equal(g16[k], g32[k]) for k in g32)


# ---- the whole step, twenty optimizer steps ---------------------------------------------------------------------------------------------
def _round_decoder(model):
    for mod in model.modules():
        if isinstance(mod, nn.ConvTranspose2d):
            mod.forward = (lambda m: lambda inp: _RoundedConvT.apply(inp, m.weight, m.bias))(mod)


def _reference_model(dtype, decoder, gemm):
    model = sc._reference_model(dtype, gemm)
    if decoder:
        _round_decoder(model)
    return model


def network(dev, decoder, gemm="fp32", optimizer="sgd", lr=0.0, shape=sc.STEP_SHAPE):
    net = sc.network(dev, gemm, optimizer=optimizer, lr=lr, shape=shape)
    net.model.module.CONVT_GEMM_MAX_PIXELS = 0
    net.model.module.train_decoder_precision = decoder
    return net


def _device_step(dev, decoder, gemm="fp32", shape=sc.STEP_SHAPE):
    net = network(dev, decoder, gemm, shape=shape)
    ow, oh = net.trained_net_output_resolution()
    loss = float(net.train([pc.to(dev, sc.step_case(shape))], pc.to(dev, sc._target((ow, oh), shape))).item())
    return loss, {n: p.grad.detach().cpu().clone() for n, p in net.model.module.named_parameters()}, (ow, oh)


def step_yardstick(out_wh, gemm, shape=sc.STEP_SHAPE):
    """-> ({parameter: E_p}, the rounded reference's relative move of the loss) against the reference with the decoder unrounded (and the
    1x1 GEMMs rounded in both where ``gemm``): the larger of float32 / float64; computed once per process and shape."""
    return _step_yardstick(out_wh, gemm, shape)


@functools.lru_cache(maxsize=None)
def _step_yardstick(out_wh, gemm, shape):
    E, move = {}, 0.0
    for dtype in (torch.float32, torch.float64):
        res = []
        for decoder in (False, True):
            model = _reference_model(dtype, decoder, gemm)
            loss = F.mse_loss(model(sc.step_case(shape).to(dtype))[0], sc._target(out_wh, shape).to(dtype))
            loss.backward()
            res.append((float(loss), {n: p.grad.double() for n, p in model.named_parameters()}))
        (l0, g0), (l1, g1) = res
        move = max(move, abs(l1 - l0) / abs(l0))
        for n in g0:
            E[n] = max(E.get(n, 0.0), sc._rel(g1[n], g0[n]))
    return E, move


def check_step(dev, both, shape=sc.STEP_SHAPE, conditioned=sc.CONDITIONED):
    """The switch alone (against the fp32 step) or both training switches (against the step with train_gemm_precision alone).
    ``conditioned``: the tensors held at ``shape`` (fp16_resnet_step_checks.check_step)."""
    gemm = "fp16" if both else "fp32"
    l32, g32, out_wh = _device_step(dev, "fp32", gemm, shape=shape)
    l16, g16, _ = _device_step(dev, "fp16", gemm, shape=shape)
    E, move = step_yardstick(out_wh, both, shape)
    print("loss off %.9g on %.9g (relative %.3g; the rounded reference moves %.3g); E_p of the conditioned tensors %s"
          % (l32, l16, abs(l16 - l32) / l32, move, {n: "%.3g" % E[n] for n in conditioned}))
    assert move > 0 and all(E[n] > 0 for n in conditioned)
    assert abs(l16 - l32) <= 3 * move * abs(l32)
    for n in g32:
        assert bool(torch.isfinite(g16[n]).all()), n
    worst = 0.0
    for n in conditioned:
        d = sc._rel(g16[n], g32[n])
        worst = max(worst, d / E[n])
        print("  %-20s device on against off %.3g   (3 E_p = %.3g)" % (n, d, 3 * E[n]))
        assert d <= 3 * E[n], (n, d, E[n])
    print("  worst r_p / E_p %.3g" % worst)
    assert not torch.equal(g16["upsample.9.weight"], g32["upsample.9.weight"])


def rounded_training_gap(optimizer, out_wh, both):
    """The CPU reference's gap between the final losses with and without the rounded decoder, over the latter's decrease."""
    runs = []
    for decoder in (False, True):
        model = _reference_model(torch.float32, decoder, both)
        opt = (torch.optim.Adam if optimizer == "adam" else torch.optim.SGD)(model.parameters(), lr=sc.TRAIN_LR[optimizer])
        x, t, losses = sc.step_case(), sc._target(out_wh), []
        for _ in range(sc.TRAIN_STEPS):
            opt.zero_grad()
            loss = F.mse_loss(model(x)[0], t)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        runs.append(losses)
    plain, rounded = runs
    return abs(rounded[-1] - plain[-1]) / (plain[0] - plain[-1])


def check_training_trains(dev, optimizer, both):
    gemm = "fp16" if both else "fp32"
    runs = {}
    for mode in ("fp32", "fp16"):
        net = network(dev, mode, gemm, optimizer=optimizer, lr=sc.TRAIN_LR[optimizer])
        ow, oh = net.trained_net_output_resolution()
        x, t = pc.to(dev, sc.step_case()), pc.to(dev, sc._target((ow, oh)))
        runs[mode] = [float(net.train([x], t).item()) for _ in range(sc.TRAIN_STEPS)]
    ref_gap = TRAIN_GAP[optimizer, both]
    gap = abs(runs["fp16"][-1] - runs["fp32"][-1]) / (runs["fp32"][0] - runs["fp32"][-1])
    print("%s, %d steps, both=%s: off %.6g -> %.6g, on %.6g -> %.6g, gap over the decrease %.3g (reference %.3g, 3 x = %.3g)"
          % (optimizer, sc.TRAIN_STEPS, both, runs["fp32"][0], runs["fp32"][-1], runs["fp16"][0], runs["fp16"][-1], gap, ref_gap, 3 * ref_gap))
    assert ref_gap > 0 and runs["fp16"][-1] < runs["fp16"][0]
    assert gap <= 3 * ref_gap, (gap, ref_gap)
