"""Checks of ResnetSimple.inference_activation_storage="fp16" (precision="fp16" with every tensor between the image and the belief maps
stored as IEEE half), shared by the emulator and the GPU suite.

Per launch nothing is measured; the two bounds are fp16_storage_checks'.  (1) On inputs that are halfs already (normal halfs or zero,
max|x| <= 2^13) the residual form of conv_f16_kernel must equal fp16(clamp(y32)) bit for bit, y32 being the fp32-storage launch of
the same tile on the widened input and residual.  (2) Independently, against the fp64 conv of x16 and q(w) plus the residual:
    |got - ref| <= 5e-6 max|ref| + 2^-11 |ref| + 2^-25.
The gathers and the pool round nothing: bit equality with the half of their fp32 siblings.  A stride-2 conv through its gather is held
to (2) against the fp64 STRIDED conv, which pins tap order and padding.

One Bottleneck through the walk's own helper is held to an fp64 restatement that rounds the tensors the device stores, within a
bound carried along with it (block_oracle: what fp32 accumulation and one half-ulp per stored tensor can move).

End to end the bound is measured on the reference, by stored_oracle(): oracle.models.ResnetSimple with q(weight) at every conv, the
image and every tensor the device stores rounded to saturating half; E, P and the held maps come from fp16_checks._oracle."""
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import cases
import fp16_checks as fc
import fp16_storage_checks as sc
import parity_checks as pc
from dream_amd import models, ops
from oracle import models as om
from oracle import topology

HALF_MAX = sc.HALF_MAX
NUM_VARIANTS = 8

# NHWC (B, H, W, Cin, Cout, k): tile edge + odd W + paired store; the 64-channel 1x1 tile; odd Cout (generic path); several chunks
RESIDUAL_SHAPES = [(2, 5, 7, 64, 96, 1), (1, 9, 6, 32, 64, 1), (1, 6, 5, 32, 33, 3), (2, 13, 13, 128, 256, 1)]
STRIDED_SHAPES = [(2, 9, 12, 64, 96), (1, 8, 8, 32, 64)]
GATHER_SHAPES = [(2, 7, 10, 32), (1, 8, 8, 64), (1, 1, 1, 8)]
POOL_SHAPES = [(2, 7, 10, 64), (1, 8, 8, 8)]


# ---- per launch ------------------------------------------------------------------------------------------------------------------
def check_residual_conv(dev, B, H, W, Cin, Cout, k, relu, seed=0):
    """conv2d_f16_act16_res against conv2d_f16 on the widened operands (bit equality) and the fp64 conv (the derived bound)."""
    g = torch.Generator().manual_seed(seed)
    x16 = sc.half_input((B, Cin, H, W), 1.0, g)
    r16 = sc.half_input((B, Cout, H, W), 2.0, g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.1
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    flags = ops.CONV_RELU if relu else 0
    p16 = ops.pack_conv_weight_f16(pc.to(dev, w), 0)
    xd, rd, sd, td = pc.to(dev, pc._nhwc(x16)), pc.to(dev, pc._nhwc(r16)), pc.to(dev, scale), pc.to(dev, shift)
    y32, amax32 = ops.conv2d_f16(xd.float(), ops.absmax(xd.float()), p16, Cout, k, sd, td, rd.float(), flags)
    peak = ops.new_amax(xd.device)
    y16 = ops.conv2d_f16_act16_res(xd, p16, Cout, k, rd, sd, td, flags, peak=peak)
    what = ("res16", B, H, W, Cin, Cout, k, relu)
    assert y16.dtype == torch.float16 and tuple(y16.shape) == (B, H, W, Cout), what
    assert torch.equal(sc.bits(y16), sc.bits(sc.sat_half(y32))), what
    assert fc._amax_value(peak) == fc._amax_value(amax32) == float(y32.abs().max()), what
    ref = F.conv2d(x16.double(), fc.q(w).double(), None, padding=k // 2) * scale.double().view(1, -1, 1, 1) \
        + shift.double().view(1, -1, 1, 1) + r16.double()
    sc._hold(y16.cpu().permute(0, 3, 1, 2), ref.relu() if relu else ref, what)


def check_residual_launches(dev, seed=0):
    for shape in RESIDUAL_SHAPES:
        for relu in (True, False):
            check_residual_conv(dev, *shape, relu, seed=seed)


def check_residual_saturation(dev):
    """A residual that pushes the sum past 65504: a finite 65504 is stored, the peak scalar holds the unsaturated maximum."""
    g = torch.Generator().manual_seed(1)
    B, H, W, Cin, Cout = 1, 5, 7, 32, 64
    x16 = sc.half_input((B, H, W, Cin), 1.0, g)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) * 0.1
    r16 = torch.full((B, H, W, Cout), 60000.0).half()
    r16[0, 1] = -60000.0
    shift = torch.full((Cout,), 8000.0)
    shift[1::2] = -8000.0                                          # (both signs where the residual is negative)
    p16 = ops.pack_conv_weight_f16(pc.to(dev, w), 0)
    xd, rd, td = pc.to(dev, x16), pc.to(dev, r16), pc.to(dev, shift)
    y32, _ = ops.conv2d_f16(xd.float(), ops.absmax(xd.float()), p16, Cout, 1, None, td, rd.float(), 0)
    peak = ops.new_amax(xd.device)
    y16 = ops.conv2d_f16_act16_res(xd, p16, Cout, 1, rd, None, td, 0, peak=peak)
    assert float(y32.max()) > HALF_MAX and float(y32.min()) < -HALF_MAX
    assert bool(torch.isfinite(y16).all()) and float(y16.float().max()) == HALF_MAX and float(y16.float().min()) == -HALF_MAX
    assert torch.equal(sc.bits(y16), sc.bits(sc.sat_half(y32)))
    assert fc._amax_value(peak) == float(y32.abs().max()) > HALF_MAX


def check_residual_refusals(dev):
    import pytest
    x16 = pc.to(dev, torch.zeros(1, 4, 4, 32).half())
    r16 = pc.to(dev, torch.zeros(1, 4, 4, 64).half())
    p16 = ops.pack_conv_weight_f16(pc.to(dev, torch.zeros(64, 32, 3, 3)), 0)
    for flags in (ops.CONV_POOL2, ops.CONV_UPSAMPLE2X, ops.CONV_OUT_NCHW):
        with pytest.raises(RuntimeError, match="act16 \\+ residual form does not take flags"):
            ops.conv2d_f16_act16_res(x16, p16, 64, 3, r16, None, None, flags)
    with pytest.raises(RuntimeError, match="expected float16"):
        ops.conv2d_f16_act16_res(x16, p16, 64, 3, r16.float())
    with pytest.raises(RuntimeError, match="expected float16"):
        ops.conv2d_f16_act16_res(x16.float(), p16, 64, 3, r16)
    with pytest.raises(RuntimeError, match="residual must have the output's shape"):
        ops.conv2d_f16_act16_res(x16, p16, 64, 3, r16[:, :2].contiguous())


def check_gathers_and_pool(dev):
    """The four streaming kernels: bit-equal to the half of their fp32 siblings on the widened input."""
    import pytest
    g = torch.Generator().manual_seed(6)
    for shape in GATHER_SHAPES:
        x16 = pc.to(dev, (torch.randn(*shape, generator=g) * 50).half())
        for half_op, op32 in ((ops.subsample2_f16, ops.subsample2), (ops.im2col3s2_f16, ops.im2col3s2)):
            got, want = half_op(x16), op32(x16.float())
            assert got.dtype == torch.float16 and got.shape == want.shape, (half_op.__name__, shape)
            assert torch.equal(sc.bits(got), sc.bits(want.half())), (half_op.__name__, shape)
    for shape in POOL_SHAPES:
        x16 = pc.to(dev, (torch.randn(*shape, generator=g) * 50 - 200).half())          # all negative: a zero pad would win
        assert float(x16.float().max()) < 0
        got, want = ops.maxpool3s2_f16(x16), ops.maxpool3s2(x16.float())
        assert got.dtype == torch.float16 and got.shape == want.shape, shape
        assert torch.equal(sc.bits(got), sc.bits(want.half())), shape
    x = pc.to(dev, torch.randn(2, 3, 13, 18, generator=g) * 3)
    peak = ops.new_amax(x.device)
    got, want = ops.im2col_nchw_f16(x, 7, 7, 2, 3, 160, peak=peak), ops.im2col_nchw(x, 7, 7, 2, 3, 160)
    assert got.dtype == torch.float16 and tuple(got.shape) == tuple(want.shape) == (2, 7, 9, 160)
    assert torch.equal(sc.bits(got), sc.bits(want.half())) and not bool(got[..., 147:].any()) and bool(got[..., :147].any())
    assert fc._amax_value(peak) == float(x.abs().max())
    big = pc.to(dev, torch.full((1, 3, 4, 4), 1e6))
    assert float(ops.im2col_nchw_f16(big, 7, 7, 2, 3, 160).float().max()) == HALF_MAX               # saturating, never inf
    odd = pc.to(dev, torch.zeros(1, 4, 4, 12).half())
    for half_op in (ops.subsample2_f16, ops.im2col3s2_f16, ops.maxpool3s2_f16):
        with pytest.raises(RuntimeError, match="multiple of 8"):
            half_op(odd)
        with pytest.raises(RuntimeError, match="expected float16"):
            half_op(odd.float())
    with pytest.raises(RuntimeError, match="ResNet stem only"):
        ops.im2col_nchw_f16(x, 3, 3, 1, 1, 32)


@functools.lru_cache(maxsize=None)
def _host(dev):
    """A ResnetSimple whose half-storage arithmetic (models._EvalAct16) and block step (_bottleneck) the launch checks borrow; its own layers are not run."""
    return models.ResnetSimple(7, pretrained=False).eval()


def _random_bn(bn, g):
    with torch.no_grad():
        bn.weight.copy_(torch.rand(bn.weight.shape, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(bn.bias.shape, generator=g) * 0.2)
        bn.running_mean.copy_(torch.randn(bn.bias.shape, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(bn.bias.shape, generator=g) + 0.5)
    return bn.eval()


def _folded(net, name, bn):
    """The fp32 scale and shift the device folds this BatchNorm into, as float64 [1,C,1,1]."""
    scale, shift = net._fold(name, bn)
    return scale.cpu().double().view(1, -1, 1, 1), shift.cpu().double().view(1, -1, 1, 1)


def check_strided_conv(dev, B, H, W, Cin, Cout, k, seed=0):
    """A stride-2 conv as the walk runs it (gather + 1-tap conv on the fp16 matrix cores) against the fp64 strided conv of q(w)."""
    g = torch.Generator().manual_seed(seed)
    net = _host(dev)
    conv = nn.Conv2d(Cin, Cout, k, stride=2, padding=k // 2, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.1)
    bn = _random_bn(nn.BatchNorm2d(Cout), g)
    conv, bn = conv.to(dev), bn.to(dev)
    x16 = sc.half_input((B, Cin, H, W), 1.0, g)
    name = "check.s2.%d.%d.%d.%d" % (Cin, Cout, k, seed)
    peak = ops.new_amax(conv.weight.device)
    with torch.no_grad():
        y16 = models._EvalAct16(net, peak).conv(name, pc.to(dev, pc._nhwc(x16)), conv, bn, False)
        scale, shift = _folded(net, name, bn)
    ref = F.conv2d(x16.double(), fc.q(conv.weight.detach().cpu()).double(), None, stride=2, padding=k // 2) * scale + shift
    what = ("stride 2", B, H, W, Cin, Cout, k)
    assert y16.dtype == torch.float16 and tuple(y16.shape) == (B,) + tuple(ref.shape[2:]) + (Cout,), what
    sc._hold(y16.cpu().permute(0, 3, 1, 2), ref, what)
    assert abs(fc._amax_value(peak) - float(ref.abs().max())) <= 1e-3 * float(ref.abs().max()), what


def check_strided_convs(dev, seed=0):
    for shape in STRIDED_SHAPES:
        for k in (3, 1):
            check_strided_conv(dev, *shape, k, seed=seed)


# ---- one Bottleneck through the walk's helper -----------------------------------------------------------------------------------------
def block_oracle(net, name, blk, x16):
    """-> (y, e): the fp64 Bottleneck that rounds to saturating half exactly the tensors the device stores (the downsample result, the
    outputs of conv1 and conv2, the block output), and a bound on how far a correct device may be from it.  A launch differs from the
    fp64 conv of the same stored operands by fp32 accumulation, 5e-6 max|y| (fp16_checks); two values at most d apart round to halfs
    at most d + half an ulp of each apart, <= d + 2^-10 |y| + 2^-24; a difference e in a stored input moves a conv output by at most
    conv(e, |w|) |scale|; the ReLU moves nothing further."""
    def stage(cname, x, ex, conv, bn, relu, res=None, eres=None):
        w = fc.q(conv.weight.detach().cpu()).double()
        scale, shift = _folded(net, name + cname, bn)
        s, p = int(conv.stride[0]), int(conv.padding[0])
        y = F.conv2d(x, w, None, stride=s, padding=p) * scale + shift
        e = F.conv2d(ex, w.abs(), None, stride=s, padding=p) * scale.abs()
        if res is not None:
            y, e = y + res, e + eres
        if relu:
            y = y.relu()
        e = e + 5e-6 * float(y.abs().max())
        ys = sc.sat_half(y).double()
        return ys, e + 2.0 ** -10 * ys.abs() + 2.0 ** -24

    x, zero = x16.double(), torch.zeros(x16.shape, dtype=torch.float64)
    idt, eidt = stage(".ds", x, zero, blk.downsample[0], blk.downsample[1], False)
    o, eo = stage(".1", x, zero, blk.conv1, blk.bn1, True)
    o, eo = stage(".2", o, eo, blk.conv2, blk.bn2, True)
    return stage(".3", o, eo, blk.conv3, blk.bn3, True, idt, eidt)


def check_bottleneck(dev, seed=0):
    """Bottleneck(64, 32, stride 2, downsample) on 2 x 9 x 12 through the walk's block step on the half-storage arithmetic."""
    g = torch.Generator().manual_seed(seed)
    net = _host(dev)
    ds = nn.Sequential(nn.Conv2d(64, 128, 1, stride=2, bias=False), nn.BatchNorm2d(128))
    blk = topology.Bottleneck(64, 32, 2, ds).eval()
    for mod in blk.modules():
        if isinstance(mod, nn.Conv2d):
            with torch.no_grad():
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (2.0 / (mod.weight[0].numel())) ** 0.5)
        elif isinstance(mod, nn.BatchNorm2d):
            _random_bn(mod, g)
    blk = blk.to(dev)
    x16 = sc.half_input((2, 64, 9, 12), 1.0, g, outlier=8.0)
    name = "check.block.%d" % seed
    peak = ops.new_amax(blk.conv1.weight.device)
    with torch.no_grad():
        y16 = net._bottleneck(models._EvalAct16(net, peak), name, blk, pc.to(dev, pc._nhwc(x16)))
        ref, bound = block_oracle(net, name, blk, x16)
    assert y16.dtype == torch.float16 and tuple(y16.shape) == (2, 5, 6, 128)
    got = y16.cpu().permute(0, 3, 1, 2).double()
    worst = float(((got - ref).abs() / bound).max())
    loose = float((bound / (2.0 ** -11 * ref.abs() + 1e-3 * float(ref.abs().max()))).max())
    print("fp16 storage Bottleneck: worst error %.3g of the carried bound (which is at most %.3g half-ulps + 1e-3 max|ref|), peak %.4g"
          % (worst, loose, fc._amax_value(peak)))
    assert worst <= 1.0, worst
    assert float(ref.abs().max()) > 0 and float((ref > 0).double().mean()) > 0.2          # (a block that outputs zeros holds nothing)
    assert 0.0 < fc._amax_value(peak) < HALF_MAX


# ---- end to end ------------------------------------------------------------------------------------------------------------------
STORED_TENSORS = {"resnet_h": 108, "resnet_f": 109}
_stored_count = {}


def _stored_run(arch, k, weights, x, dtype):
    """The reference ResnetSimple with q(weight) at every conv (strided ones included) whose stored tensors are saturating halfs: the
    image in front of conv1; the output of every BatchNorm but each Bottleneck's bn3 (rounding commutes with the ReLU and the
    max-pool behind it); the output of every Bottleneck (after add and ReLU)."""
    model = om.build_model(arch, k)
    model.load_state_dict(weights)
    model.eval()
    model = model.to(dtype)

    def store(t):
        return sc.sat_half(t).to(t.dtype)

    stored = []

    def hook(m, inp, out):
        stored.append(m)
        return store(out)

    bn3 = {id(m.bn3) for m in model.modules() if isinstance(m, topology.Bottleneck)}
    for mod in model.modules():
        if isinstance(mod, (nn.Conv2d, nn.ConvTranspose2d)):
            with torch.no_grad():
                mod.weight.copy_(fc.q(mod.weight))
        if isinstance(mod, topology.Bottleneck) or (isinstance(mod, nn.BatchNorm2d) and id(mod) not in bn3):
            mod.register_forward_hook(hook)
    model.conv1.register_forward_pre_hook(lambda m, inp: (store(inp[0]),))
    with torch.no_grad():
        maps = model(x.to(dtype))[-1].numpy()
    _stored_count[arch] = len(stored)
    return maps


def _oracle(arch, k, weights, x, golden_maps):
    """fc._oracle (E, P, held: computed there, not here) over the half-storage runs."""
    saved = fc._rounded_run
    fc._rounded_run = _stored_run
    try:
        return fc._oracle(arch, k, weights, x, golden_maps)
    finally:
        fc._rounded_run = saved


@functools.lru_cache(maxsize=None)
def stored_oracle(case):
    arch, _, k, _, _, _, _ = cases.STRUCTURED_CASES[case]
    weights, g = fc._structured_weights(case)
    x, _ = cases.structured_input(case)
    _stored_count.pop(arch, None)
    res = _oracle(arch, k, weights, torch.from_numpy(x), g["maps"])
    assert _stored_count.get(arch) == STORED_TENSORS[arch], ("the half-storage runs did not reach fp16_checks._oracle", _stored_count)
    del res["runs"]
    res["maps"] = g["maps"]
    return res


def structured_network(dev, case, storage="fp16"):
    net = fc.structured_network(dev, case)
    net.model.module.inference_activation_storage = storage
    return net


def check_structured(dev, case):
    """fp16_storage_checks.check_structured for ResnetSimple: maps within 3 E of the golden (and more than 1e-4 away), held decisions the
    golden's, held keypoints within max(3 P, 1e-3 px), held sentinels bit for bit, at most 2 maps left out, 0 < peak < 65504.  Prints
    (does not assert) the distance from the fp32-storage maps."""
    orc = stored_oracle(case)
    E, P, held, ref_k = orc["E"], orc["P"], orc["held"], orc["ref_k"]
    x = pc.to(dev, torch.from_numpy(cases.structured_input(case)[0]))
    net = structured_network(dev, case)
    with torch.no_grad():
        maps, kps = net.inference(x)
        maps32 = structured_network(dev, case, "fp32").inference(x)[0]
    assert maps.dtype == torch.float32
    peak = net.model.module.half_storage_peak()
    y, got_k = maps.cpu().numpy(), kps.numpy()
    err = float(np.abs(y.astype(np.float64) - orc["maps"]).max())
    det = ref_k[..., 0] > -999
    both = held & det & (got_k[..., 0] > -999)
    perr = float(np.abs(got_k - ref_k)[both].max(initial=0.0))
    print("fp16 storage structured %s: E %.3g, P %.3g px, device error %.3g, keypoint error %.3g px, %d of %d maps left out, "
          "max|maps(storage fp16) - maps(storage fp32)| %.3g, stored peak %.4g"
          % (case, E, P, err, perr, int((~held).sum()), held.size, float((maps - maps32).abs().max()), peak))
    assert 0.0 < peak < HALF_MAX, (case, peak)
    assert int((~held).sum()) <= 2, (case, int((~held).sum()))
    assert err <= 3 * E, (case, err, E)
    assert err > 1e-4, (case, err)
    assert np.array_equal((got_k[..., 0] > -999)[held], det[held]), "a held detection / rejection decision differs from the golden"
    assert perr <= max(3 * P, 1e-3), (case, perr, P)
    rej = held & ~det
    assert np.array_equal(got_k[rej], ref_k[rej])
    return err, perr
