"""Checks of activation_storage="fp16" (precision="fp16" with the activations stored as IEEE half; csrc/conv_f16.hip ACT16), shared by
the emulator and the GPU suite.

Per launch nothing is measured.  (1) On inputs that are halfs already -- normal halfs or zero, max|x| <= 2^13, so that today's
fp16(x * 2^ea) is exact -- the half-storage launch must equal fp16(clamp(y32)) bit for bit, y32 being today's fp32-storage launch of
the same variant: power-of-two scaling commutes with every rounding in the kernel, so a difference means the new loader or epilogue
computes something else.  (2) Independently of the old kernel, against the fp64 conv of x16 and q(w):
    |got - ref| <= 5e-6 max|ref| + 2^-11 |ref| + 2^-25
-- the fp32-accumulation bound fp16_checks holds, half a half-ulp of the stored value, and the half subnormal floor.

End to end the bound is measured on the reference, by rounded_storage_oracle(): fp16_checks' oracle with, in addition, the input and
the output of every conv rounded to plain saturating half; E, P and the held maps come from fp16_checks._oracle itself."""
import functools
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import cases
import fp16_checks as fc
import parity_checks as pc
from dream_amd import ops
from oracle import models as om
from oracle import peaks as op

GOLD = pc.GOLD
HALF_MAX = 65504.0


def sat_half(t):
    """fp16(clamp(t, +-65504)): what activation_storage="fp16" stores for the value t."""
    return t.float().clamp(-HALF_MAX, HALF_MAX).half()


def bits(t):
    return t.contiguous().view(torch.int16)


def half_input(shape, scale, gen, outlier=40.0):
    """half(randn * scale) with one outlier; magnitudes below 2^-14 (half subnormals) set to 0, max|x| <= 2^13."""
    assert outlier * scale <= 2.0 ** 13
    x = torch.randn(*shape, generator=gen) * scale
    x.view(-1)[0] = outlier * scale
    x16 = x.half()
    x16[x16.abs() < 2.0 ** -14] = 0
    assert float(x16.abs().max()) <= 2.0 ** 13
    return x16


def _hold(got, ref, what):
    """The derived elementwise bound against an fp64 reference (already saturated)."""
    ref = ref.clamp(-HALF_MAX, HALF_MAX)
    bound = 5e-6 * float(ref.abs().max()) + 2.0 ** -11 * ref.abs() + 2.0 ** -25
    worst = float(((got.double() - ref).abs() / bound).max())
    print("fp16 storage %s: worst error %.3g of the bound" % (what, worst))
    assert worst <= 1.0, (what, worst)


def check_conv(dev, B, H, W, Cin, Cout, k, flags, x_scale=1.0, w_scale=0.1, seed=0, saturate=False):
    """conv2d_f16_act16 on x16 against today's conv2d_f16 on float(x16) (bit equality) and against the fp64 conv of x16 and q(w)."""
    g = torch.Generator().manual_seed(seed)
    ups = bool(flags & ops.CONV_UPSAMPLE2X)
    x16 = half_input((B, Cin, H // 2 if ups else H, W // 2 if ups else W), x_scale, g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * w_scale
    bias = torch.randn(Cout, generator=g) * x_scale * w_scale
    p16 = ops.pack_conv_weight_f16(pc.to(dev, w), 0)
    xd = pc.to(dev, pc._nhwc(x16))
    y32, amax32 = ops.conv2d_f16(xd.float(), ops.absmax(xd.float()), p16, Cout, k, None, pc.to(dev, bias), None, flags)
    peak = ops.new_amax(xd.device)
    y16 = ops.conv2d_f16_act16(xd, p16, Cout, k, None, pc.to(dev, bias), flags, peak=peak)
    what = (B, H, W, Cin, Cout, k, flags)
    nchw = bool(flags & ops.CONV_OUT_NCHW)
    ho, wo = (H // 2, W // 2) if flags & ops.CONV_POOL2 else (H, W)
    if nchw:
        assert y16.dtype == torch.float32 and torch.equal(y16.view(torch.int32), y32.view(torch.int32)), what
    else:
        assert y16.dtype == torch.float16 and y16.numel() * y16.element_size() == B * ho * wo * Cout * 2, what
        assert torch.equal(bits(y16), bits(sat_half(y32))), what
        assert bool(torch.isfinite(y16).all()), what
    if amax32 is not None:
        assert fc._amax_value(peak) == fc._amax_value(amax32) == float(y32.abs().max()), what     # max|y32|, before the saturation
    if saturate:
        assert float(y32.abs().max()) > HALF_MAX and float(y16.float().abs().max()) == HALF_MAX, what
    xr = F.interpolate(x16.double(), scale_factor=2) if ups else x16.double()
    ref = F.conv2d(xr, fc.q(w).double(), bias.double(), padding=k // 2)
    if flags & ops.CONV_RELU:
        ref = ref.relu()
    if flags & ops.CONV_POOL2:
        ref = F.max_pool2d(ref, 2)
    got = y16.cpu() if nchw else y16.cpu().permute(0, 3, 1, 2)
    _hold(got, ref, what)


def check_conv_transpose(dev, ksize, B, H, W, Cin, Cout, seed=0):
    """conv_transpose3x3s2_f16_act16 (the deconv decoder) / conv_transpose4x4s2_f16_act16 (upsample + conv), + bias + ReLU."""
    g = torch.Generator().manual_seed(seed)
    x16 = half_input((B, Cin, H, W), 1.0, g)
    wT = torch.randn(Cin, Cout, ksize, ksize, generator=g) * (2.0 / (ksize * Cin)) ** 0.5
    bias = torch.randn(Cout, generator=g)
    xd, bd = pc.to(dev, pc._nhwc(x16)), pc.to(dev, bias)
    peak = ops.new_amax(xd.device)
    if ksize == 3:
        p16 = ops.pack_conv_weight_f16(pc.to(dev, wT), 1)
        y32, amax32 = ops.conv_transpose3x3s2_f16(xd.float(), ops.absmax(xd.float()), p16, p16[3], bd, relu=True)
        y16 = ops.conv_transpose3x3s2_f16_act16(xd, p16, p16[3], bd, relu=True, peak=peak)
        ref = F.conv_transpose2d(x16.double(), fc.q(wT).double(), bias.double(), stride=2, padding=1, output_padding=1).relu()
    else:
        p16 = ops.pack_convT4x4_weight_f16(pc.to(dev, wT))
        y32, amax32 = ops.conv_transpose4x4s2_f16(xd.float(), ops.absmax(xd.float()), p16, p16[3], None, bd, ops.CONV_RELU)
        y16 = ops.conv_transpose4x4s2_f16_act16(xd, p16, p16[3], None, bd, ops.CONV_RELU, peak=peak)
        ref = F.conv_transpose2d(x16.double(), fc.q(wT).double(), bias.double(), stride=2, padding=1).relu()
    what = ("convT%d" % ksize, B, H, W, Cin, Cout)
    assert y16.dtype == torch.float16 and y16.numel() * y16.element_size() == B * 2 * H * 2 * W * Cout * 2, what
    assert torch.equal(bits(y16), bits(sat_half(y32))), what
    assert fc._amax_value(peak) == fc._amax_value(amax32), what
    _hold(y16.cpu().permute(0, 3, 1, 2), ref, what)


def check_launches(dev, seed=0, large=False):
    """The shapes of test_conv_f16_variants: tile edges, chunk changes, pool, upsample, phases (``large``: the GPU-only ones too)."""
    check_conv(dev, 1, 7, 9, 32, 40, 3, ops.CONV_RELU, seed=seed)
    check_conv(dev, 2, 12, 20, 64, 7, 3, ops.CONV_OUT_NCHW, x_scale=200.0, w_scale=1e-3, seed=seed)
    check_conv(dev, 1, 6, 8, 32, 64, 3, ops.CONV_RELU | ops.CONV_UPSAMPLE2X, x_scale=1e-3, w_scale=5.0, seed=seed)
    check_conv(dev, 2, 9, 11, 64, 48, 1, 0, seed=seed)
    check_conv(dev, 2, 12, 20, 32, 48, 3, ops.CONV_RELU | ops.CONV_POOL2, seed=seed)
    check_conv(dev, 1, 13, 9, 64, 32, 3, ops.CONV_RELU | ops.CONV_POOL2, seed=seed)
    check_conv_transpose(dev, 3, 1, 5, 7, 32, 48, seed=seed)
    if large:
        check_conv(dev, 2, 33, 47, 64, 96, 3, ops.CONV_RELU, seed=seed)
        check_conv(dev, 2, 25, 25, 512, 128, 1, 0, seed=seed)


def check_saturation(dev):
    """One launch whose fp32 result exceeds 65504: finite output = fp16(clamp(y32)), the peak scalar holds max|y32|."""
    check_conv(dev, 1, 7, 9, 32, 40, 3, ops.CONV_RELU, x_scale=100.0, w_scale=30.0, saturate=True)
    check_conv(dev, 1, 7, 9, 32, 40, 3, 0, x_scale=100.0, w_scale=30.0, saturate=True, seed=1)       # (both signs)


def check_first_conv(dev):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 13, 17, generator=g)
    for w_scale in (0.2, 20000.0):                                  # the second saturates
        w, bias = torch.randn(64, 3, 3, 3, generator=g) * w_scale, torch.randn(64, generator=g)
        y32, amax32 = ops.conv3x3_first_amax(pc.to(dev, x), pc.to(dev, w), pc.to(dev, bias), relu=True)
        peak = ops.new_amax(y32.device)
        y16 = ops.conv3x3_first_f16(pc.to(dev, x), pc.to(dev, w), pc.to(dev, bias), relu=True, peak=peak)
        assert y16.dtype == torch.float16 and tuple(y16.shape) == (2, 13, 17, 64)
        assert torch.equal(bits(y16), bits(sat_half(y32)))
        assert fc._amax_value(peak) == fc._amax_value(amax32) == float(y32.abs().max())
    assert float(y32.abs().max()) > HALF_MAX and bool(torch.isfinite(y16).all())


def check_maxpool(dev):
    g = torch.Generator().manual_seed(4)
    for shape in ((2, 12, 20, 64), (1, 13, 9, 32)):
        x16 = pc.to(dev, (torch.randn(*shape, generator=g) * 50).half())
        y16 = ops.maxpool2_f16(x16)
        assert y16.dtype == torch.float16 and tuple(y16.shape) == (shape[0], shape[1] // 2, shape[2] // 2, shape[3])
        assert torch.equal(bits(y16), bits(sat_half(ops.maxpool2(x16.float()))))


def check_add(dev):
    g = torch.Generator().manual_seed(5)
    a16, b16 = ((torch.randn(2, 7, 9, 40, generator=g) * 100).half() for _ in range(2))
    a16.view(-1)[:4] = torch.tensor([65504.0, -65504.0, 6e-5, 1.5], dtype=torch.float16)
    b16.view(-1)[:4] = torch.tensor([65504.0, -60000.0, -5.9e-5, 2.0 ** -24], dtype=torch.float16)
    a16, b16 = pc.to(dev, a16), pc.to(dev, b16)
    y32, amax32 = ops.add(a16.float(), b16.float(), want_amax=True)
    peak = ops.new_amax(a16.device)
    y16 = ops.add_f16(a16, b16, peak=peak)
    assert y16.dtype == torch.float16 and y16.shape == a16.shape and bool(torch.isfinite(y16).all())
    assert torch.equal(bits(y16), bits(sat_half(y32)))
    assert fc._amax_value(peak) == fc._amax_value(amax32) == 131008.0


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _storage_run(arch, k, weights, x, dtype):
    """fc._rounded_run's network -- q(weight) at every conv but the 3-channel one -- whose convs read and write plain saturating
    halfs: the input of every conv but the 3-channel one (pre-hook), the output of every conv but the last (forward hook)."""
    model = om.build_model(arch, k)
    model.load_state_dict(weights)
    model.eval()
    model = model.to(dtype)
    convs = [m for m in model.modules() if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))]
    order = []
    probes = [m.register_forward_hook(lambda m, i, o: order.append(m)) for m in convs]
    with torch.no_grad():
        model(torch.zeros(1, 3, 32, 32, dtype=dtype))
    for h in probes:
        h.remove()
    last = order[-1]

    def store(t):
        return sat_half(t).to(t.dtype)

    for mod in convs:
        first = isinstance(mod, nn.Conv2d) and tuple(mod.kernel_size) == (3, 3) and mod.in_channels == 3
        if not first:
            with torch.no_grad():
                mod.weight.copy_(fc.q(mod.weight))
            mod.register_forward_pre_hook(lambda m, inp: (store(inp[0]),))
        if mod is not last:
            mod.register_forward_hook(lambda m, inp, out: store(out))
    with torch.no_grad():
        return model(x.to(dtype))[-1].numpy()


def _oracle(arch, k, weights, x, golden_maps, compare=lambda m: m):
    """fc._oracle (E, P, held: computed there, not here) over the half-storage runs."""
    saved = fc._rounded_run
    fc._rounded_run = _storage_run
    try:
        return fc._oracle(arch, k, weights, x, golden_maps, compare)
    finally:
        fc._rounded_run = saved


@functools.lru_cache(maxsize=None)
def rounded_storage_oracle(case):
    arch, _, k, _, _, _, _ = cases.STRUCTURED_CASES[case]
    weights, g = fc._structured_weights(case)
    x, _ = cases.structured_input(case)
    res = _oracle(arch, k, weights, torch.from_numpy(x), g["maps"])
    del res["runs"]
    res["maps"] = g["maps"]
    if case == "vgg_q":
        # _oracle reaches _storage_run through fp16_checks' module global: were that binding ever made early, this would quietly be
        # today's oracle again.  For vgg_q the two differ (2.80e-3 against 3.03e-3).
        assert res["E"] != fc.rounded_operand_oracle(case)["E"], "the half-storage runs did not reach fp16_checks._oracle"
    return res


def structured_network(dev, case, storage="fp16"):
    net = fc.structured_network(dev, case)
    net.model.module.activation_storage = storage
    return net


def check_structured(dev, case):
    """fc.check_structured_f16 with activation_storage="fp16", held to the half-storage oracle: maps within 3 E of the golden (and more
    than 1e-4 away), held decisions the golden's, held keypoints within max(3 P, 1e-3 px), held sentinels bit for bit, at most 2 maps
    left out.  Prints (does not assert) the distance from the fp32-storage maps."""
    orc = rounded_storage_oracle(case)
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


def check_golden(dev, name, shape, with_fp32=True):
    """fc.check_golden_f16 with activation_storage="fp16" (the skip variants: re-rounded skip sums): maps within 3 E of the half-storage
    oracle for this very input, the peak stage bit-exact on the produced maps.  ``with_fp32``: also run and print the distance from
    the fp32-storage maps."""
    b, h, w = shape
    tag = "%dx%dx%d" % (b, h, w)
    variant = name in om.VARIANTS
    g = np.load(os.path.join(GOLD, ("variant_%s.npz" if variant else "cnn_%s.npz") % name))
    sampled = tag + "/maps" not in g
    golden = g[tag + "/maps_sample"] if sampled else g[tag + "/maps"]
    compare = (lambda m: m[:, :, ::7, ::7]) if sampled else (lambda m: m)
    k = 7 if variant else cases.CNN_CASES[name][0]
    weights = om.recipe_weights(om.build_model(name, k).state_dict())
    x = torch.from_numpy(cases.image_batch(b, h, w, seed=b * 1000 + h))
    E = _oracle(name, k, weights, x, golden, compare)["E"]
    net = pc.build_network(name, dev)
    net.enable_evaluation()
    net.model.module.precision = "fp16"
    with torch.no_grad():
        maps32 = net.inference(pc.to(dev, x))[0] if with_fp32 else None
        net.model.module.activation_storage = "fp16"
        maps, kps = net.inference(pc.to(dev, x))
    peak = net.model.half_storage_peak()                          # (raises unless the half-storage walk ran)
    assert 0.0 < peak < HALF_MAX, (name, tag, peak)
    y = maps.cpu().numpy()
    err = float(np.abs(compare(y).astype(np.float64) - golden).max())
    print("fp16 storage golden %s %s: E %.3g, device error %.3g, max|maps(storage fp16) - maps(storage fp32)| %s"
          % (name, tag, E, err, "%.3g" % float((maps - maps32).abs().max()) if with_fp32 else "not run"))
    assert err <= 3 * E, (name, tag, err, E)
    off = op.upsampling_offset(*net.trained_net_output_resolution())
    assert np.array_equal(kps.numpy(), op.keypoints_from_belief_maps(y, off))
    return err
