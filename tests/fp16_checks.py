"""Checks of precision="fp16" (fp16 operands, fp32 accumulation; csrc/conv_f16.hip), shared by the emulator and the GPU suite.

Per launch the bound is derived: the kernel computes the conv of the ROUNDED operands q(x), q(w) -- products of two halfs are exact
in fp32 --, so against an fp64 conv of those it may differ by fp32 accumulation only, the 5e-6 that check_conv_f16x3 holds the same
accumulation structure to.  The fp64 conv of the UNROUNDED operands must lie ten times further away, or the launch under test did
not round (an fp32 or split kernel wired in by mistake).

End to end the bound is measured on the reference, by rounded_operand_oracle(): oracle.models with every conv but the 3-channel
3x3 one given q(weight) and q(input), run in float32 and in float64.  E = the larger distance of the two runs' maps from the
golden maps, P = the larger keypoint error on held maps; the device is held to 3 E and max(3 P, 1e-3 px)."""
import functools
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import cases
import parity_checks as pc
from dream_amd import ops
from oracle import models as om
from oracle import peaks as op

GOLD = pc.GOLD
SENTINEL = np.float32(-999.999)


def scale_exponent(t):
    """e with max|t| * 2^e in [2^13, 2^14) (0 for a zero tensor; clamps as in conv_f16x3.hip)."""
    m = float(t.abs().max())
    if m == 0.0:
        return 0
    return max(-100, min(100, 13 - (math.frexp(m)[1] - 1)))


def q(t):
    """fp16(t * 2^e) * 2^-e in t's dtype: the one rounding the fp16 path applies to an operand (to nearest even)."""
    s = 2.0 ** scale_exponent(t)
    return ((t.float() * s).half().float() / s).to(t.dtype)


def _amax_value(amax):
    return float(np.frombuffer(amax.cpu().numpy().tobytes(), dtype=np.float32)[0])


def _hold_launch(got, amax_out, ref, ref_unrounded, what):
    scale = float(ref.abs().max())
    err = float((got.double() - ref).abs().max()) / scale
    away = float((ref_unrounded - ref).abs().max()) / scale
    print("fp16 launch %s: err %.3g of max|ref|, unrounded operands %.3g away" % (what, err, away))
    assert err <= 5e-6, (what, err)
    assert away > 5e-5, (what, away)              # (so a kernel that does not round its operands cannot pass the line above)
    assert abs(_amax_value(amax_out) - float(got.abs().max())) <= 1e-6 * scale, what
    return err


def check_conv_f16(dev, B, H, W, Cin, Cout, k, flags, x_scale=1.0, w_scale=0.1, seed=0):
    """conv2d_f16 against the fp64 conv of the rounded operands; inputs, bias, ReLU, pool and upsample as in check_conv_f16x3."""
    g = torch.Generator().manual_seed(seed)
    ups = bool(flags & ops.CONV_UPSAMPLE2X)
    x = torch.randn(B, Cin, H // 2 if ups else H, W // 2 if ups else W, generator=g) * x_scale
    x[0, 0, 0, 0] = 40 * x_scale
    w = torch.randn(Cout, Cin, k, k, generator=g) * w_scale
    bias = torch.randn(Cout, generator=g) * x_scale * w_scale

    def reference(xv, wv):
        xr = F.interpolate(xv, scale_factor=2) if ups else xv
        r = F.conv2d(xr.double(), wv.double(), bias.double(), padding=k // 2)
        if flags & ops.CONV_RELU:
            r = r.relu()
        return F.max_pool2d(r, 2) if flags & ops.CONV_POOL2 else r

    p16 = ops.pack_conv_weight_f16(pc.to(dev, w), 0)
    assert p16[1] is None and p16[0].dtype == torch.float16
    y, amax_out = ops.conv2d_f16(pc.to(dev, pc._nhwc(x)), ops.absmax(pc.to(dev, x)), p16, Cout, k, None, pc.to(dev, bias), None, flags)
    got = y.cpu() if flags & ops.CONV_OUT_NCHW else y.cpu().permute(0, 3, 1, 2)
    return _hold_launch(got, amax_out, reference(q(x), q(w)), reference(x, w), (B, H, W, Cin, Cout, k, flags))


def check_conv_transpose4x4_f16(dev, B, H, W, Cin, Cout, seed=0):
    """conv_transpose4x4s2_f16 (+bias, ReLU); inputs as in check_conv_transpose4x4_f16x3."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    x[0, 0, 0, 0] = 30.0
    wT = torch.randn(Cin, Cout, 4, 4, generator=g) * (2.0 / (4 * Cin)) ** 0.5
    bias = torch.randn(Cout, generator=g)

    def reference(xv, wv):
        return F.conv_transpose2d(xv.double(), wv.double(), bias.double(), stride=2, padding=1).relu()

    p16 = ops.pack_convT4x4_weight_f16(pc.to(dev, wT))
    y, amax = ops.conv_transpose4x4s2_f16(pc.to(dev, pc._nhwc(x)), ops.absmax(pc.to(dev, x)), p16, p16[3], None, pc.to(dev, bias),
                                          ops.CONV_RELU)
    return _hold_launch(y.cpu().permute(0, 3, 1, 2), amax, reference(q(x), q(wT)), reference(x, wT), ("convT4x4", B, H, W, Cin, Cout))


def check_conv_transpose3x3_f16(dev, B, H, W, Cin, Cout, seed=0):
    """conv_transpose3x3s2_f16: ConvTranspose2d(3, 2, 1, output_padding 1) + bias + ReLU, one outlier that sets the scale."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    x[0, 0, 0, 0] = 40.0
    wT = torch.randn(Cin, Cout, 3, 3, generator=g) * (2.0 / (3 * Cin)) ** 0.5
    bias = torch.randn(Cout, generator=g)

    def reference(xv, wv):
        return F.conv_transpose2d(xv.double(), wv.double(), bias.double(), stride=2, padding=1, output_padding=1).relu()

    p16 = ops.pack_conv_weight_f16(pc.to(dev, wT), 1)
    y, amax = ops.conv_transpose3x3s2_f16(pc.to(dev, pc._nhwc(x)), ops.absmax(pc.to(dev, x)), p16, p16[3], pc.to(dev, bias), relu=True)
    return _hold_launch(y.cpu().permute(0, 3, 1, 2), amax, reference(q(x), q(wT)), reference(x, wT), ("convT3x3s2", B, H, W, Cin, Cout))


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _rounded_run(arch, k, weights, x, dtype):
    """Maps of the reference network with q(weight) and q(input) at every conv but the 3x3 conv of 3 input channels, in ``dtype``."""
    model = om.build_model(arch, k)
    model.load_state_dict(weights)
    model.eval()
    model = model.to(dtype)
    for mod in model.modules():
        if not isinstance(mod, (nn.Conv2d, nn.ConvTranspose2d)):
            continue
        if isinstance(mod, nn.Conv2d) and tuple(mod.kernel_size) == (3, 3) and mod.in_channels == 3:
            continue
        with torch.no_grad():
            mod.weight.copy_(q(mod.weight))
        mod.register_forward_pre_hook(lambda m, inp: (q(inp[0].float()).to(inp[0].dtype),))
    with torch.no_grad():
        return model(x.to(dtype))[-1].numpy()


def _peak_scores(maps_khw, offset):
    """[(s1, s2, number of peaks)] per map: the two best peak scores (0 where there is none)."""
    out = []
    for peaks in op.peaks_from_belief_maps(maps_khw, offset):
        s = sorted((float(p[2]) for p in peaks), reverse=True) + [0.0, 0.0]
        out.append((s[0], s[1], len(peaks)))
    return out


def _oracle(arch, k, weights, x, golden_maps, compare=lambda m: m):
    """-> dict(E, P, held [B,K] bool, ref_k [B,K,2], offset).  ``compare``: the view of the maps the golden file stores."""
    runs = [_rounded_run(arch, k, weights, x, dt) for dt in (torch.float32, torch.float64)]
    E = max(float(np.abs(compare(r).astype(np.float64) - golden_maps).max()) for r in runs)
    out = {"E": E, "runs": runs}
    if compare(runs[0]).shape != runs[0].shape:                # a sampled golden: no peaks to hold
        return out
    offset = op.upsampling_offset(golden_maps.shape[3], golden_maps.shape[2])
    held = np.zeros(golden_maps.shape[:2], dtype=bool)
    for b in range(golden_maps.shape[0]):
        for j, (s1, s2, n) in enumerate(_peak_scores(golden_maps[b], offset)):
            held[b, j] = abs(s1 - s2 - 0.25) >= 6 * E and (n < 2 or s1 - s2 >= 6 * E)
    ref_k = op.keypoints_from_belief_maps(golden_maps, offset)
    P = 0.0
    for r in runs:
        kp = op.keypoints_from_belief_maps(r.astype(np.float32), offset)
        both = held & (kp[..., 0] > -999) & (ref_k[..., 0] > -999)
        P = max(P, float(np.abs(kp - ref_k)[both].max(initial=0.0)))
    out.update(P=P, held=held, ref_k=ref_k, offset=offset)
    return out


def _structured_weights(case):
    arch, _, k, last, _, recipe, _ = cases.STRUCTURED_CASES[case]
    g = cases.load_structured(GOLD, case)
    sd = om.build_model(arch, k).state_dict()
    weights = {"structured": om.structured_weights, "smooth": om.smooth_weights, "recipe": om.recipe_weights}[recipe](sd)
    weights[last + ".weight"] = torch.from_numpy(g["final_weight"])
    weights[last + ".bias"] = torch.from_numpy(g["final_bias"])
    return weights, g


@functools.lru_cache(maxsize=None)
def rounded_operand_oracle(case):
    """E, P and the held maps of a structured case (weights built as check_structured builds them), computed once per process."""
    arch, _, k, _, _, _, _ = cases.STRUCTURED_CASES[case]
    weights, g = _structured_weights(case)
    x, _ = cases.structured_input(case)
    res = _oracle(arch, k, weights, torch.from_numpy(x), g["maps"])
    del res["runs"]
    res["maps"] = g["maps"]
    return res


def structured_network(dev, case, precision="fp16"):
    arch, _, _, _, (b, h, w), _, _ = cases.STRUCTURED_CASES[case]
    weights, _ = _structured_weights(case)
    net = pc.build_network(arch, dev, weights=weights, in_res=(w, h))
    net.enable_evaluation()
    net.model.module.precision = precision
    return net


def check_structured_f16(dev, case):
    """The structured fixture at its own batch with precision="fp16": maps within 3 E of the golden (and further than the fp32
    path's 1e-4: the fp16 kernels really ran), every held decision the golden's, held keypoints within max(3 P, 1e-3 px), held
    sentinels bit for bit.  At most 2 maps of a case may be left out (ties and near-ties of the 0.25 rule)."""
    orc = rounded_operand_oracle(case)
    E, P, held, ref_k = orc["E"], orc["P"], orc["held"], orc["ref_k"]
    assert np.array_equal(ref_k, cases.load_structured(GOLD, case)["keypoints"])
    net = structured_network(dev, case)
    x, _ = cases.structured_input(case)
    with torch.no_grad():
        maps, kps = net.inference(pc.to(dev, torch.from_numpy(x)))
    y, got_k = maps.cpu().numpy(), kps.numpy()
    err = float(np.abs(y.astype(np.float64) - orc["maps"]).max())
    det = ref_k[..., 0] > -999
    both = held & det & (got_k[..., 0] > -999)
    perr = float(np.abs(got_k - ref_k)[both].max(initial=0.0))
    print("fp16 structured %s: E %.3g, P %.3g px, device error %.3g, keypoint error %.3g px, %d of %d maps left out, %d held detections"
          % (case, E, P, err, perr, int((~held).sum()), held.size, int((held & det).sum())))
    assert int((~held).sum()) <= 2, (case, int((~held).sum()))
    assert err <= 3 * E, (case, err, E)
    assert err > 1e-4, (case, err)
    assert np.array_equal((got_k[..., 0] > -999)[held], det[held]), "a held detection / rejection decision differs from the golden"
    assert perr <= max(3 * P, 1e-3), (case, perr, P)
    rej = held & ~det
    assert np.array_equal(got_k[rej], ref_k[rej])              # the -999.999 sentinels, bit for bit
    return err, perr


def check_golden_f16(dev, name, shape):
    """Golden inference case of a shipped architecture / hourglass variant with precision="fp16": maps within 3 E, E measured on
    the reference for this very input."""
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
        maps, kps = net.inference(pc.to(dev, x))
    y = maps.cpu().numpy()
    err = float(np.abs(compare(y).astype(np.float64) - golden).max())
    print("fp16 golden %s %s: E %.3g, device error %.3g (max|golden| %.3g)" % (name, tag, E, err, float(np.abs(golden).max())))
    assert err <= 3 * E, (name, tag, err, E)
    # the peak stage itself is bit-exact on the maps the fp16 CNN produced
    off = op.upsampling_offset(*net.trained_net_output_resolution())
    assert np.array_equal(kps.numpy(), op.keypoints_from_belief_maps(y, off))
    return err
