"""Checks of ResnetSimple.inference_conv_ksplit="auto" (the half-stored evaluation walk with the contraction of a small-grid launch
divided over workgroups), shared by the emulator and the GPU suite.

The plain convs run fp16_ksplit_checks' kernels (proved there); here only the rule ResnetSimple asks is checked.  New device code is
the split 4x4 transposed conv: four ksplit-form launches and convT4_f16_ksplit_finish_kernel.  Per launch nothing is measured:
(a) against the fp64 conv_transpose2d(k4, s2, p1) of the same half input and q(w), plus bias, the bound fp16_storage_checks holds:
    |got - ref| <= 5e-6 max|ref| + 2^-11 |ref| + 2^-25;
(b) the finishing pass against its own input: the test hands over a NaN-filled workspace; afterwards every element of all 4 S slices
is finite, and the stored halfs are sat_half of the same fp32 operations done here over those slices (slices added in the order
0 .. S-1, v * (2^-ew * scale) + shift, ReLU), bit for bit, the peak within 1e-6 relative of their max|.|;
(c) one slice IS conv_transpose4x4s2_f16_act16, bit for bit, and leaves the workspace NaN; two runs of any S are bit-equal.

One Bottleneck through the walk is held to fp16_resnet_storage_checks.block_oracle's carried bound, end to end to stored_oracle(),
both unchanged: the split moves a value by fp32 round-off before the one rounding those oracles model."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import cases
import fp16_checks as fc
import fp16_ksplit_checks as kc
import fp16_resnet_storage_checks as rs
import fp16_storage_checks as sc
import parity_checks as pc
from dream_amd import _hip, models, ops
from oracle import topology

HALF_MAX = sc.HALF_MAX
SPLIT_CONV = kc.SPLIT_ENTRY
SPLIT_CONVT = "dream_conv_transpose4x4s2_f16_ksplit_nhwc_f16"
SPLIT_ENTRIES = (SPLIT_CONV, SPLIT_CONVT)
# B, H, W, Cin, Cout: tile edges + odd W + 12 stages that do not divide by 5 + Cout no multiple of 32 / two frames of the layer4 map /
# 64 stages, the deep case
CONVT_CASES = [(1, 7, 9, 96, 40), (2, 13, 13, 64, 64), (1, 4, 5, 512, 32)]
REFUSED_CONVT_FLAGS = (ops.CONV_UPSAMPLE2X, ops.CONV_ZEROSTUFF2X, ops.CONV_OUT_NCHW, ops.CONV_POOL2)
forced_ksplit = kc.forced_ksplit

# (shape -> S) of dream_conv2d_f16_ksplit, the hourglass's rule, recorded from the commit before ResnetSimple's table existed:
# (B, H, W, Cin, Cout, ksize, flags) -> S
HOURGLASS_RULE = [((1, 25, 25, 512, 512, 3, 1), 6), ((1, 50, 50, 512, 512, 3, 1), 4), ((1, 50, 50, 256, 256, 3, 1), 3),
                  ((1, 100, 100, 256, 256, 3, 1), 1), ((1, 100, 100, 128, 128, 3, 1), 1), ((4, 25, 25, 512, 512, 3, 1), 4),
                  ((8, 25, 25, 512, 512, 3, 1), 2), ((1, 400, 400, 64, 64, 3, 1), 1), ((1, 25, 25, 512, 512, 3, 3), 1),
                  ((2, 13, 13, 32, 34, 1, 1), 1), ((1, 16, 16, 512, 64, 3, 1), 6), ((1, 7, 9, 96, 40, 3, 0), 1),
                  ((16, 50, 50, 512, 512, 3, 1), 1), ((2, 50, 50, 512, 256, 3, 1), 4)]


def stages(cin):
    return cin // 32 * 4


def check_convT(dev, B, H, W, Cin, Cout, S, flags=ops.CONV_RELU, x_scale=1.0, w_scale=None, seed=0, saturate=False):
    """One 4x4 transposed conv with S slices per phase forced (S > the stages of a phase: as many slices as stages)."""
    g = torch.Generator().manual_seed(seed)
    x16 = sc.half_input((B, Cin, H, W), x_scale, g)
    wT = torch.randn(Cin, Cout, 4, 4, generator=g) * ((2.0 / (4 * Cin)) ** 0.5 if w_scale is None else w_scale)
    scale = torch.rand(Cout, generator=g) + 0.5
    bias = torch.randn(Cout, generator=g) * x_scale
    p16 = ops.pack_convT4x4_weight_f16(pc.to(dev, wT))
    xd, sd, bd = pc.to(dev, pc._nhwc(x16)), pc.to(dev, scale), pc.to(dev, bias)
    what = ("convT4 ksplit", B, H, W, Cin, Cout, S, flags)
    want_s = min(S, stages(Cin))
    slice_ = B * H * W * Cout
    assert slice_ % 8 == 0
    with forced_ksplit(S):
        assert ops.conv_transpose4x4s2_f16_ksplit(B, H, W, Cin, Cout) == want_s, what
        assert ops.conv_transpose4x4s2_f16_ksplit(B, H, W, Cin, Cout + 2) == 1, what          # (Cout % 8 != 0: never split)
        nbytes = int(_hip.lib().dream_conv_transpose4x4s2_f16_ksplit_workspace(B, H, W, Cout, want_s))
        assert nbytes == 4 * want_s * slice_ * 4, what
        ws = pc.to(dev, torch.full((nbytes // 4,), float("nan")))
        peak = ops.new_amax(xd.device)
        y = ops.conv_transpose4x4s2_f16_act16_ksplit(xd, p16, Cout, sd, bd, flags, peak=peak, workspace=ws)
        peak2 = ops.new_amax(xd.device)
        y2 = ops.conv_transpose4x4s2_f16_act16_ksplit(xd, p16, Cout, sd, bd, flags, peak=peak2)     # (its own torch.empty workspace)
    assert y.dtype == torch.float16 and tuple(y.shape) == (B, 2 * H, 2 * W, Cout), what
    assert torch.equal(sc.bits(y), sc.bits(y2)) and fc._amax_value(peak) == fc._amax_value(peak2), what
    assert bool(torch.isfinite(y).all()), what
    if want_s == 1:
        peak1 = ops.new_amax(xd.device)
        y1 = ops.conv_transpose4x4s2_f16_act16(xd, p16, Cout, sd, bd, flags, peak=peak1)
        assert torch.equal(sc.bits(y), sc.bits(y1)) and fc._amax_value(peak) == fc._amax_value(peak1), what
        assert bool(torch.isnan(ws).all()), what                                                    # (the workspace is not touched)
    else:
        # the finishing pass on its own input: per phase the slices added in order, then v * (2^-ew * scale) + shift, ReLU -- fp32,
        # one rounding per operation --, phase 2a + b landing on the output pixels (2y + a, 2x + b)
        part = ws.cpu().view(4, want_s, B, H, W, Cout)
        assert bool(torch.isfinite(part).all()), (what, "a slice left part of its tile unwritten")
        inv = torch.tensor(2.0 ** -int(p16[2].cpu().view(-1)[0]), dtype=torch.float32)
        v = torch.empty((B, 2 * H, 2 * W, Cout), dtype=torch.float32)
        for ph in range(4):
            total = part[ph, 0].clone()
            for s in range(1, want_s):
                total = total + part[ph, s]
            v[:, ph >> 1::2, ph & 1::2] = total * (inv * scale).view(1, 1, 1, Cout) + bias.view(1, 1, 1, Cout)
        if flags & ops.CONV_RELU:
            v = v.relu()
        assert torch.equal(sc.bits(y.cpu()), sc.bits(sc.sat_half(v))), what
        top = float(v.abs().max())
        assert abs(fc._amax_value(peak) - top) <= 1e-6 * top, (what, fc._amax_value(peak), top)
    if saturate:
        assert fc._amax_value(peak) > HALF_MAX and float(y.float().abs().max()) == HALF_MAX, what
    ref = F.conv_transpose2d(x16.double(), fc.q(wT).double(), None, stride=2, padding=1) * scale.double().view(1, -1, 1, 1) \
        + bias.double().view(1, -1, 1, 1)
    if flags & ops.CONV_RELU:
        ref = ref.relu()
    sc._hold(y.cpu().permute(0, 3, 1, 2), ref, what)


def check_convT_case(dev, case, relu):
    """Forced S in {1, 2, 3, 5, all stages} and 1000 (clamped to the stages), with or without the ReLU."""
    B, H, W, Cin, Cout = case
    for S in (1, 2, 3, 5, stages(Cin), 1000):
        check_convT(dev, B, H, W, Cin, Cout, S, flags=ops.CONV_RELU if relu else 0, seed=S % 7)


def check_convT_tile(dev, variant):
    """Every tile of the fp16 variant table, forced, on the smallest case in two slices."""
    assert _hip.lib().dream_conv_f16_set_variant(variant) == 0
    try:
        check_convT(dev, *CONVT_CASES[0], 2, seed=variant)
    finally:
        _hip.lib().dream_conv_f16_set_variant(-1)


def check_convT_saturation(dev):
    """An input scaled so that the sum passes 65504: a finite 65504 is stored, the peak holds the unsaturated maximum."""
    check_convT(dev, *CONVT_CASES[0], 2, x_scale=100.0, w_scale=30.0, saturate=True)
    check_convT(dev, *CONVT_CASES[1], 3, flags=0, x_scale=100.0, w_scale=30.0, saturate=True, seed=1)


def _raw_convT(dev, xd, p16, bd, y, ws, S, B, H, W, Cin, Cout, flags, ws_offset=0):
    hi, _, exp, _ = p16
    ops.call(SPLIT_CONVT, ops.ptr(xd), ops.ptr(hi), ops.ptr(exp), None, ops.ptr(bd), ops.ptr(y), None,
             ops.ptr(ws) + ws_offset if ws_offset else ops.ptr(ws), S, B, H, W, Cin, Cout, int(hi.shape[-2]), flags, ops.stream())


def check_convT_refusals(dev):
    """Cout = 34 in two slices, the flags the unsplit entry refuses, a misaligned workspace: a nonzero status (ops.call raises) and
    an untouched output."""
    g = torch.Generator().manual_seed(3)
    B, H, W, Cin = 1, 7, 9, 96
    for Cout, flags, off, why in [(34, ops.CONV_RELU, 0, "multiple of 8")] \
            + [(40, ops.CONV_RELU | f, 0, "unsupported flags") for f in REFUSED_CONVT_FLAGS] + [(40, ops.CONV_RELU, 4, "16-byte aligned")]:
        wT = torch.randn(Cin, Cout, 4, 4, generator=g) * 0.1
        p16 = ops.pack_convT4x4_weight_f16(pc.to(dev, wT))
        xd = pc.to(dev, pc._nhwc(sc.half_input((B, Cin, H, W), 1.0, g)))
        bd = pc.to(dev, torch.randn(Cout, generator=g))
        with forced_ksplit(2):
            assert ops.conv_transpose4x4s2_f16_ksplit(B, H, W, Cin, Cout) == (2 if Cout % 8 == 0 else 1)
        ws = pc.to(dev, torch.full((4 * 2 * (B * H * W * Cout + 8) + 8,), float("nan")))
        y = pc.to(dev, torch.full((B, 2 * H, 2 * W, Cout), 7.0, dtype=torch.float16))
        try:
            _raw_convT(dev, xd, p16, bd, y, ws, 2, B, H, W, Cin, Cout, flags, ws_offset=off)
        except RuntimeError as e:
            assert why in str(e), (why, e)
        else:
            raise AssertionError("S = 2 with Cout %d, flags %d, workspace offset %d was not refused" % (Cout, flags, off))
        assert bool((y == 7.0).all()) and bool(torch.isnan(ws).all()), (Cout, flags, off)


# ---- the rule ResnetSimple asks: a host computation -------------------------------------------------------------------------------
def covered_launches(net, shape, monkeypatch):
    """The launches of one half-stored evaluation walk on ``meta`` -> ([(entry, b, h, w, cin, cout, ksize | 0 for a stage, flags)] of
    the plain / split convs and transposed convs, every launch that is no weight pack)."""
    import launch_trace as lt
    rec = lt.Recorder()
    rec.install(monkeypatch, ops)
    b, h, w = shape
    net.run_forward(torch.empty((b, 3, h, w), device="meta"))
    out = []
    for l in rec.launches:
        name, *args = l.split(" ")
        a = [int(v) for v in args if v.lstrip("-").isdigit()]
        if name in ("dream_conv2d_f16_nhwc_f16", SPLIT_CONV):
            a = a[-9:]                                     # b h w cin cout coutpad ksize stride flags (the split entry: S in front)
            out.append((name, a[0], a[1], a[2], a[3], a[4], a[6], a[8]))
        elif name in ("dream_conv_transpose4x4s2_f16_nhwc_f16", SPLIT_CONVT):
            a = a[-7:]                                     # b h w cin cout coutpad flags
            out.append((name, a[0], a[1], a[2], a[3], a[4], 0, a[6]))
    return out, [l for l in rec.launches if not lt.is_pack(l)]


def rule(b, h, w, cin, cout, k, flags=ops.CONV_RELU):
    """S of a covered launch: k = 0 is a decoder stage."""
    return ops.conv_transpose4x4s2_f16_ksplit(b, h, w, cin, cout) if k == 0 else ops.conv2d_f16_ksplit_resnet(b, h, w, cin, cout, k, flags)


def check_rule_properties(shapes):
    """On every covered shape (h, w, cin, cout, k): non-increasing in B for B in 1 .. 128, never more than the stages, 1 under each
    refused flag, the forced value under the hook."""
    for (h, w, cin, cout, k) in shapes:
        nst = cin // 32 * (4 if k == 0 else k * k)
        last = None
        for b in range(1, 129):
            s = rule(b, h, w, cin, cout, k)
            assert 1 <= s <= nst and (last is None or s <= last), (h, w, cin, cout, k, b, s, last)
            last = s
        for n in (1, 2, 5, 1000):
            with forced_ksplit(n):
                assert rule(1, h, w, cin, cout, k) == min(n, nst), (h, w, cin, cout, k, n)
                if k:
                    for f in kc.REFUSED_FLAGS:
                        assert rule(1, h, w, cin, cout, k, ops.CONV_RELU | f) == 1, (h, w, cin, cout, k, f)
        if k:
            for f in kc.REFUSED_FLAGS:
                assert rule(1, h, w, cin, cout, k, ops.CONV_RELU | f) == 1, (h, w, cin, cout, k, f)


# ---- one Bottleneck and one decoder stage through the walk ---------------------------------------------------------------------------
def check_bottleneck(dev, seed=0):
    """rs.check_bottleneck's block through _bottleneck on _EvalAct16(net, peak, ksplit=True) with two slices forced: its own carried bound."""
    g = torch.Generator().manual_seed(seed)
    net = rs._host(dev)
    ds = nn.Sequential(nn.Conv2d(64, 128, 1, stride=2, bias=False), nn.BatchNorm2d(128))
    blk = topology.Bottleneck(64, 32, 2, ds).eval()
    for mod in blk.modules():
        if isinstance(mod, nn.Conv2d):
            with torch.no_grad():
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (2.0 / (mod.weight[0].numel())) ** 0.5)
        elif isinstance(mod, nn.BatchNorm2d):
            rs._random_bn(mod, g)
    blk = blk.to(dev)
    x16 = sc.half_input((2, 64, 9, 12), 1.0, g, outlier=8.0)
    name = "check.ksplit.block.%d" % seed
    peak = ops.new_amax(blk.conv1.weight.device)
    with torch.no_grad(), forced_ksplit(2), kc.launch_names() as names:
        y16 = net._bottleneck(models._EvalAct16(net, peak, ksplit=True), name, blk, pc.to(dev, pc._nhwc(x16)))
    with torch.no_grad():
        ref, bound = rs.block_oracle(net, name, blk, x16)
    # the downsample conv, conv1 and conv2 (its patch rows) are split; conv3 carries the residual and is the launch it was
    assert names.count(SPLIT_CONV) == 3 and names.count("dream_conv2d_f16_res16_nhwc_f16") == 1, names
    assert y16.dtype == torch.float16 and tuple(y16.shape) == (2, 5, 6, 128)
    got = y16.cpu().permute(0, 3, 1, 2).double()
    worst = float(((got - ref).abs() / bound).max())
    print("fp16 resnet ksplit Bottleneck: worst error %.3g of the carried bound, peak %.4g" % (worst, fc._amax_value(peak)))
    assert worst <= 1.0, worst
    assert float(ref.abs().max()) > 0 and float((ref > 0).double().mean()) > 0.2
    assert 0.0 < fc._amax_value(peak) < HALF_MAX


def check_stage(dev, seed=0):
    """One decoder stage (ConvTranspose2d(k4,s2,p1) -> BatchNorm -> ReLU) through _EvalAct16.stage with two slices forced, against its
    fp64 restatement: bound (a)."""
    g = torch.Generator().manual_seed(seed)
    net = rs._host(dev)
    B, H, W, Cin, Cout = 2, 5, 6, 64, 40
    m = nn.ConvTranspose2d(Cin, Cout, 4, 2, 1, 0)
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / (4 * Cin)) ** 0.5)
        m.bias.copy_(torch.randn(Cout, generator=g) * 0.2)
    bn = rs._random_bn(nn.BatchNorm2d(Cout), g)
    m, bn = m.to(dev), bn.to(dev)
    x16 = sc.half_input((B, Cin, H, W), 1.0, g)
    name = "check.ksplit.stage.%d" % seed
    peak = ops.new_amax(m.weight.device)
    with torch.no_grad(), forced_ksplit(2), kc.launch_names() as names:
        y16 = models._EvalAct16(net, peak, ksplit=True).stage(name, m, bn, pc.to(dev, pc._nhwc(x16)))
    with torch.no_grad():
        scale, shift = net._fold(name, bn, m.bias)
    scale, shift = scale.cpu().double().view(1, -1, 1, 1), shift.cpu().double().view(1, -1, 1, 1)
    assert names.count(SPLIT_CONVT) == 1, names
    ref = (F.conv_transpose2d(x16.double(), fc.q(m.weight.detach().cpu()).double(), None, stride=2, padding=1) * scale + shift).relu()
    assert y16.dtype == torch.float16 and tuple(y16.shape) == (B, 2 * H, 2 * W, Cout)
    sc._hold(y16.cpu().permute(0, 3, 1, 2), ref, ("ksplit stage", B, H, W, Cin, Cout))
    assert float((ref > 0).double().mean()) > 0.2 and 0.0 < fc._amax_value(peak) < HALF_MAX


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def ksplit_network(dev, case, ksplit="auto"):
    net = rs.structured_network(dev, case)
    net.model.module.inference_conv_ksplit = ksplit
    return net


def check_structured(dev, case):
    """rs.check_structured with inference_conv_ksplit="auto", held to rs.stored_oracle in the same way -- and at least one launch of the
    walk really was a split one.  Prints (does not assert) the distance to the "off" maps."""
    orc = rs.stored_oracle(case)
    E, P, held, ref_k = orc["E"], orc["P"], orc["held"], orc["ref_k"]
    x = pc.to(dev, torch.from_numpy(cases.structured_input(case)[0]))
    net = ksplit_network(dev, case)
    with torch.no_grad(), kc.launch_names() as names:
        maps, kps = net.inference(x)
    nsplit = {e: names.count(e) for e in SPLIT_ENTRIES}
    with torch.no_grad():
        maps_off = ksplit_network(dev, case, "off").inference(x)[0]
    assert maps.dtype == torch.float32
    peak = net.model.module.half_storage_peak()
    y, got_k = maps.cpu().numpy(), kps.numpy()
    err = float(np.abs(y.astype(np.float64) - orc["maps"]).max())
    det = ref_k[..., 0] > -999
    both = held & det & (got_k[..., 0] > -999)
    perr = float(np.abs(got_k - ref_k)[both].max(initial=0.0))
    print("fp16 resnet ksplit structured %s: E %.3g, P %.3g px, device error %.3g, keypoint error %.3g px, %d of %d maps left out, split "
          "launches %s, max|maps(auto) - maps(off)| %.3g, stored peak %.4g"
          % (case, E, P, err, perr, int((~held).sum()), held.size, nsplit, float((maps - maps_off).abs().max()), peak))
    assert sum(nsplit.values()) >= 1, (case, "no launch of this walk was split: the test shows nothing")
    assert 0.0 < peak < HALF_MAX, (case, peak)
    assert int((~held).sum()) <= 2, (case, int((~held).sum()))
    assert err <= 3 * E, (case, err, E)
    assert err > 1e-4, (case, err)
    assert np.array_equal((got_k[..., 0] > -999)[held], det[held]), "a held detection / rejection decision differs from the golden"
    assert perr <= max(3 * P, 1e-3), (case, perr, P)
    rej = held & ~det
    assert np.array_equal(got_k[rej], ref_k[rej])
    return err, perr
