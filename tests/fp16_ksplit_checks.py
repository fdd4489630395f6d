"""Checks of conv_ksplit="auto" (precision="fp16" with activation_storage="fp16": the contraction of a small-grid conv divided over
workgroups; csrc/conv_f16.hip KSPLIT), shared by the emulator and the GPU suite.

Per launch nothing is measured.  (1) Against the fp64 conv of the same half operands x16 and q(w), elementwise, the bound that
fp16_storage_checks holds:  |got - ref| <= 5e-6 max|ref| + 2^-11 |ref| + 2^-25  -- fp32 accumulation (the slices change only the
order of the fp32 additions), half a half-ulp of the stored value, the half subnormal floor.  (2) The finishing pass against its own
input: the test hands over the workspace, filled with NaN, and afterwards adds its S slices in the order 0 .. S-1 in fp32 and applies
v * 2^-ew + bias, ReLU itself -- the same IEEE operations --: the stored halfs must be fp16(clamp(that)) bit for bit (so a slice that
skipped part of its tile shows as NaN) and the peak scalar its max|.| within 1e-6 relative.  (3) One slice IS conv2d_f16_act16, bit
for bit; two runs of any S are bit-equal.

End to end the bound is the half-storage oracle's (fp16_storage_checks.rounded_storage_oracle, unchanged): the split moves a value
by fp32 round-off before the one rounding to half that the oracle already models."""
import numpy as np
import torch
import torch.nn.functional as F

import cases
import fp16_checks as fc
import fp16_storage_checks as sc
import parity_checks as pc
from dream_amd import _hip, ops

HALF_MAX = sc.HALF_MAX
SPLIT_ENTRY = "dream_conv2d_f16_ksplit_nhwc_f16"
# B, H, W, Cin, Cout: tile edges + uneven slices (3 chunks over 2) + Cout no multiple of 32 / the 64-pixel tile / one chunk (S = 3
# leaves nothing to the third slice of a 1x1 conv) / the deepest contraction (144 stages)
LAUNCH_CASES = [(1, 7, 9, 96, 40), (1, 25, 25, 64, 64), (2, 13, 13, 32, 34), (1, 16, 16, 512, 64)]
REFUSED_FLAGS = (ops.CONV_POOL2, ops.CONV_UPSAMPLE2X, ops.CONV_OUT_NCHW)


class forced_ksplit:
    """dream_conv_f16_set_ksplit(n) for the block (the library the ops module calls: the emulator's under emulated_hip())."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        assert _hip.lib().dream_conv_f16_set_ksplit(self.n) == 0

    def __exit__(self, *exc):
        _hip.lib().dream_conv_f16_set_ksplit(-1)


def stages(cin, k):
    return cin // 32 * k * k


def check_conv(dev, B, H, W, Cin, Cout, k, S, flags=ops.CONV_RELU, x_scale=1.0, w_scale=0.1, seed=0, saturate=False):
    """One launch with S slices forced (S > the stages of the launch: as many slices as stages)."""
    g = torch.Generator().manual_seed(seed)
    x16 = sc.half_input((B, Cin, H, W), x_scale, g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * w_scale
    bias = torch.randn(Cout, generator=g) * x_scale * w_scale
    p16 = ops.pack_conv_weight_f16(pc.to(dev, w), 0)
    xd, bd = pc.to(dev, pc._nhwc(x16)), pc.to(dev, bias)
    what = (B, H, W, Cin, Cout, k, S, flags)
    want_s = min(S, stages(Cin, k))
    n = B * H * W * Cout
    slice_ = (n + 7) // 8 * 8
    with forced_ksplit(S):
        assert ops.conv2d_f16_ksplit(B, H, W, Cin, Cout, k, flags) == want_s, what
        for f in REFUSED_FLAGS:
            assert ops.conv2d_f16_ksplit(B, H, W, Cin, Cout, k, flags | f) == 1, (what, f)
        nbytes = int(_hip.lib().dream_conv2d_f16_ksplit_workspace(B, H, W, Cout, want_s))
        assert nbytes == want_s * slice_ * 4, what
        ws = pc.to(dev, torch.full((nbytes // 4,), float("nan")))
        peak = ops.new_amax(xd.device)
        y = ops.conv2d_f16_act16_ksplit(xd, p16, Cout, k, None, bd, flags, peak=peak, workspace=ws)
        peak2 = ops.new_amax(xd.device)
        y2 = ops.conv2d_f16_act16_ksplit(xd, p16, Cout, k, None, bd, flags, peak=peak2)        # (its own torch.empty workspace)
    assert y.dtype == torch.float16 and tuple(y.shape) == (B, H, W, Cout), what
    assert torch.equal(sc.bits(y), sc.bits(y2)) and fc._amax_value(peak) == fc._amax_value(peak2), what
    assert bool(torch.isfinite(y).all()), what
    if want_s == 1:
        peak1 = ops.new_amax(xd.device)
        y1 = ops.conv2d_f16_act16(xd, p16, Cout, k, None, bd, flags, peak=peak1)
        assert torch.equal(sc.bits(y), sc.bits(y1)) and fc._amax_value(peak) == fc._amax_value(peak1), what
        assert bool(torch.isnan(ws).all()), what                                               # (the workspace is not touched)
    else:
        # the finishing pass on its own input: slices added in order, then v * 2^-ew + bias, ReLU -- fp32, one rounding per operation
        part = ws.cpu()[:want_s * slice_].view(want_s, slice_)[:, :n]
        assert bool(torch.isfinite(part).all()), (what, "a slice left part of its tile unwritten")
        total = part[0].clone()
        for s in range(1, want_s):
            total = total + part[s]
        inv = torch.tensor(2.0 ** -int(p16[2].cpu().view(-1)[0]), dtype=torch.float32)
        v = total.view(B, H, W, Cout) * (inv * torch.tensor(1.0)) + bias.view(1, 1, 1, Cout)
        if flags & ops.CONV_RELU:
            v = v.relu()
        assert torch.equal(sc.bits(y.cpu()), sc.bits(sc.sat_half(v))), what
        top = float(v.abs().max())
        assert abs(fc._amax_value(peak) - top) <= 1e-6 * top, (what, fc._amax_value(peak), top)
    if saturate:
        assert fc._amax_value(peak) >= HALF_MAX and float(y.float().abs().max()) == HALF_MAX, what
    ref = F.conv2d(x16.double(), fc.q(w).double(), bias.double(), padding=k // 2)
    if flags & ops.CONV_RELU:
        ref = ref.relu()
    sc._hold(y.cpu().permute(0, 3, 1, 2), ref, ("ksplit",) + what)


def check_case(dev, case, k):
    """Forced S in {1, 2, 3, max} on one shape."""
    B, H, W, Cin, Cout = case
    for S in (1, 2, 3, stages(Cin, k)):
        check_conv(dev, B, H, W, Cin, Cout, k, S, seed=S)
    check_conv(dev, B, H, W, Cin, Cout, k, 2, flags=0, seed=5)                                   # (no ReLU: both signs)
    if Cin <= 96:
        check_conv(dev, B, H, W, Cin, Cout, k, 1000, seed=6)                                     # (clamped to the stages)


def check_tile(dev, variant):
    """The split kernel of tile ``variant`` of the fp16 variant table, forced, on the smallest launch case: 3x3 in two uneven slices,
    1x1 in as many slices as stages."""
    assert _hip.lib().dream_conv_f16_set_variant(variant) == 0
    try:
        check_conv(dev, *LAUNCH_CASES[0], 3, 2, seed=variant)
        check_conv(dev, *LAUNCH_CASES[0], 1, 3, seed=variant)
    finally:
        _hip.lib().dream_conv_f16_set_variant(-1)


def check_saturation(dev, case, k):
    B, H, W, Cin, Cout = case
    check_conv(dev, B, H, W, Cin, Cout, k, 2, x_scale=100.0, w_scale=30.0, saturate=True)
    check_conv(dev, B, H, W, Cin, Cout, k, 3, flags=0, x_scale=100.0, w_scale=30.0, saturate=True, seed=1)


def check_refused_flags(dev, case):
    """A launch with a fused pool / upsample / the NCHW output is never split: on the case's shape (3x3; the upsample form on the stored
    input of half the size) the wrapper runs conv2d_f16_act16, bit for bit, whatever S is forced, and the entry point itself refuses
    S > 1 with such a flag."""
    g = torch.Generator().manual_seed(9)
    B, H, W, Cin, Cout = case
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1
    bd = pc.to(dev, torch.randn(Cout, generator=g) * 0.1)
    p16 = ops.pack_conv_weight_f16(pc.to(dev, w), 0)
    hi, _, exp, _ = p16
    for f in REFUSED_FLAGS:
        ups = f == ops.CONV_UPSAMPLE2X
        hs, wd = (H // 2, W // 2) if ups else (H, W)                      # stored input
        ho, wo = (2 * hs, 2 * wd) if ups else (H, W)                      # the grid the launch is given
        xd = pc.to(dev, pc._nhwc(sc.half_input((B, Cin, hs, wd), 1.0, g)))
        with forced_ksplit(2):
            y = ops.conv2d_f16_act16_ksplit(xd, p16, Cout, 3, None, bd, ops.CONV_RELU | f)
        y1 = ops.conv2d_f16_act16(xd, p16, Cout, 3, None, bd, ops.CONV_RELU | f)
        assert y.dtype == y1.dtype and y.shape == y1.shape and torch.equal(y.view(torch.int16), y1.view(torch.int16)), (case, f)
        ws = pc.to(dev, torch.zeros(2 * (B * ho * wo * Cout + 8)))
        out = pc.to(dev, torch.zeros((B, ho, wo, Cout), dtype=torch.float16))
        try:
            ops.call(SPLIT_ENTRY, ops.ptr(xd), ops.ptr(hi), ops.ptr(exp), None, ops.ptr(bd), ops.ptr(out), None, ops.ptr(ws), 2,
                     B, ho, wo, Cin, Cout, int(hi.shape[-2]), 3, 1, ops.CONV_RELU | f, ops.stream())
        except RuntimeError as e:
            assert "not split" in str(e), e
        else:
            raise AssertionError("S = 2 with flag %d was not refused" % f)


def check_empty_slices(dev, case, k, extra=2):
    """The entry point itself with more slices than the launch has stages (the rule and the hook never ask for that: they clamp): the
    slices past the stages hold zeros -- written, the workspace starts as NaN -- and the result is the unsplit launch's, bit for bit
    (x + 0 is x, and the finishing pass applies the unsplit epilogue's expression)."""
    B, H, W, Cin, Cout = case
    g = torch.Generator().manual_seed(11)
    x16 = sc.half_input((B, Cin, H, W), 1.0, g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.1
    bd = pc.to(dev, torch.randn(Cout, generator=g) * 0.1)
    p16 = ops.pack_conv_weight_f16(pc.to(dev, w), 0)
    hi, _, exp, _ = p16
    xd = pc.to(dev, pc._nhwc(x16))
    full = stages(Cin, k)
    S = full + extra
    n = B * H * W * Cout
    slice_ = (n + 7) // 8 * 8
    assert int(_hip.lib().dream_conv2d_f16_ksplit_workspace(B, H, W, Cout, S)) == S * slice_ * 4
    ws = pc.to(dev, torch.full((S * slice_,), float("nan")))
    y = pc.to(dev, torch.zeros((B, H, W, Cout), dtype=torch.float16))
    peak, peak1 = ops.new_amax(xd.device), ops.new_amax(xd.device)
    ops.call(SPLIT_ENTRY, ops.ptr(xd), ops.ptr(hi), ops.ptr(exp), None, ops.ptr(bd), ops.ptr(y), ops.ptr(peak), ops.ptr(ws), S,
             B, H, W, Cin, Cout, int(hi.shape[-2]), k, 1, ops.CONV_RELU, ops.stream())
    part = ws.cpu().view(S, slice_)[:, :n]
    assert bool(torch.isfinite(part).all()), (case, k, "a slice left part of its tile unwritten")
    assert bool((part[full:] == 0).all()) and bool((part[:full] != 0).any()), (case, k)
    y1 = ops.conv2d_f16_act16(xd, p16, Cout, k, None, bd, ops.CONV_RELU, peak=peak1)
    if full == 1:
        assert torch.equal(sc.bits(y), sc.bits(y1)) and fc._amax_value(peak) == fc._amax_value(peak1), (case, k)
    ref = F.conv2d(x16.double(), fc.q(w).double(), bd.cpu().double(), padding=k // 2).relu()
    sc._hold(y.cpu().permute(0, 3, 1, 2), ref, ("ksplit, empty slices",) + tuple(case) + (k, S))


# ---- the rule: a host computation -----------------------------------------------------------------------------------------------
def check_rule_monotone(shapes):
    """S never grows with the batch."""
    for (h, w, cin, cout, k) in shapes:
        last = None
        for b in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 64, 128):
            s = ops.conv2d_f16_ksplit(b, h, w, cin, cout, k, ops.CONV_RELU)
            assert s >= 1 and (last is None or s <= last), (h, w, cin, cout, k, b, s, last)
            last = s


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def ksplit_network(dev, case, ksplit="auto"):
    net = sc.structured_network(dev, case)
    net.model.module.conv_ksplit = ksplit
    return net


class launch_names:
    """Names of the entry points ops.call reaches inside the block, in order (the calls go through)."""

    def __enter__(self):
        self.names, self._call = [], ops.call

        def spy(name, *args):
            self.names.append(name)
            return self._call(name, *args)
        ops.call = spy
        return self.names

    def __exit__(self, *exc):
        ops.call = self._call


def check_structured(dev, case):
    """sc.check_structured with conv_ksplit="auto", held to the same half-storage oracle in the same way: maps within 3 E of the golden,
    held decisions the golden's, held keypoints within max(3 P, 1e-3 px), held sentinels bit for bit, at most 2 maps left out -- and at
    least one launch of the walk really was a split one."""
    orc = sc.rounded_storage_oracle(case)
    E, P, held, ref_k = orc["E"], orc["P"], orc["held"], orc["ref_k"]
    x = pc.to(dev, torch.from_numpy(cases.structured_input(case)[0]))
    net = ksplit_network(dev, case)
    with torch.no_grad(), launch_names() as names:
        maps, kps = net.inference(x)
    nsplit = names.count(SPLIT_ENTRY)
    with torch.no_grad():
        maps_off = ksplit_network(dev, case, "off").inference(x)[0]
    assert maps.dtype == torch.float32
    peak = net.model.module.half_storage_peak()
    y, got_k = maps.cpu().numpy(), kps.numpy()
    err = float(np.abs(y.astype(np.float64) - orc["maps"]).max())
    det = ref_k[..., 0] > -999
    both = held & det & (got_k[..., 0] > -999)
    perr = float(np.abs(got_k - ref_k)[both].max(initial=0.0))
    print("fp16 ksplit structured %s: E %.3g, P %.3g px, device error %.3g, keypoint error %.3g px, %d of %d maps left out, %d split "
          "launches, max|maps(auto) - maps(off)| %.3g, stored peak %.4g"
          % (case, E, P, err, perr, int((~held).sum()), held.size, nsplit, float((maps - maps_off).abs().max()), peak))
    assert nsplit >= 1, (case, "no launch of this walk was split: the test shows nothing")
    assert 0.0 < peak < HALF_MAX, (case, peak)
    assert int((~held).sum()) <= 2, (case, int((~held).sum()))
    assert err <= 3 * E, (case, err, E)
    assert err > 1e-4, (case, err)
    assert np.array_equal((got_k[..., 0] > -999)[held], det[held]), "a held detection / rejection decision differs from the golden"
    assert perr <= max(3 * P, 1e-3), (case, perr, P)
    rej = held & ~det
    assert np.array_equal(got_k[rej], ref_k[rej])
    return err, perr
