"""Checks of ResnetSimple.inference_head_fusion="on" (the last decoder stage and the 1x1 head as one entry point on half-stored
activations; csrc/conv_head_f16.hip), shared by the emulator and the GPU suite.

The contract is identity: element by element the fused entry runs the IEEE operations of dream_conv_transpose4x4s2_f16_nhwc_f16
followed by dream_conv2d_f16_nhwc_f16 (DREAM_CONV_OUT_NCHW), in their order, so the belief maps and the peak scalar are compared bit for
bit with that pair on the same inputs -- per launch, and through the walk against inference_head_fusion="off".  Independently of the
unfused kernels the maps are held against the fp64 1x1 conv of the halfs the stage stores and q(head weight), under the per-launch
bound of fp16_storage_checks:
    |got - ref| <= 5e-6 max|ref| + 2^-11 |ref| + 2^-25
(for an fp32 output only its first term is needed; the bound is kept as it stands), and the stored halfs themselves against the fp64
transposed conv, as fp16_resnet_ksplit_checks holds them.  End to end the "on" walk goes through fp16_resnet_storage_checks.check_structured
itself.  Equality alone would pass on a network that ignores the switch: every walk check also looks at the launches that ran."""
import contextlib

import torch
import torch.nn.functional as F

import cases
import fp16_checks as fc
import fp16_ksplit_checks as kc
import fp16_resnet_storage_checks as rs
import fp16_storage_checks as sc
import parity_checks as pc
from dream_amd import models, ops

HALF_MAX = sc.HALF_MAX
FUSED = "dream_conv_transpose4x4s2_head_f16_nhwc_f16"
STAGE = "dream_conv_transpose4x4s2_f16_nhwc_f16"
SPLIT_STAGE = "dream_conv_transpose4x4s2_f16_ksplit_nhwc_f16"
CONV = "dream_conv2d_f16_nhwc_f16"
CMID = 256
# B, H, W, Cin, K: one ragged tile, one chunk / two tiles per row or column with a ragged edge, two frames, two chunks / full KPad /
# degenerate
LAUNCH_CASES = [(1, 3, 5, 32, 7), (2, 13, 13, 64, 17), (1, 9, 17, 32, 32), (1, 1, 1, 32, 1)]
forced_ksplit = kc.forced_ksplit


def _bits32(t):
    return t.contiguous().view(torch.int32)


def _hold_maps(got, ref, what):
    """fp16_storage_checks._hold for the fp32 belief maps: the same elementwise bound, the reference not clamped to the half range (the
    maps are not stored as halfs: behind a saturated stage they pass 65504)."""
    bound = 5e-6 * float(ref.abs().max()) + 2.0 ** -11 * ref.abs() + 2.0 ** -25
    worst = float(((got.double() - ref).abs() / bound).max())
    print("fp16 storage %s: worst error %.3g of the bound" % (what, worst))
    assert worst <= 1.0, (what, worst)


def _operands(dev, B, H, W, Cin, K, x_scale, w_scale, seed, cmid=CMID):
    g = torch.Generator().manual_seed(seed)
    x16 = sc.half_input((B, Cin, H, W), x_scale, g)
    wT = torch.randn(Cin, cmid, 4, 4, generator=g) * w_scale
    scale = torch.rand(cmid, generator=g) + 0.5
    shift = torch.randn(cmid, generator=g) * 4.0 * x_scale * w_scale            # (against sums of ~4 sqrt(Cin) x w: both signs in front of the ReLU)
    hw = torch.randn(K, cmid, 1, 1, generator=g)
    hb = torch.randn(K, generator=g) * 3.0
    host = dict(x16=x16, wT=wT, scale=scale, shift=shift, hw=hw, hb=hb)
    device = dict(x=pc.to(dev, pc._nhwc(x16)), p16=ops.pack_convT4x4_weight_f16(pc.to(dev, wT)), scale=pc.to(dev, scale),
                  shift=pc.to(dev, shift), h16=ops.pack_conv_weight_f16(pc.to(dev, hw), 0), hb=pc.to(dev, hb))
    return host, device


def _pair(d, K, flags, cmid=CMID):
    """The two launches the fused entry stands for -> (stored halfs, maps, peak)."""
    peak = ops.new_amax(d["x"].device)
    y16 = ops.conv_transpose4x4s2_f16_act16(d["x"], d["p16"], cmid, d["scale"], d["shift"], flags, peak=peak)
    maps = ops.conv2d_f16_act16(y16, d["h16"], K, 1, None, d["hb"], ops.CONV_OUT_NCHW)
    return y16, maps, peak


def check_launch(dev, B, H, W, Cin, K, relu=True, x_scale=1.0, w_scale=1.0, seed=0, saturate=False):
    host, d = _operands(dev, B, H, W, Cin, K, x_scale, w_scale, seed)
    flags = ops.CONV_RELU if relu else 0
    what = ("fused head", B, H, W, Cin, K, flags)
    assert ops.conv_transpose4x4s2_head_f16_applies(Cin, CMID, K), what
    y16, want, want_peak = _pair(d, K, flags)
    peak = ops.new_amax(d["x"].device)
    with kc.launch_names() as names:
        got = ops.conv_transpose4x4s2_head_f16_act16(d["x"], d["p16"], CMID, d["scale"], d["shift"], d["h16"], K, d["hb"], flags, peak=peak)
    assert names == [FUSED], names
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, K, 2 * H, 2 * W), what
    ndiff = int((_bits32(got) != _bits32(want)).sum())
    print("fused head %s: %d of %d map elements differ from the two launches, peak %.6g against %.6g"
          % (what, ndiff, got.numel(), fc._amax_value(peak), fc._amax_value(want_peak)))
    assert ndiff == 0, (what, ndiff)
    assert fc._amax_value(peak) == fc._amax_value(want_peak), what
    assert bool(torch.isfinite(got).all()), what
    # the stage's stored halfs against the fp64 transposed conv, the maps against the fp64 1x1 conv of those halfs
    stage = F.conv_transpose2d(host["x16"].double(), fc.q(host["wT"]).double(), None, stride=2, padding=1) \
        * host["scale"].double().view(1, -1, 1, 1) + host["shift"].double().view(1, -1, 1, 1)
    if relu:
        neg = float((stage < 0).double().mean())
        assert 0.1 < neg < 0.9 or H * W == 1, (what, neg)                          # both signs in front of the ReLU
        stage = stage.relu()
    stored = y16.cpu().permute(0, 3, 1, 2)
    sc._hold(stored, stage, what + ("stage",))
    ref = F.conv2d(stored.double(), fc.q(host["hw"]).double(), host["hb"].double())
    _hold_maps(got.cpu(), ref, what + ("maps",))
    if saturate:
        assert fc._amax_value(peak) >= HALF_MAX and float(stored.float().abs().max()) == HALF_MAX, what
    else:
        assert 0.0 < fc._amax_value(peak) < HALF_MAX, what


def check_saturation(dev):
    """Inputs scaled so that the stage value passes 65504: finite maps, the peak holds the unsaturated maximum, both those of the pair."""
    check_launch(dev, 1, 3, 5, 32, 7, relu=True, x_scale=100.0, w_scale=30.0, seed=1, saturate=True)
    check_launch(dev, 2, 13, 13, 64, 17, relu=False, x_scale=100.0, w_scale=30.0, seed=2, saturate=True)


def _raw(d, maps, peak, B, H, W, Cin, cmid, K, flags, x_offset=0):
    hi, _, exp, _ = d["p16"]
    hhi, _, hexp, _ = d["h16"]
    ops.call(FUSED, ops.ptr(d["x"]) + x_offset if x_offset else ops.ptr(d["x"]), ops.ptr(hi), ops.ptr(exp), ops.ptr(d["scale"]),
             ops.ptr(d["shift"]), ops.ptr(hhi), ops.ptr(hexp), ops.ptr(d["hb"]), ops.ptr(maps), ops.ptr(peak), B, H, W, Cin, cmid,
             int(hi.shape[-2]), K, int(hhi.shape[-2]), flags, ops.stream())


def check_refusals(dev):
    """128 stage channels, 33 maps, 48 input channels, a pool flag, a misaligned x: the predicate says no (for the channel counts it is
    asked about), the entry returns a nonzero status (ops.call raises), and nothing was launched: maps and peak are untouched."""
    B, H, W = 1, 3, 5
    assert ops.conv_transpose4x4s2_head_f16_applies(64, CMID, 7) and ops.conv_transpose4x4s2_head_f16_applies(2048, CMID, 32)
    for Cin, cmid, K, flags, off, why in [(64, 128, 7, ops.CONV_RELU, 0, "Cmid=128"), (64, CMID, 33, ops.CONV_RELU, 0, "K=33"),
                                          (48, CMID, 7, ops.CONV_RELU, 0, "Cin=48"),
                                          (64, CMID, 7, ops.CONV_RELU | ops.CONV_POOL2, 0, "unsupported flags"),
                                          (64, CMID, 7, ops.CONV_RELU, 2, "16-byte aligned")]:
        shapes_ok = ops.conv_transpose4x4s2_head_f16_applies(Cin, cmid, K)
        assert shapes_ok == (why in ("unsupported flags", "16-byte aligned")), (Cin, cmid, K)
        host, d = _operands(dev, B, H, W + 1 if off else W, Cin, K, 1.0, 1.0, 3, cmid=cmid)        # (a row to spare behind the offset)
        maps = pc.to(dev, torch.full((B, K, 2 * H, 2 * W), 7.0))
        peak = ops.new_amax(d["x"].device)
        try:
            _raw(d, maps, peak, B, H, W, Cin, cmid, K, flags, x_offset=off)
        except RuntimeError as e:
            assert why in str(e), (why, e)
        else:
            raise AssertionError("Cin %d, Cmid %d, K %d, flags %d, x offset %d was not refused" % (Cin, cmid, K, flags, off))
        assert bool((maps == 7.0).all()) and fc._amax_value(peak) == 0.0, (Cin, cmid, K, flags, off)


# ---- the decoder through the walk's own step (the emulator's walk: ResNet-101's trunk takes minutes there) ------------------------------
def _decoder_net(dev, k, full, seed):
    g = torch.Generator().manual_seed(seed)
    net = models.ResnetSimple(k, pretrained=False, full=full).eval()
    for name, m, bn in net._decoder():
        with torch.no_grad():
            if bn is not None:
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / (4 * int(m.weight.shape[0]))) ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                rs._random_bn(bn, g)
            else:
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 0.1)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g))
    return net.to(dev), g


def run_decoder(net, y16, fuse_head, ksplit=False):
    """-> (maps, peak value, entry-point names) of ResnetSimple._run_decoder on the half-stored arithmetic."""
    peak = ops.new_amax(y16.device)
    with torch.no_grad(), kc.launch_names() as names:
        maps = net._run_decoder(models._EvalAct16(net, peak, ksplit, fuse_head), y16)
    return maps, fc._amax_value(peak), [n for n in names if n in (FUSED, STAGE, SPLIT_STAGE, CONV)]


def check_decoder_walk(dev, k=7, full=False, hw=(1, 1), seed=0):
    """The decoder of ResnetSimple(k, full) on a [1, h, w, 2048] half input, "on" against "off": bit-equal maps and peak; "on" ran
    the fused entry in place of the last stage and the head where the entry applies (k <= 32) and the pair of launches where not."""
    net, g = _decoder_net(dev, k, full, seed)
    y16 = pc.to(dev, sc.half_input((1, hw[0], hw[1], 2048), 1.0, g))
    n = 5 if full else 4
    off, peak_off, names_off = run_decoder(net, y16, False)
    on, peak_on, names_on = run_decoder(net, y16, True)
    assert names_off == [STAGE] * n + [CONV], names_off
    assert names_on == ([STAGE] * (n - 1) + [FUSED] if k <= 32 else names_off), names_on
    assert on.dtype == torch.float32 and tuple(on.shape) == (1, k, hw[0] << n, hw[1] << n)
    assert torch.equal(_bits32(on), _bits32(off)) and peak_on == peak_off and 0.0 < peak_on < HALF_MAX
    assert float(on.abs().max()) > 0 and bool(torch.isfinite(on).all())
    # with inference_conv_ksplit="auto": the fusion yields exactly where the rule splits the last stage
    for force in (None, 2):
        with forced_ksplit(force) if force else contextlib.nullcontext():
            s = ops.conv_transpose4x4s2_f16_ksplit(1, hw[0] << (n - 1), hw[1] << (n - 1), CMID, CMID)
            split, peak_split, names_split = run_decoder(net, y16, True, ksplit=True)
            ref, peak_ref, _ = run_decoder(net, y16, False, ksplit=True)
        assert (FUSED in names_split) == (s == 1 and k <= 32) and (names_split[-1] == CONV) == (s > 1 or k > 32), (force, s, names_split)
        assert torch.equal(_bits32(split), _bits32(ref)) and peak_split == peak_ref, force
    return names_on


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def head_network(dev, case, fusion="on", ksplit="off"):
    net = rs.structured_network(dev, case)
    net.model.module.inference_conv_ksplit = ksplit
    net.model.module.inference_head_fusion = fusion
    return net


def structured_x(dev, case, frames=None):
    x = torch.from_numpy(cases.structured_input(case)[0])
    return pc.to(dev, x if frames is None else x[:frames].contiguous())


def run_walk(net, x):
    with torch.no_grad(), kc.launch_names() as names:
        maps, kps = net.inference(x)
    return maps, kps, net.model.module.half_storage_peak(), names


def check_walk_identity(dev, case, ksplit="off", frames=None):
    """inference() with "on" against "off" on a structured fixture: maps, keypoints and half_storage_peak() equal; "on" ran the fused
    entry exactly where the rule leaves the last stage in one slice, in place of one stage launch and the head launch."""
    x = structured_x(dev, case, frames)
    m0, k0, p0, n0 = run_walk(head_network(dev, case, "off", ksplit), x)
    m1, k1, p1, n1 = run_walk(head_network(dev, case, "on", ksplit), x)
    b, _, ho, wo = (int(v) for v in m0.shape)
    s = ops.conv_transpose4x4s2_f16_ksplit(b, ho // 2, wo // 2, CMID, CMID) if ksplit == "auto" else 1
    print("fused head walk %s (ksplit %s, %d frames): last stage in %d slice(s), fused launches %d, peak %.6g"
          % (case, ksplit, b, s, n1.count(FUSED), p1))
    assert n0.count(FUSED) == 0 and n1.count(FUSED) == (1 if s == 1 else 0)
    if s == 1:
        assert n1.count(CONV) == n0.count(CONV) - 1
        assert n1.count(STAGE) + n1.count(SPLIT_STAGE) == n0.count(STAGE) + n0.count(SPLIT_STAGE) - 1
    else:
        assert n1 == n0
    assert torch.equal(_bits32(m1), _bits32(m0)) and torch.equal(k1, k0) and p1 == p0
    return n1


def check_structured(dev, case):
    """fp16_resnet_storage_checks.check_structured, the check the unfused walk passes, on a network with the switch on."""
    plain = rs.structured_network

    def fused(dev_, case_, storage="fp16"):
        net = plain(dev_, case_, storage)
        net.model.module.inference_head_fusion = "on" if storage == "fp16" else "off"
        return net

    rs.structured_network = fused
    try:
        with kc.launch_names() as names:
            out = rs.check_structured(dev, case)
    finally:
        rs.structured_network = plain
    assert names.count(FUSED) == 1, names.count(FUSED)
    return out


def check_fallback(dev, k=33, hw=(64, 64)):
    """A ResnetSimple with 33 keypoints: "on" runs the unfused launches and gives the maps of "off"."""
    torch.manual_seed(5)
    net = models.ResnetSimple(k, pretrained=False).eval().to(dev)
    net.precision = net.inference_activation_storage = "fp16"
    x = pc.to(dev, torch.from_numpy(cases.image_batch(1, hw[0], hw[1], seed=4)))
    out = {}
    for fusion in ("off", "on"):
        net.inference_head_fusion = fusion
        with torch.no_grad(), kc.launch_names() as names:
            out[fusion] = (net.run_forward(x), net.half_storage_peak(), [n for n in names if n in (FUSED, STAGE, CONV)])
    assert out["on"][2] == out["off"][2] and FUSED not in out["on"][2] and out["on"][2][-1] == CONV
    assert tuple(out["on"][0].shape) == (1, k, hw[0] // 2, hw[1] // 2)
    assert torch.equal(_bits32(out["on"][0]), _bits32(out["off"][0])) and out["on"][1] == out["off"][1]
