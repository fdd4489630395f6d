"""What the CPU suite (kernels under the SIMT emulator) and the GPU suite share for ResnetSimple's train_gemm_precision="fp16"
(csrc/gemm1x1_f16.hip, the amax form of bn_bwd_apply): every launch against the fp64 product of its ROUNDED operands.

Bounds.  A launch rounds each operand once -- an activation as half(clamp(x, +-65504)), a gradient as
half(dz 2^e_g) 2^-e_g with e_g = 13 - exponent(max|dz|) (0 for a zero tensor), a weight as half(w 2^e_w) 2^-e_w -- and accumulates in
fp32.  So against the fp64 product of the rounded operands it may differ by the fp32-accumulation bound, 5e-6 of the reference's
maximum; and the fp64 product of the UNROUNDED operands has to lie more than 5e-5 of that maximum away (a half has 11 significant
bits: 2^-12 relative rounding error per operand, summed over K >= 64 random terms), so a kernel that does not round cannot pass.
"""
import math

import torch

import parity_checks as pc
from dream_amd import ops

ACC_BOUND, ROUNDING_GAP = 5e-6, 5e-5

# (M, K, N): two row tiles, the second with 6 rows; a partial column block and several statistics rows; the deepest contraction
GEMM_SHAPES = [(70, 64, 64), (200, 128, 72), (70, 2048, 64)]
GEMM_FORMS = ["plain_act", "plain_grad", "res", "bn", "bn_pre", "mask_zab", "mask_zab_res", "mask_yact", "mask_yact_res"]
# (M, Cin, Cout, Cdy, PRE)
WGRAD_SHAPES = [(70, 64, 64, 64, False), (4112, 64, 68, 72, False), (70, 128, 64, 64, True)]


def scale_exponent(t):
    """half_scale.h: e with max|t| 2^e in [2^13, 2^14), 0 for a zero tensor, clamped to +-100."""
    amax = float(t.abs().max())
    if amax == 0.0:
        return 0
    return max(-100, min(100, 13 - (math.frexp(amax)[1] - 1)))


def q_act(x):
    """the activation operand as the kernel sees it, in fp64"""
    return x.float().clamp(-65504.0, 65504.0).half().double()


def q_scaled(t):
    """the gradient / weight operand as the kernel sees it, in fp64 (the scaling is exact: a power of two)"""
    e = scale_exponent(t)
    return (t.float() * 2.0 ** e).half().double() * 2.0 ** -e


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bn(c, g):
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.1)
    return bn


def _ctr(dev):
    return pc.to(dev, torch.zeros(4096, dtype=torch.int32))


def _amax_of(dev, t):
    """the scalar a producing launch would publish: the bit pattern of max|t|"""
    return pc.to(dev, torch.tensor([float(t.abs().max())], dtype=torch.float32).view(torch.int32))


def _pre_operand(x, ab):
    """relu(fmaf(a, x, b)) in fp32: the product is exact in fp64, the sum rounded once more only at fp32 ties of measure zero"""
    return (ab[0].double() * x.double() + ab[1].double()).float().clamp_min(0.0)


def _assert_close(got, ref, unrounded, what):
    top = float(ref.abs().max())
    err = float((got.double() - ref).abs().max())
    gap = float((unrounded - ref).abs().max())
    print("%s: max|ref| %.4g, error %.3g of it (bound %.1g), unrounded product %.3g of it away (needs > %.1g)"
          % (what, top, err / top, ACC_BOUND, gap / top, ROUNDING_GAP))
    assert err <= ACC_BOUND * top, (what, err / top)
    assert gap > ROUNDING_GAP * top, (what, gap / top)


def check_gemm(dev, shape, form, ks, stride_pad=0, seed=0):
    """One launch of gemm1x1_f16_kernel in ``form`` with the K split forced to ``ks`` (0: by shape) -> the output (for repeat checks)."""
    M, K, N = shape
    g = _gen(seed + 17 * ks + len(form))
    grad = form.startswith(("plain_grad", "res", "mask"))
    w = torch.randn(N, K, 1, 1, generator=g) * 0.1                     # the forward operator [N][K] ...
    if grad:
        w = w.reshape(K, N, 1, 1).clone()                               # ... or a conv weight [Cout = K][Cin = N] read by mode 1
        x = torch.randn(M, K, generator=g) * 3e-4
        xq = q_scaled(x)
        wq, wu = q_scaled(w).reshape(K, N), w.double().reshape(K, N)
    else:
        x = torch.randn(M, K, generator=g).abs() * 1.5 if form != "bn_pre" else torch.randn(M, K, generator=g) * 2.0
        wq, wu = q_scaled(w).reshape(N, K).t(), w.double().reshape(N, K).t()
    xd = pc.to(dev, x.reshape(1, 1, M, K).contiguous())
    p16 = ops.pack_conv1x1_weight_f16(pc.to(dev, w), 1 if grad else 0)
    assert int(p16[1].cpu()) == scale_exponent(w) and p16[2] == N
    ops.call("dream_conv1x1_f16_set_ksplit", ks)
    try:
        if form in ("plain_act", "plain_grad", "res"):
            res = torch.randn(M, N, generator=g) * float(x.abs().max()) if form == "res" else None
            amax = _amax_of(dev, x) if grad else None
            if stride_pad:
                xp = torch.cat([x, torch.full((M, stride_pad), 7.0)], dim=1).contiguous()          # (the padding must not be read)
                y, xpd, resd = pc.to(dev, torch.empty(M, N)), pc.to(dev, xp), pc.to(dev, res) if res is not None else None
                ops.call("dream_conv1x1_f16_nhwc_f32", ops.ptr(xpd), ops.ptr(amax), ops.ptr(p16[0]), ops.ptr(p16[1]), None,
                         ops.ptr(resd), ops.ptr(y), M, K, N, K + stride_pad, ops.stream())
                y = y.cpu()
            else:
                y = ops.conv1x1_f16(xd, amax, p16, N, residual=pc.to(dev, res.reshape(1, 1, M, N)) if res is not None else None).cpu().reshape(M, N)
            if not grad:
                xq = q_act(x)
            extra = res.double() if res is not None else 0.0
            _assert_close(y, xq @ wq + extra, x.double() @ wu + extra, "%s %s ks=%d" % (form, shape, ks))
            return y
        if form in ("bn", "bn_pre"):
            bn = _bn(N, g)
            pre_ab = None
            if form == "bn_pre":                                        # about half of the loader's elements masked
                pre_ab = torch.stack([torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.2])
                xin = _pre_operand(x, pre_ab)
                assert 0.3 < float((xin == 0).float().mean()) < 0.7
            else:
                xin = x
            bias = torch.randn(N, generator=g) * 0.1
            z, ab, mean, invstd = ops.conv1x1_bn_f16(xd, p16, N, bn.to(dev) if dev != "cpu" else bn, _ctr(dev),
                                                     pre_ab=pc.to(dev, pre_ab) if pre_ab is not None else None, shift=pc.to(dev, bias))
            z2 = z.cpu().reshape(M, N)
            _assert_close(z2, q_act(xin) @ wq + bias.double(), xin.double() @ wu + bias.double(), "%s %s ks=%d" % (form, shape, ks))
            # the statistics are those of the y the launch returned, in fp64, at the fp32 form's tolerances (parity_checks.
            # check_resnet_training_ops: the normalised activation within 2e-5, the running statistics within 1e-5)
            zd = z2.double()
            mu, var = zd.mean(0), zd.var(0, unbiased=False)
            istd = 1.0 / torch.sqrt(var + bn.eps)
            assert float((mean.cpu().double() - mu).abs().max()) <= 1e-5 * max(1.0, float(mu.abs().max()))
            assert float((invstd.cpu().double() / istd - 1.0).abs().max()) <= 1e-5
            a_ref = bn.weight.detach().cpu().double() * istd
            b_ref = bn.bias.detach().cpu().double() - mu * a_ref
            y_ref = zd * a_ref + b_ref
            y_got = zd * ab.cpu()[0].double() + ab.cpu()[1].double()
            assert float((y_got - y_ref).abs().max()) < 2e-5
            assert float((bn.running_mean.cpu().double() - 0.1 * mu).abs().max()) < 1e-5
            assert float((bn.running_var.cpu().double() - (0.9 + 0.1 * zd.var(0, unbiased=True))).abs().max()) < 1e-5
            assert int(bn.num_batches_tracked.item()) == 1
            return torch.cat([z2.reshape(-1), ab.cpu().reshape(-1), mean.cpu(), invstd.cpu()])
        # the masked data gradient: g = (dz . w (+ residual)) [mask], dbeta = sum g, dgamma = sum g xhat
        zin = torch.randn(M, N, generator=g)
        zab = torch.stack([torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2])
        zmean, zinvstd = torch.randn(N, generator=g) * 0.1, torch.rand(N, generator=g) + 0.5
        res = torch.randn(M, N, generator=g) * float(x.abs().max()) if form.endswith("_res") else None
        if form.startswith("mask_yact"):
            y_act = (torch.randn(M, N, generator=g)).clamp_min(0.0)     # a stored Bottleneck output: its sign is the mask
            mask = y_act > 0
        else:
            y_act = None
            # the fp32 rule fmaf(a, z, b) > 0: the sign of the exactly rounded sum is the sign of the exact sum, which fp64 holds
            mask = (zab[0].double() * zin.double() + zab[1].double()) > 0
        assert 0.3 < float(mask.float().mean()) < 0.7
        gm, dgam, dbet = ops.conv1x1_bwd_bnmask_f16(
            xd, _amax_of(dev, x), p16, N, pc.to(dev, zin.reshape(1, 1, M, N)), pc.to(dev, zab), pc.to(dev, zmean), pc.to(dev, zinvstd),
            _ctr(dev), y_act=pc.to(dev, y_act.reshape(1, 1, M, N)) if y_act is not None else None,
            residual=pc.to(dev, res.reshape(1, 1, M, N)) if res is not None else None)
        gm = gm.cpu().reshape(M, N)
        extra = res.double() if res is not None else 0.0
        assert bool((gm[~mask] == 0).all()) and bool((gm[mask] != 0).any())            # the mask, element for element
        _assert_close(gm, (xq @ wq + extra) * mask, (x.double() @ wu + extra) * mask, "%s %s ks=%d" % (form, shape, ks))
        # The sums over the returned g in fp64.  The kernel rounds xhat = (z - mean) invstd to fp32 (2^-23 relative, two operations) before
        # an fp64 product and sum, and rounds the total to fp32: <= 3 2^-24 sum |g xhat| + 2^-24 |total|  <  2e-5 of the largest total
        gd = gm.double()
        xh = (zin.double() - zmean.double()) * zinvstd.double()
        for got, ref in ((dbet, gd.sum(0)), (dgam, (gd * xh).sum(0))):
            assert float((got.cpu().double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
        return torch.cat([gm.reshape(-1), dgam.cpu(), dbet.cpu()])
    finally:
        ops.call("dream_conv1x1_f16_set_ksplit", 0)


def check_gemm_repeat(dev):
    """Two runs give the same bits (the K split sums through LDS in wave order, the statistics in row order)."""
    for form in ("bn_pre", "mask_zab_res"):
        a = check_gemm(dev, (200, 128, 72), form, 4)
        b = check_gemm(dev, (200, 128, 72), form, 4)
        assert torch.equal(a, b), form


def check_wgrad(dev, shape, seed=0):
    M, Cin, Cout, Cdy, pre = shape
    g = _gen(seed + M)
    dy = torch.randn(M, Cdy, generator=g) * 3e-4
    pre_ab = None
    if pre:
        x = torch.randn(M, Cin, generator=g) * 2.0
        pre_ab = torch.stack([torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.2])
        xin = _pre_operand(x, pre_ab)
    else:
        x = torch.randn(M, Cin, generator=g).abs() * 1.5
        xin = x
    split = ops.conv1x1_wgrad_f16_workspace(M, Cin, Cout) // (Cout * Cin * 4)
    run = lambda: ops.conv1x1_wgrad_f16(pc.to(dev, x.reshape(1, 1, M, Cin)), pc.to(dev, dy.reshape(1, 1, M, Cdy)), _amax_of(dev, dy), Cout, Cin,   # noqa: E731
                                        pre_ab=pc.to(dev, pre_ab) if pre_ab is not None else None).cpu().reshape(Cout, Cin)
    dw = run()
    _assert_close(dw, q_scaled(dy)[:, :Cout].t() @ q_act(xin), dy.double()[:, :Cout].t() @ xin.double(), "wgrad %s split %d" % (shape, split))
    assert torch.equal(run(), dw)                                       # no floating-point atomics: the same bits
    return split


def check_scales(dev):
    """Powers of two travel exactly; a zero gradient gives exact zeros; an outlier activation saturates to 65504 and stays finite."""
    M, K, N = 70, 64, 64
    g = _gen(5)
    dz = torch.randn(M, K, generator=g) * 3e-4
    w = torch.randn(K, N, 1, 1, generator=g) * 0.1
    x = torch.randn(M, N, generator=g).abs()
    p16 = ops.pack_conv1x1_weight_f16(pc.to(dev, w), 1)
    conv = lambda t: ops.conv1x1_f16(pc.to(dev, t.reshape(1, 1, M, K)), _amax_of(dev, t), p16, N).cpu()                  # noqa: E731
    wgrad = lambda t: ops.conv1x1_wgrad_f16(pc.to(dev, x.reshape(1, 1, M, N)), pc.to(dev, t.reshape(1, 1, M, K)), _amax_of(dev, t), K, N).cpu()   # noqa: E731
    y1, d1 = conv(dz), wgrad(dz)
    for s in (2.0 ** -20, 2.0 ** 10):
        assert torch.equal(conv(dz * s) / s, y1) and torch.equal(wgrad(dz * s) / s, d1), s
    zero = torch.zeros_like(dz)
    assert float(conv(zero).abs().max()) == 0.0 and float(wgrad(zero).abs().max()) == 0.0
    gm, dgam, dbet = ops.conv1x1_bwd_bnmask_f16(pc.to(dev, zero.reshape(1, 1, M, K)), _amax_of(dev, zero), p16, N,
                                                pc.to(dev, x.reshape(1, 1, M, N)), pc.to(dev, torch.ones(2, N)), pc.to(dev, torch.zeros(N)),
                                                pc.to(dev, torch.ones(N)), _ctr(dev))
    assert float(gm.abs().max()) == 0.0 and float(dgam.abs().max()) == 0.0 and float(dbet.abs().max()) == 0.0
    # forward operand with one 1e6 outlier
    wf = torch.randn(N, K, 1, 1, generator=g) * 0.1
    xa = torch.randn(M, K, generator=g).abs()
    xa[3, 5] = 1e6
    y = ops.conv1x1_f16(pc.to(dev, xa.reshape(1, 1, M, K)), None, ops.pack_conv1x1_weight_f16(pc.to(dev, wf), 0), N).cpu().reshape(M, N)
    ref = q_act(xa) @ q_scaled(wf).reshape(N, K).t()
    assert bool(torch.isfinite(y).all()) and float(q_act(xa).max()) == 65504.0
    assert float((y.double() - ref).abs().max()) <= ACC_BOUND * float(ref.abs().max())


def check_bn_bwd_apply_amax(dev):
    """dz (and g) bit-equal to the plain form's, the scalar exactly max|dz|; every mask mode; a zero gradient leaves the scalar zero."""
    g = _gen(9)
    M, C = 150, 72
    z, dy = torch.randn(1, 1, M, C, generator=g), torch.randn(1, 1, M, C, generator=g) * 1e-3
    y_act = torch.randn(1, 1, M, C, generator=g).clamp_min(0.0)
    ab = torch.stack([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2])
    gamma, mean, invstd = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    dgam, dbet = torch.randn(C, generator=g) * 1e-2, torch.randn(C, generator=g) * 1e-2
    d = lambda t: pc.to(dev, t)                                         # noqa: E731
    for kw in (dict(), dict(y_act=d(y_act), want_g=True), dict(ab=d(ab))):
        for grad in (dy, torch.zeros_like(dy)):
            dg, db = (dgam, dbet) if grad is dy else (torch.zeros(C), torch.zeros(C))
            amax = pc.to(dev, torch.full((1,), 12345, dtype=torch.int32))                # stale: the launch zeroes it first
            dz0, g0 = ops.bn_bwd_apply(d(z), d(grad), d(gamma), d(mean), d(invstd), d(dg), d(db), **kw)
            dz1, g1 = ops.bn_bwd_apply_amax(d(z), d(grad), d(gamma), d(mean), d(invstd), d(dg), d(db), amax, **kw)
            assert torch.equal(dz0, dz1) and (g0 is None) == (g1 is None) and (g0 is None or torch.equal(g0, g1))
            assert float(amax.cpu().view(torch.float32)) == float(dz0.abs().max()), kw.keys()


def check_batched_pack(dev):
    """Every half copy by the batched pack: the one-tensor packer's halfs and exponents, bit for bit (a zero weight included)."""
    g = _gen(3)
    ws = [pc.to(dev, w) for w in (torch.randn(64, 128, 1, 1, generator=g) * 0.1, torch.randn(256, 64, 1, 1, generator=g) * 3.0,
                                   torch.zeros(64, 64, 1, 1), torch.randn(72, 2048, 1, 1, generator=g) * 1e-3)]
    entries = []
    for w in ws:
        for mode in ((0, 1) if int(w.shape[0]) % 32 == 0 else (0,)):
            want = ops.pack_conv1x1_weight_f16(w, mode)
            entries.append((w, (torch.full_like(want[0], 7.0), torch.full_like(want[1], 99), want[2]), mode, want))
    table, scratch = ops.pack16_job_table([e[:3] for e in entries], ws[0].device)
    scratch.fill_(12345)                                                # stale: the launch zeroes the words first
    ops.pack_conv1x1_weights_f16_batched(table, scratch, workgroups_per_job=3)
    for w, got, mode, want in entries:
        assert torch.equal(got[0], want[0]) and int(got[1].cpu()) == int(want[1].cpu()) == scale_exponent(w.cpu()), (tuple(w.shape), mode)


def check_refusals(dev):
    """Null pointers, K % 32, oversize tensors: refused by the entry points before any launch."""
    t = pc.to(dev, torch.zeros(64, 64))
    i = pc.to(dev, torch.zeros(1, dtype=torch.int32))
    p, s = ops.ptr, ops.stream()

    def refused(name, *args):
        try:
            ops.call(name, *args)
        except RuntimeError as e:
            return str(e)
        raise AssertionError("%s%r was accepted" % (name, args))

    assert "null" in refused("dream_conv1x1_f16_nhwc_f32", p(t), None, None, p(i), None, None, p(t), 64, 64, 64, 64, s)
    assert "K % 32" in refused("dream_conv1x1_f16_nhwc_f32", p(t), None, p(t), p(i), None, None, p(t), 64, 48, 64, 48, s)
    assert "too large" in refused("dream_conv1x1_f16_nhwc_f32", p(t), None, p(t), p(i), None, None, p(t), 1 << 23, 64, 64, 64, s)
    assert "null" in refused("dream_conv1x1_wgrad_f16_nhwc_f32", p(t), p(t), None, p(t), p(t), 64, 64, 64, 64, None, s)
    assert "Cin % 64" in refused("dream_conv1x1_wgrad_f16_nhwc_f32", p(t), p(t), p(i), p(t), p(t), 64, 32, 64, 64, None, s)
    assert "too large" in refused("dream_conv1x1_wgrad_f16_nhwc_f32", p(t), p(t), p(i), p(t), p(t), 1 << 23, 64, 64, 64, None, s)
    assert "null" in refused("dream_conv1x1_bwd_bnmask_f16_nhwc_f32", p(t), None, p(t), p(i), None, p(t), 64, 64, 64, 64, p(t), p(t), None, p(t),
                             p(t), p(t), p(t), p(t), p(i), s)
    assert "null" in refused("dream_bn_bwd_apply_amax_nhwc_f32", p(t), p(t), None, None, p(t), p(t), p(t), p(t), p(t), p(t), None, None, 64, 64, 0, s)
    assert "multiple of 32" in refused("dream_pack_conv1x1_weight_f16", p(t), p(t), p(i), p(i), 64, 48, 0, s)
    assert ops.conv1x1_wgrad_f16_workspace(64, 32, 64) == 0
