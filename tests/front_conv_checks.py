"""Checks of the front of the VGG encoder shared by the CPU suite (SIMT emulator) and the GPU suite: the first conv
(csrc/conv_first.hip: dwordx4 stores, persistent workgroups) and the narrow workgroup shape of the F(4x4,3x3) kernel with its paired
weight layout (csrc/conv_wino4.hip, csrc/pack_device.h)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from dream_amd import _hip, ops
import parity_checks as pc

# ---- narrow F(4x4) -------------------------------------------------------------------------------------------------------------
NARROW_CIN = (16, 32, 64)                                  # two chunks of eight channels (the minimum), four, eight
NARROW_COUT = (48, 64)                                     # ragged rows, full rows
NARROW_SIZES = ((1, 8, 12), (2, 13, 9), (2, 40, 40))       # one tile block; odd extents; 13 blocks: two per workgroup under the cap of 8
NARROW_MODES = ("plain", "pooled", "pooled_and_full", "residual", "relu_mask")
CAP = 8                                                    # workgroups: one per XCD, each walks its XCD's share of the tile blocks
F4_TOL = 1e-5                                              # the bound of the existing F(4x4) checks (parity_checks.check_conv_winograd4)


def check_narrow_winograd4(dev, size, cin, cout, mode, seed=0):
    """One narrow-shape layer against the fp64 direct convolution, error relative to the output maximum <= 1e-5, the capped grid (a
    workgroup walks several tile blocks, the running weight offset wraps to the next block's chunk 0) giving the uncapped grid's bits."""
    b, h, w = size
    assert cout <= 64
    if mode == "plain":
        return pc.check_conv_winograd4(dev, b, h, w, cin, cout, 0, seed=seed, max_workgroups=(CAP,), tol=F4_TOL)
    if mode == "pooled":
        return pc.check_conv_winograd4(dev, b, h, w, cin, cout, ops.CONV_RELU | ops.CONV_POOL2, seed=seed, max_workgroups=(CAP,), tol=F4_TOL)
    if mode == "residual":
        return pc.check_conv_winograd4(dev, b, h, w, cin, cout, ops.CONV_RELU, seed=seed, with_scale=True, residual="add", max_workgroups=(CAP,), tol=F4_TOL)
    if mode == "relu_mask":
        return pc.check_conv_winograd4(dev, b, h, w, cin, cout, ops.CONV_RELUMASK, seed=seed, residual="mask", max_workgroups=(CAP,), tol=F4_TOL)
    assert mode == "pooled_and_full"
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    bias = torch.randn(cout, generator=g)
    u, rows = ops.pack_weight_winograd4(pc.to(dev, wt), 0)
    xin = pc.to(dev, x.permute(0, 2, 3, 1).contiguous())
    y, p = ops.conv3x3_winograd4_pool_both(xin, u, rows, pc.to(dev, bias), ops.CONV_RELU)
    _hip.lib().dream_conv3x3_winograd4_set_max_workgroups(CAP)
    try:
        y_cap, p_cap = ops.conv3x3_winograd4_pool_both(xin, u, rows, pc.to(dev, bias), ops.CONV_RELU)
        # the one launch gives what the plain and the pooled launch give, bit for bit
        pc.check_conv_winograd4_pool_both(dev, b, h, w, cin, cout, seed=seed)
    finally:
        _hip.lib().dream_conv3x3_winograd4_set_max_workgroups(0)
    assert torch.equal(y, y_cap) and torch.equal(p, p_cap), "persistent grid"
    ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1).relu()
    errs = []
    for got, want in ((y, ref), (p, F.max_pool2d(ref, 2))):
        got = got.cpu().permute(0, 3, 1, 2)
        assert got.shape == want.shape
        errs.append(float((got.double() - want).abs().max()) / max(1.0, float(want.abs().max())))
    assert max(errs) <= F4_TOL, (size, cin, cout, mode, errs)
    return max(errs)


# ---- packing -------------------------------------------------------------------------------------------------------------------
G4 = np.array([[1.0, 0.0, 0.0], [1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0], [-1.0 / 3.0, 1.0 / 3.0, -1.0 / 3.0],
               [-16.0 / 15.0, -8.0 / 15.0, -4.0 / 15.0], [1.0 / 15.0, -2.0 / 15.0, 4.0 / 15.0], [0.0, 0.0, 1.0]])


def narrow_index(ch, pp, n, kk):
    """Float offset of (chunk ch of eight input channels, position pp of 36, row n of 64, channel kk of the chunk) in the narrow
    shape's packed weights: [Cin/8][18 pairs][64 rows][4 lane groups][2 positions][2 k] (csrc/pack_device.h)."""
    return ((((ch * 18 + pp // 2) * 64 + n) * 4 + kk // 2) * 2 + pp % 2) * 2 + kk % 2


def check_narrow_pack_layout(dev, cout, cin, mode, seed=0):
    """Unpacked by the stated index formula, the packed weights are G g G^T computed in fp64 and rounded once; rows past the operator's
    are the transform of a zero filter (zeros of either sign), and the tail the weight stream runs into (16 positions = 8 pairs) is zero."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    packed, rows = ops.pack_weight_winograd4(pc.to(dev, w), mode)
    packed = packed.cpu().numpy()
    cols = cin if mode == 0 else cout
    assert rows == (cout if mode == 0 else cin) and rows <= 64
    assert packed.size == ((cols // 8) * 36 + 16) * 64 * 8
    w64 = w.double().numpy()
    filt = np.zeros((64, cols, 3, 3))                                                   # [64 rows][cols][3][3]; data gradient: taps flipped
    filt[:rows] = w64 if mode == 0 else np.transpose(w64, (1, 0, 2, 3))[:, :, ::-1, ::-1]
    # the products and sums of the device code, in its order, in fp64 (no contraction)
    col = lambda j: G4[:, j][None, None, :, None]                                       # G[a][j] along axis a
    row = lambda i: filt[:, :, i, :][:, :, None, :]                                     # g[i][b] along axis b
    t = (col(0) * row(0) + col(1) * row(1)) + col(2) * row(2)                           # (G g)[a][b]
    u = (t[..., 0, None] * G4[:, 0] + t[..., 1, None] * G4[:, 1]) + t[..., 2, None] * G4[:, 2]       # ((G g) G^T)[a][b']
    want = np.ascontiguousarray(np.transpose(u.reshape(64, cols // 8, 8, 36), (1, 3, 0, 2)).astype(np.float32))
    assert not want[:, :, rows:, :].any()
    ch, pp, n, kk = np.meshgrid(np.arange(cols // 8), np.arange(36), np.arange(64), np.arange(8), indexing="ij")
    idx = narrow_index(ch, pp, n, kk)
    body = (cols // 8) * 36 * 64 * 8
    assert np.array_equal(np.sort(idx.ravel()), np.arange(body))                        # a permutation of the body
    got = packed[idx]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
    assert not packed[body:].any()


def check_narrow_pack_batched_equals_lazy(dev, seed=5):
    """dream_pack_weights_batched / _spans (pack_batched.hip) and the one-tensor entry point (conv_wino4.hip) write the same bytes."""
    g = torch.Generator().manual_seed(seed)
    jobs, singles = [], []
    for cout, cin, mode in [(48, 16, 0), (64, 32, 0), (64, 64, 0), (20, 32, 0), (64, 48, 1), (32, 64, 1)]:
        w = pc.to(dev, torch.randn(cout, cin, 3, 3, generator=g))
        with ops.record_packs() as descs:
            ref = ops.pack_weight_winograd4(w, mode)[0]
        assert len(descs) == 1 and descs[0][0] == ops.PACK_WINOGRAD4
        out = ref.clone()
        out[:out.numel() - 16 * 64 * 8] = float("nan")                                   # the batched kernel rewrites the body, not the tail
        jobs.append((ops.PACK_WINOGRAD4, w, out, cout, cin, mode))
        singles.append(ref)
    table = ops.pack_job_table(jobs, dev)
    spans, nspans = ops.pack_span_table(jobs, dev, floats_per_workgroup=1 << 12)
    poisoned = [j[2].clone() for j in jobs]
    ops.pack_weights_spans(table, spans, nspans)
    for job, ref, before in zip(jobs, singles, poisoned):
        assert torch.equal(job[2], ref), job[3:]
        job[2].copy_(before)
    ops.pack_weights_batched(table, len(jobs), workgroups_per_job=3)
    for job, ref in zip(jobs, singles):
        assert torch.equal(job[2], ref), job[3:]


# ---- first conv ----------------------------------------------------------------------------------------------------------------
FIRST_SIZES = ((1, 16, 16), (2, 17, 19), (1, 33, 40))      # one tile; ragged in both directions; 3 x 3 tiles, the last column 8 wide
FIRST_CIN = (1, 3, 4)
FIRST_COUT = (64, 128)


def fmaf32(a, b, c):
    """fmaf on float32 arrays, exactly: the product of two floats is exact in fp64; its sum with c is rounded to ODD in fp64 (TwoSum
    gives the rounding error), which makes the final rounding to float32 the single rounding of the fused operation."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    fix = (e != 0) & ((bits & 1) == 0)
    away = (e > 0) == (s > 0)                               # the exact sum lies further from zero than s
    bits[fix & away] += 1
    bits[fix & ~away] -= 1
    return bits.view(np.float64).astype(np.float32)


def first_conv_host(x, w, b, relu):
    """Every output element starts from the bias and takes one fmaf per tap in the order channel, filter row, filter column."""
    B, cin, H, W = x.shape
    cout = w.shape[0]
    xp = np.zeros((B, cin, H + 2, W + 2), dtype=np.float32)
    xp[:, :, 1:-1, 1:-1] = x
    acc = np.broadcast_to(b.astype(np.float32), (B, H, W, cout)).copy()
    for c in range(cin):
        for ky in range(3):
            for kx in range(3):
                acc = fmaf32(np.broadcast_to(xp[:, c, ky:ky + H, kx:kx + W, None], acc.shape), np.broadcast_to(w[:, c, ky, kx], acc.shape), acc)
    return np.maximum(acc, 0.0) if relu else acc


def check_first_conv(dev, size, cin, cout, relu, seed=0):
    """csrc/conv_first.hip against the oracle with the existing bound, bit for bit against the host loop, and the same bits from a grid
    of two workgroups (each walks over several tiles through both patch buffers); the amax variant: same tensor, max |y| exactly."""
    b, h, w = size
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
    bias = torch.randn(cout, generator=g)
    args = (pc.to(dev, x), pc.to(dev, wt), pc.to(dev, bias))
    y = ops.conv3x3_first(*args, relu=relu).cpu()
    ref = F.conv2d(x, wt, bias, padding=1)
    ref = ref.relu() if relu else ref
    assert float((y.permute(0, 3, 1, 2) - ref).abs().max()) <= pc.tol(ref.numpy())
    host = first_conv_host(x.numpy(), wt.numpy(), bias.numpy(), relu)
    assert np.array_equal(y.numpy().view(np.uint32), host.view(np.uint32)), float(np.abs(y.numpy() - host).max())
    os.environ["DREAM_FIRST_MAX_WORKGROUPS"] = "2"
    try:
        y_cap = ops.conv3x3_first(*args, relu=relu).cpu()
        y_amax, amax = ops.conv3x3_first_amax(*args, relu=relu)
    finally:
        del os.environ["DREAM_FIRST_MAX_WORKGROUPS"]
    assert torch.equal(y, y_cap), "persistent grid"
    assert torch.equal(y, y_amax.cpu())
    assert int(amax.cpu().item()) == int(y.abs().max().view(torch.int32).item())
    y_amax, amax = ops.conv3x3_first_amax(*args, relu=relu)
    assert torch.equal(y, y_amax.cpu()) and int(amax.cpu().item()) == int(y.abs().max().view(torch.int32).item())
