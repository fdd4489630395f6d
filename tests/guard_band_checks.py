"""TEST INFRASTRUCTURE: the guard-band harness.  Every other check of the suite runs its kernels on fresh, private allocations: a store
past the end of an output lands in the allocator's slack, an over-read sees finite garbage that a zero weight silences, and an element a
launch never writes holds the previous, nearly identical result.  Here the same checks run inside poisoned arenas:

  * ``Arena.alloc`` places every tensor between two guard bands of GUARD bytes of 0xFF, and fills the body with 0xFF as well.  0xFF.. is
    a NaN in float16 / float32 / float64, -1 in int32 / int64 and 255 in uint8: an element the launch leaves unwritten fails any parity
    assertion, and an over-read whose value enters the arithmetic (garbage * 0) turns the result into NaN.
  * ``guarded(dev, skew)`` hands the arena to dream_amd/ops.py (``ops.torch`` becomes a proxy whose empty / empty_like / zeros allocate
    there: every output and workspace) and to the checks' own ``to`` helper (every input a check moves with ``pc.to``).  skew = 16 puts
    every body at an address that is 16-byte aligned and no more -- the declared contract of the entry points (DREAM_REQUIRE(.. & 15)).
  * ``Arena.assert_intact`` synchronises and holds every byte of every guard band to 0xFF.

GUARD is a condition, not a measurement: 64 KiB per side, twice the largest plausible overshoot of one row of tiles (16 pixels x 512
channels x 4 bytes).

CASES is the table: each entry calls an EXISTING check, with its own assertions unchanged, at the smallest shape at which that kernel
can still go wrong; tests/test_guard_bands_emulated.py (SIMT emulator) and tests/test_gpu_guard_bands.py (-m gpu) run every entry under
both skews.  One direct case, check_bn_buffers_guarded, puts BatchNorm2d's own parameters and buffers into the arena (the kernels write
running_mean / running_var / num_batches_tracked through raw pointers; the existing checks build their own module).

Entries that run output-guarded only (their unmodified check cannot hold on embedded inputs for a reason that is no kernel or wrapper
defect): none -- OUTPUT_GUARDED_ONLY is empty.

Not covered: the allocations of models.py, packed_weights.py and optim.py (network level)."""
import contextlib
import os
import sys

import torch

import parity_checks as pc
import step_checks  # noqa: F401  (binds ``to`` by name: patched with parity_checks)
import fp16_checks
import fp16_grad_storage_checks
import fp16_ksplit_checks
import fp16_resnet_decoder_checks
import fp16_resnet_head_checks
import fp16_resnet_ksplit_checks
import fp16_resnet_storage_checks
import fp16_resnet_train_checks
import fp16_storage_checks
import fp16_train_checks
import fp16_train_storage_checks
import front_conv_checks
from dream_amd import _hip, ops

GUARD = 64 * 1024
POISON = 0xFF
SKEWS = (0, 16)
_HERE = os.path.dirname(os.path.abspath(__file__))
_OWN_FRAMES = ("alloc", "embed", "_alloc", "empty", "zeros", "empty_like", "to")        # the harness's own frames between a caller and Arena.alloc
_ACTIVE = []                    # the arenas of the guarded() contexts in force, innermost last


class _Block:
    def __init__(self, index, buf, lo, nbytes, shape, dtype, owner):
        self.index, self.buf, self.lo, self.nbytes, self.shape, self.dtype, self.owner = index, buf, lo, nbytes, shape, dtype, owner

    def describe(self):
        return "allocation %d %s %s of %s" % (self.index, tuple(self.shape), str(self.dtype).replace("torch.", ""), self.owner)


def _caller():
    """The function that asked for the allocation: the first frame outside this module (``ops.<name>`` for dream_amd/ops.py)."""
    f = sys._getframe(1)
    while f is not None and f.f_globals.get("__name__") == __name__ and f.f_code.co_name in _OWN_FRAMES:
        f = f.f_back
    if f is None:
        return "?"
    mod = f.f_globals.get("__name__", "?")
    return "%s.%s" % ("ops" if mod == ops.__name__ else mod, f.f_code.co_name)


def _shape_of(size):
    if len(size) == 1 and not isinstance(size[0], int):
        size = tuple(size[0])
    return tuple(int(v) for v in size)


class Arena:
    def __init__(self, skew=0):
        assert skew in SKEWS
        self.skew = skew
        self.blocks = []

    def alloc(self, shape, dtype=torch.float32, device="cpu", fill=None):
        """A contiguous ``dtype`` tensor of ``shape`` between two guard bands; body 0xFF, or ``fill`` (0 for torch.zeros)."""
        shape = _shape_of((shape,))
        dtype = dtype or torch.get_default_dtype()
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = item
        for v in shape:
            nbytes *= v
        # GUARD + (alignment of the body to 32 bytes, part of the front band) + skew + body padded to 16 + GUARD
        buf = torch.full((GUARD + 32 + self.skew + (nbytes + 15) // 16 * 16 + GUARD,), POISON, dtype=torch.uint8, device=device)
        lo = GUARD + (-(buf.data_ptr() + GUARD)) % 32 + self.skew
        body = buf[lo:lo + nbytes]
        if fill is not None:
            body.fill_(fill)
        self.blocks.append(_Block(len(self.blocks), buf, lo, nbytes, shape, dtype, _caller()))
        return body.view(dtype).view(shape)

    def embed(self, t):
        """A copy of ``t`` inside the arena (same device, dtype, shape, requires_grad).  What has no dense contiguous body stays as it is."""
        if not isinstance(t, torch.Tensor) or t.layout != torch.strided or t.device.type == "meta" or not t.is_contiguous():
            return t
        out = self.alloc(tuple(t.shape), t.dtype, t.device)
        with torch.no_grad():
            out.copy_(t.detach())
        return out.requires_grad_() if t.requires_grad else out

    def violations(self):
        """One line per touched guard band: which allocation, which side, the first and last touched byte relative to the body."""
        for b in self.blocks:
            if b.buf.is_cuda:
                torch.cuda.synchronize(b.buf.device)
        found = []
        for b in self.blocks:
            for side, band, origin in (("before", b.buf[:b.lo], b.lo), ("after", b.buf[b.lo + b.nbytes:], 0)):
                if bool((band == POISON).all()):
                    continue
                hit = (band != POISON).nonzero().flatten()
                first, last = int(hit[0]) - origin, int(hit[-1]) - origin
                found.append("%s: %d byte(s) written %s the body, offsets %+d .. %+d from its %s"
                             % (b.describe(), int(hit.numel()), side, first, last, "start" if side == "before" else "end"))
        return found

    def assert_intact(self):
        found = self.violations()
        assert not found, "guard bands touched:\n  " + "\n  ".join(found)


class _TorchProxy:
    """``torch`` as dream_amd/ops.py sees it while guarded: empty / empty_like / zeros allocate from the arena, the rest is torch's."""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    def _alloc(self, real, size, dtype, device, fill, kw):
        if kw or (device is not None and torch.device(device).type == "meta"):        # (pin_memory=...: not device memory of a kernel)
            return real(*size, dtype=dtype, device=device, **kw)
        return self._arena.alloc(_shape_of(size), dtype, "cpu" if device is None else device, fill)

    def empty(self, *size, dtype=None, device=None, **kw):
        return self._alloc(torch.empty, size, dtype, device, None, kw)

    def zeros(self, *size, dtype=None, device=None, **kw):
        return self._alloc(torch.zeros, size, dtype, device, 0, kw)

    def empty_like(self, t, dtype=None, **kw):
        if kw or t.device.type == "meta" or not t.is_contiguous():
            return torch.empty_like(t, dtype=dtype, **kw)
        return self._arena.alloc(tuple(t.shape), dtype or t.dtype, t.device)


def _modules_binding_to():
    """parity_checks and every module of the suite that binds its ``to`` by name (``from parity_checks import to``)."""
    real = pc.to
    return [m for m in list(sys.modules.values())
            if os.path.dirname(getattr(m, "__file__", None) or "") == _HERE and m.__dict__.get("to") is real]


@contextlib.contextmanager
def guarded(dev, skew=0, inputs=True):
    """-> the Arena that holds, while the context is active, every tensor ops.py allocates and (``inputs``) every tensor the checks move
    with ``to``.  ``dev`` is where the checks will run ("cpu": the emulator).  Restores everything on exit."""
    arena = Arena(skew)
    real_to = pc.to

    def to(dev_, t):
        return arena.embed(real_to(dev_, t))

    patched = [(ops, "torch", ops.torch)] + ([(m, "to", real_to) for m in _modules_binding_to()] if inputs else [])
    _ACTIVE.append(arena)
    try:
        ops.torch = _TorchProxy(arena)
        for m, name, _ in patched[1:]:
            setattr(m, name, to)
        yield arena
    finally:
        _ACTIVE.pop()
        for m, name, old in patched:
            setattr(m, name, old)


# ---- harness self-tests: plain torch on arena memory, no kernel ------------------------------------------------------------------------
def selfcheck_stray_writes_are_reported(dev):
    for side, where in (("before", -1), ("after", 0)):
        arena = Arena()
        keep = arena.alloc((3, 5), torch.float32, dev)
        t = arena.alloc((7,), torch.float32, dev, fill=0)
        arena.assert_intact()
        blk = arena.blocks[1]
        flat = blk.buf[blk.lo - 4:blk.lo + blk.nbytes + 4].view(torch.float32)           # the body and one element either side
        flat[0 if where < 0 else 8] = 1.0
        found = arena.violations()
        assert len(found) == 1 and "allocation 1 (7,) float32" in found[0] and "written %s the body" % side in found[0], found
        assert ("offsets -4 .. -1 from its start" if where < 0 else "offsets +0 .. +3 from its end") in found[0], found
        assert "selfcheck_stray_writes_are_reported" in found[0], found
        try:
            arena.assert_intact()
        except AssertionError as err:
            assert "guard bands touched" in str(err)
        else:
            raise AssertionError("assert_intact passed over a touched band")
        assert float(t.abs().max()) == 0.0 and bool(torch.isnan(keep).all())
    arena = Arena()                                   # a single byte, the last one of the far band
    arena.alloc((2,), torch.uint8, dev)
    arena.blocks[0].buf[-1] = 0
    assert len(arena.violations()) == 1 and "1 byte(s) written after" in arena.violations()[0]


def selfcheck_bodies(dev):
    arena = Arena()
    for dtype in (torch.float32, torch.float16, torch.float64):
        assert bool(torch.isnan(arena.alloc((4, 3), dtype, dev)).all())
    assert bool((arena.alloc(5, torch.int32, dev) == -1).all()) and bool((arena.alloc((5,), torch.int64, dev) == -1).all())
    assert bool((arena.alloc((5,), torch.uint8, dev) == 255).all())
    z = arena.alloc((2, 3), torch.float16, dev, fill=0)
    blk = arena.blocks[-1]
    assert float(z.abs().max()) == 0.0 and z.is_contiguous() and blk.nbytes == 12
    assert bool((blk.buf[:blk.lo] == POISON).all()) and bool((blk.buf[blk.lo + 12:] == POISON).all())
    assert blk.lo >= GUARD and blk.buf.numel() - blk.lo - blk.nbytes >= GUARD
    src = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4).to(dev)
    e = arena.embed(src)
    assert torch.equal(e, src) and e.data_ptr() != src.data_ptr() and e.device == src.device
    arena.assert_intact()


def selfcheck_skew(dev):
    for skew in SKEWS:
        arena = Arena(skew)
        for shape, dtype in (((3,), torch.float32), ((1, 5, 7, 3), torch.float16), ((2,), torch.int64), ((9,), torch.uint8)):
            assert arena.alloc(shape, dtype, dev).data_ptr() % 32 == skew
        arena.assert_intact()


def selfcheck_proxy_and_restore(dev):
    real_torch, real_to = ops.torch, pc.to
    assert step_checks.to is real_to
    try:
        with guarded(dev, 16) as arena:
            assert ops.torch is not real_torch and pc.to is not real_to and step_checks.to is pc.to
            assert ops.torch.float16 is torch.float16 and ops.torch.Tensor is torch.Tensor
            a = ops.torch.empty((2, 3), dtype=torch.float16, device=dev)
            b = ops.torch.empty(5, dtype=torch.int32, device=dev)
            c = ops.torch.zeros((4,), dtype=torch.int32, device=dev)
            d = ops.torch.empty_like(a)
            e = ops.torch.empty_like(a, dtype=torch.float32)
            f = pc.to(dev, torch.ones(3, 2))
            assert len(arena.blocks) == 6 and all(t.data_ptr() % 32 == 16 for t in (a, b, c, d, e, f))
            assert (a.shape, a.dtype, d.shape, d.dtype, e.shape, e.dtype) == ((2, 3), torch.float16) * 2 + ((2, 3), torch.float32)
            assert bool(torch.isnan(a).all()) and bool((b == -1).all()) and int(c.abs().sum()) == 0 and bool(torch.isnan(e).all())
            assert float(f.sum()) == 6.0 and f.device.type == torch.device(dev).type
            assert arena.blocks[0].owner.endswith("selfcheck_proxy_and_restore")
            assert ops.torch.empty((3,), dtype=torch.int64, pin_memory=False).shape == (3,) and len(arena.blocks) == 6
            arena.assert_intact()
            raise KeyError("inside")
    except KeyError:
        pass
    assert ops.torch is real_torch and pc.to is real_to and step_checks.to is real_to and not _ACTIVE


SELFCHECKS = [selfcheck_stray_writes_are_reported, selfcheck_bodies, selfcheck_skew, selfcheck_proxy_and_restore]


# ---- the direct case -----------------------------------------------------------------------------------------------------------------------
def check_bn_buffers_guarded(dev):
    """BatchNorm2d(48) with every parameter and buffer inside the arena: ops.bn_train_fwd and ops.bn_stats on a (1,6,5,48) input against
    a float64 evaluation.  Running statistics: the bounds of check_resnet_training_ops (1e-6 / 1e-5).  mean, invstd, y: 1e-5 -- sums of
    n = 30 values of |x| <= ~6 in fp32 carry at most n * 2^-24 * max|x| ~ 1e-5 whatever the order; invstd and the affine map are O(1)."""
    arena = _ACTIVE[-1]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 6, 5, 48, generator=g) * 1.5 + 0.3
    gamma, beta = torch.rand(48, generator=g) + 0.5, torch.randn(48, generator=g)
    x64 = x.double().reshape(30, 48)
    mean_ref, var_ref = x64.mean(0), x64.var(0, unbiased=False)
    invstd_ref = (var_ref + 1e-5).rsqrt()
    y_ref = ((x64 - mean_ref) * invstd_ref * gamma.double() + beta.double()).clamp_min(0.0).reshape(1, 6, 5, 48)
    rm_ref, rv_ref = 0.1 * mean_ref, 0.9 + 0.1 * var_ref * 30 / 29
    xd = pc.to(dev, x)
    ctr = pc.to(dev, torch.zeros(4096, dtype=torch.int32))
    for launch in ("bn_train_fwd", "bn_stats"):
        bn = torch.nn.BatchNorm2d(48)
        bn.weight.data.copy_(gamma)
        bn.bias.data.copy_(beta)
        bn = bn.to(dev) if dev != "cpu" else bn
        for t in list(bn.parameters()) + list(bn.buffers()):
            t.data = arena.embed(t.data)
        if launch == "bn_train_fwd":
            y, mean, invstd = ops.bn_train_fwd(xd, bn, None, True)
        else:
            ab, mean, invstd = ops.bn_stats(xd, bn, ctr)
            y = ops.bn_apply_ab(xd, ab, None, True)
            assert float((ab[0].cpu().double() - gamma.double() * invstd_ref).abs().max()) < 1e-5
            assert int(ctr.cpu().abs().sum()) == 0
        assert float((mean.cpu().double() - mean_ref).abs().max()) < 1e-5, launch
        assert float((invstd.cpu().double() - invstd_ref).abs().max()) < 1e-5, launch
        assert float((y.cpu().double() - y_ref).abs().max()) < 1e-5, launch
        assert float((bn.running_mean.cpu().double() - rm_ref).abs().max()) < 1e-6, launch
        assert float((bn.running_var.cpu().double() - rv_ref).abs().max()) < 1e-5, launch
        assert int(bn.num_batches_tracked.item()) == 1, launch
        assert torch.equal(bn.weight.detach().cpu(), gamma) and torch.equal(bn.bias.detach().cpu(), beta)
    arena.assert_intact()


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
RELU, NCHW, POOL2 = ops.CONV_RELU, ops.CONV_OUT_NCHW, ops.CONV_POOL2


def _case(fn, *args, **kw):
    return lambda dev: fn(dev, *args, **kw)


def _with_conv3x3_variant(variant):
    def run(dev):
        _hip.lib().dream_conv3x3_set_variant(variant)
        try:
            pc.check_conv(dev, 2, 12, 20, 64, 7, NCHW)             # every tile of the table meets a 7-channel NCHW output
        finally:
            _hip.lib().dream_conv3x3_set_variant(-1)
    return run


CASES = [
    ("conv_direct", _case(pc.check_conv, 3, 5, 3, 16, 16, 0)),
    ("conv_direct_relu_pool", _case(pc.check_conv, 2, 6, 4, 48, 7, RELU | POOL2)),
    ("conv_winograd2", _case(pc.check_conv_winograd, 3, 5, 3, 32, 7, 0)),
    ("conv_winograd4", _case(pc.check_conv_winograd4, 2, 13, 9, 32, 48, RELU)),
    ("conv1x1", _case(pc.check_conv1x1, 2, 5, 7, 64, 36)),
    ("first_conv", _case(pc.check_first_conv, 2, 5, 7)),
    ("pool_and_layouts", pc.check_pool_and_layouts),
    ("streaming_forms", pc.check_streaming_forms),
    ("softargmax", pc.check_softargmax),
    ("conv_f16x3", _case(pc.check_conv_f16x3, 2, 5, 7, 32, 7, 3, RELU)),
    ("conv_transpose4x4", _case(pc.check_conv_transpose4x4, 1, 3, 5, 64, 32)),
    ("conv2d_general_3x3s2", _case(pc.check_conv2d_general, 2, 7, 9, 32, 48, 3, 2)),
    ("wgrad", _case(pc.check_wgrad, 2, 5, 7, 32, 16)),
    ("resnet_training_ops", pc.check_resnet_training_ops),
    ("backward_ops", pc.check_backward_ops),
    ("conv3x3_bn_fused", _case(pc.check_conv3x3_bn_fused, cases=[(1, 4, 4, 64, 64), (2, 9, 11, 64, 64)])),
    ("wgrad_winograd_padded_dy", _case(pc.check_wgrad_winograd, 2, 5, 3, 64, 16, pad_dy=16)),
    ("convT4x4_wgrad_winograd", _case(pc.check_convT4x4_wgrad_winograd, 3, 7, 5, 64, 128, seed=3)),
    ("peaks_fused", _case(pc.check_peaks_fused_equals_three_kernels, sizes=((1, 7, 5, 9), (2, 3, 37, 45)))),
    ("conv_f16", _case(fp16_checks.check_conv_f16, 2, 5, 7, 32, 7, 3, RELU)),
    ("conv_transpose4x4_f16", _case(fp16_checks.check_conv_transpose4x4_f16, 1, 3, 5, 64, 32)),
    ("conv_transpose3x3_f16", _case(fp16_checks.check_conv_transpose3x3_f16, 1, 3, 5, 64, 32)),
    ("act16_launches", fp16_storage_checks.check_launches),
    ("ksplit_conv3x3", _case(fp16_ksplit_checks.check_case, fp16_ksplit_checks.LAUNCH_CASES[0], 3)),
    ("head_fusion_7_maps", _case(fp16_resnet_head_checks.check_launch, *fp16_resnet_head_checks.LAUNCH_CASES[0])),
    ("head_fusion_1x1_pixel", _case(fp16_resnet_head_checks.check_launch, *fp16_resnet_head_checks.LAUNCH_CASES[3])),
    ("decoder_f16_dgrad", _case(fp16_resnet_decoder_checks.check_dgrad, fp16_resnet_decoder_checks.SHAPES[0])),
    ("decoder_f16_wgrad", _case(fp16_resnet_decoder_checks.check_wgrad, fp16_resnet_decoder_checks.SHAPES[0])),
    ("decoder_f16_forward_1x1_pixel", _case(fp16_resnet_decoder_checks.check_forward, fp16_resnet_decoder_checks.SHAPES[2])),
    ("ksplit_convT", _case(fp16_resnet_ksplit_checks.check_convT_case, fp16_resnet_ksplit_checks.CONVT_CASES[0], True)),
    ("gemm_f16_bn", _case(fp16_resnet_train_checks.check_gemm, fp16_resnet_train_checks.GEMM_SHAPES[0], "bn", 0)),
    ("gemm_f16_mask_zab_res", _case(fp16_resnet_train_checks.check_gemm, fp16_resnet_train_checks.GEMM_SHAPES[1], "mask_zab_res", 0)),
    ("gemm_f16_wgrad", _case(fp16_resnet_train_checks.check_wgrad, fp16_resnet_train_checks.WGRAD_SHAPES[0])),
    ("wgrad_f16", _case(fp16_train_checks.check_wgrad_f16, *fp16_train_checks.WGRAD_SHAPES[0])),
    ("narrow_winograd4_pooled_and_full", _case(front_conv_checks.check_narrow_winograd4, front_conv_checks.NARROW_SIZES[1], 16, 48,
                                               "pooled_and_full")),
    ("front_first_conv", _case(front_conv_checks.check_first_conv, front_conv_checks.FIRST_SIZES[1], 3, 64, True)),
    # ---- beyond the prototype ----
    ("bn_fused_ops", _case(pc.check_bn_fused_ops, ksplits=(0, 2))),
    ("conv_transpose3x3", _case(pc.check_conv_transpose3x3, 2, 5, 3, 48, 7)),
    ("upsample_conv_as_convT", _case(pc.check_upsample_conv_as_convT, 2, 5, 3, 48, 7)),
    # ConvTranspose2d(k4,s2,p1) on the Winograd kernels, odd extents with ragged channels and one block per phase: the data gradient
    # [.., 96 / 128] <- [.., 48 / 32], and the forward of the same layers [.., 48 / 32] -> [.., 96 / 128] (the entry point takes more
    # than 64 output channels only; F(4x4) packs multiples of 32 channels only: its odd-extent shape has 64 for the 48)
    ("conv4x4s2_winograd_tile2_odd", _case(pc.check_conv4x4s2_winograd, 2, 13, 9, 96, 48, tile=2)),
    ("conv4x4s2_winograd_tile2_one_block", _case(pc.check_conv4x4s2_winograd, 1, 8, 8, 128, 32, tile=2)),
    ("conv4x4s2_winograd_tile4_odd", _case(pc.check_conv4x4s2_winograd, 2, 13, 9, 96, 64, tile=4)),
    ("conv4x4s2_winograd_tile4_one_block", _case(pc.check_conv4x4s2_winograd, 1, 8, 8, 128, 32, tile=4)),
    ("convT4x4_winograd_tile2_odd", _case(pc.check_convT4x4_winograd, 2, 13, 9, 48, 96, tile=2)),
    ("convT4x4_winograd_tile2_one_block", _case(pc.check_convT4x4_winograd, 1, 8, 8, 32, 128, tile=2)),
    ("convT4x4_winograd_tile4_odd", _case(pc.check_convT4x4_winograd, 2, 13, 9, 64, 96, tile=4)),
    ("convT4x4_winograd_tile4_one_block", _case(pc.check_convT4x4_winograd, 1, 8, 8, 32, 128, tile=4)),
    ("dataprep", pc.check_dataprep),
    ("act16_residual_launches", fp16_resnet_storage_checks.check_residual_launches),
    ("act16_gathers_and_pool", fp16_resnet_storage_checks.check_gathers_and_pool),
    ("act16_strided_convs", fp16_resnet_storage_checks.check_strided_convs),
    ("train_storage_dgrad_mask16", fp16_train_storage_checks.check_dgrad_mask16_shapes),
    ("train_storage_pool_bwd_x16", fp16_train_storage_checks.check_pool_bwd_x16),
    ("train_storage_widen", fp16_train_storage_checks.check_widen),
    ("grad_storage_dgrad", fp16_grad_storage_checks.check_dgrad_shapes),
    ("grad_storage_pool_bwd_dy16", fp16_grad_storage_checks.check_pool_bwd_dy16),
    ("bn_buffers", check_bn_buffers_guarded),
    # the Winograd epilogues next to a tensor's end: channel counts that are no multiple of 4 (narrow and wide kernel), the fused pool on
    # odd extents, the residual / mask reads, the data-gradient packing, both outputs of the pooling training forward
    ("conv_winograd4_7_channels", _case(pc.check_conv_winograd4, 3, 5, 3, 48, 7, 0, seed=3)),
    ("conv_winograd4_71_channels", _case(pc.check_conv_winograd4, 3, 5, 3, 64, 71, 0, seed=3)),
    ("conv_winograd4_pool_odd", _case(pc.check_conv_winograd4, 2, 13, 9, 16, 64, RELU | POOL2, seed=8)),
    ("conv_winograd4_scale_residual", _case(pc.check_conv_winograd4, 1, 10, 14, 64, 32, RELU, seed=5, with_scale=True, residual="add")),
    ("conv_winograd4_relumask", _case(pc.check_conv_winograd4, 1, 9, 11, 32, 48, ops.CONV_RELUMASK, seed=6, residual="mask")),
    ("conv_winograd4_dgrad", _case(pc.check_conv_winograd4, 2, 7, 9, 32, 64, 0, seed=7, mode=1)),
    ("conv_winograd4_pool_both", _case(pc.check_conv_winograd4_pool_both, 2, 13, 9, 32, 48)),
    ("conv_winograd2_pool_odd", _case(pc.check_conv_winograd, 2, 13, 9, 32, 64, RELU | POOL2, seed=8)),
    ("conv_winograd2_relumask", _case(pc.check_conv_winograd, 1, 9, 11, 32, 48, ops.CONV_RELUMASK, seed=6, residual="mask")),
    ("conv1x1_wgrad_ragged", _case(pc.check_conv1x1_wgrad, 2, 5, 7, 128, 36, seed=1)),
    ("conv1x1_wgrad_padded_dy", _case(pc.check_conv1x1_wgrad, 3, 4, 3, 192, 64, seed=3, pad_dy=16)),
    ("conv_transpose4x4_f16x3", _case(pc.check_conv_transpose4x4_f16x3, 1, 5, 6, 32, 48)),
    ("resnet_stem", _case(pc.check_resnet_stem, 2, 30, 37)),
]
CASES += [("conv_direct_variant%d" % v, _with_conv3x3_variant(v)) for v in range(11)]
CASES += [("decoder_f16_dgrad_variant%d" % v, _case(fp16_resnet_decoder_checks.check_dgrad, fp16_resnet_decoder_checks.VARIANT_SHAPE, variant=v))
          for v in range(fp16_resnet_decoder_checks.NUM_VARIANTS)]
CASE_IDS = [name for name, _ in CASES]
OUTPUT_GUARDED_ONLY = {}        # id -> reason (at most three; listed in the module docstring)
assert len(set(CASE_IDS)) == len(CASE_IDS) and len(OUTPUT_GUARDED_ONLY) <= 3 and set(OUTPUT_GUARDED_ONLY) <= set(CASE_IDS)


def run_case(dev, name, skew):
    """One table entry under the harness: the check's own assertions, then every guard band of every allocation it caused."""
    fn = dict(CASES)[name]
    with guarded(dev, skew, inputs=name not in OUTPUT_GUARDED_ONLY) as arena:
        try:
            fn(dev)
        except AssertionError as err:
            found = arena.violations()
            if found:
                raise AssertionError("%s\nand guard bands touched:\n  %s" % (err, "\n  ".join(found))) from err
            raise
        arena.assert_intact()
        return len(arena.blocks)
