"""Direct float64 parity checks of the kernels that turn a forward / backward pass into a training step -- the fused losses, Adam / SGD,
SoftArgmax and the glue kernels of csrc/elementwise.hip --, shared by the emulator suite (test_step_kernels_emulated.py) and the GPU
suite (test_gpu_step_kernels.py).

Every reference is computed in float64 (numpy / torch on the CPU) from the same fp32 inputs.  Every tolerance is a count of roundings,
written where it is used, with u = 2^-24 the unit round-off of fp32, or an existing project tolerance (SoftArgmax: 1e-4 max(1, |ref|));
none is read off the kernel under test.  Each check prints its worst error / budget ratio ("step-check <name>: ...") and keeps it in
RATIOS; for the bit-exact checks the figure is the number of differing words, which must be 0."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dream_amd import _hip, data_parallel, ops, optim
from parity_checks import to

U = 2.0 ** -24
TINY = 2.0 ** -149                 # the smallest fp32 denormal: what one rounding can cost below the normal range
RATIOS = {}

LOSS_SIZES = (1, 3, 255, 256, 257, 1003, 524288, 524289, 1048653)     # the grid cap is 2048 x 256 = 524288: the last two wrap the grid-stride loop
PLANTED = (0.0, 1.0, -1.0, 0.99999994, -0.99999994, 1.0000001, -1.0000001, 3.0)     # d = o - t around the Huber kink (1 -+ one ulp)


def _report(name, ratio):
    ratio = float(ratio)
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print("step-check %s: worst error / budget = %.3g" % (name, ratio))
    return ratio


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(name, got, want):
    """fp32 arrays / tensors equal bit for bit (so -0 != +0 and a NaN equals itself)."""
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (name, g.shape, w.shape)
    bad = int((g != w).sum())
    _report(name + " [differing words]", bad)
    assert bad == 0, "%s: %d of %d words differ" % (name, bad, g.size)


def _ulp(x):
    """Spacing of fp32 at |x| (x: float64 array of fp32 values)."""
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _amax_word(amax):
    return int(amax.cpu().numpy().view(np.uint32)[0])


def _f32_word(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


# ---- losses ---------------------------------------------------------------------------------------------------------------------------
def loss_inputs(n, seed=0):
    """o ~ N(0, 2), t ~ N(0, 1); for n > 8 the first eight differences are PLANTED exactly (o = 0, t = -d)."""
    g = torch.Generator().manual_seed(1000 + seed + n % 9973)
    o = torch.randn(n, generator=g) * 2.0
    t = torch.randn(n, generator=g)
    if n > 8:
        d = np.array(PLANTED, dtype=np.float32)
        o[:8] = 0.0
        t[:8] = torch.from_numpy(-d)
        assert np.array_equal((o[:8] - t[:8]).numpy(), d)
    return o, t


def loss_reference(o, t, kind):
    """-> (fp32 gradient the kernel must reproduce bit for bit, float64 loss) from the fp32 difference d = o - t."""
    on, tn = o.detach().cpu().numpy().reshape(-1), t.detach().cpu().numpy().reshape(-1)
    n = on.size
    d = on - tn                                                  # fp32, one rounding: the kernel's first operation
    d64 = d.astype(np.float64)
    if kind == "mse":
        grad = d * np.float32(2.0 / n)
        loss = float((d64 * d64).sum()) / n
    else:
        inner = np.abs(d) < np.float32(1.0)
        grad = np.where(inner, d, np.sign(d)).astype(np.float32) * np.float32(1.0 / n)
        loss = float(np.where(inner, 0.5 * d64 * d64, np.abs(d64) - 0.5).sum()) / n
    return grad, loss


def _hold_loss(name, o, t, kind):
    n = o.numel()
    grad_ref, loss_ref = loss_reference(o, t, kind)
    loss, grad = ops.mse_fwd_bwd(o, t, want_grad=True, kind=kind)
    assert grad.shape == o.shape and grad.is_contiguous()
    _same_bits(name + " gradient", grad.reshape(-1), grad_ref)
    # the double sum of non-negative terms (each rounded once, n - 1 additions: n 2^-52 covers both), rounded to fp32 by the kernel
    # and once more by the division by n: (1 + u)^2 - 1 < 2^-23
    budget = (2.0 ** -23 + n * 2.0 ** -52) * loss_ref
    err = abs(float(loss.double()) - loss_ref)
    assert math.isfinite(float(loss))
    ratio = _report(name + " loss", err / budget if budget > 0 else (0.0 if err == 0 else math.inf))
    assert err <= budget, (name, float(loss), loss_ref, ratio)
    # determinism: the partial sums are added in a fixed order
    loss2, _ = ops.mse_fwd_bwd(o, t, want_grad=True, kind=kind)
    loss3, none = ops.mse_fwd_bwd(o, t, want_grad=False, kind=kind)
    assert none is None
    _same_bits(name + " loss repeated", torch.stack([loss2.reshape(()), loss3.reshape(())]), torch.stack([loss.reshape(()), loss.reshape(())]))
    return loss, grad, grad_ref


def check_loss(dev, kind, n):
    o, t = loss_inputs(n)
    _hold_loss("%s n=%d" % (kind, n), to(dev, o), to(dev, t), kind)


def check_loss_stacked_target(dev, kind):
    """The multi-stage loss (network.py: torch.stack(outputs) against target.unsqueeze(0).expand(...)): the target is not contiguous."""
    S, B, K, H, W = 3, 2, 7, 5, 6
    g = torch.Generator().manual_seed(7)
    outs = [to(dev, torch.randn(B, K, H, W, generator=g) * 2.0) for _ in range(S)]
    target = to(dev, torch.randn(B, K, H, W, generator=g))
    o = torch.stack(outs)
    t = target.unsqueeze(0).expand([S] + [-1] * target.dim())
    assert not t.is_contiguous() and o.shape == t.shape
    _hold_loss("%s stacked [S,B,K,H,W]" % kind, o, t, kind)


def check_loss_module(dev, kind):
    """HipMSELoss / HipSmoothL1Loss through autograd: the kernel's gradient, times the upstream factor."""
    crit = optim.HipMSELoss() if kind == "mse" else optim.HipSmoothL1Loss()
    for n in (1003, 524289):
        o, t = loss_inputs(n)
        grad_ref, loss_ref = loss_reference(o, t, kind)
        od, td = to(dev, o), to(dev, t)
        direct, _ = ops.mse_fwd_bwd(od, td, want_grad=False, kind=kind)
        for factor in (None, 3.0):
            leaf = od.clone().requires_grad_()
            loss = crit(leaf, td)
            _same_bits("%s module n=%d loss" % (kind, n), loss.reshape(1), direct.reshape(1))
            (loss if factor is None else factor * loss).backward()
            want = grad_ref if factor is None else grad_ref * np.float32(factor)      # one more fp32 product
            _same_bits("%s module n=%d gradient x %s" % (kind, n, factor), leaf.grad.reshape(-1), want)
        with torch.no_grad():                                                           # nothing requires a gradient: none is computed
            assert crit(od, td).requires_grad is False


# ---- Adam / SGD kernels ---------------------------------------------------------------------------------------------------------------
ADAM_STEPS = (1, 2, 7, 1000, 100000)
ADAM_HYPER = ((1e-4, 0.9, 0.999, 1e-8), (1.5e-4, 0.9, 0.999, 1e-8), (1e-2, 0.5, 0.9, 1e-3))
GRAD_CLASSES = (1e-30, 1e-12, None, 1.0, 1e4)            # None: 1e-3 |N(0,1)|, redrawn every step.  (|g| > 1e15: g^2 overflows, out of scope)
GUARD = 12345.0


def _buffers(dev, n, view, count):
    """``count`` fp32 buffers of n elements; view: each is flat[1:1+n] of a longer buffer (4-byte aligned only) between guard words."""
    if not view:
        return [to(dev, torch.zeros(n)) for _ in range(count)], []
    flats = [to(dev, torch.full((n + 6,), GUARD)) for _ in range(count)]
    return [f[1:1 + n] for f in flats], flats


def _guards_intact(flats, n):
    for f in flats:
        h = f.cpu()
        assert float(h[0]) == GUARD and bool((h[1 + n:] == GUARD).all()), "write outside the view"


def adam_reference(p, m, v, g, lr, b1, b2, eps, t):
    """One torch.optim.Adam step in float64 from fp32 state, with the constants torch's fp32 step uses: the weights float32(1 - beta)
    (complement taken in double), float32(beta2), bias corrections 1 - beta^t in double.  -> m, v, update, denominator, step size."""
    w1, w2, b2f = float(np.float32(1.0 - b1)), float(np.float32(1.0 - b2)), float(np.float32(b2))
    m_ref = m + (g - m) * w1
    v_ref = v * b2f + w2 * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    step_size = lr / bc1
    den = np.sqrt(v_ref) / math.sqrt(bc2) + eps
    return m_ref, v_ref, step_size * m_ref / den, den, step_size, w1


def _hold_adam_launch(name, before, after, g, hyper, t, worst):
    lr, b1, b2, eps = hyper
    p0, m0, v0 = (_np64(x) for x in before)
    p1, m1, v1 = (_np64(x) for x in after)
    g64 = _np64(g)
    m_ref, v_ref, dp_ref, den, step_size, w1 = adam_reference(p0, m0, v0, g64, lr, b1, b2, eps, t)
    # m = m + (g - m) w1: the difference, the product and the sum round once each
    m_budget = U * (2.0 * w1 * np.abs(g64 - m0) + np.abs(m_ref))
    # v = v b2 + (w2 g) g: three products and a sum of non-negative terms, 4u; 2^-149 where a term falls below the normal range
    v_budget = 4.0 * U * v_ref + TINY
    # update = step_size (m / (sqrt(v) inv_sqrt_bc2 + eps)): sqrt of a v that is 4u off (2u), sqrt, inv_sqrt_bc2, their product, eps,
    # the sum, the quotient, lr and step_size rounded on the way in (2), the final product: 11 roundings, held to 12u; plus what the
    # m budget moves it by; plus the rounding of p - update (half an ulp of the result)
    dp_budget = 12.0 * U * np.abs(dp_ref) + step_size * m_budget / den + 0.5 * _ulp(p1)
    failed = []
    for key, err, budget in (("m", np.abs(m1 - m_ref), m_budget), ("v", np.abs(v1 - v_ref), v_budget),
                             ("dp", np.abs((p0 - p1) - dp_ref), dp_budget)):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(budget > 0, err / budget, np.where(err == 0, 0.0, np.inf))
        worst[key] = max(worst[key], float(r.max()))
        if key == "v":
            worst["v_rel"] = max(worst["v_rel"], float((err / np.maximum(v_ref, 1e-30)).max()))
        if not (err <= budget).all():
            failed.append("%s off by %.3g budgets at element %d" % (key, float(r.max()), int(r.argmax())))
    assert not failed, "%s step %d: %s (worst |v - v_ref| / v_ref = %.3g)" % (name, t, "; ".join(failed), worst["v_rel"])
    assert np.isfinite(p1).all() and np.isfinite(v1).all()


def adam_gradient(n, mode, gen, fixed):
    """mode "classes": per-element fixed sign and magnitude class (GRAD_CLASSES); "random": N(0,1), a new sign every step."""
    if mode == "random":
        return torch.randn(n, generator=gen)
    sign, cls = fixed
    mags = torch.empty(n)
    drawn = torch.randn(n, generator=gen).abs() * 1e-3
    for ci, c in enumerate(GRAD_CLASSES):
        sel = cls == ci
        mags[sel] = drawn[sel] if c is None else c
    return sign * mags


def check_adam_kernel(dev, n, view=False, hyper=ADAM_HYPER[0], p_init="zero", mode="classes", seed=0):
    """dream_adam_step_f32, one launch at a time: the launch is held to the float64 step of the kernel's OWN previous state, then the
    sequence continues from the kernel's state (errors do not compound).  The step count goes straight into the entry point."""
    name = "adam n=%d%s lr=%g b=(%g,%g) eps=%g p0=%s g=%s" % ((n, " view[1:]" if view else "") + tuple(hyper) + (p_init, mode))
    gen = torch.Generator().manual_seed(seed + n)
    (p, m, v, g), flats = _buffers(dev, n, view, 4)
    if p_init == "randn":
        p.copy_(to(dev, torch.randn(n, generator=gen)))
    else:
        p.zero_()
    m.zero_()
    v.zero_()
    fixed = (torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0), torch.randint(0, len(GRAD_CLASSES), (n,), generator=gen))
    worst = {"m": 0.0, "v": 0.0, "dp": 0.0, "v_rel": 0.0}
    lr, b1, b2, eps = hyper
    for t in ADAM_STEPS:
        g.copy_(to(dev, adam_gradient(n, mode, gen, fixed)))
        before = [x.clone() for x in (p, m, v)]
        ops.adam_step_(p, g, m, v, lr, b1, b2, eps, t)
        _hold_adam_launch(name, before, (p, m, v), g, hyper, t, worst)
    _guards_intact(flats, n)
    for key in ("m", "v", "dp"):
        _report("%s: %s" % (name, key), worst[key])
    print("step-check %s: worst |v - v_ref| / v_ref = %.3g" % (name, worst["v_rel"]))
    RATIOS["adam worst relative v deviation"] = max(RATIOS.get("adam worst relative v deviation", 0.0), worst["v_rel"])
    return worst


def check_adam_zero_gradient(dev, n, view=False):
    """g = 0 on m = v = 0: 0 / eps = 0, the parameter keeps its bits (a -0 included) and the moments stay 0."""
    gen = torch.Generator().manual_seed(n)
    (p, m, v, g), flats = _buffers(dev, n, view, 4)
    p0 = torch.randn(n, generator=gen)
    p0[0] = -0.0
    p.copy_(to(dev, p0))
    for x in (m, v, g):
        x.zero_()
    for t in (1, 1000):
        ops.adam_step_(p, g, m, v, 1e-4, 0.9, 0.999, 1e-8, t)
    _same_bits("adam zero gradient n=%d p" % n, p, p0)
    _same_bits("adam zero gradient n=%d m, v" % n, torch.stack([m, v]), torch.zeros(2, n))
    _guards_intact(flats, n)


def check_sgd_kernel(dev, n, view=False, lr=1e-4):
    name = "sgd n=%d%s lr=%g" % (n, " view[1:]" if view else "", lr)
    gen = torch.Generator().manual_seed(n + 5)
    (p, g), flats = _buffers(dev, n, view, 2)
    p.copy_(to(dev, torch.randn(n, generator=gen)))
    fixed = (torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0), torch.randint(0, len(GRAD_CLASSES), (n,), generator=gen))
    worst = 0.0
    for _ in range(2):
        g.copy_(to(dev, adam_gradient(n, "classes", gen, fixed)))
        p0, g64 = _np64(p), _np64(g)
        ops.sgd_step_(p, g, lr)
        p1 = _np64(p)
        ref = p0 - float(np.float32(lr)) * g64
        # p - lr g: the product rounds once, the difference once (half an ulp of the result)
        budget = U * np.abs(float(np.float32(lr)) * g64) + 0.5 * _ulp(p1)
        err = np.abs(p1 - ref)
        worst = max(worst, float((err / budget).max()))
        assert (err <= budget).all(), (name, worst)
    _guards_intact(flats, n)
    _report(name, worst)


# ---- HipAdam / HipSGD against torch.optim -----------------------------------------------------------------------------------------
def _small_module(dev, flat):
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3))       # 35, 7, 21, 3 parameters: none a multiple of 4
    net = net.to(dev) if dev != "cpu" else net
    if flat:
        data_parallel.flatten_module_(net)
        assert data_parallel.flat_is_intact(net)
    return net


OPT_CASES = ("plain", "lr_changes", "two_groups", "grad_none_once")


def _make_optimizer(kind, case, params, hip, lr):
    groups = [{"params": params[:2], "lr": lr}, {"params": params[2:], "lr": 3.0 * lr}] if case == "two_groups" else params
    if kind == "adam":
        return optim.HipAdam(groups, lr=lr) if hip else torch.optim.Adam(groups, lr=lr, foreach=False)
    return optim.HipSGD(groups, lr=lr) if hip else torch.optim.SGD(groups, lr=lr, foreach=False)


def check_optimizer(dev, kind, case, steps=5):
    """HipAdam / HipSGD on a flattened module (one launch over the flat buffer) and on an unflattened one (one launch per tensor)
    against torch.optim on float64 copies; the two paths run the same kernel on the same numbers: bit-identical."""
    lr = 1e-3 if kind == "adam" else 1e-2
    nets = {"flat": _small_module(dev, True), "per_tensor": _small_module(dev, False)}
    if kind == "adam":
        assert optim._flat_span([p.data for p in nets["flat"].parameters()]) is not None
        assert optim._flat_span([p.data for p in nets["per_tensor"].parameters()]) is None
    opts = {k: _make_optimizer(kind, case, list(n.parameters()), True, lr) for k, n in nets.items()}
    ref_params = [torch.nn.Parameter(p.detach().cpu().double().clone()) for p in nets["flat"].parameters()]
    ref_opt = _make_optimizer(kind, case, ref_params, False, lr)
    gen = torch.Generator().manual_seed(11)
    max_dp = [0.0] * len(ref_params)
    for step in range(1, steps + 1):
        grads = [torch.randn(p.shape, generator=gen) for p in ref_params]
        if case == "lr_changes" and step == 3:
            for o in list(opts.values()) + [ref_opt]:
                for group in o.param_groups:
                    group["lr"] = 0.37 * lr
        skip = 1 if (case == "grad_none_once" and step == 2) else None
        for net in nets.values():
            for i, p in enumerate(net.parameters()):
                p.grad = None if i == skip else to(dev, grads[i].clone())
        for i, p in enumerate(ref_params):
            p.grad = None if i == skip else grads[i].double()
        before = [p.detach().clone() for p in ref_params]
        for o in opts.values():
            o.step()
        ref_opt.step()
        max_dp = [max(a, float((b - p.detach()).abs().max())) for a, b, p in zip(max_dp, before, ref_params)]
        worst = 0.0
        for key, net in nets.items():
            for i, (p, r) in enumerate(zip(net.parameters(), ref_params)):
                p64, r64 = _np64(p), r.detach().numpy()
                # per step: the rounding of the stored parameter (half an ulp) and 32u of the largest update -- the kernel's own
                # budget is 12u of the update plus the moments' (the kernel checks), and the moments carry from step to step
                budget = step * (0.5 * _ulp(p64) + 32.0 * U * max_dp[i])
                err = np.abs(p64 - r64)
                worst = max(worst, float((err / budget).max()))
                assert (err <= budget).all(), "%s %s %s step %d parameter %d: %.3g budgets" % (kind, case, key, step, i, worst)
    _report("Hip%s %s vs torch.optim (float64)" % (kind.upper() if kind == "sgd" else "Adam", case), worst)
    flat_p, tens_p = list(nets["flat"].parameters()), list(nets["per_tensor"].parameters())
    _same_bits("Hip%s %s flat vs per-tensor parameters" % (kind, case), torch.cat([p.detach().reshape(-1) for p in flat_p]),
               torch.cat([p.detach().reshape(-1) for p in tens_p]))
    if kind == "adam":
        for key in ("exp_avg", "exp_avg_sq"):
            _same_bits("HipAdam %s flat vs per-tensor %s" % (case, key),
                       torch.cat([opts["flat"].state[p][key].reshape(-1) for p in flat_p]),
                       torch.cat([opts["per_tensor"].state[p][key].reshape(-1) for p in tens_p]))
        for o, ps in ((opts["flat"], flat_p), (opts["per_tensor"], tens_p)):
            counts = [int(o.state[p]["step"]) for p in ps]
            want = [steps - 1 if (case == "grad_none_once" and i == 1) else steps for i in range(len(ps))]
            assert counts == want and counts == [int(ref_opt.state[r]["step"]) for r in ref_params], (case, counts, want)


# ---- SoftArgmax -------------------------------------------------------------------------------------------------------------------------
SOFTARGMAX_BETAS = (0.5, 1.0, 5.0, 25.0, 100.0)
SOFTARGMAX_MAPS = ((1, 1), (3, 5), (9, 13), (33, 21), (100, 100))


def softargmax_reference(maps, beta, size_mult):
    """SoftArgmaxPavlo in float64: 7x7 average pool (zero padding, divisor 49), minus the per-map max, exp(beta_k .),
    / (sum + 1e-8), expected column (x) and row (y) index times size_mult.  maps [B,K,H,W], beta [K] -> [B,K,2]."""
    m = maps.double()
    b, k, h, w = m.shape
    pooled = F.avg_pool2d(m, 7, stride=1, padding=3, count_include_pad=True)
    flat = pooled.reshape(b, k, h * w)
    e = torch.exp(beta.double().view(1, k, 1) * (flat - flat.max(dim=2, keepdim=True).values))
    prob = (e / (e.sum(dim=2, keepdim=True) + 1e-8)).reshape(b, k, h, w)
    xs = torch.arange(w, dtype=torch.float64) * size_mult
    ys = torch.arange(h, dtype=torch.float64) * size_mult
    return torch.stack([(prob.sum(2) * xs).sum(2), (prob.sum(3) * ys).sum(2)], dim=2)


def _hold_softargmax(dev, name, maps, beta, size_mult):
    ref = softargmax_reference(maps, beta, size_mult).numpy()
    out = ops.softargmax(to(dev, maps), to(dev, beta), size_mult).cpu().numpy()
    assert out.shape == ref.shape and np.isfinite(out).all(), name
    tol = 1e-4 * max(1.0, float(np.abs(ref).max()))                    # the project's SoftArgmax tolerance (parity_checks.check_softargmax)
    ratio = _report("softargmax " + name, float(np.abs(out - ref).max()) / tol)
    assert ratio <= 1.0, (name, ratio)
    return ref


def check_softargmax_distinct_betas(dev, hw, size_mult):
    """K = 5 distinct betas on B = 2 frames (map n uses beta[n % K], neither beta[0] nor beta[n / K])."""
    h, w = hw
    g = torch.Generator().manual_seed(h * 1000 + w)
    maps = torch.randn(2, 5, h, w, generator=g)
    beta = torch.tensor(SOFTARGMAX_BETAS)
    ref = _hold_softargmax(dev, "%dx%d size_mult %g" % (h, w, size_mult), maps, beta, size_mult)
    if h * w >= 100:
        # the case can tell the betas apart: with beta[0] for every keypoint the reference itself moves by far more than the tolerance
        tol = 1e-4 * max(1.0, float(np.abs(ref).max()))
        assert float(np.abs(softargmax_reference(maps, beta[:1].expand(5), size_mult).numpy() - ref).max()) > 100 * tol


def check_softargmax_large_values(dev):
    """Values around 1e4 under beta 25: exp(25 x 1e4) overflows unless the per-map max is subtracted first.  The maps are 1e4 + 1000 N(0,1):
    pooled values differ by tens of units (times beta: hundreds of e-folds), so the 1e-3 that the fp32 sum of 49 such values is off by
    (times beta: 2.5 % of a weight that is already nothing) does not move the result."""
    g = torch.Generator().manual_seed(5)
    maps = 1e4 + 1000.0 * torch.randn(2, 5, 9, 13, generator=g)
    _hold_softargmax(dev, "values ~1e4, beta 25", maps, torch.full((5,), 25.0), 1.0)


def check_softargmax_constant_map(dev):
    """A constant map: the pooled map is flat inside and falls off at the zero-padded border; the result is its soft centroid."""
    maps = torch.full((2, 5, 9, 13), 0.75)
    ref = _hold_softargmax(dev, "constant map", maps, torch.tensor(SOFTARGMAX_BETAS), 2.5)
    assert np.allclose(ref[..., 0], 6.0 * 2.5) and np.allclose(ref[..., 1], 4.0 * 2.5)       # symmetric: the centre


# ---- glue kernels -------------------------------------------------------------------------------------------------------------------------
def check_add(dev, n):
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a[n - 1], b[n - 1] = 60.0, 40.5                       # the maximum sits in the last element: the scalar tail whenever n % 4 != 0
    want = a.numpy() + b.numpy()
    out, amax = ops.add(to(dev, a), to(dev, b), want_amax=True)
    _same_bits("add n=%d" % n, out, want)
    assert _amax_word(amax) == _f32_word(np.abs(want).max()) == _f32_word(100.5), (n, _amax_word(amax))
    out, none = ops.add(to(dev, a), to(dev, b))
    assert none is None
    _same_bits("add n=%d (no amax)" % n, out, want)
    dst = to(dev, a.clone())
    assert ops.add_(dst, to(dev, b)) is dst
    _same_bits("add_ n=%d" % n, dst, want)
    if n > 4:                                             # ... and in the vector body
        a[n - 1], b[n - 1], a[1] = 0.0, 0.0, -200.0
        want = a.numpy() + b.numpy()
        out, amax = ops.add(to(dev, a), to(dev, b), want_amax=True)
        _same_bits("add n=%d, maximum in the body" % n, out, want)
        assert _amax_word(amax) == _f32_word(np.abs(want).max())
    z = to(dev, torch.zeros(n))
    out, amax = ops.add(z, z, want_amax=True)
    _same_bits("add n=%d zeros" % n, out, np.zeros(n, dtype=np.float32))
    assert _amax_word(amax) == 0


def check_alignment_contract(dev):
    """dream_add_f32, dream_add_inplace_f32 and dream_relu_bwd_f32 move float4 unconditionally: a pointer that is not 16-byte aligned is
    an error return (no launch: the destination keeps its bits)."""
    n = 1003
    g = torch.Generator().manual_seed(0)
    flat = to(dev, torch.randn(n + 1, generator=g))
    off, ok, ok2 = flat[1:], to(dev, torch.randn(n, generator=g)), to(dev, torch.randn(n, generator=g))
    assert ops.ptr(off) % 16 == 4 and ops.ptr(ok) % 16 == 0 and ops.ptr(ok2) % 16 == 0
    kept_flat, kept_ok = flat.clone(), ok.clone()
    for args in ((off, ok, ok2), (ok, off, ok2), (ok, ok2, off)):
        with pytest.raises(RuntimeError, match="16-byte"):
            _hip.call("dream_add_f32", ops.ptr(args[0]), ops.ptr(args[1]), ops.ptr(args[2]), n, None, ops.stream())
        with pytest.raises(RuntimeError, match="16-byte"):
            _hip.call("dream_relu_bwd_f32", ops.ptr(args[0]), ops.ptr(args[1]), ops.ptr(args[2]), n, ops.stream())
    for args in ((off, ok), (ok, off)):
        with pytest.raises(RuntimeError, match="16-byte"):
            _hip.call("dream_add_inplace_f32", ops.ptr(args[0]), ops.ptr(args[1]), n, ops.stream())
    with pytest.raises(RuntimeError, match="16-byte"):
        ops.add(off, ok)
    with pytest.raises(RuntimeError, match="16-byte"):
        ops.add_(off, ok)
    with pytest.raises(RuntimeError, match="16-byte"):
        ops.relu_bwd_(off, ok)
    _same_bits("refused calls leave their operands alone", torch.cat([flat, ok]), torch.cat([kept_flat, kept_ok]))


def check_stage_input(dev, up, k, cpad):
    ci, b, hm, wm = 3, 2, 5, 3
    h, w = hm * up, wm * up
    g = torch.Generator().manual_seed(up * 100 + k + cpad)
    img, maps = torch.randn(b, ci, h, w, generator=g), torch.randn(b, k, hm, wm, generator=g)
    maps[1, k - 1, hm - 1, wm - 1] = -77.0
    cat = torch.cat([img, F.interpolate(maps, scale_factor=up, mode="nearest")], 1)
    want = torch.zeros(b, h, w, cpad)
    want[..., :ci + k] = cat.permute(0, 2, 3, 1)
    out, amax = ops.stage_input(to(dev, img), to(dev, maps), up, cpad, want_amax=True)
    _same_bits("stage_input up=%d K=%d Cpad=%d" % (up, k, cpad), out, want)
    assert _amax_word(amax) == _f32_word(77.0)
    out, none = ops.stage_input(to(dev, img), to(dev, maps), up, cpad)
    assert none is None
    _same_bits("stage_input up=%d K=%d Cpad=%d (no amax)" % (up, k, cpad), out, want)
    # backward: float64 sums over each up x up block of channels ci .. ci+k-1
    gr = torch.randn(b, h, w, cpad, generator=g)
    terms = gr[..., ci:ci + k].permute(0, 3, 1, 2).double().reshape(b, k, hm, up, wm, up)
    ref, mag = terms.sum((3, 5)).numpy(), terms.abs().sum((3, 5)).numpy()
    got = ops.stage_input_bwd(to(dev, gr), ci, k, up)
    assert tuple(got.shape) == (b, k, hm, wm)
    name = "stage_input_bwd up=%d K=%d Cpad=%d" % (up, k, cpad)
    # up^2 terms added one after another: up^2 - 1 roundings, held to up^2 u sum|terms|
    budget = up * up * U * mag
    ratio = _report(name, float((np.abs(_np64(got) - ref) / budget).max()))
    assert ratio <= 1.0, (name, ratio)
    # accumulate = 1 (no caller in the tree): added to what the output holds -- one more term, one more rounding
    pre = torch.randn(b, k, hm, wm, generator=g)
    acc = to(dev, pre.clone())
    _hip.call("dream_stage_input_bwd_f32", ops.ptr(to(dev, gr)), ops.ptr(acc), b, h, w, ci, k, up, cpad, 1, ops.stream())
    budget = up * up * U * (mag + pre.abs().double().numpy())
    ratio = _report(name + " accumulate", float((np.abs(_np64(acc) - (ref + pre.double().numpy())) / budget).max()))
    assert ratio <= 1.0, (name, ratio)


def check_stage_input_refuses_narrow_padding(dev):
    img, maps = to(dev, torch.zeros(2, 3, 5, 3)), to(dev, torch.zeros(2, 17, 5, 3))
    with pytest.raises(RuntimeError, match="Cpad"):
        ops.stage_input(img, maps, 1, 16)                     # 3 + 17 channels do not fit 16


def check_relu_bwd(dev, n):
    g = torch.Generator().manual_seed(n)
    dy, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    special = torch.tensor([0.0, -0.0, 1e-45, 1.1754944e-38, -1e-45, 1e-30], dtype=torch.float32)      # +0, -0, tiny positives (a denormal too)
    for start in (0, max(0, n - len(special))):                                      # in the vector body and in the scalar tail
        m = min(n - start, len(special))
        y[start:start + m] = special[:m]
    want = np.where(y.numpy() > 0, dy.numpy(), np.float32(0.0))
    d = to(dev, dy.clone())
    assert ops.relu_bwd_(d, to(dev, y)) is d
    _same_bits("relu_bwd n=%d" % n, d, want)


def check_upsample2_bwd(dev, shape):
    b, h, w, c = shape
    g = torch.Generator().manual_seed(h * w)
    dy = torch.randn(b, h, w, c, generator=g)
    terms = dy.double().reshape(b, h // 2, 2, w // 2, 2, c)
    ref, mag = terms.sum((2, 4)).numpy(), terms.abs().sum((2, 4)).numpy()
    got = ops.upsample2_bwd(to(dev, dy))
    assert tuple(got.shape) == (b, h // 2, w // 2, c)
    # (a + b) + (c + d): three additions, each within u of at most the sum of the magnitudes
    ratio = _report("upsample2_bwd %s" % (shape,), float((np.abs(_np64(got) - ref) / (3.0 * U * mag)).max()))
    assert ratio <= 1.0, (shape, ratio)


LAYOUT_C = (1, 7, 64, 65, 130)
LAYOUT_HW = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 4097: (17, 241)}


def check_layout(dev, c, hw):
    """NCHW <-> NHWC through the 64 x 64 LDS tile (ragged in both directions) and the zero-padding variant: pure data movement."""
    b, (h, w) = 2, LAYOUT_HW[hw]
    g = torch.Generator().manual_seed(c * 10000 + hw)
    x = torch.randn(b, c, h, w, generator=g)
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    _same_bits("nchw_to_nhwc C=%d HW=%d" % (c, hw), ops.nchw_to_nhwc(to(dev, x)), nhwc)
    _same_bits("nhwc_to_nchw C=%d HW=%d" % (c, hw), ops.nhwc_to_nchw(to(dev, nhwc)), x)
    for cpad in (ops.round_up(c + 1, 4), c + 31):
        want = torch.zeros(b, h, w, cpad)
        want[..., :c] = nhwc
        _same_bits("nchw_to_nhwc C=%d HW=%d cpad=%d" % (c, hw, cpad), ops.nchw_to_nhwc(to(dev, x), cpad=cpad), want)


def check_multi_copy(dev):
    """ops.MultiCopyPlan (dream_multi_copy_f32): the optimizer's gather of per-parameter gradients into its flat buffer -- aligned and
    unaligned sources, tensors longer than one 64 K chunk, the padding between the views untouched, repeated calls (the pointer ring)."""
    torch.manual_seed(0)
    sizes = [1, 3, 64, 65537, 200000, 7, 131072, 5]
    flat = to(dev, torch.zeros(sum((n + 63) // 64 * 64 for n in sizes)))
    views, o = [], 0
    for n in sizes:
        views.append(flat[o:o + n])
        o += (n + 63) // 64 * 64
    plan = ops.MultiCopyPlan(views)
    assert plan.nchunks == sum((n + 65535) // 65536 for n in sizes)
    for rep in range(6):
        srcs = [to(dev, torch.randn(n + 1))[1:] if (i + rep) % 2 else to(dev, torch.randn(n)) for i, n in enumerate(sizes)]    # every other source 4 bytes off
        assert plan.matches(srcs)
        plan.run(srcs)
        for v, s_ in zip(views, srcs):
            assert torch.equal(v, s_)
        o = 0
        for n in sizes:                                                   # the padding between the views stays zero
            pad = (n + 63) // 64 * 64
            assert float(flat[o + n:o + pad].abs().sum()) == 0.0
            o += pad
    assert not plan.matches(srcs[:-1]) and not plan.matches([t.double() for t in srcs])
