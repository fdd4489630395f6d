#!/usr/bin/env python
"""Whole-step A/B of train_upsample_precision: "fp32" (the convs behind nn.Upsample(2) on the fp32 Winograd / nine-position kernels) and
"fp16" (their three products on the fp16 matrix cores, as the equivalent 4x4 transposed conv), alternating in ONE process so that clock and
thermal drift hit both arms alike.  vgg_q, 128 frames of 400 x 400, net.train(), with train_precision, train_activation_storage and
train_gradient_storage all "fp16" in both arms: both arms are warmed up, then --rounds rounds of --steps steps per arm are timed with device
events.  Prints the per-round times, each arm's spread and the ratio; then each covered launch (forward, data gradient, weight gradient of
every covered conv) against what the fp32 path chooses for it, in ms; then the same whole-step A/B for vgg with full_output at
--full-batch frames (four covered convs, two of them on 200^2 and 400^2 maps).  --json FILE also writes the record as JSON.

    python tools/microbench_train_upsample_precision.py [--rounds 5] [--steps 10] [--batch 128] [--res 400] [--full-batch 32] [--json FILE]"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402
import bench  # noqa: E402
import cases  # noqa: E402
import dream_amd  # noqa: E402
from dream_amd import ops  # noqa: E402

ARMS = ("fp32", "fp16")


def build(batch, res, full_output=False):
    n_kp, manip = bench.ARCH_K["vgg_q"]
    cfg = dream_amd.default_network_config("vgg_q", manip, batch_size=batch)
    if full_output:                       # the quarter-resolution hourglass with the two further upsample blocks: maps at input resolution
        cfg["architecture"].update(full_output=True, deconv_decoder=False)
    cfg["training"]["config"]["net_input_resolution"] = [res, res]
    cfg["training"]["platform"]["gpu_ids"] = [0]
    with contextlib.redirect_stdout(io.StringIO()):
        net = dream_amd.create_network_from_config_data(cfg)
    net.model.load_state_dict(bench.synthetic_weights(net.model.state_dict()))
    net.enable_training()
    m = net.model.module
    m.train_precision = m.train_activation_storage = m.train_gradient_storage = "fp16"
    x = torch.from_numpy(cases.image_batch(batch, res, res, seed=0)).cuda()
    ow, oh = net.trained_net_output_resolution()
    t = torch.from_numpy(cases.target_batch(batch, n_kp, (ow, oh), in_wh=(res, res), seed=0)).cuda()
    return net, x, t


def timed(fn, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def step_ab(net, x, t, rounds, steps, what):
    module = net.model.module
    step = lambda: net.train([x], t)      # noqa: E731
    for arm in ARMS:                      # warm up every shape of both arms (packing, LDS attributes, allocator)
        module.train_upsample_precision = arm
        timed(step, 2)
    ms = {arm: [] for arm in ARMS}
    for _ in range(rounds):
        for arm in ARMS:
            module.train_upsample_precision = arm
            ms[arm].append(timed(step, steps))
    module.train_upsample_precision = "fp32"
    batch = int(x.shape[0])
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    spread = {arm: (max(v) - min(v)) / med[arm] for arm, v in ms.items()}
    print("%s, %d frames of %d x %d, %d rounds of %d steps (ms per step), %s"
          % (what, batch, int(x.shape[2]), int(x.shape[3]), rounds, steps, torch.cuda.get_device_name(0)))
    for arm in ARMS:
        print("  train_upsample_precision=%-5s %s | median %.2f ms = %.0f frames/s, spread %.1f %%"
              % (arm, " ".join("%.2f" % v for v in ms[arm]), med[arm], batch / med[arm] * 1e3, 100 * spread[arm]))
    gain, worst = med["fp32"] / med["fp16"] - 1.0, max(spread.values())
    print("  fp16 vs fp32: %+.1f %% frames/s, ratio %.3f (largest spread of an arm: %.1f %%) -> %s"
          % (100 * gain, med["fp32"] / med["fp16"], 100 * worst,
             "faster by more than the spread" if gain > worst else "NOT faster by more than the spread"))
    return {"batch": batch, "ms_per_step": ms, "median_ms": med, "spread": spread, "ratio_fp32_over_fp16": med["fp32"] / med["fp16"]}


def covered(module, x):
    """[(name, module, (B, H, W) of the low-resolution input)] of the plan's covered convs."""
    with torch.no_grad():
        _, saved = module.run_forward(x, [p.detach() for p in module.plan_parameters()], True)
    out = []
    for (kind, cname, child, flags), (_, mod, _), (inp, _) in zip(module._plan, module.plan_layers(), saved):
        if mod is not None and module._half_ups_entry(kind, mod, flags, inp.shape[3]):
            out.append(("%s.%s" % (cname, child), mod, tuple(int(v) for v in inp.shape[:3])))
    return out


def launch_table(module, entries, rounds, iters):
    """Each covered launch against what the fp32 path chooses for it -> rows of (layer, launch, fp32 ms, fp16 ms)."""
    rows = []
    gen = torch.Generator(device="cuda").manual_seed(0)
    for name, mod, (b, h, w) in entries:
        cout, cin = int(mod.weight.shape[0]), int(mod.weight.shape[1])
        inp = torch.randn((b, h, w, cin), device="cuda", generator=gen)
        g = torch.randn((b, 2 * h, 2 * w, cout), device="cuda", generator=gen) * 1e-3
        ax, ag = ops.absmax(inp), ops.absmax(g)
        bias = mod.bias.detach()
        pk4, p16b = module._packed.get(mod.weight, "ups_f16"), module._packed.get(mod.weight, "ups_f16b")
        pairs = [
            ("forward", lambda: module._ups_conv(mod, 0, inp, bias, ops.CONV_RELU),
             lambda: ops.conv_transpose4x4s2_f16(inp, ax, pk4, pk4[3], None, bias, ops.CONV_RELU, direct_taps=36)),
            ("dgrad", lambda: module._ups_conv(mod, 1, g), lambda: ops.conv_transpose4x4s2_dgrad_f16(g, ag, p16b, cin)),
            ("wgrad", lambda: module._wgrad_fp32(inp, g, cout, cin, ops.CONV_UPSAMPLE2X),
             lambda: ops.upsample_conv3x3_wgrad_f16(inp, ax, g, ag, cout, cin)),
        ]
        for launch, f32, f16 in pairs:
            f32(), f16()
            t32, t16 = [], []
            for _ in range(rounds):
                t32.append(timed(f32, iters))
                t16.append(timed(f16, iters))
            rows.append(dict(layer=name, shape=[b, h, w, cin, cout], launch=launch, fp32_ms=statistics.median(t32), fp16_ms=statistics.median(t16),
                             fp32_spread=(max(t32) - min(t32)) / statistics.median(t32), fp16_spread=(max(t16) - min(t16)) / statistics.median(t16),
                             splitk=ops.upsample_conv3x3_wgrad_f16_splitk(b, h, w, cin, cout)))
        del inp, g
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--full-batch", type=int, default=32, help="frames of the vgg full_output arm (0: skip it)")
    ap.add_argument("--layer-iters", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the record to this file")
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 10, "at least 5 rounds of at least 10 steps"
    record = {"rounds": args.rounds, "steps": args.steps, "res": args.res, "device": torch.cuda.get_device_name(0)}
    net, x, t = build(args.batch, args.res)
    record["vgg_q"] = step_ab(net, x, t, args.rounds, args.steps,
                              "vgg_q training (train_precision, train_activation_storage, train_gradient_storage = fp16)")
    module = net.model.module
    rows = launch_table(module, covered(module, x), args.rounds, args.layer_iters)
    record["launches"] = rows
    print("covered launches against the fp32 path's choice (median of %d rounds of %d launches, ms)" % (args.rounds, args.layer_iters))
    print("  %-16s %-26s %-8s %9s %9s %7s %6s  %s" % ("layer", "B x H x W x cin x cout", "launch", "fp32 ms", "fp16 ms", "ratio", "split", ""))
    tot32 = tot16 = 0.0
    for r in rows:
        tot32, tot16 = tot32 + r["fp32_ms"], tot16 + r["fp16_ms"]
        lost = r["fp16_ms"] > r["fp32_ms"] * (1.0 + max(r["fp32_spread"], r["fp16_spread"]))
        print("  %-16s %-26s %-8s %9.3f %9.3f %7.2f %6s  %s"
              % (r["layer"], "x".join(str(v) for v in r["shape"]), r["launch"], r["fp32_ms"], r["fp16_ms"], r["fp32_ms"] / r["fp16_ms"],
                 r["splitk"] if r["launch"] == "wgrad" else "", "fp16 SLOWER by more than the spread" if lost else ""))
    print("  all covered launches of a step: fp32 %.2f ms, fp16 %.2f ms" % (tot32, tot16))
    record["launch_total_ms"] = {"fp32": tot32, "fp16": tot16}
    del net, x, t, module
    torch.cuda.empty_cache()
    if args.full_batch:
        net, x, t = build(args.full_batch, args.res, full_output=True)
        assert net.model.module.full_output
        record["vgg_full_output"] = step_ab(net, x, t, args.rounds, args.steps, "vgg (full_output) training, the same three switches at fp16")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
