#!/usr/bin/env python
"""Whole-step A/B of train_activation_storage with train_precision="fp16": "fp32" (every saved activation fp32; the parent's step, its
kernels instruction-identical) against "fp16" (the encoder's half run stored as IEEE half and read as half by the backward),
alternating in ONE process so that clock and thermal drift hit both arms alike.  vgg_q, 128 frames of 400 x 400, net.train(): both
arms are warmed up, then --rounds rounds of --steps steps per arm are timed with device events.  Prints the per-round times, each arm's
spread, the ratio and torch.cuda.max_memory_allocated() of a step per arm; then, per distinct shape of the plain convs that read a half
input, the weight-gradient launch alone: the half-x kernel against the fp32-x kernel (csrc/wgrad_f16.hip), round-robin, with a check
that both give the same bits on a half-exact x.  --json FILE also writes the record as JSON.

    python tools/microbench_train_activation_storage.py [--rounds 5] [--steps 10] [--batch 128] [--res 400] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from dream_amd import ops  # noqa: E402
from microbench_train_precision import F16_PEAK_TFLOPS, build, timed  # noqa: E402

ARMS = ("fp32", "fp16")


def run_shapes(module, x):
    """Distinct (B, H, W, cin, cout) of the plain convs that read a half input, with how many entries have each, in plan order."""
    module.train_activation_storage = "fp16"
    with torch.no_grad():
        _, saved = module.run_forward(x, [p.detach() for p in module.plan_parameters()], True)
    shapes = {}
    for li in sorted(saved.half_in):
        mod, inp = module.plan_layers()[li][1], saved[li][0]
        key = tuple(int(v) for v in inp.shape[:3]) + (int(mod.weight.shape[1]), int(mod.weight.shape[0]))
        shapes[key] = shapes.get(key, 0) + 1
    return shapes


def layer_table(shapes, rounds, iters):
    rows = []
    gen = torch.Generator(device="cuda").manual_seed(0)
    for (b, h, w, cin, cout), n in shapes.items():
        xh = torch.randn((b, h, w, cin), device="cuda", generator=gen).relu_().half()
        xh[(xh != 0) & (xh.abs() < 2.0 ** -14)] = 0            # half-exact: both kernels multiply the same operand
        xf = xh.float()
        g = torch.randn((b, h, w, cout), device="cuda", generator=gen) * 1e-3
        ax, ag = ops.absmax(xf), ops.absmax(g)
        old, new = ops.conv3x3_wgrad_f16(xf, ax, g, ag, cout, cin), ops.conv3x3_wgrad_f16_x16(xh, g, ag, cout, cin)
        same = bool(torch.equal(old[0], new[0]) and torch.equal(old[1], new[1]))
        timed(lambda: ops.conv3x3_wgrad_f16(xf, ax, g, ag, cout, cin), iters)            # warm-up of both (clocks, workspace)
        timed(lambda: ops.conv3x3_wgrad_f16_x16(xh, g, ag, cout, cin), iters)
        t32, t16 = [], []
        for _ in range(rounds):
            t32.append(timed(lambda: ops.conv3x3_wgrad_f16(xf, ax, g, ag, cout, cin), iters))
            t16.append(timed(lambda: ops.conv3x3_wgrad_f16_x16(xh, g, ag, cout, cin), iters))
        m32, m16 = statistics.median(t32), statistics.median(t16)
        tflop = 2.0 * 9 * b * h * w * cin * cout * 1e-12
        rows.append(dict(shape=[b, h, w, cin, cout], entries=n, fp32_x_ms=m32, half_x_ms=m16, same_bits=same,
                         fp32_x_spread=(max(t32) - min(t32)) / m32, half_x_spread=(max(t16) - min(t16)) / m16,
                         fp32_x_fraction_of_f16_peak=tflop / (m32 * 1e-3) / F16_PEAK_TFLOPS,
                         half_x_fraction_of_f16_peak=tflop / (m16 * 1e-3) / F16_PEAK_TFLOPS,
                         splitk=ops.conv3x3_wgrad_f16_splitk(b, h, w, cin, cout)))
        del xh, xf, g, old, new
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--layer-iters", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the record to this file")
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 10, "at least 5 rounds of at least 10 steps"
    net, x, t = build(args.batch, args.res)
    module = net.model.module
    module.train_precision = "fp16"
    step = lambda: net.train([x], t)      # noqa: E731
    peak_bytes, half_peak = {}, None
    for arm in ARMS:                      # warm up both arms (packing, LDS attributes, allocator); the footprint of one step per arm
        module.train_activation_storage = arm
        timed(step, 2)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        timed(step, 1)
        peak_bytes[arm] = torch.cuda.max_memory_allocated()
        if arm == "fp16":
            half_peak = module.half_storage_peak()
    for arm in ARMS:                      # (empty_cache() above gave the arms' blocks back: let the allocator settle for both again)
        module.train_activation_storage = arm
        timed(step, 2)
    ms = {arm: [] for arm in ARMS}
    for _ in range(args.rounds):
        for arm in ARMS:
            module.train_activation_storage = arm
            ms[arm].append(timed(step, args.steps))
    module.train_activation_storage = "fp32"
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    spread = {arm: (max(v) - min(v)) / med[arm] for arm, v in ms.items()}
    print("vgg_q training, train_precision=fp16, %d frames of %d x %d, %d rounds of %d steps (ms per step), %s"
          % (args.batch, args.res, args.res, args.rounds, args.steps, torch.cuda.get_device_name(0)))
    for arm in ARMS:
        print("  train_activation_storage=%-5s %s | median %.2f ms = %.0f frames/s, spread %.1f %%, max_memory_allocated %.2f GiB"
              % (arm, " ".join("%.2f" % v for v in ms[arm]), med[arm], args.batch / med[arm] * 1e3, 100 * spread[arm],
                 peak_bytes[arm] / 2.0 ** 30))
    gain, worst = med["fp32"] / med["fp16"] - 1.0, max(spread.values())
    print("  fp16 vs fp32 storage: %+.1f %% frames/s, ratio %.3f (largest spread of an arm: %.1f %%) -> %s; footprint x %.3f; "
          "half_storage_peak() %.6g"
          % (100 * gain, med["fp32"] / med["fp16"], 100 * worst,
             "faster by more than the spread" if gain > worst else
             ("SLOWER by more than the spread" if -gain > worst else "within the spread"),
             peak_bytes["fp16"] / peak_bytes["fp32"], half_peak))
    record = {"rounds": args.rounds, "steps": args.steps, "batch": args.batch, "res": args.res, "device": torch.cuda.get_device_name(0),
              "ms_per_step": ms, "median_ms": med, "spread": spread, "frames_per_s": {a: args.batch / med[a] * 1e3 for a in ARMS},
              "ratio_fp32_over_fp16": med["fp32"] / med["fp16"], "max_memory_allocated": peak_bytes, "half_storage_peak": half_peak}
    rows = layer_table(run_shapes(module, x), args.rounds, args.layer_iters)
    module.train_activation_storage = "fp32"
    record["wgrad_layers"] = rows
    print("weight-gradient launch per shape of the run's plain convs: fp32 x against half x (median of %d rounds of %d launches, "
          "round-robin; fraction of the 2500 TFLOP/s fp16 MFMA peak)" % (args.rounds, args.layer_iters))
    print("  %-26s %3s  %9s %6s %6s  %9s %6s %6s  %6s %6s %s"
          % ("B x H x W x cin x cout", "n", "fp32-x ms", "peak", "spread", "half-x ms", "peak", "spread", "gain", "split", ""))
    tot32 = tot16 = 0.0
    for r in rows:
        tot32, tot16 = tot32 + r["entries"] * r["fp32_x_ms"], tot16 + r["entries"] * r["half_x_ms"]
        note = ("" if r["same_bits"] else "BITS DIFFER ") + ("half x SLOWER" if r["half_x_ms"] > r["fp32_x_ms"] else "")
        print("  %-26s %3d  %9.3f %6.3f %5.1f%%  %9.3f %6.3f %5.1f%%  %+5.1f%% %6d %s"
              % ("x".join(str(v) for v in r["shape"]), r["entries"], r["fp32_x_ms"], r["fp32_x_fraction_of_f16_peak"],
                 100 * r["fp32_x_spread"], r["half_x_ms"], r["half_x_fraction_of_f16_peak"], 100 * r["half_x_spread"],
                 100 * (r["fp32_x_ms"] / r["half_x_ms"] - 1.0), r["splitk"], note))
    print("  all such convs of a step: fp32 x %.2f ms, half x %.2f ms" % (tot32, tot16))
    record["wgrad_total_ms"] = {"fp32_x": tot32, "half_x": tot16}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
