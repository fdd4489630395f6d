#!/usr/bin/env python
"""Whole-step and per-layer A/B of activation_storage with precision="fp16": activations in HBM as fp32 (the default) against IEEE
half, round-robin in ONE process so that clock and thermal drift hit both arms alike.  For each workload (vgg_q, 128 frames of
400 x 400; vgg_f, 32 frames) both arms are warmed up, then --rounds rounds of --steps net.inference() calls per arm are timed with
device events; torch.cuda.max_memory_allocated is taken per arm.  Then four layers of the vgg_q step on their own, the same way:
the first conv, 64->64 @ 400^2 + pool, 128->128 @ 200^2 + pool, 512->512 @ 50^2.

    python tools/microbench_activation_storage.py [--rounds 5] [--steps 20] [--workloads vgg_q:128,vgg_f:32] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from dream_amd import ops  # noqa: E402
from microbench_precision import build, timed  # noqa: E402

ARMS = ("fp32", "fp16")


def events(fn, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def report(ms, unit_count=None):
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    spread = {arm: (max(v) - min(v)) / med[arm] for arm, v in ms.items()}
    for arm in ARMS:
        rate = " = %.0f frames/s" % (unit_count / med[arm] * 1e3) if unit_count else ""
        print("  storage %-5s %s | median %.3f ms%s, spread %.1f %%" % (arm, " ".join("%.3f" % t for t in ms[arm]), med[arm], rate, 100 * spread[arm]))
    gain, worst = med["fp32"] / med["fp16"] - 1.0, max(spread.values())
    print("  storage fp16 vs fp32: %+.1f %% (largest spread of a round: %.1f %%) -> %s"
          % (100 * gain, 100 * worst, "faster by more than the spread" if gain > worst else "NOT faster by more than the spread"))
    return med, spread


def whole_step(arch, batch, res, rounds, steps):
    net, x = build(arch, batch, res)
    mod = net.model.module
    mod.precision = "fp16"
    peak_mem = {}
    with torch.no_grad():
        for arm in ARMS:
            mod.activation_storage = arm
            timed(net, x, 2)
        ms = {arm: [] for arm in ARMS}
        for r in range(rounds):
            for arm in ARMS:
                mod.activation_storage = arm
                if r == 0:
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
                ms[arm].append(timed(net, x, steps))
                if r == 0:
                    peak_mem[arm] = torch.cuda.max_memory_allocated()
        mod.activation_storage = "fp16"
        net.inference(x)
        stored_peak = mod.half_storage_peak()
    mod.activation_storage, mod.precision = "fp32", "fp32"
    print("%s, %d frames of %d x %d, precision fp16, %d rounds of %d steps (ms per step)" % (arch, batch, res, res, rounds, steps))
    med, spread = report(ms, batch)
    print("  max_memory_allocated: storage fp32 %.2f GiB, storage fp16 %.2f GiB; half_storage_peak %.4g"
          % (peak_mem["fp32"] / 2 ** 30, peak_mem["fp16"] / 2 ** 30, stored_peak))
    del net, x
    torch.cuda.empty_cache()
    return {"batch": batch, "res": res, "ms_per_step": ms, "median_ms": med, "spread": spread, "max_memory_allocated": peak_mem,
            "half_storage_peak": stored_peak}


def layer(name, b, h, cin, cout, flags, rounds, steps):
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).cuda()
    bias = torch.randn(cout, generator=g).cuda()
    if cin == 3:
        x = torch.randn(b, 3, h, h, generator=g).cuda()
        arms = {"fp32": lambda: ops.conv3x3_first_amax(x, w, bias, relu=True), "fp16": lambda: ops.conv3x3_first_f16(x, w, bias, relu=True)}
    else:
        x16 = torch.randn(b, h, h, cin, generator=g).half().cuda()
        x32 = x16.float()
        amax, p16 = ops.absmax(x32), ops.pack_conv_weight_f16(w, 0)
        arms = {"fp32": lambda: ops.conv2d_f16(x32, amax, p16, cout, 3, None, bias, None, flags),
                "fp16": lambda: ops.conv2d_f16_act16(x16, p16, cout, 3, None, bias, flags)}
    for arm in ARMS:
        events(arms[arm], 2)
    ms = {arm: [] for arm in ARMS}
    for _ in range(rounds):
        for arm in ARMS:
            ms[arm].append(events(arms[arm], steps))
    print("layer %s, %d frames (ms per launch)" % (name, b))
    med, spread = report(ms)
    torch.cuda.empty_cache()
    return {"ms_per_launch": ms, "median_ms": med, "spread": spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--workloads", default="vgg_q:128,vgg_f:32")
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--json", default=None, help="also write the record to this file")
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 20, "at least 5 rounds of at least 20 steps"
    record = {"rounds": args.rounds, "steps": args.steps, "device": torch.cuda.get_device_name(0), "workloads": {}, "layers": {}}
    for item in args.workloads.split(","):
        arch, batch = item.split(":")[0], int(item.split(":")[1])
        record["workloads"][arch] = whole_step(arch, batch, args.res, args.rounds, args.steps)
    if not args.no_layers:
        relu, pool = ops.CONV_RELU, ops.CONV_RELU | ops.CONV_POOL2
        for name, h, cin, cout, flags in (("first conv 3->64 @ 400^2", 400, 3, 64, relu), ("64->64 @ 400^2 + pool", 400, 64, 64, pool),
                                          ("128->128 @ 200^2 + pool", 200, 128, 128, pool), ("512->512 @ 50^2", 50, 512, 512, relu)):
            record["layers"][name] = layer(name, 128, h, cin, cout, flags, args.rounds, args.steps)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
