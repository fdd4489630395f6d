#!/usr/bin/env python
"""Whole-step A/B of train_gradient_storage with train_precision="fp16" and train_activation_storage="fp16" in both arms: "fp32" (every
data gradient fp32; the parent's step, its kernels instruction-identical) against "fp16" (the data gradients of the encoder's half run
stored as IEEE half times one power of two per backward pass), alternating in ONE process so that clock and thermal drift hit both arms
alike.  vgg_q, 128 frames of 400 x 400, net.train(): both arms are warmed up, then --rounds rounds of --steps steps per arm are timed
with device events.  Prints the per-round times, each arm's spread, the ratio and torch.cuda.max_memory_allocated() of a step per arm;
then, per reader of the run (distinct shapes once), each launch the switch replaces against its replacement, round-robin: the data
gradient (entry / interior / exit form against the fp32 launch, which behind a pool is preceded by an absmax pass over g), the weight
gradient (half dy against fp32 dy) and, per pool, its backward.  --json FILE also writes the record as JSON.

    python tools/microbench_train_gradient_storage.py [--rounds 5] [--steps 10] [--batch 128] [--res 400] [--json FILE]"""
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
from microbench_train_precision import build, timed  # noqa: E402

ARMS = ("fp32", "fp16")


def run_launches(module, x):
    """Per reader of the half run and per pool, in backward order: (role, B, H, W, cin, cout, masked) -> how many entries."""
    module.train_gradient_storage = "fp16"
    with torch.no_grad():
        _, saved = module.run_forward(x, [p.detach() for p in module.plan_parameters()], True)
    layers, out = module.plan_layers(), {}
    for li in range(len(layers) - 1, 0, -1):
        kind, mod, flags = layers[li]
        inp = saved[li][0]
        b, h, w = (int(v) for v in inp.shape[:3])
        if kind == "pool" and li in saved.grad16:
            key = ("pool", b, h, w, int(inp.shape[3]), int(inp.shape[3]), True)
        elif li in saved.half_in:
            role = "entry" if li not in saved.grad16 else ("exit" if li - 1 not in saved.grad16 else "interior")
            key = (role, b, h, w, int(mod.weight.shape[1]), int(mod.weight.shape[0]), layers[li - 1][0] != "pool")
        else:
            continue
        out[key] = out.get(key, 0) + 1
    return out


def _ab(old, new, rounds, iters):
    timed(old, iters)
    timed(new, iters)
    t_old, t_new = [], []
    for _ in range(rounds):
        t_old.append(timed(old, iters))
        t_new.append(timed(new, iters))
    return statistics.median(t_old), statistics.median(t_new), max((max(t) - min(t)) / statistics.median(t) for t in (t_old, t_new))


def layer_table(launches, rounds, iters):
    rows = []
    gen = torch.Generator(device="cuda").manual_seed(0)
    e_amax = ops.absmax(torch.full((8,), 3e-3, device="cuda"))
    for (role, b, h, w, cin, cout, masked), n in launches.items():
        xh = torch.randn((b, h, w, cin), device="cuda", generator=gen).relu_().half()           # the saved input: x of the weight gradient, the mask
        if role == "pool":
            gh = torch.randn((b, h // 2, w // 2, cin), device="cuda", generator=gen).half()
            g32 = gh.float()
            old, new, spread = _ab(lambda: ops.maxpool2_bwd_x16(g32, xh, relu=True), lambda: ops.maxpool2_bwd_x16_dy16(gh, xh, relu=True),
                                   rounds, iters)
            rows.append(dict(role=role, shape=[b, h, w, cin, cout], entries=n, launch="pool backward", old_ms=old, new_ms=new, spread=spread))
            del xh, gh, g32
            torch.cuda.empty_cache()
            continue
        gh = (torch.randn((b, h, w, cout), device="cuda", generator=gen) * 100).half()
        g32 = gh.float()
        wt = torch.randn((cout, cin, 3, 3), device="cuda", generator=gen) * 0.05
        p16 = ops.pack_conv_weight_f16(wt, 1)
        ag = ops.absmax(g32)
        mask = xh if masked else None
        if masked:
            old_d = lambda: ops.conv2d_f16_mask16(g32, ag, p16, p16[3], 3, xh)                   # noqa: E731
        else:                                                                                     # behind a pool: one absmax pass, then the conv
            old_d = lambda: ops.conv2d_f16(g32, ops.absmax(g32), p16, p16[3], 3)                 # noqa: E731
        if role == "entry":
            new_d = lambda: ops.conv2d_f16_g16_entry(g32, ag, p16, p16[3], 3, e_amax, relu_mask=mask)      # noqa: E731
        elif role == "exit":
            new_d = lambda: ops.conv2d_f16_g16_exit(gh, p16, p16[3], 3, e_amax, mask)            # noqa: E731
        else:
            new_d = lambda: ops.conv2d_f16_g16(gh, p16, p16[3], 3, relu_mask=mask)               # noqa: E731
        old, new, spread = _ab(old_d, new_d, rounds, iters)
        rows.append(dict(role=role, shape=[b, h, w, cin, cout], entries=n, old_ms=old, new_ms=new, spread=spread,
                         launch="data gradient%s" % ("" if masked else " (+ absmax, behind a pool)")))
        if role != "entry":                                                                       # (the boundary conv keeps today's x16 launch)
            old, new, spread = _ab(lambda: ops.conv3x3_wgrad_f16_x16(xh, g32, ag, cout, cin),
                                   lambda: ops.conv3x3_wgrad_f16_x16_dy16(xh, gh, e_amax, cout, cin), rounds, iters)
            rows.append(dict(role=role, shape=[b, h, w, cin, cout], entries=n, launch="weight gradient", old_ms=old, new_ms=new, spread=spread))
        del xh, gh, g32, wt, p16
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
    module.train_precision = module.train_activation_storage = "fp16"
    step = lambda: net.train([x], t)      # noqa: E731
    peak_bytes, grad_peak = {}, None
    for arm in ARMS:                      # warm up both arms (packing, LDS attributes, allocator); the footprint of one step per arm
        module.train_gradient_storage = arm
        timed(step, 2)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        timed(step, 1)
        peak_bytes[arm] = torch.cuda.max_memory_allocated()
        if arm == "fp16":
            grad_peak = module.half_gradient_peak()
    for arm in ARMS:                      # (empty_cache() above gave the arms' blocks back: let the allocator settle for both again)
        module.train_gradient_storage = arm
        timed(step, 2)
    ms = {arm: [] for arm in ARMS}
    for _ in range(args.rounds):
        for arm in ARMS:
            module.train_gradient_storage = arm
            ms[arm].append(timed(step, args.steps))
    module.train_gradient_storage = "fp32"
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    spread = {arm: (max(v) - min(v)) / med[arm] for arm, v in ms.items()}
    print("vgg_q training, train_precision=fp16, train_activation_storage=fp16, %d frames of %d x %d, %d rounds of %d steps (ms per step), %s"
          % (args.batch, args.res, args.res, args.rounds, args.steps, torch.cuda.get_device_name(0)))
    for arm in ARMS:
        print("  train_gradient_storage=%-5s %s | median %.2f ms = %.0f frames/s, spread %.1f %%, max_memory_allocated %.2f GiB"
              % (arm, " ".join("%.2f" % v for v in ms[arm]), med[arm], args.batch / med[arm] * 1e3, 100 * spread[arm],
                 peak_bytes[arm] / 2.0 ** 30))
    gain, worst = med["fp32"] / med["fp16"] - 1.0, max(spread.values())
    print("  fp16 vs fp32 gradients: %+.1f %% frames/s, ratio %.3f (largest spread of an arm: %.1f %%) -> %s; footprint x %.3f; "
          "half_gradient_peak() %.6g"
          % (100 * gain, med["fp32"] / med["fp16"], 100 * worst,
             "faster by more than the spread" if gain > worst else
             ("SLOWER by more than the spread" if -gain > worst else "within the spread"),
             peak_bytes["fp16"] / peak_bytes["fp32"], grad_peak))
    record = {"rounds": args.rounds, "steps": args.steps, "batch": args.batch, "res": args.res, "device": torch.cuda.get_device_name(0),
              "ms_per_step": ms, "median_ms": med, "spread": spread, "frames_per_s": {a: args.batch / med[a] * 1e3 for a in ARMS},
              "ratio_fp32_over_fp16": med["fp32"] / med["fp16"], "max_memory_allocated": peak_bytes, "half_gradient_peak": grad_peak}
    rows = layer_table(run_launches(module, x), args.rounds, args.layer_iters)
    module.train_gradient_storage = "fp32"
    record["launches"] = rows
    print("per launch of the run, in backward order: what the fp32 arm launches against what replaces it (median ms per launch of %d "
          "rounds of %d launches, round-robin)" % (args.rounds, args.layer_iters))
    print("  %-9s %-26s %2s  %-42s %9s %9s %7s %6s" % ("form", "B x H x W x cin x cout", "n", "launch", "fp32-g ms", "half-g ms", "gain", "spread"))
    tot_old = tot_new = 0.0
    for r in rows:
        tot_old, tot_new = tot_old + r["entries"] * r["old_ms"], tot_new + r["entries"] * r["new_ms"]
        print("  %-9s %-26s %2d  %-42s %9.3f %9.3f %+6.1f%% %5.1f%% %s"
              % (r["role"], "x".join(str(v) for v in r["shape"]), r["entries"], r["launch"], r["old_ms"], r["new_ms"],
                 100 * (r["old_ms"] / r["new_ms"] - 1.0), 100 * r["spread"], "half g SLOWER" if r["new_ms"] > r["old_ms"] else ""))
    print("  all such launches of a step: fp32 gradients %.2f ms, half gradients %.2f ms" % (tot_old, tot_new))
    record["launch_total_ms"] = {"fp32_g": tot_old, "half_g": tot_new}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
