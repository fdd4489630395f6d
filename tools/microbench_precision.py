#!/usr/bin/env python
"""Whole-step A/B of the inference precisions: fp32 (Winograd on the fp32 MFMA), fp16x3 (split precision) and fp16 (plain fp16
operands), round-robin in ONE process so that clock and thermal drift hit every arm alike.  For each workload (vgg_q, 128 frames of
400 x 400; resnet_f, 32 frames) every arm is warmed up, then --rounds rounds of --steps net.inference() calls per arm are timed
with device events.  Prints the per-round times, each arm's spread and the ratios; --json FILE also writes them as JSON.

    python tools/microbench_precision.py [--rounds 5] [--steps 20] [--workloads vgg_q:128,resnet_f:32] [--json FILE]"""
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

ARMS = ("fp32", "fp16x3", "fp16")
VGG_Q_STEP_TFLOP = 18.15            # algorithmic conv work of one vgg_q step at 128 frames of 400 x 400
F16_PEAK_TFLOPS = 2500.0


def build(arch, batch, res):
    n_kp, manip = bench.ARCH_K[arch]
    cfg = dream_amd.default_network_config(arch, manip, batch_size=batch)
    cfg["training"]["config"]["net_input_resolution"] = [res, res]
    cfg["training"]["platform"]["gpu_ids"] = [0]
    with contextlib.redirect_stdout(io.StringIO()):
        net = dream_amd.create_network_from_config_data(cfg)
    net.model.load_state_dict(bench.synthetic_weights(net.model.state_dict()))
    net.enable_evaluation()
    x = torch.from_numpy(cases.image_batch(batch, res, res, seed=0)).cuda()
    return net, x


def timed(net, x, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        net.inference(x)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--workloads", default="vgg_q:128,resnet_f:32")
    ap.add_argument("--json", default=None, help="also write the record to this file")
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 20, "at least 5 rounds of at least 20 steps"
    record = {"rounds": args.rounds, "steps": args.steps, "device": torch.cuda.get_device_name(0), "workloads": {}}
    for item in args.workloads.split(","):
        arch, batch = item.split(":")[0], int(item.split(":")[1])
        net, x = build(arch, batch, args.res)
        with torch.no_grad():
            for arm in ARMS:                                   # warm up every shape of every arm (packing, LDS attributes, allocator)
                net.model.module.precision = arm
                timed(net, x, 2)
            ms = {arm: [] for arm in ARMS}
            for _ in range(args.rounds):
                for arm in ARMS:
                    net.model.module.precision = arm
                    ms[arm].append(timed(net, x, args.steps))
        net.model.module.precision = "fp32"
        med = {arm: statistics.median(v) for arm, v in ms.items()}
        spread = {arm: (max(v) - min(v)) / med[arm] for arm, v in ms.items()}
        print("%s, %d frames of %d x %d, %d rounds of %d steps (ms per step)" % (arch, batch, args.res, args.res, args.rounds, args.steps))
        for arm in ARMS:
            print("  %-7s %s | median %.2f ms = %.0f frames/s, spread %.1f %%"
                  % (arm, " ".join("%.2f" % t for t in ms[arm]), med[arm], batch / med[arm] * 1e3, 100 * spread[arm]))
        worst = max(spread.values())
        gain = med["fp16x3"] / med["fp16"] - 1.0
        print("  fp16 vs fp16x3: %+.1f %% frames/s (largest spread of a round: %.1f %%) -> %s"
              % (100 * gain, 100 * worst, "faster by more than the spread" if gain > worst else "NOT faster by more than the spread"))
        print("  fp16 vs fp32:   %+.1f %% frames/s" % (100 * (med["fp32"] / med["fp16"] - 1.0)))
        entry = {"batch": batch, "res": args.res, "ms_per_step": ms, "median_ms": med, "spread": spread,
                 "frames_per_s": {arm: batch / med[arm] * 1e3 for arm in ARMS}}
        if arch == "vgg_q" and batch == 128 and args.res == 400:
            frac = VGG_Q_STEP_TFLOP / (med["fp16"] * 1e-3) / F16_PEAK_TFLOPS
            entry["fp16_fraction_of_f16_peak"] = frac
            print("  fp16 whole step: %.2f TFLOP in %.2f ms = %.1f %% of the %.0f TFLOP/s fp16 matrix peak"
                  % (VGG_Q_STEP_TFLOP, med["fp16"], 100 * frac, F16_PEAK_TFLOPS))
        record["workloads"][arch] = entry
        del net, x
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
