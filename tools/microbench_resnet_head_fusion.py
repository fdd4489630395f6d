#!/usr/bin/env python
"""Whole-step and per-piece A/B of ResnetSimple.inference_head_fusion with precision="fp16" and inference_activation_storage="fp16": the
last decoder stage and the head as two launches ("off": the parent's code path, kernels instruction-identical) against the fused entry
("on"), round-robin in ONE process so that clock and thermal drift hit both arms alike.  For each workload (resnet_f, 32 frames of
400 x 400; resnet_h, 128 frames; one frame of each replayed as a hipGraph with inference_conv_ksplit="auto") both arms are warmed up,
then --rounds rounds of --steps net.inference() calls per arm are timed with device events; torch.cuda.max_memory_allocated is taken
per arm in an untimed pass before them (emptying the allocator's cache inside a timed round costs that round its allocations).  Then
the piece "last stage + head" on its own at 32 frames of resnet_f (208 x 208 x 256 -> 17 maps of 416 x 416), the same way, and the
fused entry's maps compared bit for bit with the pair's on the timed inputs.

    python tools/microbench_resnet_head_fusion.py [--rounds 5] [--steps 20]
                                                  [--workloads resnet_f:32,resnet_h:128,resnet_f:1:graph,resnet_h:1:graph] [--json FILE]"""
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
from microbench_activation_storage import events  # noqa: E402
from microbench_precision import build, timed  # noqa: E402

ARMS = ("off", "on")


def report(ms, unit_count=None):
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    spread = {arm: (max(v) - min(v)) / med[arm] for arm, v in ms.items()}
    for arm in ARMS:
        rate = " = %.0f frames/s" % (unit_count / med[arm] * 1e3) if unit_count else ""
        print("  head fusion %-3s %s | median %.3f ms%s, spread %.1f %%" % (arm, " ".join("%.3f" % t for t in ms[arm]), med[arm], rate, 100 * spread[arm]))
    gain, worst = med["off"] / med["on"] - 1.0, max(spread.values())
    verdict = "faster by more than the spread" if gain > worst else ("SLOWER by more than the spread" if -gain > worst else "a tie within the spread")
    print("  head fusion on vs off: %+.1f %% (largest spread of a round: %.1f %%) -> %s" % (100 * gain, 100 * worst, verdict))
    return med, spread


def whole_step(arch, batch, res, rounds, steps, graph=False):
    net, x = build(arch, batch, res)
    mod = net.model.module
    mod.precision = mod.inference_activation_storage = "fp16"
    mod.inference_conv_ksplit = "auto" if graph else "off"
    net.hip_graph = graph
    peak_mem, fused = {}, {}
    with torch.no_grad():
        for arm in ARMS:
            mod.inference_head_fusion = arm
            timed(net, x, 3)                                   # (with hip_graph: capture + replays)
            if not graph:                                      # the arm's peak, in a pass of its own: emptying the cache costs the next calls
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                timed(net, x, 2)
                peak_mem[arm] = torch.cuda.max_memory_allocated()
        for arm in ARMS:                                       # (the allocator's blocks of both arms are cached again)
            mod.inference_head_fusion = arm
            timed(net, x, 3)
        ms = {arm: [] for arm in ARMS}
        for r in range(rounds):
            for arm in ARMS:
                mod.inference_head_fusion = arm
                ms[arm].append(timed(net, x, steps))
        # which branch the "on" walk took (eager, counted once)
        net.hip_graph = False
        names, call = [], ops.call

        def spy(name, *args):
            names.append(name)
            return call(name, *args)
        ops.call = spy
        try:
            mod.inference_head_fusion = "on"
            maps_on = net.inference(x)[0]
        finally:
            ops.call = call
        fused = names.count("dream_conv_transpose4x4s2_head_f16_nhwc_f16")
        mod.inference_head_fusion = "off"
        same = bool(torch.equal(maps_on, net.inference(x)[0]))
    print("%s, %d frame(s) of %d x %d, precision fp16, half storage%s, %d rounds of %d steps (ms per step)"
          % (arch, batch, res, res, ", hip_graph, ksplit auto" if graph else "", rounds, steps))
    med, spread = report(ms, batch)
    print("  the \"on\" walk ran %d fused launch(es); maps bit-equal to \"off\": %s" % (fused, same))
    if peak_mem:
        print("  max_memory_allocated: off %.2f GiB, on %.2f GiB" % (peak_mem["off"] / 2 ** 30, peak_mem["on"] / 2 ** 30))
    del net, x
    torch.cuda.empty_cache()
    return {"batch": batch, "res": res, "hip_graph": graph, "ms_per_step": ms, "median_ms": med, "spread": spread,
            "max_memory_allocated": peak_mem, "fused_launches": fused, "maps_bit_equal": same}


def piece(b, rounds, steps, k=17, hw=208):
    """The last decoder stage + head of resnet_f at ``b`` frames of 400 x 400, on their own."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(b, hw, hw, 256, generator=g).half().cuda()
    wT = (torch.randn(256, 256, 4, 4, generator=g) * (2.0 / (4 * 256)) ** 0.5).cuda()
    p16 = ops.pack_convT4x4_weight_f16(wT)
    scale, shift = (torch.rand(256, generator=g) + 0.5).cuda(), torch.randn(256, generator=g).cuda()
    h16 = ops.pack_conv_weight_f16((torch.randn(k, 256, 1, 1, generator=g) * 0.1).cuda(), 0)
    bias = torch.randn(k, generator=g).cuda()
    relu = ops.CONV_RELU
    arms = {"off": lambda: ops.conv2d_f16_act16(ops.conv_transpose4x4s2_f16_act16(x, p16, 256, scale, shift, relu), h16, k, 1, None, bias,
                                                ops.CONV_OUT_NCHW),
            "on": lambda: ops.conv_transpose4x4s2_head_f16_act16(x, p16, 256, scale, shift, h16, k, bias, relu)}
    same = bool(torch.equal(arms["off"](), arms["on"]()))
    for arm in ARMS:
        events(arms[arm], 2)
    ms = {arm: [] for arm in ARMS}
    for _ in range(rounds):
        for arm in ARMS:
            ms[arm].append(events(arms[arm], steps))
    print("piece last stage + head: convT 256->256 @ %d^2 -> %d^2, 1x1 conv to %d maps, %d frames (ms); maps bit-equal: %s" % (hw, 2 * hw, k, b, same))
    med, spread = report(ms)
    # the bytes the unfused pair moves through the half tensor between the launches: written once, read once
    print("  the half tensor between the two launches: %.2f GB written + %.2f GB read" % ((b * 4 * hw * hw * 256 * 2 / 1e9,) * 2))
    torch.cuda.empty_cache()
    return {"ms": ms, "median_ms": med, "spread": spread, "maps_bit_equal": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--workloads", default="resnet_f:32,resnet_h:128,resnet_f:1:graph,resnet_h:1:graph")
    ap.add_argument("--no-piece", action="store_true")
    ap.add_argument("--json", default=None, help="also write the record to this file")
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 20, "at least 5 rounds of at least 20 steps"
    record = {"rounds": args.rounds, "steps": args.steps, "device": torch.cuda.get_device_name(0), "workloads": {}, "piece": {}}
    for item in [w for w in args.workloads.split(",") if w]:
        parts = item.split(":")
        record["workloads"][item] = whole_step(parts[0], int(parts[1]), args.res, args.rounds, args.steps, graph=parts[2:] == ["graph"])
    if not args.no_piece:
        record["piece"] = piece(32, args.rounds, args.steps)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
