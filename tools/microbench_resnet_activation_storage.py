#!/usr/bin/env python
"""Whole-step and per-layer A/B of ResnetSimple.inference_activation_storage with precision="fp16": activations in HBM as fp32 (the
default: the parent's code path, kernels instruction-identical) against IEEE half, round-robin in ONE process so that clock and
thermal drift hit both arms alike.  For each workload (resnet_f, 32 frames of 400 x 400; resnet_h, 128 frames; one frame of resnet_h
replayed as a hipGraph) both arms are warmed up, then --rounds rounds of --steps net.inference() calls per arm are timed with device
events; torch.cuda.max_memory_allocated is taken per arm.  Then five pieces of the 32-frame step on their own, the same way: the stem
(im2col + conv + pool), a layer1 conv3 with its residual, layer2.0.conv2 (patch rows + 1-tap conv against the fp32 direct kernel),
layer3's 1x1 pair, the first decoder conv.

    python tools/microbench_resnet_activation_storage.py [--rounds 5] [--steps 20] [--workloads resnet_f:32,resnet_h:128,resnet_h:1:graph]
                                                         [--json FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from dream_amd import ops  # noqa: E402
from microbench_activation_storage import ARMS, events, report  # noqa: E402
from microbench_precision import build, timed  # noqa: E402


def whole_step(arch, batch, res, rounds, steps, graph=False):
    net, x = build(arch, batch, res)
    mod = net.model.module
    mod.precision = "fp16"
    net.hip_graph = graph
    peak_mem = {}
    with torch.no_grad():
        for arm in ARMS:
            mod.inference_activation_storage = arm
            timed(net, x, 3)                                   # (with hip_graph: capture + replays)
        ms = {arm: [] for arm in ARMS}
        for r in range(rounds):
            for arm in ARMS:
                mod.inference_activation_storage = arm
                if r == 0 and not graph:
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
                ms[arm].append(timed(net, x, steps))
                if r == 0 and not graph:
                    peak_mem[arm] = torch.cuda.max_memory_allocated()
        mod.inference_activation_storage = "fp16"
        net.inference(x)
        stored_peak = mod.half_storage_peak()
    print("%s, %d frame(s) of %d x %d, precision fp16%s, %d rounds of %d steps (ms per step)"
          % (arch, batch, res, res, ", hip_graph" if graph else "", rounds, steps))
    med, spread = report(ms, batch)
    if peak_mem:
        print("  max_memory_allocated: storage fp32 %.2f GiB, storage fp16 %.2f GiB; half_storage_peak %.4g"
              % (peak_mem["fp32"] / 2 ** 30, peak_mem["fp16"] / 2 ** 30, stored_peak))
    else:
        print("  half_storage_peak %.4g" % stored_peak)
    del net, x
    torch.cuda.empty_cache()
    return {"batch": batch, "res": res, "hip_graph": graph, "ms_per_step": ms, "median_ms": med, "spread": spread,
            "max_memory_allocated": peak_mem, "half_storage_peak": stored_peak}


def _bn(c, g):
    return (torch.rand(c, generator=g) + 0.5).cuda(), torch.randn(c, generator=g).cuda()


def _w(cout, cin, k, g):
    return (torch.randn(cout, cin, k, k, generator=g) * (2.0 / (k * k * cin)) ** 0.5).cuda()


def layer_arms(b):
    """name -> {"fp32": fn, "fp16": fn}: the launches of one piece of the 32-frame, 400 x 400 step in either storage."""
    g = torch.Generator().manual_seed(0)
    relu = ops.CONV_RELU
    arms = {}
    # the stem: im2col rows (K 147 -> 160) + 1-tap conv 160 -> 64 + BatchNorm + ReLU, MaxPool(3, 2, 1)
    img = torch.randn(b, 3, 400, 400, generator=g).cuda()
    p1, (s1, t1) = ops.pack_conv_weight_f16(_w(64, 147, 1, g), 0), _bn(64, g)        # (the plane's columns are padded to 160)
    arms["stem: im2col + conv 160->64 @ 200^2 + pool"] = {
        "fp32": lambda: ops.maxpool3s2(ops.conv2d_f16(ops.im2col_nchw(img, 7, 7, 2, 3, 160), ops.absmax(img), p1, 64, 1, s1, t1, None, relu)[0]),
        "fp16": lambda: ops.maxpool3s2_f16(ops.conv2d_f16_act16(ops.im2col_nchw_f16(img, 7, 7, 2, 3, 160), p1, 64, 1, s1, t1, relu))}

    def half(*shape):
        t = torch.randn(*shape, generator=g).half().cuda()
        return t, t.float()

    # layer1 conv3: 64 -> 256 @ 100^2, + identity, ReLU
    x16, x32 = half(b, 100, 100, 64)
    r16, r32 = half(b, 100, 100, 256)
    p3, (s3, t3), a3 = ops.pack_conv_weight_f16(_w(256, 64, 1, g), 0), _bn(256, g), ops.absmax(x32)
    arms["layer1 conv3 64->256 @ 100^2 + residual"] = {
        "fp32": lambda: ops.conv2d_f16(x32, a3, p3, 256, 1, s3, t3, r32, relu),
        "fp16": lambda: ops.conv2d_f16_act16_res(x16, p3, 256, 1, r16, s3, t3, relu)}
    # layer2.0.conv2: 128 -> 128, 3x3 stride 2, 100^2 -> 50^2: the exact-fp32 direct kernel against patch rows + the 1-tap conv
    y16, y32 = half(b, 100, 100, 128)
    w2, (s2, t2) = _w(128, 128, 3, g), _bn(128, g)
    pk2, rows2, _ = ops.pack_conv_weight(w2, 0)
    pc2 = ops.pack_conv_weight_f16(w2.permute(0, 2, 3, 1).reshape(128, -1, 1, 1).contiguous(), 0)
    arms["layer2.0.conv2 128->128 3x3 s2 @ 100^2 -> 50^2"] = {
        "fp32": lambda: ops.conv2d_amax(y32, pk2, rows2, 3, 2, s2, t2, None, relu),
        "fp16": lambda: ops.conv2d_f16_act16(ops.im2col3s2_f16(y16), pc2, 128, 1, s2, t2, relu)}
    # layer3's 1x1 pair: conv1 1024 -> 256 and conv3 256 -> 1024 + identity @ 25^2
    z16, z32 = half(b, 25, 25, 1024)
    pa, (sa, ta), aa = ops.pack_conv_weight_f16(_w(256, 1024, 1, g), 0), _bn(256, g), ops.absmax(z32)
    pb, (sb, tb) = ops.pack_conv_weight_f16(_w(1024, 256, 1, g), 0), _bn(1024, g)

    def pair32():
        o, a = ops.conv2d_f16(z32, aa, pa, 256, 1, sa, ta, None, relu)
        return ops.conv2d_f16(o, a, pb, 1024, 1, sb, tb, z32, relu)

    arms["layer3 1x1 pair 1024->256->1024 @ 25^2"] = {
        "fp32": pair32,
        "fp16": lambda: ops.conv2d_f16_act16_res(ops.conv2d_f16_act16(z16, pa, 256, 1, sa, ta, relu), pb, 1024, 1, z16, sb, tb, relu)}
    # the first decoder conv: ConvTranspose2d(2048, 256, 4, 2, 1) @ 13^2 -> 26^2
    d16, d32 = half(b, 13, 13, 2048)
    wT = (torch.randn(2048, 256, 4, 4, generator=g) * (2.0 / (4 * 2048)) ** 0.5).cuda()
    pT, (sT, tT), aT = ops.pack_convT4x4_weight_f16(wT), _bn(256, g), ops.absmax(d32)
    arms["decoder convT 2048->256 @ 13^2 -> 26^2"] = {
        "fp32": lambda: ops.conv_transpose4x4s2_f16(d32, aT, pT, 256, sT, tT, relu),
        "fp16": lambda: ops.conv_transpose4x4s2_f16_act16(d16, pT, 256, sT, tT, relu)}
    return arms


def layers(b, rounds, steps):
    out = {}
    for name, arms in layer_arms(b).items():
        for arm in ARMS:
            events(arms[arm], 2)
        ms = {arm: [] for arm in ARMS}
        for _ in range(rounds):
            for arm in ARMS:
                ms[arm].append(events(arms[arm], steps))
        print("piece %s, %d frames (ms)" % (name, b))
        med, spread = report(ms)
        out[name] = {"ms": ms, "median_ms": med, "spread": spread}
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--workloads", default="resnet_f:32,resnet_h:128,resnet_h:1:graph")
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--json", default=None, help="also write the record to this file")
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 20, "at least 5 rounds of at least 20 steps"
    record = {"rounds": args.rounds, "steps": args.steps, "device": torch.cuda.get_device_name(0), "workloads": {}, "layers": {}}
    for item in [w for w in args.workloads.split(",") if w]:
        parts = item.split(":")
        record["workloads"][item] = whole_step(parts[0], int(parts[1]), args.res, args.rounds, args.steps, graph=parts[2:] == ["graph"])
    if not args.no_layers:
        record["layers"] = layers(32, args.rounds, args.steps)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
