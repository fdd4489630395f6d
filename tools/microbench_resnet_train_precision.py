#!/usr/bin/env python
"""Whole-step A/B of ResnetSimple's training precisions: train_gemm_precision "fp32" (today's step) and "fp16" (the fused 1x1 GEMMs on the
fp16 matrix cores, csrc/gemm1x1_f16.hip), alternating in ONE process so that clock and thermal drift hit both arms alike.  resnet_h at 16
and at 128 frames of 400 x 400, net.train(): both arms are warmed up, then --rounds rounds of --steps steps per arm are timed with device
events.  Then every distinct covered launch shape of the 16-frame step -- forward (with the statistics), data gradient (masked where the
step masks), weight gradient -- against the fp32 launch it replaces, on synthetic operands.  --json FILE also writes the record.

    python tools/microbench_resnet_train_gemm_precision.py [--rounds 5] [--steps 10] [--batches 16,128] [--res 400] [--json FILE]"""
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


def build(batch, res):
    n_kp, manip = bench.ARCH_K["resnet_h"]
    cfg = dream_amd.default_network_config("resnet_h", manip, batch_size=batch)
    cfg["training"]["config"]["net_input_resolution"] = [res, res]
    cfg["training"]["platform"]["gpu_ids"] = [0]
    with contextlib.redirect_stdout(io.StringIO()):
        net = dream_amd.create_network_from_config_data(cfg)
    net.model.load_state_dict(bench.synthetic_weights(net.model.state_dict()))
    net.enable_training()
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


def step_ab(batch, res, rounds, steps):
    net, x, t = build(batch, res)
    module = net.model.module
    step = lambda: net.train([x], t)      # noqa: E731
    for arm in ARMS:                      # warm up both arms (packing, allocator)
        module.train_gemm_precision = arm
        timed(step, 3)
    ms = {arm: [] for arm in ARMS}
    for _ in range(rounds):
        for arm in ARMS:
            module.train_gemm_precision = arm
            ms[arm].append(timed(step, steps))
    module.train_gemm_precision = "fp32"
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    spread = {arm: (max(v) - min(v)) / med[arm] for arm, v in ms.items()}
    print("resnet_h training, %d frames of %d x %d, %d rounds of %d steps (ms per step), %s"
          % (batch, res, res, rounds, steps, torch.cuda.get_device_name(0)))
    for arm in ARMS:
        print("  train_gemm_precision=%-5s %s | median %.2f ms = %.0f frames/s, spread %.1f %%"
              % (arm, " ".join("%.2f" % v for v in ms[arm]), med[arm], batch / med[arm] * 1e3, 100 * spread[arm]))
    gain, worst = med["fp32"] / med["fp16"] - 1.0, max(spread.values())
    print("  fp16 vs fp32: %+.1f %% frames/s, ratio %.3f (largest spread of an arm: %.1f %%) -> %s"
          % (100 * gain, med["fp32"] / med["fp16"], 100 * worst,
             "faster by more than the spread" if gain > worst else "NOT faster by more than the spread"))
    shapes = covered_shapes(module, x) if batch == 16 else None
    del net
    torch.cuda.empty_cache()
    return dict(batch=batch, ms_per_step=ms, median_ms=med, spread=spread, ratio_fp32_over_fp16=med["fp32"] / med["fp16"]), shapes


def covered_shapes(module, x):
    """Distinct (M, cin, cout, pre) of the covered units of a training forward, with how many units have each, in tape order."""
    module.train_gemm_precision = "fp16"
    with torch.no_grad():
        _, tape = module.run_forward_train(x)
    module.train_gemm_precision = "fp32"
    shapes = {}
    for rec in tape:
        if module._half_unit(rec):
            xin = rec["x"]
            key = (xin.numel() // int(xin.shape[3]), int(xin.shape[3]), int(rec["z"].shape[3]), bool(rec["pre"]))
            shapes[key] = shapes.get(key, 0) + 1
    return shapes


def launch_table(shapes, rounds, iters):
    rows = []
    gen = torch.Generator(device="cuda").manual_seed(0)
    ctr = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    for (m, cin, cout, pre), n in shapes.items():
        bn = torch.nn.BatchNorm2d(cout).cuda()
        x = torch.randn((1, 1, m, cin), device="cuda", generator=gen)
        if not pre:
            x.relu_()
        dz = torch.randn((1, 1, m, cout), device="cuda", generator=gen) * 1e-3
        ab = torch.stack([torch.rand(cin, device="cuda", generator=gen) + 0.5, torch.randn(cin, device="cuda", generator=gen) * 0.2])
        mean, invstd = torch.zeros(cin, device="cuda"), torch.ones(cin, device="cuda")
        w = torch.randn((cout, cin, 1, 1), device="cuda", generator=gen) * 0.05
        g0, g1 = ops.pack_conv1x1_weight(w, 0), ops.pack_conv1x1_weight(w, 1)
        h0, h1 = ops.pack_conv1x1_weight_f16(w, 0), ops.pack_conv1x1_weight_f16(w, 1)
        amax = ops.absmax(dz)
        pre_ab = ab if pre else None
        pairs = {"forward": (lambda: ops.conv1x1_bn(x, g0[0], cout, bn, ctr, pre_ab=pre_ab),
                             lambda: ops.conv1x1_bn_f16(x, h0, cout, bn, ctr, pre_ab=pre_ab))}
        if pre:
            pairs["dgrad (masked)"] = (lambda: ops.conv1x1_bwd_bnmask(dz, g1[0], cin, x, ab, mean, invstd, ctr),
                                       lambda: ops.conv1x1_bwd_bnmask_f16(dz, amax, h1, cin, x, ab, mean, invstd, ctr))
        else:
            pairs["dgrad"] = (lambda: ops.conv1x1(dz, g1[0], cin), lambda: ops.conv1x1_f16(dz, amax, h1, cin))
        if ops.conv1x1_wgrad_applies(x, dz, cout):
            pairs["wgrad"] = (lambda: ops.conv1x1_wgrad(x, dz, cout, cin, pre_ab=pre_ab),
                              lambda: ops.conv1x1_wgrad_f16(x, dz, amax, cout, cin, pre_ab=pre_ab))
        for what, (f32, f16) in pairs.items():
            f32(), f16()
            t32, t16 = [], []
            for _ in range(rounds):
                t32.append(timed(f32, iters))
                t16.append(timed(f16, iters))
            rows.append(dict(shape=[m, cin, cout], pre=pre, units=n, launch=what, fp32_ms=statistics.median(t32), fp16_ms=statistics.median(t16)))
        del x, dz, w
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batches", default="16,128")
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--launch-iters", type=int, default=10)
    ap.add_argument("--json", default=None, help="also write the record to this file")
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 10, "at least 5 rounds of at least 10 steps"
    record, shapes = {"device": torch.cuda.get_device_name(0), "steps": []}, None
    for batch in (int(b) for b in args.batches.split(",")):
        rec, sh = step_ab(batch, args.res, args.rounds, args.steps)
        record["steps"].append(rec)
        shapes = sh or shapes
    if shapes:
        rows = record["launches"] = launch_table(shapes, args.rounds, args.launch_iters)
        print("covered launch shapes of the 16-frame step (median of %d rounds of %d launches, ms)" % (args.rounds, args.launch_iters))
        print("  %-20s %-4s %3s  %-15s %9s %9s  %s" % ("M x cin x cout", "pre", "n", "launch", "fp32 ms", "fp16 ms", ""))
        for r in rows:
            print("  %-20s %-4s %3d  %-15s %9.4f %9.4f  %s" % ("x".join(str(v) for v in r["shape"]), "pre" if r["pre"] else "", r["units"],
                                                              r["launch"], r["fp32_ms"], r["fp16_ms"],
                                                              "fp16 SLOWER" if r["fp16_ms"] > r["fp32_ms"] else ""))
        print("  all covered launches of a step (units x ms): fp32 %.2f ms, fp16 %.2f ms"
              % (sum(r["units"] * r["fp32_ms"] for r in rows), sum(r["units"] * r["fp16_ms"] for r in rows)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
