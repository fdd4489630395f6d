#!/usr/bin/env python
"""Whole-step A/B of the training precisions: train_precision "fp32" (today's step: Winograd forward / data gradient and
Winograd-domain weight gradient on the fp32 MFMA) and "fp16" (the plain convs on the fp16 matrix cores), alternating in ONE process so
that clock and thermal drift hit both arms alike.  vgg_q, 128 frames of 400 x 400, net.train(): both arms are warmed up, then --rounds
rounds of --steps steps per arm are timed with device events.  Prints the per-round times, each arm's spread and the ratio; then, per
distinct plain-conv shape of the plan, the weight-gradient launch alone: the fp16 kernel (csrc/wgrad_f16.hip) against whatever the fp32
path chooses for that layer, in ms and as a fraction of the respective MFMA peak.  --json FILE also writes the record as JSON.

    python tools/microbench_train_precision.py [--rounds 5] [--steps 10] [--batch 128] [--res 400] [--json FILE]"""
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
F32_PEAK_TFLOPS = 157.0             # v_mfma_f32_32x32x2_f32
F16_PEAK_TFLOPS = 2500.0            # v_mfma_f32_32x32x16_f16


def build(batch, res):
    n_kp, manip = bench.ARCH_K["vgg_q"]
    cfg = dream_amd.default_network_config("vgg_q", manip, batch_size=batch)
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


def plain_shapes(module, x):
    """Distinct (B, H, W, cin, cout) of the plan's plain convs, with how many entries have each, in plan order."""
    with torch.no_grad():
        _, saved = module.run_forward(x, [p.detach() for p in module.plan_parameters()], True)
    shapes = {}
    for (kind, mod, flags), (inp, _) in zip(module.plan_layers(), saved):
        if mod is not None and module._half_train_entry(kind, mod, flags, inp.shape[3]):
            key = tuple(int(v) for v in inp.shape[:3]) + (int(mod.weight.shape[1]), int(mod.weight.shape[0]))
            shapes[key] = shapes.get(key, 0) + 1
    return shapes


def wgrad_fp32(module, inp, g, cout, cin):
    """What DreamHourglass.run_backward launches for this layer with train_precision="fp32" -> name of the path."""
    if module.conv_algorithm == "winograd" and ops.wgrad_winograd_pays(g.shape[0] * g.shape[1] * g.shape[2], cin, cout):
        ops.conv3x3_wgrad_winograd(inp, g, cout, cin)
        return "winograd"
    ops.conv3x3_wgrad(inp, g, cout, cin, 0)
    return "direct"


def layer_table(module, shapes, rounds, iters):
    rows = []
    gen = torch.Generator(device="cuda").manual_seed(0)
    for (b, h, w, cin, cout), n in shapes.items():
        inp = torch.randn((b, h, w, cin), device="cuda", generator=gen).relu_()
        g = torch.randn((b, h, w, cout), device="cuda", generator=gen) * 1e-3
        ax, ag = ops.absmax(inp), ops.absmax(g)
        path = wgrad_fp32(module, inp, g, cout, cin)
        ops.conv3x3_wgrad_f16(inp, ax, g, ag, cout, cin)
        t32, t16 = [], []
        for _ in range(rounds):
            t32.append(timed(lambda: wgrad_fp32(module, inp, g, cout, cin), iters))
            t16.append(timed(lambda: ops.conv3x3_wgrad_f16(inp, ax, g, ag, cout, cin), iters))
        m32, m16 = statistics.median(t32), statistics.median(t16)
        tflop = 2.0 * 9 * b * h * w * cin * cout * 1e-12
        rows.append(dict(shape=[b, h, w, cin, cout], entries=n, fp32_path=path, fp32_ms=m32, fp16_ms=m16,
                         fp32_fraction_of_f32_peak=tflop / (m32 * 1e-3) / F32_PEAK_TFLOPS,
                         fp16_fraction_of_f16_peak=tflop / (m16 * 1e-3) / F16_PEAK_TFLOPS,
                         splitk=ops.conv3x3_wgrad_f16_splitk(b, h, w, cin, cout)))
        del inp, g
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
    step = lambda: net.train([x], t)      # noqa: E731
    for arm in ARMS:                      # warm up every shape of both arms (packing, LDS attributes, allocator)
        module.train_precision = arm
        timed(step, 2)
    ms = {arm: [] for arm in ARMS}
    for _ in range(args.rounds):
        for arm in ARMS:
            module.train_precision = arm
            ms[arm].append(timed(step, args.steps))
    module.train_precision = "fp32"
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    spread = {arm: (max(v) - min(v)) / med[arm] for arm, v in ms.items()}
    print("vgg_q training, %d frames of %d x %d, %d rounds of %d steps (ms per step), %s"
          % (args.batch, args.res, args.res, args.rounds, args.steps, torch.cuda.get_device_name(0)))
    for arm in ARMS:
        print("  train_precision=%-5s %s | median %.2f ms = %.0f frames/s, spread %.1f %%"
              % (arm, " ".join("%.2f" % v for v in ms[arm]), med[arm], args.batch / med[arm] * 1e3, 100 * spread[arm]))
    gain, worst = med["fp32"] / med["fp16"] - 1.0, max(spread.values())
    print("  fp16 vs fp32: %+.1f %% frames/s, ratio %.3f (largest spread of an arm: %.1f %%) -> %s"
          % (100 * gain, med["fp32"] / med["fp16"], 100 * worst,
             "faster by more than the spread" if gain > worst else "NOT faster by more than the spread"))
    record = {"rounds": args.rounds, "steps": args.steps, "batch": args.batch, "res": args.res, "device": torch.cuda.get_device_name(0),
              "ms_per_step": ms, "median_ms": med, "spread": spread, "frames_per_s": {a: args.batch / med[a] * 1e3 for a in ARMS},
              "ratio_fp32_over_fp16": med["fp32"] / med["fp16"]}
    rows = layer_table(module, plain_shapes(module, x), args.rounds, args.layer_iters)
    record["wgrad_layers"] = rows
    print("weight-gradient launch per plain-conv shape (median of %d rounds of %d launches; fraction of the 157 / 2500 TFLOP/s MFMA peak)"
          % (args.rounds, args.layer_iters))
    print("  %-26s %3s  %-8s %9s %6s  %9s %6s  %6s %s" % ("B x H x W x cin x cout", "n", "fp32 is", "fp32 ms", "peak", "fp16 ms", "peak", "split", ""))
    tot32 = tot16 = 0.0
    for r in rows:
        tot32, tot16 = tot32 + r["entries"] * r["fp32_ms"], tot16 + r["entries"] * r["fp16_ms"]
        print("  %-26s %3d  %-8s %9.3f %6.3f  %9.3f %6.3f  %6d %s"
              % ("x".join(str(v) for v in r["shape"]), r["entries"], r["fp32_path"], r["fp32_ms"], r["fp32_fraction_of_f32_peak"],
                 r["fp16_ms"], r["fp16_fraction_of_f16_peak"], r["splitk"], "fp16 SLOWER" if r["fp16_ms"] > r["fp32_ms"] else ""))
    print("  all plain convs of a step: fp32 %.2f ms, fp16 %.2f ms" % (tot32, tot16))
    record["wgrad_total_ms"] = {"fp32": tot32, "fp16": tot16}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
