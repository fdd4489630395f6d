#!/usr/bin/env python
"""Whole-step A/B of ResnetSimple's train_decoder_precision: "fp32" (today's step) and "fp16" (the decoder's transposed convs on the fp16
matrix cores: csrc/conv_f16.hip, csrc/wgrad_f16.hip), alternating in ONE process so that clock and thermal drift hit both arms alike.
resnet_h at 16 and at 128 frames and resnet_f at 16 frames of 400 x 400, net.train(): both arms are warmed up, then --rounds rounds of
--steps steps per arm are timed with device events; max_memory_allocated of either arm.  Then, for every covered stage shape of each
workload, the three launches -- forward, data gradient, weight gradient (with the bias sums) -- against what the fp32 path chooses for
them, in ms and as a fraction of the 157 (fp32) / 2500 (fp16) TFLOP/s MFMA peaks, counting the direct conv's FLOPs.  --json FILE also
writes the record.

    python tools/microbench_resnet_decoder_precision.py [--rounds 5] [--steps 10] [--workloads h:16,h:128,f:16] [--res 400] [--json FILE]"""
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
PEAK = {"fp32": 157e12, "fp16": 2500e12}


def build(arch, batch, res):
    n_kp, manip = bench.ARCH_K[arch]
    cfg = dream_amd.default_network_config(arch, manip, batch_size=batch)
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


def step_ab(arch, batch, res, rounds, steps, launch_iters):
    net, x, t = build(arch, batch, res)
    module = net.model.module
    step = lambda: net.train([x], t)      # noqa: E731
    for arm in ARMS:                      # warm up both arms (packing, allocator)
        module.train_decoder_precision = arm
        timed(step, 3)
    ms = {arm: [] for arm in ARMS}
    for _ in range(rounds):
        for arm in ARMS:
            module.train_decoder_precision = arm
            ms[arm].append(timed(step, steps))
    peak = {}
    for arm in ARMS:
        module.train_decoder_precision = arm
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        timed(step, 2)
        peak[arm] = torch.cuda.max_memory_allocated()
    module.train_decoder_precision = "fp32"
    med = {arm: statistics.median(v) for arm, v in ms.items()}
    spread = {arm: (max(v) - min(v)) / med[arm] for arm, v in ms.items()}
    print("dream_%s training, %d frames of %d x %d, %d rounds of %d steps (ms per step), %s"
          % (arch, batch, res, res, rounds, steps, torch.cuda.get_device_name(0)))
    for arm in ARMS:
        print("  train_decoder_precision=%-5s %s | median %.2f ms = %.0f frames/s, spread %.1f %%, max_memory_allocated %.0f MiB"
              % (arm, " ".join("%.2f" % v for v in ms[arm]), med[arm], batch / med[arm] * 1e3, 100 * spread[arm], peak[arm] / 2 ** 20))
    gain, worst = med["fp32"] / med["fp16"] - 1.0, max(spread.values())
    print("  fp16 vs fp32: %+.1f %% frames/s, ratio %.3f (largest spread of an arm: %.1f %%) -> %s"
          % (100 * gain, med["fp32"] / med["fp16"], 100 * worst,
             "faster by more than the spread" if gain > worst else "NOT faster by more than the spread"))
    rows = launch_table(module, x, rounds, launch_iters)
    del net
    torch.cuda.empty_cache()
    return dict(arch=arch, batch=batch, ms_per_step=ms, median_ms=med, spread=spread, max_memory_allocated=peak,
                ratio_fp32_over_fp16=med["fp32"] / med["fp16"], launches=rows)


def launch_table(module, x, rounds, iters):
    """Per covered stage of this workload: the three launches, fp32 (what the path chooses) against fp16, on the stage's own weights."""
    module.train_decoder_precision = "fp16"
    with torch.no_grad():
        _, tape = module.run_forward_train(x)
    module.train_decoder_precision = "fp32"
    stages = [(r["name"], r["conv"], tuple(int(v) for v in r["x"].shape)) for r in tape if module._half_decoder(r)]
    del tape
    torch.cuda.empty_cache()
    repack_table(module, stages, rounds, iters)
    rows, seen = [], {}
    gen = torch.Generator(device="cuda").manual_seed(0)
    for name, m, (b, h, w, cin) in stages:
        cout = int(m.weight.shape[1])
        key = (b, h, w, cin, cout)
        if key in seen:
            seen[key]["stages"] += 1
            continue
        y = torch.randn((b, h, w, cin), device="cuda", generator=gen).relu_()
        dz = torch.randn((b, 2 * h, 2 * w, cout), device="cuda", generator=gen) * 1e-3
        amax = ops.absmax(dz)
        bias = m.bias.detach()
        rec32 = dict(kind="convT", name=name, conv=m, f16=False)
        rec16 = dict(kind="convT", name=name, conv=m, f16=True, dz_amax=amax)
        with torch.no_grad():
            p16 = module._w("wT16", name, m.weight)
            wgrad32 = ((lambda: ops.convT4x4_wgrad_winograd(y, dz)) if ops.convT4x4_wgrad_winograd_applies(y, dz)
                       else (lambda: (ops.convT4x4_wgrad(y, dz), ops.channel_sum(dz))))
            pairs = {"forward": (lambda: module._convT_forward(name, m, y, None, bias, 0, gemm=False),
                                 lambda: ops.conv_transpose4x4s2_f16_sat(y, p16, cout, None, bias, 0)),
                     "dgrad": (lambda: module._convT_dgrad(rec32, dz), lambda: module._convT_dgrad(rec16, dz)),
                     "wgrad": (wgrad32, lambda: (ops.convT4x4_wgrad_f16(y, dz, amax), ops.channel_sum(dz)))}
            flop = 2.0 * b * h * w * cin * cout * 16
            for what, (f32, f16) in pairs.items():
                f32(), f16()
                t32, t16 = [], []
                for _ in range(rounds):
                    t32.append(timed(f32, iters))
                    t16.append(timed(f16, iters))
                m32, m16 = statistics.median(t32), statistics.median(t16)
                sp = max((max(v) - min(v)) / statistics.median(v) for v in (t32, t16))
                kept = what != "wgrad" or ops.convT4x4_wgrad_f16_pays(b, h, w, cin, cout)       # (the rule: a loser stays on the fp32 launch)
                row = dict(shape=list(key), stages=1, launch=what, fp32_ms=m32, fp16_ms=m16, spread=sp, covered=kept,
                           fp32_of_peak=flop / (m32 * 1e-3) / PEAK["fp32"], fp16_of_peak=flop / (m16 * 1e-3) / PEAK["fp16"])
                rows.append(row)
                if what == "forward":
                    seen[key] = row
        del y, dz
        torch.cuda.empty_cache()
    for r in rows:
        r["stages"] = seen[tuple(r["shape"])]["stages"]
    print("  covered stage shapes (median of %d rounds of %d launches; fraction of the 157 / 2500 TFLOP/s peaks, direct-conv FLOPs)" % (rounds, iters))
    print("    %-22s %2s  %-8s %9s %6s %9s %6s %7s  %s" % ("B x H x W x cin x cout", "n", "launch", "fp32 ms", "peak", "fp16 ms", "peak", "spread", ""))
    for r in rows:
        verdict = "fp16 faster" if r["fp16_ms"] < r["fp32_ms"] * (1 - r["spread"]) else ("fp16 SLOWER" if r["fp16_ms"] > r["fp32_ms"] else "within the spread")
        if not r["covered"]:
            verdict += " -- not covered: the step keeps the fp32 launch (ops.convT4x4_wgrad_f16_pays)"
        print("    %-22s %2d  %-8s %9.4f %6.3f %9.4f %6.3f %6.1f%%  %s" % ("x".join(str(v) for v in r["shape"]), r["stages"], r["launch"], r["fp32_ms"],
                                                                  r["fp32_of_peak"], r["fp16_ms"], r["fp16_of_peak"], 100 * r["spread"], verdict))
    print("    all these launches of a step (stages x ms): fp32 %.2f ms, with the switch on %.2f ms"
          % (sum(r["stages"] * r["fp32_ms"] for r in rows), sum(r["stages"] * (r["fp16_ms"] if r["covered"] else r["fp32_ms"]) for r in rows)))
    return rows


def repack_table(module, stages, rounds, iters):
    """The per-step re-pack of the half planes of the covered stages: one by one (three launches a plane) against the batched pack they
    join from the second step on (three launches for all)."""
    if not stages:
        return
    with torch.no_grad():
        entries = []
        for name, m, _ in stages:
            w = m.weight.detach()
            entries += [(w, module._w("wT16", name, m.weight), 2), (w, module._w("wT16b", name, m.weight), 3)]
        table, scratch = ops.pack16_job_table(entries, entries[0][0].device)
        one = lambda: [ops.pack_convT4x4_weight_f16(w) if mode == 2 else ops.pack_convT4x4_dgrad_weight_f16(w) for w, _, mode in entries]     # noqa: E731
        wgs = min(256, max(16, max(int(e[1][0].numel()) for e in entries) >> 15))       # (PackedWeights._repack_half's rule)
        bat = lambda: ops.pack_conv1x1_weights_f16_batched(table, scratch, workgroups_per_job=wgs)      # noqa: E731
        one(), bat()
        t1 = statistics.median(timed(one, iters) for _ in range(rounds))
        tb = statistics.median(timed(bat, iters) for _ in range(rounds))
    print("  re-pack of the %d half planes of a step: one by one %.3f ms (%d launches), batched %.3f ms (3 launches)"
          % (len(entries), t1, 3 * len(entries), tb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--workloads", default="h:16,h:128,f:16")
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--launch-iters", type=int, default=10)
    ap.add_argument("--json", default=None, help="also write the record to this file")
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 10, "at least 5 rounds of at least 10 steps"
    record = {"device": torch.cuda.get_device_name(0), "workloads": []}
    for wl in args.workloads.split(","):
        arch, batch = wl.split(":")
        record["workloads"].append(step_ab("resnet_" + arch, int(batch), args.res, args.rounds, args.steps, args.launch_iters))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
