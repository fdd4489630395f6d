#!/usr/bin/env python
"""Whole ResnetSimple net.inference() at the batch sizes of the reference's own callers (1 frame: keypoints_from_image; 8: the
visualisation script; 16: the dataset analysis), inference_conv_ksplit "off" against "auto", alternating in one process: hip_graph
on, precision="fp16", inference_activation_storage="fp16", 400 x 400 frames.  The "off" arm is the walk as it was before the switch
existed (same kernels: profiles/isa_same_resnet_ksplit.txt).  Per point the median over --rounds of the ms per call (--calls calls
between two host clock readings, the device drained at both) and the spread (max - min) of the rounds.  Where the rule splits nothing
both arms run the same launches: such a point shows the noise floor.

    python tools/microbench_resnet_small_batch.py [--rounds 5] [--calls 50] [--out profiles/microbench_resnet_small_batch.txt]"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import dream_amd  # noqa: E402

ARMS = ("off", "auto")
FRAMES = {"resnet_h": (1, 2, 4, 8, 16, 128), "resnet_f": (1, 2, 4, 8, 16, 32)}


def network(arch):
    with contextlib.redirect_stdout(io.StringIO()):
        net = dream_amd.create_network_from_config_data(dream_amd.default_network_config(arch, "panda"))
    net.enable_evaluation()
    net.model.module.precision = net.model.module.inference_activation_storage = "fp16"
    net.hip_graph = True
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--archs", nargs="+", default=sorted(FRAMES, reverse=True))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit("whole net.inference(), 400 x 400, hip_graph, precision=fp16, inference_activation_storage=fp16; inference_conv_ksplit off | "
         "auto: median ms per call of %d rounds of %d calls (10 calls from 32 frames on), spread of the rounds in brackets; %s"
         % (args.rounds, args.calls, torch.cuda.get_device_name(0)))
    for arch in args.archs:
        net = network(arch)
        for b in FRAMES[arch]:
            x = torch.rand(b, 3, 400, 400, device="cuda")
            calls = args.calls if b < 32 else 10
            times = {a: [] for a in ARMS}
            with torch.no_grad():
                for r in range(args.rounds + 1):                   # round 0 captures and warms up
                    for arm in ARMS:
                        net.model.module.inference_conv_ksplit = arm
                        net.inference(x)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(calls):
                            net.inference(x)
                        torch.cuda.synchronize()
                        if r > 0:
                            times[arm].append((time.perf_counter() - t0) * 1e3 / calls)
            med = {a: statistics.median(t) for a, t in times.items()}
            spread = {a: max(t) - min(t) for a, t in times.items()}
            emit("%-8s %3d frames | off %8.3f ms (%.3f) %7.1f frames/s | auto %8.3f ms (%.3f) %7.1f frames/s | auto / off %.3f"
                 % (arch, b, med["off"], spread["off"], b * 1e3 / med["off"], med["auto"], spread["auto"], b * 1e3 / med["auto"],
                    med["auto"] / med["off"]))
            del x
        del net


if __name__ == "__main__":
    main()
