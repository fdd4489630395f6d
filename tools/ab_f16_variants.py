#!/usr/bin/env python
"""Interleaved per-layer A/B of the fp16 conv variants (csrc/conv_f16.hip) at the bench batch size, with the split kernel's own
choice (fp16x3) as the yardstick: every arm of a layer runs once per round, so drift hits all arms alike.  Median of --rounds.

    python tools/ab_f16_variants.py [--batch 128] [--rounds 5]

Layers: the 3x3 convs of vgg_q (400 .. 25 px), its 1x1-like narrow tail, the 4x4 transposed convs of both decoders and two 1x1
bottleneck convs of the ResNet trunk (one channel chunk per stage: the shape where the double-buffered patch matters most)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from dream_amd import _hip, ops  # noqa: E402

NAMES = ["m2n2w2x2 db", "m2n2w4x1 db", "m2n1w4x1 db", "m1n2w2x2 db", "m2n2w4x2 db", "m2n2w4x1 sb", "m2n2w4x2 sb", "m2n2w4x2 db prio"]
# (kind, res, cin, cout, flags, frames per 128 of the bench batch)
LAYERS = [("conv3", 400, 64, 64, 1 | 16, 128), ("conv3", 200, 64, 128, 1, 128), ("conv3", 200, 128, 128, 1 | 16, 128),
          ("conv3", 100, 128, 256, 1, 128), ("conv3", 100, 256, 256, 1, 128), ("conv3", 50, 256, 512, 1, 128),
          ("conv3", 50, 512, 512, 1, 128), ("conv3", 25, 512, 512, 1, 128), ("conv3", 100, 64, 32, 1, 128),
          ("convT4", 25, 512, 256, 1, 128), ("convT4", 50, 256, 128, 1, 128),
          ("conv1", 100, 256, 64, 1, 32), ("conv1", 25, 1024, 256, 1, 32), ("convT4", 13, 2048, 256, 1, 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    lib = _hip.lib()
    print("arms: " + ", ".join("v%d = %s" % (i, n) for i, n in enumerate(NAMES)) + "; x3 = the fp16x3 kernel's own choice; rule = fp16, no forced variant")
    for kind, res, cin, cout, flags, share in LAYERS:
        b = max(1, args.batch * share // 128)
        x = torch.randn(b, res, res, cin, device="cuda")
        bias = torch.randn(cout, device="cuda")
        amax = ops.absmax(x)
        if kind == "convT4":
            w = torch.randn(cin, cout, 4, 4, device="cuda") * 0.05
            p3, p1 = ops.pack_convT4x4_weight_f16x3(w), ops.pack_convT4x4_weight_f16(w)
            run3 = lambda: ops.conv_transpose4x4s2_f16x3(x, amax, p3, cout, None, bias, flags & 1)
            run1 = lambda: ops.conv_transpose4x4s2_f16(x, amax, p1, cout, None, bias, flags & 1)
            flops = 2.0 * b * (2 * res) ** 2 * cin * cout * 4
        else:
            k = 3 if kind == "conv3" else 1
            w = torch.randn(cout, cin, k, k, device="cuda") * 0.05
            p3, p1 = ops.pack_conv_weight_f16x3(w, 0), ops.pack_conv_weight_f16(w, 0)
            run3 = lambda: ops.conv2d_f16x3(x, amax, p3, cout, k, None, bias, None, flags)
            run1 = lambda: ops.conv2d_f16(x, amax, p1, cout, k, None, bias, None, flags)
            flops = 2.0 * b * res * res * cin * cout * k * k
        arms = ["x3", "rule"] + ([0, 1, 3, 4, 5, 6, 7] if cout > 32 else [1, 2, 5])
        times = {a: [] for a in arms}
        for r in range(args.rounds + 1):                       # round 0 warms up
            for a in arms:
                lib.dream_conv_f16_set_variant(a if isinstance(a, int) else -1)
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                (run3 if a == "x3" else run1)()
                e.record()
                torch.cuda.synchronize()
                if r > 0:
                    times[a].append(s.elapsed_time(e))
        lib.dream_conv_f16_set_variant(-1)
        med = {a: statistics.median(t) for a, t in times.items()}
        best = min((a for a in arms if isinstance(a, int)), key=lambda a: med[a])
        print("%-6s b%-3d %4d %4d->%3d f%-2d | " % (kind, b, res, cin, cout, flags)
              + "  ".join("%s %.3f ms (%.0f TF)" % (("v%d" % a) if isinstance(a, int) else a, med[a], flops / med[a] / 1e9) for a in arms)
              + " | best v%d" % best, flush=True)
        del x


if __name__ == "__main__":
    main()
