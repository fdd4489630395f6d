#!/usr/bin/env python
"""Interleaved per-layer A/B of the split-K half-storage conv (csrc/conv_f16.hip KSPLIT; conv_ksplit="auto") at small batches: every
arm of a layer runs once per round, so drift hits all arms alike.  Median of --rounds, with the spread (max - min) of the rounds.

    python tools/ab_f16_ksplit.py [--frames 1 4 16] [--rounds 5] [--reps 100]

Layers: every distinct plain 3x3 conv launch (no fused pool / upsample, NHWC output: what the rule may split) of the vgg_q and vgg_f
inference walks at 400 x 400, found by tracing the models on the ``meta`` device.  Arms: S in {1, 2, 4, 8, 16} slices (S = 1 is the
unsplit launch) on the rule's own tile and, from 128 output channels on, on the 128 x 128 (v0), 64 x 128 (v3) and 256 x 64 (v1)
tiles.  A timing is --reps back-to-back launches between two device events, divided by --reps (100: a window of 2 ms and more even
on the layers at the launch floor).  `rule`: what
dream_conv2d_f16_ksplit answers for the layer."""
import argparse
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from dream_amd import _hip, models, ops  # noqa: E402

SLICES = (1, 2, 4, 8, 16)
PLAIN = "dream_conv2d_f16_nhwc_f16"


def plain_conv_shapes(frames=1, res=400):
    """[(h, w, cin, cout)] of the splittable launches of both hourglasses, in walk order, each once."""
    found = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        nets = [models.DreamHourglass(7, internalize_spatial_softmax=False, **v).to("meta") for v in ({}, dict(deconv_decoder=True))]
    saved = ops.call, ops.ptr, ops.stream

    def record(name, *args):
        a = [v for v in args if type(v) is int]
        if name == PLAIN and not a[-1] & ~ops.CONV_RELU and tuple(a[1:5]) not in found:
            found.append(tuple(a[1:5]))
    ops.call, ops.ptr, ops.stream = record, (lambda t: None), (lambda: None)
    try:
        for net in nets:
            net.precision = net.activation_storage = "fp16"
            net.run_forward(torch.empty((frames, 3, res, res), device="meta"), [p.detach() for p in net.plan_parameters()], False)
    finally:
        ops.call, ops.ptr, ops.stream = saved
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=100)
    args = ap.parse_args()
    lib = _hip.lib()
    shapes = plain_conv_shapes()
    print("arms: S slices x tile (r = the rule's tile, v0 = 128 x 128, v3 = 64 x 128, v1 = 256 x 64); ms per launch, median of %d rounds "
          "of %d launches (spread of the rounds in brackets)" % (args.rounds, args.reps))
    for b in args.frames:
        for h, w, cin, cout in shapes:
            x = torch.randn(b, h, w, cin, device="cuda").half()
            wt = torch.randn(cout, cin, 3, 3, device="cuda") * 0.05
            bias = torch.randn(cout, device="cuda")
            p16 = ops.pack_conv_weight_f16(wt, 0)
            rule = ops.conv2d_f16_ksplit(b, h, w, cin, cout, 3, ops.CONV_RELU)
            tiles = (-1, 0, 3, 1) if cout > 64 else (-1,)
            arms = [(s, v) for v in tiles for s in SLICES if s <= cin // 32 * 9]
            if (rule, -1) not in arms:
                arms.append((rule, -1))
            times = {a: [] for a in arms}
            for r in range(args.rounds + 1):                       # round 0 warms up
                for s, v in arms:
                    lib.dream_conv_f16_set_variant(v)
                    lib.dream_conv_f16_set_ksplit(s)
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(args.reps):
                        ops.conv2d_f16_act16_ksplit(x, p16, cout, 3, None, bias, ops.CONV_RELU)
                    t1.record()
                    torch.cuda.synchronize()
                    if r > 0:
                        times[(s, v)].append(t0.elapsed_time(t1) / args.reps)
            lib.dream_conv_f16_set_variant(-1)
            lib.dream_conv_f16_set_ksplit(-1)
            med = {a: statistics.median(t) for a, t in times.items()}
            spread = {a: max(t) - min(t) for a, t in times.items()}
            best = min(arms, key=lambda a: med[a])
            base = med[(1, -1)]
            print("b%-2d %3dx%-3d %3d->%-3d rule S=%-2d | " % (b, h, w, cin, cout, rule)
                  + "  ".join("%s/S%d %.4f (%.4f)" % ("r" if v < 0 else "v%d" % v, s, med[(s, v)], spread[(s, v)]) for s, v in arms)
                  + " | best %s/S%d %.4f = %.2fx of r/S1; rule's pick %.4f"
                  % ("r" if best[1] < 0 else "v%d" % best[1], best[0], med[best], base / med[best], med.get((rule, -1), float("nan"))), flush=True)
            del x


if __name__ == "__main__":
    main()
