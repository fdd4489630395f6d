#!/usr/bin/env python
"""Interleaved per-layer A/B of the split-K launches of ResnetSimple's half-stored walk (inference_conv_ksplit="auto")
at small batches, the sibling of tools/ab_f16_ksplit.py: every arm of a layer runs once per round, so drift hits all arms alike.
Median of --rounds, with the spread (max - min) of the rounds.

    python tools/ab_resnet_ksplit.py [--rounds 5] [--reps 100] [--out profiles/ab_resnet_ksplit.txt]

Layers: every distinct covered launch of the resnet_h and resnet_f inference walks at 400 x 400 -- the convs without a residual
(conv1, conv2, the downsample conv; the stride-2 ones as the 1-tap conv over their gathered rows, which is what is launched) and the
4x4 transposed convs of the decoder --, found by tracing the models on the ``meta`` device; at 1, 2, 4, 8 and 16 frames, resnet_f's
also at 32 and resnet_h's at 128.  The two conv3 shapes (256->1024 at 25 x 25, 512->2048 at 13 x 13) are timed WITHOUT their residual
through the plain split entry, as a record of whether a residual finishing pass could pay ("conv3*").  Arms: S in {1, 2, 4, 8, 16}
slices (S = 1 is the unsplit launch) on the rule's own tile, forced with dream_conv_f16_set_ksplit; an arm whose workspace would pass
--max-workspace-mb is not run ("-": such a launch has thousands of workgroups).  A timing is --reps back-to-back eager launches between
two device events, divided by --reps.  `rule`: what dream_conv2d_f16_ksplit_resnet / dream_conv_transpose4x4s2_f16_ksplit answer."""
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
PLAIN, STAGE = "dream_conv2d_f16_nhwc_f16", "dream_conv_transpose4x4s2_f16_nhwc_f16"
NETWORKS = {"h": dict(n_keypoints=7, full=False), "f": dict(n_keypoints=17, full=True)}
FRAMES = {"h": (1, 2, 4, 8, 16, 128), "f": (1, 2, 4, 8, 16, 32)}
CONV3 = [(25, 25, 256, 1024, 1), (13, 13, 512, 2048, 1)]


def covered_shapes(res=400):
    """{(h, w, cin, cout, k; k = 0: a decoder stage): set of networks} of the covered launches, in walk order."""
    found = {}
    saved = ops.call, ops.ptr, ops.stream
    for name, kw in NETWORKS.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            net = models.ResnetSimple(pretrained=False, **kw).to("meta").eval()
        net.precision = net.inference_activation_storage = "fp16"
        seen = []

        def record(entry, *args):
            a = [v for v in args if type(v) is int]
            if entry == PLAIN and not a[-1] & ~ops.CONV_RELU:
                seen.append((a[1], a[2], a[3], a[4], a[6]))
            elif entry == STAGE:
                seen.append((a[1], a[2], a[3], a[4], 0))
        ops.call, ops.ptr, ops.stream = record, (lambda t: None), (lambda: None)
        try:
            net.run_forward(torch.empty((1, 3, res, res), device="meta"))
        finally:
            ops.call, ops.ptr, ops.stream = saved
        for shape in seen[1:]:                                     # (the first plain launch is the stem: not covered)
            found.setdefault(shape, set()).add(name)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--max-workspace-mb", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _hip.lib()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit("arms: S slices on the rule's tile; ms per launch, median of %d rounds of %d eager launches (spread of the rounds in brackets); "
         "k0 = a 4x4 transposed conv (S per sub-pixel phase), conv3* = conv3's shape without its residual; %s"
         % (args.rounds, args.reps, torch.cuda.get_device_name(0)))
    jobs = [(shape, sorted({b for n in nets for b in FRAMES[n]}), "") for shape, nets in covered_shapes().items()]
    jobs += [(shape, (1, 2, 4, 8, 16), "conv3*") for shape in CONV3]
    for (h, w, cin, cout, k), frames, tag in jobs:
        wt = torch.randn(cin, cout, 4, 4, device="cuda") * 0.02 if k == 0 else torch.randn(cout, cin, k, k, device="cuda") * 0.05
        p16 = ops.pack_convT4x4_weight_f16(wt) if k == 0 else ops.pack_conv_weight_f16(wt, 0)
        scale, shift = torch.rand(cout, device="cuda") + 0.5, torch.randn(cout, device="cuda")
        nstages = cin // 32 * (4 if k == 0 else k * k)
        for b in frames:
            x = torch.randn(b, h, w, cin, device="cuda").half()
            if k == 0:
                rule = ops.conv_transpose4x4s2_f16_ksplit(b, h, w, cin, cout)
                nbytes = lib.dream_conv_transpose4x4s2_f16_ksplit_workspace
                launch = lambda: ops.conv_transpose4x4s2_f16_act16_ksplit(x, p16, cout, scale, shift, ops.CONV_RELU)   # noqa: E731
            else:
                rule = ops.conv2d_f16_ksplit_resnet(b, h, w, cin, cout, k, ops.CONV_RELU)
                nbytes = lib.dream_conv2d_f16_ksplit_workspace
                launch = lambda: ops.conv2d_f16_act16_ksplit(x, p16, cout, k, scale, shift, ops.CONV_RELU,              # noqa: E731
                                                             rule=ops.conv2d_f16_ksplit_resnet)
            arms = [s for s in SLICES if s <= nstages and (s == 1 or int(nbytes(b, h, w, cout, s)) <= args.max_workspace_mb << 20)]
            times = {s: [] for s in arms}
            for r in range(args.rounds + 1):                       # round 0 warms up
                for s in arms:
                    lib.dream_conv_f16_set_ksplit(s)
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(args.reps):
                        launch()
                    t1.record()
                    torch.cuda.synchronize()
                    if r > 0:
                        times[s].append(t0.elapsed_time(t1) / args.reps)
            lib.dream_conv_f16_set_ksplit(-1)
            med = {s: statistics.median(t) for s, t in times.items()}
            spread = {s: max(t) - min(t) for s, t in times.items()}
            best = min(arms, key=lambda s: med[s])
            emit("b%-3d %3dx%-3d %4d->%-4d k%d %6s st %3d rule S=%-2d | " % (b, h, w, cin, cout, k, tag, nstages, rule)
                 + "  ".join("S%d %.4f (%.4f)" % (s, med[s], spread[s]) if s in med else "S%d -" % s for s in SLICES)
                 + " | best S%d %.4f = %.2fx of S1" % (best, med[best], med[1] / med[best]))
            del x


if __name__ == "__main__":
    main()
