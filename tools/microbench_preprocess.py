"""Raw frames -> network input: HIP-event time of dream_preprocess_frames_u8_f32 (image_proc.preprocess_frames) for a batch of
128 frames at 640x480, 1280x720 and 1920x1080 into 400x400 (shrink-and-crop), its HBM bytes (crop read once + fp32 written) and
fraction of the 8 TB/s peak; then the host path it replaces (PIL crop + resize + NumPy normalise) per frame on one core.

    python tools/microbench_preprocess.py [--batch 128] [--iters 50] [--host-frames 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dream_amd import image_proc  # noqa: E402

HBM_PEAK = 8.0e12
MEAN, STDEV = [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]


def device_time(frames, iters, warmup=5):
    for _ in range(warmup):
        image_proc.preprocess_frames(frames, (400, 400), "shrink-and-crop", MEAN, STDEV)
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        image_proc.preprocess_frames(frames, (400, 400), "shrink-and-crop", MEAN, STDEV)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times)), float(np.min(times))


def host_time(frame, n):
    from PIL import Image
    img = Image.fromarray(frame)
    t0 = None
    for i in range(n + 2):                      # two warm-up frames
        if i == 2:
            t0 = time.perf_counter()
        pre = image_proc.preprocess_image(img, (400, 400), "shrink-and-crop")
        arr = np.asarray(pre.convert("RGB"), dtype=np.float32) / np.float32(255.0)
        ((arr - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1).copy()
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-frames", type=int, default=20)
    args = ap.parse_args()
    torch.set_num_threads(1)
    rows = []
    for w, h in [(640, 480), (1280, 720), (1920, 1080)]:
        frames = torch.randint(0, 256, (args.batch, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(w))
        plan = image_proc.preprocess_plan((w, h), (400, 400), "shrink-and-crop")
        cw, ch = plan["crop"][2], plan["crop"][3]
        nbytes = args.batch * (cw * ch * 3 + 3 * 400 * 400 * 4)
        med, best = device_time(frames.cuda(), args.iters)
        host = host_time(frames[0].numpy(), args.host_frames)
        rows.append({"raw": [w, h], "batch": args.batch, "tile_rows": plan["tile_rows"], "span": [plan["span_rows"], plan["span_cols"]],
                     "kernel_us_median": round(med * 1e6, 1), "kernel_us_min": round(best * 1e6, 1), "bytes": nbytes,
                     "TBps": round(nbytes / med / 1e12, 2), "hbm_fraction": round(nbytes / med / HBM_PEAK, 3),
                     "host_ms_per_frame": round(host * 1e3, 2), "host_ms_per_batch": round(host * 1e3 * args.batch, 1)})
        print(json.dumps(rows[-1]), flush=True)


if __name__ == "__main__":
    main()
