"""Training batches from raw frames: HIP-event time of image_proc.preprocess_frames alone and of
image_proc.training_batch_from_frames without and with augmentation (b=128, 640x480 -> 400x400 shrink-and-crop -> 100x100, K=7),
alternating in one process, beside a vgg_q b=128 training step of the same process; the bytes the preparation moves and their
share of the 8 TB/s HBM peak; then the host path per frame on one core (PIL + the NumPy augmentation restatement of
tests/test_training_frames.py).

    python tools/microbench_train_frames.py [--batch 128] [--iters 30] [--host-frames 5] [--no-train]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dream_amd import image_proc  # noqa: E402

HBM_PEAK = 8.0e12
MEAN, STDEV = [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]
NET_IN, NET_OUT, MODE, K = (400, 400), (100, 100), "shrink-and-crop", 7


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--host-frames", type=int, default=5)
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(1)
    b, (w, h) = args.batch, (640, 480)
    rs = np.random.RandomState(0)
    frames_host = rs.randint(0, 256, (b, h, w, 3)).astype(np.uint8)
    frames = torch.from_numpy(frames_host).cuda()
    kps = torch.from_numpy(np.stack([rs.uniform(0, w, (b, K)), rs.uniform(0, h, (b, K))], axis=2)).cuda()
    table = image_proc.sample_augmentation(b, NET_IN, np.random.RandomState(1), p=1.0)         # every stage on for every frame
    packed = torch.from_numpy(table.packed()).cuda()
    jobs = {
        "preprocess_frames": lambda: image_proc.preprocess_frames(frames, NET_IN, MODE, MEAN, STDEV),
        "batch_plain": lambda: image_proc.training_batch_from_frames(frames, kps, NET_IN, NET_OUT, MODE, MEAN, STDEV),
        "batch_augmented": lambda: image_proc.training_batch_from_frames(frames, kps, NET_IN, NET_OUT, MODE, MEAN, STDEV,
                                                                         augmentation=packed),
    }
    if not args.no_train:
        import dream_amd
        net = dream_amd.create_network_from_config_data(dream_amd.default_network_config("vgg_q", "panda"))
        net.enable_training()
        batch = jobs["batch_augmented"]()
        jobs["train_step_vgg_q"] = lambda: net.train([batch["image_rgb_input"]], batch["belief_maps"])
    times = {name: [] for name in jobs}
    for _ in range(3):                                           # alternating rounds
        for name, fn in jobs.items():
            times[name] += timed(fn, max(args.iters // 3, 1))
    crop = image_proc.preprocess_plan((w, h), NET_IN, MODE)["crop"]
    u8 = NET_IN[0] * NET_IN[1] * 3
    bytes_plain = b * (crop[2] * crop[3] * 3 + 4 * u8 + K * NET_OUT[0] * NET_OUT[1] * 4)
    bytes_aug = bytes_plain + b * 4 * u8          # resized uint8 written and read, noised uint8 written and read (taps from cache)
    nbytes = {"preprocess_frames": b * (crop[2] * crop[3] * 3 + 4 * u8), "batch_plain": bytes_plain, "batch_augmented": bytes_aug}
    out = {"batch": b, "raw": [w, h]}
    for name, t in times.items():
        med = float(np.median(t))
        out[name] = {"ms_median": round(med * 1e3, 4), "ms_min": round(min(t) * 1e3, 4)}
        if name in nbytes:
            out[name].update(bytes=nbytes[name], TBps=round(nbytes[name] / med / 1e12, 3),
                             hbm_fraction=round(nbytes[name] / med / HBM_PEAK, 3))
    if "train_step_vgg_q" in out:
        out["augmented_share_of_train_step"] = round(out["batch_augmented"]["ms_median"] / out["train_step_vgg_q"]["ms_median"], 5)
    print(json.dumps(out), flush=True)

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from PIL import Image
    from test_training_frames import restated_augment
    inv = table.inverse
    t0 = time.perf_counter()
    for i in range(args.host_frames):
        pre = np.asarray(image_proc.preprocess_image(Image.fromarray(frames_host[i]), NET_IN, MODE))
        aug = restated_augment(pre, table.noise_sigma[i], table.noise_seed[i], table.alpha[i], table.beta[i], inv[i])
        ((aug.astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1).copy()
    print(json.dumps({"host_ms_per_frame_pil_plus_numpy_augmentation":
                      round((time.perf_counter() - t0) / args.host_frames * 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
