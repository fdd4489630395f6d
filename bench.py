#!/usr/bin/env python
"""Benchmark of the DREAM belief-map hot path on MI355X (driver contract: see the task brief).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Main workload (BASELINE.json configs[1]): DREAM-vgg-Q inference, batch 128 of synthetic 400x400 frames already resident in
HBM, one "step" = DreamNetwork.inference(x) = CNN forward + peak extraction, result = [B,K,2] float32 keypoints on the host
(the reference's return contract).  With N ranks each rank processes its own batch of 128 (embarrassingly parallel, no
data-path collective): weak scaling.

`--gpus N` with N > 1 and no launcher environment (WORLD_SIZE unset) re-executes this file under
`python -m torch.distributed.run --nproc-per-node N` -- one process per GPU over RCCL -- and rank 0 prints the line:
`n_gpus` = N, `rccl_ranks` = the world size of the nccl (= RCCL) process group.  (`--single-process` instead drives the N GPUs
from ONE process through training.platform.gpu_ids, the reference's nn.DataParallel contract.)

One JSON line on rank 0.  `roofline` is measured live: every launch of the conv kernels is bracketed by HIP events on the
launch stream inside the timed region; achieved = algorithmic FLOPs of those launches / their summed duration.

A plain run sets up, warms up, times the K steps and prints the line.  `--dump-outputs DIR` then also writes what the last timed
step returned (belief maps + keypoints, or the loss in training) as DIR/<name>.npy.  `--full` adds the blocks below, each of which
takes runs of its own:
  * N == 1: `secondary` = the other single-GPU configurations of BASELINE.json under the same clock: configs[2] (vgg_q
    training b=128) and one GPU's share of configs[3] (resnet_h training, 16 frames) and configs[4] (resnet_f inference, 32
    frames), two timed steps each, every one with its executed-multiplication roofline fraction; `cpu_baseline` times the CPU
    oracle by the protocol of BASELINE.md section 3 (torch-CPU restatement: forward B=1 / B=16, train() step B=8, resnet_h
    forward B=1 on all host threads; plain-C peak extraction on one core; median of the timed iterations after the warm-ups).
  * N > 1: `scale` = the sharded configurations BASELINE.json names: configs[3] (resnet_h training, 128 frames split over the
    N GPUs, RCCL all-reduce of the gradients every step) and configs[4] (resnet_f inference, 256 frames split over the N
    GPUs), each with whole-job and per-GPU frames/s (strong scaling), next to the weak-scaling vgg_q metric in `value`.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

PEAK_F32_MFMA_TFLOPS = 157.3          # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_F16_MFMA_TFLOPS = 2500.0         # MI355X_MICROARCH.md: dense fp16/bf16 MFMA peak (not the 2:1-sparse figure)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=128, help="frames per GPU (weak scaling, the default)")
    ap.add_argument("--global-batch", type=int, default=0, help="strong scaling: this many frames in total, split evenly over "
                    "the GPUs (BASELINE configs[3]: 128 over 8, configs[4]: 256 over 8); overrides --batch")
    ap.add_argument("--single-process", action="store_true", help="N GPUs from ONE process through training.platform.gpu_ids "
                    "(the reference's nn.DataParallel contract, dream_amd/data_parallel.py) instead of one process per GPU")
    ap.add_argument("--conv-algorithm", choices=["winograd", "winograd2", "direct"], default="winograd",
                    help="fp32 3x3 stride-1 convs: Winograd on the fp32 MFMA (default: F(4x4,3x3) where it pays, F(2x2,3x3) elsewhere; "
                         "winograd2: F(2x2,3x3) everywhere) or the direct implicit GEMM")
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--mode", choices=["inference", "train"], default="inference")
    ap.add_argument("--precision", choices=["fp32", "fp16x3"], default="fp32",
                    help="conv kernel for inference: exact fp32 MFMA, or split-precision fp16x3 (fp32 in/out, fp32-class error)")
    ap.add_argument("--arch", choices=["vgg_q", "vgg_f", "resnet_h", "resnet_f"], default="vgg_q")
    ap.add_argument("--full", action="store_true", help="besides the headline: the `secondary` (N = 1) / `scale` (N > 1) blocks of the "
                    "other BASELINE.json configurations and the `cpu_baseline` block (a plain run times the headline workload only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one returned as "
                    "DIR/<name>.npy (float32; at most 64 MB in all, a fixed seeded sample of the frames beyond that)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--graph", action="store_true", help="inference through DreamNetwork.hip_graph (hipGraph replay; "
                    "per-launch HIP events are not recorded then)")
    ap.add_argument("--split-leg", action="store_true", help="also time the split-precision conv kernel (fp16x3: fp32 in/out, 3 fp16 MFMAs per "
                    "product) on the same workload and report it beside the exact-fp32 value (off by default since round 3: with the "
                    "F(4x4,3x3) kernel the exact path is the faster one)")
    ap.add_argument("--no-split-leg", action="store_true", help="(accepted for older command lines; the leg is off by default)")
    ap.add_argument("--dp-check", action="store_true", help="training: add `dp_check` to the line -- the per-step loss averaged over the "
                    "ranks and the largest difference of any parameter between ranks after the last step (tests/test_gpu_parity.py: the "
                    "first multi-GPU contact is a test, not a bench)")
    ap.add_argument("--concat-ranks", type=int, default=0, help="one process, one GPU: the batch is the concatenation of what ranks 0..N-1 "
                    "of a `--gpus N` run would see (the single-device reference of --dp-check)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the `secondary` (N = 1) / `scale` (N > 1) blocks")
    ap.add_argument("--secondary-steps", type=int, default=5, help="timed steps of the inference legs of `secondary` / `scale`")
    ap.add_argument("--secondary-train-steps", type=int, default=10, help="timed steps of the training legs (the ResNet step has a known "
                    "occasional slow mode: three steps were too few to see it)")
    ap.add_argument("--cpu-seconds", type=float, default=24.0, help="budget of the cpu_baseline block (each CNN leg gets a quarter; a leg whose 3 + 5 iterations do not fit falls back to 1 + 3)")
    return ap.parse_args()


def bench_sha():
    with open(os.path.abspath(__file__), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def pmc_traffic(spec):
    """HBM bytes per launch of the conv kernels from the PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate runs
    of this same command, FETCH_SIZE doubled per the gfx950 note in MI355X_MICROARCH.md and calibrated on the max-pool
    kernel).  Counters cannot be read from inside the process, so the committed summary of the newest round is reported -- but
    only when it was taken with THIS bench.py (the summary records the file's hash) on this workload; null otherwise."""
    key = (spec["arch"], spec["mode"], spec["batch"], spec["res"], spec["conv_algorithm"])
    if key == ("resnet_h", "train", 16, 400, "winograd"):
        # one GPU's share of configs[3]: the same two passes over `bench.py --arch resnet_h --mode train --batch 16` (tools/pmc_traffic.py,
        # generic mode: totals per kernel family); the conv families are the ones this leg's roofline times
        names = sorted((n for n in os.listdir(os.path.join(ROOT, "profiles")) if n.endswith("_pmc_traffic_resnet_train.json") and n[0] == "r"),
                       reverse=True)
        for name in names:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                d = json.load(f)
            if d.get("bench_py_sha") != bench_sha():
                continue
            fams = [v for k, v in d.get("families", {}).items() if k in ("gemm1x1_kernel", "conv_mfma_kernel", "conv_wino_kernel",
                                                                          "conv_wino_stat_kernel", "conv_wino4_kernel")]
            n = sum(v["dispatches"] for v in fams)
            if n:
                return sum(v["fetch_gb_corrected"] + v["write_gb"] for v in fams) * 1e9 / n
        return None
    if key != ("vgg_q", "inference", 128, 400, "winograd"):
        return None
    names = sorted((n for n in os.listdir(os.path.join(ROOT, "profiles")) if n.endswith("_pmc_traffic.json") and n[0] == "r"),
                   reverse=True)
    for name in names:
        with open(os.path.join(ROOT, "profiles", name)) as f:
            d = json.load(f)
        if d.get("bench_py_sha") == bench_sha() and "conv_kernels" in d:
            return d["conv_kernels"]["traffic_gb_per_launch"] * 1e9
    return None


ARCH_K = {"vgg_q": (7, "panda"), "vgg_f": (7, "panda"), "resnet_h": (7, "panda"), "resnet_f": (17, "baxter")}


def synthetic_weights(state_dict):
    """Random-init weights of the architecture (there are no checkpoints here): fan-in scaled uniform conv / deconv
    weights so activations stay O(1) through the 23-100 layers and the belief maps cross the 0.01 peak threshold,
    non-trivial BatchNorm statistics so the folded eval-mode BN is exercised.  Deterministic per tensor name."""
    import zlib
    import torch
    out = {}
    for key, t in state_dict.items():
        g = torch.Generator().manual_seed(zlib.crc32(key.encode()) & 0x7FFFFFFF)

        def uni(lo, hi):
            return torch.rand(tuple(t.shape), generator=g, dtype=torch.float64) * (hi - lo) + lo
        if key.endswith("num_batches_tracked"):
            v = torch.zeros_like(t)
        elif key.endswith("running_mean"):
            v = uni(-0.1, 0.1)
        elif key.endswith("running_var"):
            v = uni(0.8, 1.2)
        elif t.dim() == 4:
            transposed = "deconv" in key or ("upsample" in key and t.shape[-1] == 4)      # ConvTranspose2d: [Cin,Cout,k,k]
            fan_in = t.shape[0] * t.shape[2] * t.shape[3] / 4.0 if transposed else t.shape[1] * t.shape[2] * t.shape[3]
            b = (6.0 / fan_in) ** 0.5
            v = uni(-b, b)
        elif key.endswith("beta"):
            v = t.detach().cpu()
        elif key.endswith("weight"):                                                      # BatchNorm gamma
            v = uni(0.8, 1.2) * (0.25 if ("bn3." in key or "downsample.1." in key) else 1.0)
        else:
            v = uni(-0.05, 0.05)
        out[key] = v.to(t.dtype)
    return out


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _timed_leg(fn, budget_s, frames):
    """BASELINE.md section 3 protocol: >= 3 warm-ups, >= 5 timed iterations, MEDIAN.  One probe iteration sizes the leg: when eight
    iterations do not fit ``budget_s`` the leg falls back to 1 warm-up + 3 timed and says so."""
    t0 = time.perf_counter()
    fn()
    probe = time.perf_counter() - t0
    warm, timed = (2, 5) if probe * 8 <= budget_s else (0, 3)          # the probe is the first warm-up
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(timed):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    med = ts[len(ts) // 2]
    return {"frames_per_s": frames / med, "median_s": med, "warmups": warm + 1, "timed": timed, "frames": frames}


def cpu_baseline(arch, res, seconds):
    """The CPU oracle timed on the GPU box's host cores, by the plan of BASELINE.md section 3 / SURVEY.md 8d: forward B=1 and B=16
    and a train() step B=8 of the torch-CPU restatement (all host threads), resnet_h forward B=1, and the plain-C restatement of
    peaks_from_belief_maps on ONE core (as the reference runs it) over 128 x K maps; median of >= 5 timed iterations after >= 3
    warm-ups per leg.  ``value`` = frames/s of the B=16 forward INCLUDING its single-core peak extraction -- the same work the
    bench's metric counts.  ``seconds``: budget of the whole block (each CNN leg gets a quarter)."""
    import numpy as np
    import torch
    import cases
    from oracle import models as omodels, peaks as opeaks
    k = ARCH_K[arch][0]
    model = omodels.build_model(arch, k)
    model.load_state_dict(omodels.recipe_weights(model.state_dict()))
    model.eval()
    threads = torch.get_num_threads()
    leg_budget = max(2.0, seconds / 4.0)

    def forward(m, x):
        def run():
            with torch.no_grad():
                return m(x)[0]
        return run

    legs = {}
    x1 = torch.from_numpy(cases.image_batch(1, res, res, seed=0))
    x16 = torch.from_numpy(cases.image_batch(16, res, res, seed=0))
    legs["forward_b1"] = _timed_leg(forward(model, x1), leg_budget, 1)
    legs["forward_b16"] = _timed_leg(forward(model, x16), leg_budget, 16)
    # train() step, B = 8: forward + MSE + backward + Adam (dream/network.py:328-364), torch-CPU
    tm = omodels.build_model(arch, k)
    tm.load_state_dict(omodels.recipe_weights(tm.state_dict()))
    tm.train()
    opt = torch.optim.Adam([p for p in tm.parameters() if p.requires_grad], lr=1e-4)
    crit = torch.nn.MSELoss()
    x8 = torch.from_numpy(cases.image_batch(8, res, res, seed=1))
    with torch.no_grad():
        oh, ow = tm(x8[:1])[0].shape[2:]
    t8 = torch.from_numpy(cases.target_batch(8, k, (ow, oh), in_wh=(res, res), seed=1))

    def train_step():
        opt.zero_grad()
        loss = crit(tm(x8)[0], t8)
        loss.backward()
        opt.step()
    legs["train_b8"] = _timed_leg(train_step, leg_budget, 8)
    del tm, opt
    if arch != "resnet_h":
        rm = omodels.build_model("resnet_h", 7)
        rm.load_state_dict(omodels.recipe_weights(rm.state_dict()))
        rm.eval()
        legs["resnet_h_forward_b1"] = _timed_leg(forward(rm, x1), leg_budget, 1)
        del rm
    # peak extraction: the C restatement (oracle/peaks_c.c), one core, 128 frames x K maps at the network's output resolution
    with torch.no_grad():
        maps16 = model(x16)[0].numpy()
    maps128 = np.ascontiguousarray(np.concatenate([maps16] * 8, axis=0))
    off = 0.0 if maps128.shape[-1] >= 400 else 0.4395
    legs["peaks_1core_b128"] = _timed_leg(lambda: opeaks.c_keypoints_from_belief_maps(maps128, off), leg_budget, 128)
    f16 = legs["forward_b16"]["median_s"] + 16.0 / legs["peaks_1core_b128"]["frames_per_s"]
    for v in legs.values():
        v["frames_per_s"] = round(v["frames_per_s"], 3)
        v["median_s"] = round(v["median_s"], 4)
    return {"value": 16.0 / f16, "unit": "frames/s", "cores": threads, "cpu": _cpu_model(), "kind": "port",
            "protocol": "BASELINE.md section 3: median of the timed iterations after the warm-ups, per leg",
            "legs": legs,
            "sample": "oracle torch-CPU %s at %dx%d on %d threads: forward B=1 / B=16, train() step B=8 (MSE + Adam)%s; plain-C "
                      "peaks_from_belief_maps on 1 core over 128 x %d maps of %dx%d; value = 16 frames / (median B=16 forward + "
                      "their single-core peak extraction)" % (arch, res, res, threads, "" if arch == "resnet_h" else
                                                              ", resnet_h forward B=1", k, maps128.shape[-1], maps128.shape[-2])}


def self_launch(args):
    """`python bench.py --gpus N` (N > 1, no launcher environment): one process per GPU under torch.distributed.run, RCCL."""
    import torch
    n_visible = torch.cuda.device_count()
    if n_visible < args.gpus and not os.environ.get("DREAM_BENCH_BACKEND"):
        print(json.dumps({"metric": "frames/s DREAM-%s %dx%d b=%d %s" % (args.arch.replace("_", "-"), args.res, args.res, args.batch, args.mode),
                          "value": None, "unit": "frames/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
                          "error": "bench.py --gpus %d: only %d GPU(s) visible" % (args.gpus, n_visible)}), flush=True)
        raise SystemExit(2)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    raise SystemExit(subprocess.call(cmd, env=env))


# dream_amd.ops entry point -> the kernel family its launches belong to (the names rocprofv3 reports)
FAMILY = {"conv3x3_winograd4": "conv_wino4_kernel", "conv_transpose4x4s2_winograd4": "conv_wino4_kernel", "conv4x4s2_winograd4": "conv_wino4_kernel",
          "conv3x3_winograd": "conv_wino_kernel", "conv_transpose4x4s2_winograd": "conv_wino_kernel", "conv4x4s2_winograd": "conv_wino_kernel",
          "conv3x3": "conv_mfma_kernel", "conv2d": "conv_mfma_kernel", "conv_transpose3x3s2": "conv_mfma_kernel",
          "conv_transpose4x4s2": "conv_mfma_kernel", "conv2d_amax": "conv_mfma_kernel",
          "conv1x1": "gemm1x1_kernel", "conv1x1_bn": "gemm1x1_kernel", "conv1x1_bwd_bnmask": "gemm1x1_kernel",
          "conv2d_f16x3": "conv_f16x3_kernel", "conv_transpose3x3s2_f16x3": "conv_f16x3_kernel", "conv_transpose4x4s2_f16x3": "conv_f16x3_kernel"}


class ConvTimer:
    """Per-launch timing of the conv kernels (HIP events on the launch stream): wraps the dream_amd.ops conv entry points once;
    while `recording`, every call is bracketed by two events and its algorithmic / executed FLOPs are noted."""

    def __init__(self, ops, torch):
        self.events, self.recording, self.torch = [], False, torch
        C = ops.CONV_POOL2

        def pooled(flags):                    # a fused 2x2 max-pool stores 1/4 of the conv outputs it computed
            return 4.0 if flags & C else 1.0

        def w(orig, flops_of, kernel_launches=1, executed=1.0, issued=None):
            return self.wrap(orig, flops_of, kernel_launches, executed, issued, family=FAMILY.get(getattr(orig, "__name__", ""), "other"))

        def wino4_issued(y, x, u, cout, *a, **k):
            # multiplications the F(4x4,3x3) kernel really issues: 36 per tile and channel pair, tiles counted in whole 16-tile
            # blocks of the (image, tile row, tile column) numbering, output channels in whole 128- (wide shape) or 64-blocks (narrow)
            b, h, wd, cin = (int(v) for v in x.shape)
            tiles = (b * ((h + 3) // 4) * ((wd + 3) // 4) + 15) // 16 * 16
            cpad = (cout + 127) // 128 * 128 if cout > 64 else 64
            return 2.0 * tiles * 36 * cin * cpad
        # algorithmic FLOPs of one launch = 2 * outputs * (input channels * taps); y is NHWC or NCHW [B,...]
        ops.conv3x3 = w(ops.conv3x3, lambda y, x, packed, bias, cout, flags=0, relu_mask=None: 2.0 * y.numel() * pooled(flags) * x.shape[3] * 9)
        ops.conv2d = w(ops.conv2d, lambda y, x, packed, cout, ksize, stride=1, scale=None, shift=None, residual=None, flags=0:
                       2.0 * y.numel() * pooled(flags) * x.shape[3] * ksize * ksize)
        ops.conv3x3_winograd = w(ops.conv3x3_winograd, lambda y, x, u, cout, scale=None, shift=None, residual=None, flags=0:
                                 2.0 * y.numel() * pooled(flags) * x.shape[3] * 9, executed=16.0 / 36.0)
        if hasattr(ops, "conv3x3_winograd4"):
            ops.conv3x3_winograd4 = w(ops.conv3x3_winograd4, lambda y, x, u, cout, scale=None, shift=None, residual=None, flags=0, out=None:
                                      2.0 * y.numel() * pooled(flags) * x.shape[3] * 9, executed=36.0 / 144.0, issued=wino4_issued)
        ops.conv1x1 = w(ops.conv1x1, lambda y, x, packed, cout, *a, **k: 2.0 * y.numel() * x.shape[3])
        if hasattr(ops, "conv1x1_bn"):        # the same GEMM with a train-mode BatchNorm folded in on either side (round 4)
            ops.conv1x1_bn = w(ops.conv1x1_bn, lambda y, x, packed, cout, *a, **k: 2.0 * y[0].numel() * x.shape[3])
            ops.conv1x1_bwd_bnmask = w(ops.conv1x1_bwd_bnmask, lambda y, dy, packed_t, cin, *a, **k: 2.0 * y[0].numel() * dy.shape[3])
        ops.conv_transpose3x3s2 = w(ops.conv_transpose3x3s2, lambda y, x, packed, bias, cout, *a, **k: 2.0 * x.numel() * cout * 9,
                                    kernel_launches=4)        # the sub-pixel ops are four kernel launches each
        ops.conv_transpose4x4s2 = w(ops.conv_transpose4x4s2, lambda y, x, packed, cout, *a, **k: 2.0 * x.numel() * cout * k.get("direct_taps", 16),
                                    kernel_launches=4, executed=lambda k: 16.0 / k.get("direct_taps", 16))
        ops.conv_transpose4x4s2_winograd = w(ops.conv_transpose4x4s2_winograd, lambda y, x, u4, cout, *a, **k: 2.0 * x.numel() * cout * k.get("direct_taps", 16),
                                             kernel_launches=4, executed=lambda k: 9.0 / k.get("direct_taps", 16))     # minimal filtering: 9 multiplications
        if hasattr(ops, "conv_transpose4x4s2_winograd4"):     # F(4x4,2x2): 25 multiplications per 4x4 outputs of a phase (64 direct)
            ops.conv_transpose4x4s2_winograd4 = w(ops.conv_transpose4x4s2_winograd4, lambda y, x, u4, cout, *a, **k: 2.0 * x.numel() * cout * k.get("direct_taps", 16),
                                                  kernel_launches=4, executed=lambda k: 6.25 / k.get("direct_taps", 16))
        if hasattr(ops, "conv4x4s2_winograd4"):
            ops.conv4x4s2_winograd4 = w(ops.conv4x4s2_winograd4, lambda y, dy, u4, cin: 2.0 * y.numel() * dy.shape[3] * 16,
                                        kernel_launches=4, executed=6.25 / 16.0)
        ops.conv4x4s2_winograd = w(ops.conv4x4s2_winograd, lambda y, dy, u4, cin: 2.0 * y.numel() * dy.shape[3] * 16,
                                   kernel_launches=4, executed=9.0 / 16.0)
        ops.conv_transpose3x3s2_f16x3 = w(ops.conv_transpose3x3s2_f16x3, lambda y, x, amax, p16, cout, *a, **k: 2.0 * x.numel() * cout * 9,
                                          kernel_launches=4)
        ops.conv_transpose4x4s2_f16x3 = w(ops.conv_transpose4x4s2_f16x3, lambda y, x, amax, p16, cout, *a, **k: 2.0 * x.numel() * cout * k.get("direct_taps", 16),
                                          kernel_launches=4, executed=lambda k: 16.0 / k.get("direct_taps", 16))
        ops.conv2d_amax = w(ops.conv2d_amax, lambda y, x, packed, cout, ksize, *a, **k: 2.0 * y[0].numel() * x.shape[3] * ksize * ksize)
        ops.conv2d_f16x3 = w(ops.conv2d_f16x3,
                             lambda y, x, amax, p16, cout, ksize, scale=None, shift=None, residual=None, flags=0, want_amax=True:
                             2.0 * y[0].numel() * pooled(flags) * x.shape[3] * ksize * ksize)

    def wrap(self, orig, flops_of, kernel_launches=1, executed=1.0, issued=None, family="other"):
        """executed: executed MACs / direct-algorithm MACs of this operator (Winograd F(2x2): 16 / 36), or a callable of the kwargs.
        issued: FLOPs of the multiplications the kernel really issues (tile and channel padding included), default = executed."""
        def wrapper(*a, **k):
            if not self.recording or k.get("relu_mask") is not None:     # conv3x3(relu_mask=..) forwards to conv2d: timed there
                return orig(*a, **k)
            s_ev = self.torch.cuda.Event(enable_timing=True)
            e_ev = self.torch.cuda.Event(enable_timing=True)
            s_ev.record()
            y = orig(*a, **k)
            e_ev.record()
            fl = flops_of(y, *a, **k)
            ex = fl * (executed(k) if callable(executed) else executed)
            self.events.append((s_ev, e_ev, fl, kernel_launches, ex, family, issued(y, *a, **k) if issued is not None else ex))
            return y
        return wrapper

    def summary(self):
        per = {}
        for ev in self.events:
            f = per.setdefault(ev[5], {"ms": 0.0, "flops": 0.0, "launches": 0, "executed": 0.0, "issued": 0.0})
            f["ms"] += ev[0].elapsed_time(ev[1])
            f["flops"] += ev[2]
            f["launches"] += ev[3]
            f["executed"] += ev[4]
            f["issued"] += ev[6]
        return {"ms": sum(f["ms"] for f in per.values()), "flops": sum(f["flops"] for f in per.values()),
                "launches": sum(f["launches"] for f in per.values()), "executed": sum(f["executed"] for f in per.values()),
                "families": per}


class Context:
    pass


def build_network(ctx, spec):
    import io
    import contextlib
    import torch
    import cases
    import dream_amd
    n_kp, manip = ARCH_K[spec["arch"]]
    cfg = dream_amd.default_network_config(spec["arch"], manip, batch_size=spec["batch"])
    cfg["training"]["config"]["net_input_resolution"] = [spec["res"], spec["res"]]
    # an empty gpu_ids list means "every visible GPU" in one process (the reference's DataParallel contract); this process
    # drives exactly the device(s) it was given
    cfg["training"]["platform"]["gpu_ids"] = list(ctx.single_ids) if ctx.single else [ctx.device_index]
    with contextlib.redirect_stdout(io.StringIO()):
        net = dream_amd.create_network_from_config_data(cfg)
    net.model.load_state_dict(synthetic_weights(net.model.state_dict()))
    from dream_amd import ops
    net.model.module.conv_algorithm = "direct" if spec["conv_algorithm"] == "direct" else "winograd"
    ops.set_winograd_tile(2 if spec["conv_algorithm"] == "winograd2" else 0)
    frames = spec["batch"] * (len(ctx.single_ids) if ctx.single else 1)               # frames this PROCESS handles per step
    seeds = list(range(spec["concat_ranks"])) if spec.get("concat_ranks") else [ctx.rank]
    if len(seeds) > 1:
        frames = spec["batch"] * len(seeds)
    per = frames // len(seeds)
    x = torch.cat([torch.from_numpy(cases.image_batch(per, spec["res"], spec["res"], seed=sd)) for sd in seeds]).cuda()
    tgt = None
    if spec["mode"] == "train":
        net.enable_training()
        ow, oh = net.trained_net_output_resolution()
        tgt = torch.cat([torch.from_numpy(cases.target_batch(per, n_kp, (ow, oh), in_wh=(spec["res"], spec["res"]), seed=sd))
                         for sd in seeds]).cuda()
    else:
        net.enable_evaluation()
        net.hip_graph = bool(spec.get("graph"))
        if spec.get("precision", "fp32") != "fp32":
            net.model.module.precision = spec["precision"]
    n_dev = len(net.model.devices())
    assert n_dev == (len(ctx.single_ids) if ctx.single else 1), "network spreads over %d devices" % n_dev
    return net, x, tgt, frames


def timed_region(ctx, net, x, tgt, spec):
    """W warm-up steps, then exactly K steps between barrier+synchronize pairs; max over ranks.
    -> (seconds, conv timer summary, output of the last step)."""
    import torch
    import torch.distributed as dist
    timer = ctx.timer

    def step():
        if spec["mode"] == "train":
            loss = net.train([x], tgt)
            if spec.get("dp_check"):
                ctx.losses.append(loss.detach().double().reshape(1).clone())
            return loss
        with torch.no_grad():
            return net.inference(x)

    def sync():
        if ctx.single:
            for i in set(ctx.single_ids):
                torch.cuda.synchronize(i)
        else:
            torch.cuda.synchronize()

    def barrier():
        if ctx.world > 1:
            dist.barrier()

    del timer.events[:]
    for _ in range(spec["warmup"]):
        step()
    # experiment switch (tools/gpu_round.sh gcx): the cyclic garbage collector during the timed steps -- "off": disabled, "freeze": every
    # object alive after the warm-up moved to the permanent generation (a full collection then has little to traverse)
    _gc_mode = os.environ.get("DREAM_BENCH_GC", "")
    if _gc_mode in ("off", "freeze"):
        import gc
        gc.collect()
        if _gc_mode == "off":
            gc.disable()
        else:
            gc.freeze()
    if os.environ.get("DREAM_BENCH_PMC_CALIBRATE") == "1":
        # the HBM-traffic PMC passes (tools/pmc_traffic.py): two stand-alone max-pool launches on tensors of known size, OUTSIDE the
        # timed region -- pure streaming reads whose algorithmic byte count is exact, against which the FETCH_SIZE counter's unit
        # on this device is calibrated (every pool of the product path is fused into a conv epilogue since round 3)
        from dream_amd import ops as _ops
        for shape in ((spec["batch"], 100, 100, 256), (spec["batch"], 50, 50, 512)):
            _ops.maxpool2(torch.ones(shape, dtype=torch.float32, device="cuda"))
    sync()
    barrier()
    timer.recording = not spec.get("graph") and not ctx.single        # events cannot be timed inside a captured graph
    sync()
    t0 = time.perf_counter()
    out = None
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(spec["steps"] + 1)] if not ctx.single else []
    host = [t0]
    if marks:
        marks[0].record()
    for i in range(spec["steps"]):
        out = step()
        if marks:
            marks[i + 1].record()                   # (no synchronisation: the events ride on the stream the step ends on)
        host.append(time.perf_counter())
    sync()
    barrier()
    dt = time.perf_counter() - t0
    timer.recording = False
    # per-step GPU time between consecutive end-of-step events and host enqueue time per step: an occasional slow run (round 5: about one
    # 10-step run in eight of the ResNet step is 4-8 % slow) shows here as ONE long step or as a uniformly slower run
    ctx.step_ms = None
    if marks:
        gpu = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(spec["steps"]))
        hst = sorted((host[i + 1] - host[i]) * 1e3 for i in range(spec["steps"]))
        ctx.step_ms = {"gpu_min": gpu[0], "gpu_median": gpu[len(gpu) // 2], "gpu_max": gpu[-1],
                       "host_median": hst[len(hst) // 2], "host_max": hst[-1]}
    ctx.rank_seconds = [dt]
    if ctx.world > 1:
        mine = torch.tensor([dt], dtype=torch.float64, device="cuda")
        every = [torch.zeros_like(mine) for _ in range(ctx.world)]
        dist.all_gather(every, mine)
        ctx.rank_seconds = [float(t.item()) for t in every]
        dt = max(ctx.rank_seconds)                  # the contract: MAX over the ranks
    return dt, timer.summary(), out


def dominant_of(conv, steps, peak):
    """The kernel family with the largest share of the timed conv launches (HIP events on the launch stream): its own time per step
    and its fraction of the MFMA peak on the multiplications it issues (tile / channel padding included) and on the useful ones."""
    fams = conv.get("families") or {}
    if not fams:
        return None
    name = max(fams, key=lambda k: fams[k]["ms"])
    f = fams[name]
    sec = f["ms"] * 1e-3
    return {"kernel": name, "ms_per_step": f["ms"] / max(steps, 1), "launches_per_step": f["launches"] / max(steps, 1),
            "share_of_conv_time": f["ms"] / conv["ms"] if conv["ms"] > 0 else None,
            "direct_frac": f["flops"] / sec / 1e12 / peak if sec > 0 else None,
            "issued_frac": f["issued"] / sec / 1e12 / peak if sec > 0 else None,
            "useful_frac": f["executed"] / sec / 1e12 / peak if sec > 0 else None}


def roofline_of(spec, conv, dt, peak):
    ms, fl, ex = conv["ms"], conv["flops"], conv["executed"]
    wino = spec["conv_algorithm"] != "direct"
    kernel = (("conv_wino4_kernel + " if spec["conv_algorithm"] == "winograd" else "") + "conv_wino_kernel + conv_mfma_kernel" if wino else "conv_mfma_kernel") + \
             (" + gemm1x1_kernel" if spec["arch"].startswith("resnet") else "")
    if spec.get("precision", "fp32") != "fp32" and spec["mode"] == "inference":
        kernel = "conv_f16x3_kernel"
    return {
        "bound": "mfma", "kernel": kernel,
        "achieved": fl / (ms * 1e-3) / 1e12 if ms > 0 else None, "peak": peak, "unit": "TFLOP/s",
        "frac": (fl / (ms * 1e-3) / 1e12 / peak) if ms > 0 else None,
        # frac above counts the DIRECT algorithm's FLOPs; executed_frac counts the multiplications the kernels
        # actually issue (Winograd F(2x2,3x3) 16/36 of direct, upsample + conv as a transposed conv by minimal filtering 9/36)
        "executed_frac": (ex / (ms * 1e-3) / 1e12 / peak) if ms > 0 else None,
        "executed_over_direct": ex / fl if fl > 0 else None,
        "launches": conv["launches"], "avg_launch_ms": ms / max(conv["launches"], 1),
        "algorithmic_gflop_per_launch": fl / max(conv["launches"], 1) / 1e9,
        "share_of_step_time": ms * 1e-3 / dt if dt > 0 else None,
        "dominant": dominant_of(conv, spec["steps"], peak),
    }


def workload_text(spec, n_kp, manip, baseline_index=None):
    what = ("forward + MSE belief-map loss + backward + Adam step (DreamNetwork.train)" if spec["mode"] == "train"
            else "CNN forward + belief-map peak extraction (DreamNetwork.inference)")
    return ("DREAM-%s (%s, %d keypoints) %s, batch %d per GPU, synthetic %dx%d RGB frames resident in HBM; %s%s"
            % (spec["arch"], manip, n_kp, spec["mode"], spec["batch"], spec["res"], spec["res"], what,
               " (BASELINE.json configs[%d])" % baseline_index if baseline_index is not None else ""))


def run_side_workload(ctx, spec, label, baseline_index, sharded_total=None):
    """One more configuration under the same clock -> a compact result block."""
    import gc
    import torch
    net, x, tgt, frames = build_network(ctx, spec)
    dt, conv, _ = timed_region(ctx, net, x, tgt, spec)
    n_kp, manip = ARCH_K[spec["arch"]]
    total = frames * spec["steps"] * ctx.world
    roof = roofline_of(spec, conv, dt, PEAK_F32_MFMA_TFLOPS)
    roof["traffic"] = pmc_traffic(spec)                   # bytes per conv launch from the PMC passes of this bench.py, or null
    block = {"config": label, "workload": workload_text(spec, n_kp, manip, baseline_index),
             "value": total / dt, "unit": "frames/s", "ms_per_step": dt / spec["steps"] * 1e3, "step_ms": ctx.step_ms, "steps": spec["steps"],
             "warmup": spec["warmup"], "batch_per_gpu": spec["batch"], "dtype": "f32",
             "roofline": {k: roof[k] for k in ("kernel", "achieved", "peak", "unit", "frac", "executed_frac", "share_of_step_time", "dominant", "traffic",
                                              "algorithmic_gflop_per_launch", "launches")}}
    if sharded_total is not None:
        n = ctx.n_gpus
        block.update({"global_batch": sharded_total, "scaling": "strong", "per_gpu_frames_per_s": total / dt / n,
                      "rccl_ranks": ctx.rccl_ranks,
                      "ms_per_step_ranks": {"min": min(ctx.rank_seconds) / spec["steps"] * 1e3, "max": max(ctx.rank_seconds) / spec["steps"] * 1e3}})
    del net, x, tgt
    gc.collect()
    torch.cuda.empty_cache()
    return block


def dp_check(ctx, net):
    """--dp-check: per-step losses averaged over the ranks, and the largest difference of any parameter between the ranks."""
    import torch
    import torch.distributed as dist
    losses = torch.cat(ctx.losses) if ctx.losses else torch.zeros(0, dtype=torch.float64, device="cuda")
    flat = torch.cat([p.detach().reshape(-1) for p in net.model.parameters()])
    hi, lo = flat.clone(), flat.clone()
    if ctx.world > 1:
        dist.all_reduce(losses, op=dist.ReduceOp.SUM)
        losses /= ctx.world
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    return {"losses": [float(v) for v in losses.cpu()], "param_spread_between_ranks": float((hi - lo).abs().max()),
            "param_l2": float(flat.double().norm()), "ranks": ctx.world}


DUMP_BYTES = 64 * 10 ** 6


def dump_outputs(out, mode, directory):
    """--dump-outputs: what a caller of the timed path received from its last step, as DIR/<name>.npy in float32 -- the belief maps
    [B,K,H,W] and the keypoints [B,K,2] of an inference step, the loss of a training step.  Beyond DUMP_BYTES in all, the same fixed
    seeded sample of the frames is kept from every array (their indices in sampled_frames.npy).  -> the names written."""
    import numpy as np
    named = [("loss", out)] if mode == "train" else [("belief_maps", out[0]), ("keypoints", out[1])]
    arrays = {n: t.detach().float().cpu().numpy() for n, t in named}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_BYTES:
        frames = arrays["belief_maps"].shape[0]
        keep = max(1, frames * (DUMP_BYTES - 2 ** 16) // (total + 8 * frames))      # room for the headers and the indices
        idx = np.sort(np.random.default_rng(0).choice(frames, keep, replace=False))
        arrays = {n: np.ascontiguousarray(a[idx]) for n, a in arrays.items()}
        arrays["sampled_frames"] = idx.astype(np.float64)
    os.makedirs(directory, exist_ok=True)
    for n, a in arrays.items():
        np.save(os.path.join(directory, n + ".npy"), a)
    return sorted(arrays)


def main():
    """A failure (RCCL initialisation on a multi-GPU node, a device that is missing ...) leaves ONE JSON line with an `error` field (from
    the rank that failed) and a non-zero exit status instead of N interleaved tracebacks, so that a SCALE record is diagnosable."""
    args = parse()
    stage = ["start"]
    try:
        return _main(args, stage)
    except SystemExit:
        raise
    except BaseException as e:  # noqa: BLE001
        import traceback
        # the FAILING rank prints the line, tagged with its rank (rank 0 is usually blocked in a collective when another rank fails; the
        # launcher then ends the group): one line per failing rank, normally exactly one
        print(json.dumps({"metric": "frames/s DREAM-%s %dx%d b=%d %s" % (args.arch.replace("_", "-"), args.res, args.res, args.batch, args.mode),
                          "value": None, "unit": "frames/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
                          "error": "%s during %s: %s" % (type(e).__name__, stage[0], str(e)[:600]),
                          "rank": int(os.environ.get("RANK", "0")), "world_size": int(os.environ.get("WORLD_SIZE", "1"))}), flush=True)
        traceback.print_exc(file=sys.stderr)
        raise SystemExit(1)


def _main(args, stage):
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and not args.single_process:
        self_launch(args)
    import torch
    import torch.distributed as dist
    import dream_amd  # noqa: F401
    from dream_amd import ops

    ctx = Context()
    ctx.world = int(os.environ.get("WORLD_SIZE", "1"))
    ctx.rank = int(os.environ.get("RANK", "0"))
    ctx.single = bool(args.single_process and ctx.world == 1 and args.gpus > 1)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    assert ctx.world == args.gpus or ctx.single or (ctx.world == 1 and args.gpus == 1), \
        "launched with %d ranks but --gpus %d" % (ctx.world, args.gpus)
    # One process per GPU over RCCL.  (Rehearsal of the N > 1 path on a single-GPU box: DREAM_BENCH_BACKEND=gloo lets
    # the ranks share device 0 -- RCCL refuses two ranks on one device; numbers from such a run mean nothing.)
    backend = os.environ.get("DREAM_BENCH_BACKEND", "nccl")
    ctx.device_index = local_rank % torch.cuda.device_count()   # == local_rank unless the launcher exposes one device per rank
    torch.cuda.set_device(ctx.device_index)
    ids = os.environ.get("DREAM_BENCH_GPU_IDS")                 # 0,0: rehearsal of the N-replica path on a one-GPU box
    ctx.single_ids = ([int(v) for v in ids.split(",")] if ids else list(range(args.gpus))) if ctx.single else [ctx.device_index]
    ctx.n_gpus = len(ctx.single_ids) if ctx.single else ctx.world
    assert ctx.n_gpus == args.gpus, "running on %d GPUs but --gpus %d" % (ctx.n_gpus, args.gpus)
    if ctx.world == 1 and os.environ.get("DREAM_FORCE_REDUCER"):      # rehearsal: exercise the gradient exchange with one rank
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29555")
        dist.init_process_group("gloo", rank=0, world_size=1)
    stage[0] = "process-group initialisation (%s, %d ranks)" % ("RCCL" if backend == "nccl" else backend, ctx.world)
    if ctx.world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", ctx.device_index))
        else:
            dist.init_process_group(backend)
    ctx.losses = []
    # ranks of the RCCL (= nccl) process group; 1: one rank, no collective; 0: no RCCL process group at all (the single-process path's
    # exchange is csrc/collective.hip's own communicator; a gloo rehearsal of the N-rank path on a one-GPU box)
    ctx.rccl_ranks = dist.get_world_size() if ctx.world > 1 and backend == "nccl" else (1 if ctx.world == 1 and not ctx.single else 0)
    ctx.backend = backend if ctx.world > 1 else ("single-process" if ctx.single else "none")
    if args.global_batch:
        assert args.global_batch % ctx.n_gpus == 0, "--global-batch must divide evenly over the GPUs"
        args.batch = args.global_batch // ctx.n_gpus
    ctx.timer = ConvTimer(ops, torch)

    spec = {"arch": args.arch, "mode": args.mode, "batch": args.batch, "res": args.res, "steps": args.steps,
            "warmup": args.warmup, "precision": args.precision, "conv_algorithm": args.conv_algorithm, "graph": args.graph,
            "dp_check": args.dp_check and args.mode == "train", "concat_ranks": args.concat_ranks}
    n_kp, manip = ARCH_K[args.arch]
    stage[0] = "network construction"
    net, x, tgt, frames = build_network(ctx, spec)
    stage[0] = "the timed region (first RCCL collective in it for N > 1)"
    dt, conv, out_main = timed_region(ctx, net, x, tgt, spec)
    main_rank_seconds = list(ctx.rank_seconds)
    main_step_ms = ctx.step_ms
    if args.dump_outputs and ctx.rank == 0 and out_main is not None:
        stage[0] = "writing the outputs (--dump-outputs)"
        dump_outputs(out_main, args.mode, args.dump_outputs)
    check = dp_check(ctx, net) if spec["dp_check"] else None
    stage[0] = "reporting"
    # roofline peak: the fp32 MFMA rate for the exact kernel; for the split kernel every algorithmic MAC costs three
    # fp16 MFMA MACs, so its ceiling in ALGORITHMIC flops is the dense fp16 MFMA peak / 3
    peak = PEAK_F32_MFMA_TFLOPS if args.precision == "fp32" or args.mode == "train" else PEAK_F16_MFMA_TFLOPS / 3.0

    # optional informational leg (--split-leg): the same workload on the split-precision conv kernel (fp32 in/out, 3 fp16 MFMAs
    # per product).  The headline `value` stays the exact-fp32 path unless --precision fp16x3 is given explicitly.
    split = None
    if args.mode == "inference" and args.precision == "fp32" and args.split_leg and not args.no_split_leg and not ctx.single:
        net.model.module.precision = "fp16x3"
        dt2, conv2, out2 = timed_region(ctx, net, x, tgt, spec)
        net.model.module.precision = "fp32"
        diff = float((out_main[0] - out2[0]).abs().max())
        scale = max(1.0, float(out_main[0].abs().max()))
        k32, k16 = out_main[1], out2[1]
        both = (k32 != -999.999) & (k16 != -999.999)
        ach2 = conv2["flops"] / (conv2["ms"] * 1e-3) / 1e12 if conv2["ms"] > 0 else None
        split = {"value": frames * args.steps * ctx.world / dt2, "unit": "frames/s", "ms_per_step": dt2 / args.steps * 1e3,
                 "dtype": "f32 in/out; products as 3 x f16 MFMA (hi*hi + hi*lo + lo*hi), f32 accumulate",
                 "roofline": {"bound": "mfma", "kernel": "conv_f16x3_kernel",
                              "achieved": ach2, "peak": PEAK_F16_MFMA_TFLOPS / 3.0, "unit": "TFLOP/s",
                              "frac": ach2 / (PEAK_F16_MFMA_TFLOPS / 3.0) if ach2 else None, "launches": conv2["launches"],
                              "note": "algorithmic FLOPs; each costs 3 f16 MFMA MACs, so the ceiling is 2500/3 TFLOP/s"},
                 "max_abs_diff_vs_fp32_path": diff, "tolerance": 1e-4 * scale,
                 "max_keypoint_diff_px": float((k32 - k16).abs()[both].max()) if bool(both.any()) else 0.0,
                 "detections_agree": float(((k32 == -999.999) == (k16 == -999.999)).float().mean())}
    del net, x, tgt, out_main
    import gc
    gc.collect()
    torch.cuda.empty_cache()

    # ---- the other BASELINE.json configurations under the same clock -------------------------------------------------------
    side = None
    default_main = (args.arch, args.mode, args.res, args.precision, args.conv_algorithm) == ("vgg_q", "inference", 400, "fp32", "winograd") \
        and not args.global_batch and not args.graph
    if default_main and args.full and not args.no_secondary:
        base = {"res": 400, "steps": args.secondary_steps, "warmup": 1, "precision": "fp32", "conv_algorithm": "winograd"}
        # a training step is in its steady state from the third on (the first records which packed weight copies it builds, the
        # second builds the one-launch packing table: models._repack_weights)
        train = dict(base, warmup=3, steps=args.secondary_train_steps)
        side = []
        if ctx.n_gpus == 1:
            side.append(run_side_workload(ctx, dict(train, arch="vgg_q", mode="train", batch=128), "configs[2]", 2))
            side.append(run_side_workload(ctx, dict(train, arch="resnet_h", mode="train", batch=16),
                                          "configs[3], one GPU's share (16 of 128 frames)", None))
            side.append(run_side_workload(ctx, dict(base, arch="resnet_f", mode="inference", batch=32),
                                          "configs[4], one GPU's share (32 of 256 frames)", None))
        else:
            n = ctx.n_gpus
            if 128 % n == 0:
                side.append(run_side_workload(ctx, dict(train, arch="resnet_h", mode="train", batch=128 // n), "configs[3]", 3,
                                              sharded_total=128))
            if 256 % n == 0:
                side.append(run_side_workload(ctx, dict(base, arch="resnet_f", mode="inference", batch=256 // n), "configs[4]", 4,
                                              sharded_total=256))

    if ctx.rank == 0:
        total = frames * args.steps * ctx.world
        roof = roofline_of(spec, conv, dt, peak)
        roof["traffic"] = pmc_traffic(spec)
        roof["traffic_unit"] = "bytes/launch (PMC passes of this bench.py, profiles/rNN_pmc_traffic.json; null when none matches)"
        line = {
            "metric": "frames/s DREAM-%s %dx%d b=%d %s" % (args.arch.replace("_", "-"), args.res, args.res, args.batch, args.mode),
            "value": total / dt, "unit": "frames/s", "n_gpus": ctx.n_gpus, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "step_ms": main_step_ms, "higher_is_better": True,
            "scaling": "strong" if args.global_batch else "weak",
            "vs_baseline": None, "dtype": "f32" if args.precision == "fp32" else "f32 (f16x3 split MFMA, f32 accumulate)",
            "data": "synthetic",
            "rccl_ranks": ctx.rccl_ranks, "collective_backend": ctx.backend,
            "per_gpu_frames_per_s": total / dt / ctx.n_gpus,
            "ms_per_step_ranks": {"min": min(main_rank_seconds) / args.steps * 1e3, "max": max(main_rank_seconds) / args.steps * 1e3},
            "config": {"workload": workload_text(spec, n_kp, manip, (2 if args.mode == "train" else 1)
                                                 if (args.arch, args.batch, args.res) == ("vgg_q", 128, 400) else None),
                       "batch_per_gpu": args.batch, "resolution": [args.res, args.res],
                       "parallelism": "dp%d%s" % (ctx.n_gpus, " (single process, gpu_ids)" if ctx.single
                                                  else (" (one process per GPU, %s)" % ("RCCL" if backend == "nccl" else backend)
                                                        if ctx.world > 1 else "")),
                       "conv_algorithm": (("winograd F(4x4,3x3) for the stride-1 3x3 convs with >= 48 output channels where the map and the batch "
                                           "fill its 4x4 tiles (wide workgroup shape from 128 output channels, narrow shape for 48-64), F(2x2,3x3) "
                                           "on the remaining stride-1 3x3 convs and the transposed-conv phases, direct implicit GEMM elsewhere" if args.conv_algorithm == "winograd" else
                                           "winograd F(2x2,3x3) for the stride-1 3x3 convs with >= 64 output channels, direct implicit GEMM "
                                           "elsewhere" if args.conv_algorithm == "winograd2" else "direct implicit GEMM")
                                          + ("; stride-1 1x1 convs as LDS-free GEMMs" if args.arch.startswith("resnet") else ""))},
            "roofline": roof,
        }
        if split is not None:
            line["split_precision"] = split
        if check is not None:
            line["dp_check"] = check
        if side:
            line["secondary" if ctx.n_gpus == 1 else "scale"] = side
        if args.full and ctx.world == 1 and not ctx.single and not args.no_cpu_baseline and args.mode == "inference":
            line["cpu_baseline"] = cpu_baseline(args.arch, args.res, args.cpu_seconds)
        print(json.dumps(line), flush=True)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
