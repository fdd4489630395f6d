#!/usr/bin/env python
"""Knock-out timing of the Winograd F(4x4,3x3) kernel: libraries built with -DDREAM_W4_DIAG=k (bit 0: no patch loads, bit 1: no
weight stream, bit 2: no barriers, bit 3: no pass 1 / pass 2, bit 7: no epilogue, bit 8: epilogue without stores; results are wrong by construction) against the product library, same
layer, same box.  `build` runs here (hipcc), `run` on the GPU box.   python tools/wino4_diag.py build | run [--batch 128] [--narrow]
--narrow: the layers of the narrow workgroup shape (up to 64 output channels).  Variant 7000 is the narrow shape with the
position-major weight layout (one dwordx2 load per position, -DDREAM_W4_NARROW_PAIRS=0); it packs its own weights."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = [128, 256, 15, 2, 32, 64, 96]          # 1000 + r: product code with weight-ring size r; 2001..: schedule variants
if os.environ.get("DREAM_W4_DIAG_KS"):          # a subset of the variants: DREAM_W4_DIAG_KS=1008,128
    KS = [int(v) for v in os.environ["DREAM_W4_DIAG_KS"].split(",")]
OUT = os.path.join(ROOT, "build", "diag")             # travels with the snapshot only while it exists: `rm -rf build/diag` after the measurement
SCALAR = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops", "-DDREAM_PACKED_F32=0"]     # __graft_entry__.SCALAR_F32_FLAGS
VARIANTS = {4001: SCALAR, 4005: ["-DDREAM_PACKED_F32=1"], 2001: ["-DDREAM_W4_S1=6", "-DDREAM_W4_S2=9", "-DDREAM_W4_LX=3"], 2002: ["-DDREAM_W4_S1=8", "-DDREAM_W4_S2=13", "-DDREAM_W4_LX=3"],
            2003: ["-DDREAM_W4_S1=10", "-DDREAM_W4_S2=13", "-DDREAM_W4_LX=1"], 2004: ["-DDREAM_W4_S1=11", "-DDREAM_W4_S2=14", "-DDREAM_W4_LX=3"],
            2005: ["-DDREAM_W4_S1=4", "-DDREAM_W4_S2=8", "-DDREAM_W4_LX=1"], 7000: SCALAR + ["-DDREAM_W4_NARROW_PAIRS=0"]}
# (the variants of the retired build forks -- cache policies, staggered patch loads, s_setprio, table weight offsets, non-temporal stores, the
# mid-chunk barrier -- went with them: conv_wino4.hip lists their results)
NAMES = {0: "product", 4001: "scalar fp32 VALU (no v_pk_*)", 4005: "packed fp32 VALU", 128: "no epilogue", 256: "epilogue without stores", 143: "MFMAs + operand reads only, no epilogue", 32: "weights from L1 (one position)", 64: "patches: chunk 0 only", 96: "weights from L1 + patches chunk 0", 48: "weights from L1 + patches out of range", 2001: "S1 6 S2 9", 2002: "S1 8 S2 13", 2003: "S1 10 S2 13, loads in slot 0", 2004: "S1 11 S2 14",
         2005: "S1 4 S2 8, loads in slot 0", 16: "patch loads out of range", 18: "patch loads out of range, no weight stream", 1: "no patch loads", 2: "no weight stream", 4: "no barriers", 8: "no passes (loads kept)", 9: "no loads, no passes",
         11: "no loads / passes / weights", 15: "MFMAs + operand reads only", 1006: "weight ring 6 (4 ahead; the product has 8)", 1112: "narrow shape: weight ring 12 (product 18)",
         7000: "narrow shape: one dwordx2 weight load per position (product: one dwordx4 per pair)"}


def variant_flags(k):
    """k < 512: knock-out bits; 1000 + r / 1100 + r: weight ring r of the wide / narrow shape; else a key of VARIANTS."""
    if 0 < k < 512:
        return ["-DDREAM_W4_DIAG=%d" % k]
    if 1000 <= k < 1100:
        return ["-DDREAM_W4_RING=%d" % (k - 1000)]
    if 1100 <= k < 2000:
        return ["-DDREAM_W4_NARROW_RING=%d" % (k - 1100)]
    if k not in VARIANTS:
        sys.exit("wino4_diag: unknown variant %d" % k)
    return VARIANTS[k]


def build():
    os.makedirs(OUT, exist_ok=True)
    csrc = os.path.join(ROOT, "dream_amd", "csrc")
    procs = []
    for k in KS:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
               "-I", os.path.join(csrc, "include")] + variant_flags(k) + [os.path.join(csrc, "conv_wino4.hip"),
               os.path.join(csrc, "conv_wino.hip"), os.path.join(csrc, "api.hip"), "-o", os.path.join(OUT, "libwino4_diag_%d.so" % k)]
        procs.append(subprocess.Popen(cmd))
    assert all(p.wait() == 0 for p in procs)


def run(batch, narrow=False):
    import torch
    from dream_amd import _hip, ops
    libs = {0: _hip.lib()}
    for k in KS:
        variant_flags(k)                              # an unknown number is an error here too
        h = ctypes.CDLL(os.path.join(OUT, "libwino4_diag_%d.so" % k))
        fn = h.dream_conv3x3_winograd4_nhwc_f32
        fn.restype, fn.argtypes = _hip._SIGNATURES["dream_conv3x3_winograd4_nhwc_f32"]
        libs[k] = h
    layers = [(400, 64, 64, 1), (200, 64, 128, 1), (200, 128, 128, 1), (100, 256, 256, 1), (50, 512, 512, 1), (25, 512, 512, 1)]
    if narrow:                                        # conv1_2 (ReLU + fused pool: flags 3) and the decoder's 64-channel layers
        layers = [(400, 64, 64, 3), (100, 128, 64, 1), (100, 64, 64, 1)]
    for (res, cin, cout, flags) in layers:
        x = torch.randn(batch, res, res, cin, device="cuda")
        w = torch.randn(cout, cin, 3, 3, device="cuda") * 0.05
        u, _ = ops.pack_weight_winograd4(w, 0)
        packed = {k: u for k in [0] + KS}
        if 7000 in KS:                                # another weight layout: packed by the variant's own kernel
            packed[7000] = torch.empty_like(u)
            pack = libs[7000].dream_pack_conv3x3_winograd4_weight
            pack.restype, pack.argtypes = _hip._SIGNATURES["dream_pack_conv3x3_winograd4_weight"]
            assert pack(w.data_ptr(), packed[7000].data_ptr(), cout, cin, 0, torch.cuda.current_stream().cuda_stream) == 0
        y = torch.empty(batch, res, res, cout, device="cuda")
        flops = 2.0 * batch * res * res * cin * cout * 9 / 4.0
        # round-robin over the variants, minimum per variant: whatever runs first after a pause is a few per cent slower (clocks),
        # which a variant-by-variant loop books to the first variant
        calls = {}
        for k in [0] + KS:
            fn = libs[k].dream_conv3x3_winograd4_nhwc_f32

            def call(fn=fn, uk=packed[k]):
                rc = fn(x.data_ptr(), uk.data_ptr(), None, None, None, y.data_ptr(), batch, res, res, cin, cout, flags,
                        torch.cuda.current_stream().cuda_stream)
                assert rc == 0
            call()
            calls[k] = call
        torch.cuda.synchronize()
        best = {k: 1e9 for k in calls}
        for _ in range(6):
            for k, call in calls.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                call()
                e.record()
                torch.cuda.synchronize()
                best[k] = min(best[k], s.elapsed_time(e))
        line = ["%s %.3f ms (%.2f)" % (NAMES.get(k, "variant %d" % k), best[k], flops / best[k] / 1e9 / 157.3) for k in calls]
        print("%d %d->%d b=%d: " % (res, cin, cout, batch) + " | ".join(line), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "build":
        build()
    else:
        run(int(sys.argv[sys.argv.index("--batch") + 1]) if "--batch" in sys.argv else 128, "--narrow" in sys.argv)
