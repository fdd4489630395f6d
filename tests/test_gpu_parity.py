"""GPU suite (-m gpu): parity of the real libdream_hip.so (through the C ABI, on an MI355X) with the CPU
oracle and with the committed golden outputs of the real reference.  Nothing here reads /root/reference."""
import os

import numpy as np
import pytest
import torch

import cases
import parity_checks as pc
from dream_amd import _hip, ops
from oracle import models as om
from oracle import peaks as op

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_library():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    _hip.check_symbols()
    with open("/proc/self/maps") as f:
        assert "libdream_hip.so" in f.read(), "the native HIP library is not loaded"
    yield


# ---- every distinct DREAM-vgg-Q conv layer shape, batch 1, at full resolution -----
VGG_Q_LAYERS = [
    (400, 64, 64, 1), (200, 64, 128, 1), (200, 128, 128, 1), (100, 128, 256, 1), (100, 256, 256, 1),
    (50, 256, 512, 1), (50, 512, 512, 1), (25, 512, 512, 1),
    (50, 512, 256, 3), (50, 256, 256, 0), (100, 256, 128, 3), (100, 128, 64, 0),
    (100, 64, 64, 1), (100, 64, 32, 1), (100, 32, 7, 4), (100, 32, 17, 4),
]


@pytest.mark.parametrize("res,cin,cout,flags", VGG_Q_LAYERS)
def test_conv_layer_shapes(res, cin, cout, flags):
    pc.check_conv(DEV, 1, res, res, cin, cout, flags, seed=res + cin)


@pytest.mark.parametrize("variant", range(11))              # every selectable tile variant; the big-patch one: see below
def test_conv_variants(variant):
    lib = _hip.lib()
    lib.dream_conv3x3_set_variant(variant)
    try:
        pc.check_conv(DEV, 2, 33, 47, 64, 96, 1, seed=variant)
        pc.check_conv(DEV, 2, 12, 20, 64, 7, 4, seed=variant)
        pc.check_conv(DEV, 1, 26, 38, 32, 64, 3, seed=variant)
    finally:
        lib.dream_conv3x3_set_variant(-1)


def test_conv_big_patch_variant():
    """Variant 11 (128 px x 128 cout with a 608-pixel patch) is what a strided 3x3 conv runs on, whatever is forced."""
    assert _hip.lib().dream_conv3x3_variant_name(11) == b"m2n2w2x2k16"
    pc.check_conv2d_general(DEV, 2, 37, 51, 64, 160, 3, 2, seed=11)
    pc.check_conv2d_general(DEV, 1, 100, 100, 128, 128, 3, 2, seed=12)


def test_conv_odd_shapes_and_transpose():
    pc.check_conv(DEV, 3, 5, 3, 16, 16, 0)
    pc.check_conv(DEV, 1, 13, 31, 48, 32, 1)
    pc.check_conv(DEV, 2, 133, 100, 64, 64, 1)
    pc.check_conv_transpose(DEV, 2, 25, 25, 64, 32)


def test_first_conv_pool_layouts():
    pc.check_first_conv(DEV, 1, 400, 400)
    pc.check_first_conv(DEV, 2, 21, 37)
    pc.check_pool_and_layouts(DEV)


def test_streaming_forms():
    pc.check_streaming_forms(DEV)


@pytest.mark.parametrize("name", sorted(cases.peak_cases().keys()))
def test_peaks_bit_exact(name):
    pc.check_peaks_case(DEV, name)


def test_peak_rule_settings():
    pc.check_peak_rule_settings(DEV)


def test_peaks_api_reference_kat():
    pc.check_peaks_api(DEV)


def test_softargmax():
    pc.check_softargmax(DEV)


def test_backward_ops():
    pc.check_backward_ops(DEV)


@pytest.mark.parametrize("shape", cases.CNN_CASES["vgg_q"][2])
def test_vgg_q_inference_golden(shape):
    pc.check_model_inference(DEV, "vgg_q", shape)


def test_vgg_f_inference_golden():
    pc.check_model_inference(DEV, "vgg_f", (2, 64, 80))


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_train_steps_golden(opt):
    pc.check_train_steps(DEV, opt, steps=3)


RESNET_LAYERS = [   # (H, Cin, Cout, k, stride): one of each kind in ResNet101 @400x400
    (100, 64, 64, 1, 1), (100, 64, 256, 1, 1), (100, 256, 128, 1, 1), (100, 128, 128, 3, 2), (100, 256, 512, 1, 2),
    (50, 512, 256, 1, 1), (50, 256, 256, 3, 2), (25, 256, 1024, 1, 1), (25, 1024, 512, 1, 1), (25, 512, 512, 3, 2),
    (13, 512, 2048, 1, 1), (13, 2048, 512, 1, 1), (13, 512, 512, 3, 1),
]


@pytest.mark.parametrize("res,cin,cout,k,stride", RESNET_LAYERS)
def test_resnet_layer_shapes(res, cin, cout, k, stride):
    pc.check_conv2d_general(DEV, 2, res, res, cin, cout, k, stride, seed=res + cin + k)


def test_resnet_decoder_and_stem_ops():
    pc.check_conv_transpose4x4(DEV, 2, 13, 13, 2048, 256)
    pc.check_conv_transpose4x4(DEV, 1, 52, 52, 256, 256)
    pc.check_resnet_stem(DEV, 2, 400, 400)


def test_resnet_h_inference_golden():
    pc.check_model_inference(DEV, "resnet_h", (2, 64, 96))


def test_resnet_f_inference_golden():
    pc.check_model_inference(DEV, "resnet_f", (1, 64, 64))


def test_resnet_f_full_resolution_matches_oracle():
    """configs[4] shape (400x400 -> 416x416 maps, 17 keypoints), 2 frames: HIP vs the CPU oracle."""
    net = pc.build_network("resnet_f", DEV)
    net.enable_evaluation()
    ref = om.build_model("resnet_f", 17)
    ref.load_state_dict(om.recipe_weights(ref.state_dict()))
    ref.eval()
    x = torch.from_numpy(cases.image_batch(2, 400, 400, seed=41))
    with torch.no_grad():
        maps, kps = net.inference(x.to(DEV))
        ref_maps = ref(x)[0].numpy()
    assert maps.shape == (2, 17, 416, 416)
    y = maps.cpu().numpy()
    assert np.abs(y - ref_maps).max() <= pc.tol(ref_maps)
    assert np.array_equal(kps.numpy(), op.keypoints_from_belief_maps(y, 0.0))


def test_resnet_training_ops():
    pc.check_resnet_training_ops(DEV)


@pytest.mark.parametrize("case", sorted(cases.RESNET_TRAIN_CASES))
def test_resnet_train_step_reference_golden(case):
    res = pc.check_resnet_train_golden(DEV, case)
    print("resnet train golden", case, res)


def test_bn_fused_ops():
    """Round 4: BatchNorm statistics finished inside the producing launch ("last arriver finishes" across the eight XCDs), BN + ReLU
    in the consumer's loader, the backward reductions in the data-gradient epilogue."""
    pc.check_bn_fused_ops(DEV)


def test_bn_fused_statistics_are_deterministic_and_tickets_rearm():
    """The in-launch finalisation sums the partial rows in a fixed order: repeated launches on one ticket buffer (which every launch
    must leave zero) give the same bits, on a tensor large enough for every XCD to contribute partial rows."""
    torch.manual_seed(5)
    bn = torch.nn.BatchNorm2d(256).to(DEV)
    z = torch.randn(16, 25, 25, 256, device=DEV) * 2 + 0.5
    ctr = torch.zeros(4096, dtype=torch.int32, device=DEV)
    outs = [ops.bn_stats(z, bn, ctr) for _ in range(5)]
    assert int(ctr.abs().sum()) == 0
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))
    ref = z.double().mean((0, 1, 2))
    assert float((outs[0][1].double() - ref).abs().max()) < 1e-6
    w = torch.randn(1024, 256, 1, 1, device=DEV) * 0.05
    packed, rows = ops.pack_conv1x1_weight(w, 0)
    bn2 = torch.nn.BatchNorm2d(1024).to(DEV)
    ctr2 = torch.zeros(4096, dtype=torch.int32, device=DEV)
    runs = [ops.conv1x1_bn(z, packed, rows, bn2, ctr2, pre_ab=outs[0][0]) for _ in range(5)]
    assert int(ctr2.abs().sum()) == 0
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r, runs[0]))
    zz = runs[0][0].double()
    assert float((runs[0][2].double() - zz.mean((0, 1, 2))).abs().max()) < 1e-5 * float(zz.abs().max())


def test_bn_fused_launches_stress_mixed_shapes_two_streams(monkeypatch):
    """Stress of the "last arriver finishes" launches (round-4 advice; the ordering they rely on -- relaxed agent-scope atomics, an
    inline s_waitcnt, sc1 loads -- is outside the formal memory model and cannot be exercised by the CPU emulator): 60 rounds of mixed
    shapes (few rows / many rows per channel block, one- and two-level ticket trees, the K splits of the GEMM) issued on TWO streams
    at once from one shared ticket buffer, under DREAM_BN_DEBUG=1 -- outputs NaN-filled before every launch, finite afterwards, ticket
    words zero again.  Every result must equal the first round's bit for bit and torch's batch statistics to round-off."""
    monkeypatch.setattr(ops, "BN_DEBUG", True)
    torch.manual_seed(11)
    shapes = [(2, 13, 13, 512), (16, 25, 25, 256), (4, 100, 100, 64), (16, 50, 50, 128), (1, 7, 9, 64), (16, 104, 104, 256)]
    zs = [torch.randn(*sh, device=DEV) * 1.5 + 0.25 for sh in shapes]
    bns = [torch.nn.BatchNorm2d(sh[3]).to(DEV) for sh in shapes]
    gemm_in = zs[1]
    w = torch.randn(1024, 256, 1, 1, device=DEV) * 0.05
    packed, rows = ops.pack_conv1x1_weight(w, 0)
    bn_g = torch.nn.BatchNorm2d(1024).to(DEV)
    buf = ops.bn_counter_buffer(torch.device(DEV), words=1 << 14)
    pos = [0]

    def take(n):                                           # as ResnetSimple._ctr: every launch its own slice, the cursor wraps
        if pos[0] + n > buf.numel():
            pos[0] = 0
        out = buf[pos[0]:pos[0] + n]
        pos[0] += n
        return out

    side = torch.cuda.Stream()
    first = None
    for rnd in range(60):
        res = []
        for i, (z, bn) in enumerate(zip(zs, bns)):
            if i % 2:                                      # odd shapes on the side stream, concurrently with the even ones
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    res.append(ops.bn_stats(z, bn, take))
            else:
                res.append(ops.bn_stats(z, bn, take))
        torch.cuda.current_stream().wait_stream(side)
        zg, ab, mean, invstd = ops.conv1x1_bn(gemm_in, packed, rows, bn_g, take, pre_ab=res[1][0])
        dy = zs[1]
        dgam, dbet = ops.bn_bwd_stats(zs[1], dy, res[1][1], res[1][2], take, ab=res[1][0])
        flat = [t for r in res for t in r] + [ab, mean, invstd, dgam, dbet]
        torch.cuda.synchronize()
        if first is None:
            first = [t.clone() for t in flat]
            for z, r in zip(zs, res):
                zd = z.double()
                assert float((r[1].double() - zd.mean((0, 1, 2))).abs().max()) < 1e-5
        else:
            for a, b in zip(flat, first):
                assert torch.equal(a, b), rnd
    assert int(buf.abs().max()) == 0


def test_resnet_h_train_step():
    pc.check_resnet_train_step(DEV, "resnet_h", (4, 128, 128))


def test_resnet_h_train_step_three_launch_batchnorm(monkeypatch):
    """DREAM_BN_FUSION=0: the BatchNorm kernels of rounds 1-3 stay selectable (A/B runs) and correct."""
    monkeypatch.setenv("DREAM_BN_FUSION", "0")
    pc.check_resnet_train_step(DEV, "resnet_h", (4, 128, 128))


def test_resnet_h_train_step_downsample_on_direct_kernels(monkeypatch):
    """DREAM_DS_GEMM=0: the stride-2 downsample convs on the direct kernels (rounds 1-6) stay selectable and correct; the default
    (gathered pixels + 1x1 GEMM in all three directions) is what every other ResNet training test runs."""
    monkeypatch.setenv("DREAM_DS_GEMM", "0")
    pc.check_resnet_train_step(DEV, "resnet_h", (4, 128, 128))


def test_resnet_downsample_on_gemm_is_used_and_close_to_direct(monkeypatch):
    """The default training forward gathers the input of the three stride-2 downsample convs (tape records carry `sub2`), and one
    step's loss and gradients agree with the direct-kernel path (two fp32 algorithms: relative 1e-4 on the loss, direction and norm
    of every gradient)."""
    wts = om.recipe_weights(om.build_model("resnet_h", 7).state_dict(), ("upsample.12.weight", "upsample.12.bias"), 0.1)
    x = torch.from_numpy(cases.image_batch(4, 128, 128, seed=7)).to(DEV)
    runs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("DREAM_DS_GEMM", flag)
        net = _dp_network("resnet_h", [0], optimizer="sgd", lr=0.0, in_res=(128, 128), weights=wts)
        net.enable_training()
        mod = net.model.module
        assert mod.ds_on_gemm == (flag == "1")
        ow, oh = net.trained_net_output_resolution()
        t = torch.from_numpy(cases.target_batch(4, 7, (ow, oh), in_wh=(128, 128), seed=7)).to(DEV)
        if flag == "1":
            with torch.no_grad():
                _, tape = mod.run_forward_train(x)
            assert sum(1 for r in tape if r.get("kind") == "conv" and r.get("sub2") is not None) == 3
        loss = net.train([x], t).item()
        runs.append((loss, [p.grad.clone() for p in net.model.parameters()]))
    assert abs(runs[0][0] - runs[1][0]) <= 1e-4 * abs(runs[1][0])
    top = max(float(b.norm()) for b in runs[1][1])
    checked = 0
    for a, b in zip(runs[0][1], runs[1][1]):
        na, nb = float(a.norm()), float(b.norm())
        if nb > 1e-6 * top:                      # (gradients that are zero in exact arithmetic -- a shift in front of a BatchNorm -- are rounding noise)
            assert float((a * b).sum()) / (na * nb) > 0.999 and abs(na - nb) <= 2e-2 * nb
            checked += 1
    assert checked > 200


def test_resnet_f_train_step():
    pc.check_resnet_train_step(DEV, "resnet_f", (2, 64, 64))


def test_vgg_f_train_step():
    pc.check_vgg_train_grads(DEV, "vgg_f", (2, 64, 96))


def test_every_architecture_branch_constructs_on_the_hip_path():
    import dream_amd
    for patch, cls in (({"n_stages": 2, "deconv_decoder": False, "full_output": True}, "DreamHourglassMultiStage"),
                       ({"skip_connections": True}, "DreamHourglass")):
        cfg = dream_amd.default_network_config("vgg_q")
        cfg["architecture"].update(patch)
        assert type(dream_amd.create_network_from_config_data(cfg).model.module).__name__ == cls
    cfg = dream_amd.default_network_config("vgg_q")
    cfg["architecture"]["loss"]["type"] = "huber"
    assert type(dream_amd.create_network_from_config_data(cfg).criterion).__name__ == "HipSmoothL1Loss"


def test_full_size_batch_properties():
    """BASELINE.json configs[1] size (batch 128 of 400x400): size-independent properties.
    (a) batch-position independence: the batch holds 4 distinct frames repeated 32x; every copy must give
        bit-identical belief maps and keypoints (tiling/XCD placement must not leak into results);
    (b) the first copy equals the CPU oracle within TOL and the peak stage is bit-exact on the HIP maps."""
    net = pc.build_network("vgg_q", DEV)
    net.enable_evaluation()
    base = torch.from_numpy(cases.image_batch(4, 400, 400, seed=77))
    x = base.repeat(32, 1, 1, 1).to(DEV)
    with torch.no_grad():
        maps, kps = net.inference(x)
    maps = maps.cpu()
    assert maps.shape == (128, 7, 100, 100) and kps.shape == (128, 7, 2)
    for r in range(1, 32):
        assert torch.equal(maps[4 * r:4 * r + 4], maps[:4])
        assert torch.equal(kps[4 * r:4 * r + 4], kps[:4])
    ref = om.build_model("vgg_q", 7)
    ref.load_state_dict(om.recipe_weights(ref.state_dict()))
    ref.eval()
    with torch.no_grad():
        ref_maps = ref(base[:2])[0].numpy()
    # ABSOLUTE bound (round 6; was 1e-4 x max|ref| = 1.06e-3 on these recipe-weight maps, which reach 10.6): measured 4.9e-5 on the
    # F(4x4,3x3) path this batch selects -- the north-star's 1e-4 holds on maps ten times the magnitude it was stated for
    err = float(np.abs(maps[:2].numpy() - ref_maps).max())
    print("b=128 recipe-weight maps (max |ref| %.1f): max |error| %.2e absolute" % (float(np.abs(ref_maps).max()), err))
    assert err <= 1e-4, err
    assert np.array_equal(kps[:4].numpy(), op.keypoints_from_belief_maps(maps[:4].numpy(), 0.4395))


def test_first_conv_pair_in_sub_batches_same_bits(monkeypatch):
    """DREAM_FIRST_SUBBATCH=n (round 6, dream/models.py:591-599): conv1_1 -> conv1_2 (+ pool) of an inference pass over sub-batches of n
    frames, the full-resolution 64-channel tensor between them an n-frame buffer that stays in the Infinity Cache.  Same kernels on
    the same frames: bit-identical maps and keypoints; the two layers really run per sub-batch."""
    net = pc.build_network("vgg_q", DEV)
    net.enable_evaluation()
    x = torch.from_numpy(cases.image_batch(8, 400, 400, seed=12)).to(DEV)
    with torch.no_grad():
        maps0, kps0 = net.inference(x)
    calls = []
    orig = ops.conv3x3_first
    monkeypatch.setattr(ops, "conv3x3_first", lambda *a, **k: calls.append(int(a[0].shape[0])) or orig(*a, **k))
    monkeypatch.setenv("DREAM_FIRST_SUBBATCH", "2")
    with torch.no_grad():
        maps1, kps1 = net.inference(x)
    assert calls == [2, 2, 2, 2], calls
    assert torch.equal(maps0, maps1) and torch.equal(kps0, kps1)


def test_full_size_peak_stage():
    """896 maps of 100x100 (batch 128 x 7): gaussian linearity-free check -- compare a strided subset
    with the oracle bit-for-bit and all counts with a NumPy recount on the device-smoothed maps."""
    rs = np.random.RandomState(5)
    maps = (rs.normal(0.05, 0.05, (896, 100, 100))).astype(np.float32)
    maps[::3, 40:49, 50:59] += 0.8
    m = torch.from_numpy(maps).to(DEV)
    sm = ops.gaussian_sigma3(m).cpu().numpy()
    kps, counts = ops.keypoints_from_belief_maps(m.view(128, 7, 100, 100), 0.4395)
    kps, counts = kps.cpu().numpy().reshape(896, 2), counts.cpu().numpy().reshape(896)
    for i in range(0, 896, 37):
        assert np.array_equal(sm[i], op.gaussian_filter_sigma3(maps[i]))
        assert np.array_equal(kps[i][None], op.keypoints_from_belief_maps(maps[i][None, None], 0.4395)[0])
    for i in range(896):
        assert counts[i] == int(op.peak_mask(sm[i]).sum())


# ---- split-precision (fp16x3) path ------------------------------------------------------------------------------
@pytest.mark.parametrize("res,cin,cout,flags", [l for l in VGG_Q_LAYERS if l[1] % 32 == 0])
def test_split_precision_layer_shapes(res, cin, cout, flags):
    pc.check_conv_f16x3(DEV, 1, res, res, cin, cout, 3, flags, seed=res + cin)


def test_split_precision_variants_and_scales():
    lib = _hip.lib()
    for v in range(6):
        lib.dream_conv_f16x3_set_variant(v)
        try:
            pc.check_conv_f16x3(DEV, 2, 33, 47, 64, 96, 3, 1, seed=v)
            pc.check_conv_f16x3(DEV, 2, 12, 20, 64, 7, 3, 4, x_scale=300.0, w_scale=1e-3, seed=v)
            pc.check_conv_f16x3(DEV, 1, 26, 38, 32, 64, 3, 3, x_scale=1e-3, w_scale=5.0, seed=v)
            pc.check_conv_f16x3(DEV, 2, 25, 25, 512, 128, 1, 0, seed=v)
        finally:
            lib.dream_conv_f16x3_set_variant(-1)


@pytest.mark.parametrize("shape", cases.CNN_CASES["vgg_q"][2])
def test_vgg_q_inference_golden_split_precision(shape):
    pc.check_model_inference(DEV, "vgg_q", shape, precision="fp16x3")


def test_vgg_f_inference_golden_split_precision():
    pc.check_model_inference(DEV, "vgg_f", (2, 64, 80), precision="fp16x3")


def test_split_precision_vs_fp32_path_full_size():
    """B=16 of 400x400: the two conv paths must agree far inside the 1e-4 tolerance and give the same detections."""
    net = pc.build_network("vgg_q", DEV)
    net.enable_evaluation()
    x = torch.from_numpy(cases.image_batch(16, 400, 400, seed=5)).to(DEV)
    with torch.no_grad():
        m32, k32 = net.inference(x)
        net.model.module.precision = "fp16x3"
        m16, k16 = net.inference(x)
    scale = max(1.0, float(m32.abs().max()))
    assert float((m32 - m16).abs().max()) <= 0.25 * pc.TOL * scale
    same = (k32 == -999.999) == (k16 == -999.999)
    assert same.float().mean() >= 0.97
    both = (k32 != -999.999) & (k16 != -999.999)
    assert float((k32 - k16).abs()[both].max()) < 0.05


def test_fused_maxpool_epilogue():
    for (res, cin, cout) in [(400, 64, 64), (200, 128, 128), (100, 256, 256), (50, 512, 512), (37, 64, 96)]:
        pc.check_conv(DEV, 1, res, res, cin, cout, 1 | 16, seed=res)
        pc.check_conv_f16x3(DEV, 1, res, res, cin, cout, 3, 1 | 16, seed=res)


def test_on_device_dataprep():
    pc.check_dataprep(DEV)


def test_resnet_split_precision():
    pc.check_conv_transpose4x4_f16x3(DEV, 2, 13, 13, 2048, 256)
    pc.check_conv_transpose4x4_f16x3(DEV, 1, 52, 52, 256, 256)
    pc.check_model_inference(DEV, "resnet_h", (2, 64, 96), precision="fp16x3")
    pc.check_model_inference(DEV, "resnet_f", (1, 64, 64), precision="fp16x3")


@pytest.mark.parametrize("name", sorted(cases.VARIANT_CASES))
def test_hourglass_variants(name):
    pc.check_variant(DEV, name)


@pytest.mark.parametrize("name", ["vgg_q_skip", "vgg_f_ms2_skip", "vgg_ms2", "vgg_ms3_full"])
def test_hourglass_variants_split_precision(name):
    pc.check_variant(DEV, name, precision="fp16x3")


@pytest.mark.parametrize("arch,shape", [("vgg_q", (1, 400, 400)), ("resnet_h", (2, 64, 96)), ("vgg_q", (3, 50, 75))])
def test_hip_graph_inference_is_bit_identical(arch, shape):
    """DreamNetwork.hip_graph: the captured launch sequence replays to exactly the eager results, for fresh inputs, after a
    weight update (re-capture), and on the split-precision kernel."""
    b, h, w = shape
    net = pc.build_network(arch, DEV)
    net.enable_evaluation()
    xs = [torch.from_numpy(cases.image_batch(b, h, w, seed=s)).to(DEV) for s in (1, 2)]
    with torch.no_grad():
        eager = [net.inference(x) for x in xs]
        net.hip_graph = True
        for rep in range(2):
            for x, (m0, k0) in zip(xs, eager):
                m1, k1 = net.inference(x)
                assert torch.equal(m0, m1) and torch.equal(k0, k1)
        assert len(net._graphs) == 1
        first = next(iter(net.model.parameters()))
        first.mul_(1.5)                                      # bumps the parameter version: packed copies are stale
        m2, k2 = net.inference(xs[0])
        net.hip_graph = False
        m3, k3 = net.inference(xs[0])
        assert torch.equal(m2, m3) and torch.equal(k2, k3) and not torch.equal(m2, eager[0][0])
        net.hip_graph = True
        net.model.module.precision = "fp16x3"
        m4, k4 = net.inference(xs[1])
        net.hip_graph = False
        m5, k5 = net.inference(xs[1])
        assert torch.equal(m4, m5) and torch.equal(k4, k5)


def test_full_size_resnet_f_properties():
    """BASELINE.json configs[4] at one GPU's share: resnet_f, 17 keypoints, 32 frames of 400x400 -> 416x416 maps:
    batch-position independence, the CPU oracle on one frame, bit-exact peak stage."""
    net = pc.build_network("resnet_f", DEV)
    net.enable_evaluation()
    base = torch.from_numpy(cases.image_batch(2, 400, 400, seed=78))
    x = base.repeat(16, 1, 1, 1).to(DEV)
    with torch.no_grad():
        maps, kps = net.inference(x)
        net.model.module.precision = "fp16x3"
        maps16, kps16 = net.inference(x)
    maps, maps16 = maps.cpu(), maps16.cpu()
    assert maps.shape == (32, 17, 416, 416) and kps.shape == (32, 17, 2)
    for r in range(1, 16):
        assert torch.equal(maps[2 * r:2 * r + 2], maps[:2]) and torch.equal(kps[2 * r:2 * r + 2], kps[:2])
        assert torch.equal(maps16[2 * r:2 * r + 2], maps16[:2])
    ref = om.build_model("resnet_f", 17)
    ref.load_state_dict(om.recipe_weights(ref.state_dict()))
    ref.eval()
    with torch.no_grad():
        ref_maps = ref(base[:1])[0].numpy()
    assert np.abs(maps[:1].numpy() - ref_maps).max() <= pc.tol(ref_maps)
    assert np.abs(maps16[:1].numpy() - ref_maps).max() <= pc.tol(ref_maps)
    assert np.array_equal(kps[:1].numpy(), op.keypoints_from_belief_maps(maps[:1].numpy(), 0.0))


@pytest.mark.parametrize("arch,shape", [("vgg_q", (4, 200, 200)), ("resnet_h", (4, 128, 160)), ("vgg_f_ms2_skip", (2, 64, 96))])
def test_training_is_deterministic(arch, shape):
    """Two runs of the same three training steps from the same weights give bit-identical losses and parameters: split-K
    partials are reduced in a fixed order, BatchNorm statistics in fp64 with a fixed tree, and nothing uses fp32 atomics."""
    b, h, w = shape
    k = 7
    results = []
    for run in range(2):
        wts = om.recipe_weights(om.build_model(arch, k).state_dict(), cases.TRAIN_FINAL_KEYS, cases.TRAIN_FINAL_SCALE)
        net = pc.build_network(arch, DEV, weights=wts, optimizer="adam", lr=1e-5, in_res=(w, h))
        net.enable_training()
        ow, oh = net.trained_net_output_resolution()
        x = torch.from_numpy(cases.image_batch(b, h, w, seed=3)).to(DEV)
        t = torch.from_numpy(cases.target_batch(b, k, (ow, oh), in_wh=(w, h), seed=3)).to(DEV)
        losses = [net.train([x], t).item() for _ in range(3)]
        assert all(np.isfinite(losses))
        results.append((losses, [p.detach().clone() for p in net.model.parameters()]))
    assert all(torch.equal(a, b_) for a, b_ in zip(results[0][1], results[1][1]))
    assert results[0][0] == results[1][0]


@pytest.mark.parametrize("arch,shape", [("vgg_q", (1, 70, 93)), ("vgg_q", (2, 401, 399)), ("vgg_f", (1, 70, 93)),
                                        ("resnet_h", (1, 75, 101)), ("resnet_f", (2, 33, 47))])
def test_ragged_resolutions_match_oracle(arch, shape):
    """Resolutions the pools / strides do not divide (floor semantics everywhere, ragged last tiles in every kernel):
    HIP maps against the CPU oracle on the same weights, fp32 and split precision, and bit-exact peaks on the HIP maps."""
    b, h, w = shape
    k = cases.CNN_CASES[arch][0]
    net = pc.build_network(arch, DEV, in_res=(w, h))
    net.enable_evaluation()
    ref = om.build_model(arch, k)
    ref.load_state_dict(om.recipe_weights(ref.state_dict()))
    ref.eval()
    x = torch.from_numpy(cases.image_batch(b, h, w, seed=h))
    with torch.no_grad():
        want = ref(x)[0].numpy()
        maps, kps = net.inference(x.to(DEV))
        net.model.module.precision = "fp16x3"
        maps16, _ = net.inference(x.to(DEV))
    assert tuple(maps.shape) == want.shape == (b, k) + tuple(reversed(net.net_output_resolution_from_input_resolution((w, h))))
    assert np.abs(maps.cpu().numpy() - want).max() <= pc.tol(want)
    assert np.abs(maps16.cpu().numpy() - want).max() <= pc.tol(want)
    off = op.upsampling_offset(*net.trained_net_output_resolution())
    assert np.array_equal(kps.numpy(), op.keypoints_from_belief_maps(maps.cpu().numpy(), off))


def test_keypoint_frame_conversions():
    pc.check_keypoint_conversions(DEV)


def test_convT4x4_wgrad_winograd():
    """ConvTranspose2d(4,2,1) weight gradient on nine Winograd positions (round 6) against fp64 torch and the direct kernel: the
    decoder's layer shapes at small batches, odd extents, fewer tiles than a stage, several splits."""
    errs = [pc.check_convT4x4_wgrad_winograd(DEV, 2, 13, 13, 2048, 256),
            pc.check_convT4x4_wgrad_winograd(DEV, 2, 26, 26, 256, 256, seed=1),
            pc.check_convT4x4_wgrad_winograd(DEV, 1, 52, 52, 256, 256, seed=2),
            pc.check_convT4x4_wgrad_winograd(DEV, 3, 7, 5, 64, 128, seed=3),
            pc.check_convT4x4_wgrad_winograd(DEV, 1, 104, 104, 256, 256, seed=4)]
    print("convT4x4 wgrad (F(2x2,2x2), 9 positions) max err / sum|terms|", max(errs))


def test_conv_transpose3x3_subpixel():
    pc.check_conv_transpose3x3(DEV, 2, 25, 25, 512, 256)
    pc.check_conv_transpose3x3(DEV, 1, 50, 37, 256, 128, relu=False, seed=1)
    pc.check_conv_transpose3x3(DEV, 1, 200, 200, 64, 64, seed=2)


def test_upsample_conv_as_transposed_conv():
    pc.check_upsample_conv_as_convT(DEV, 2, 25, 25, 512, 256)
    pc.check_upsample_conv_as_convT(DEV, 1, 50, 37, 256, 128, relu=False, seed=1)


def test_randomised_conv_geometries():
    """The emulator suite's seeded sweep (ragged extents down to 1 pixel, odd channel counts, every fusion flag, both
    transposed-conv forms, weight gradients) on the device, with more cases."""
    rs = np.random.RandomState(2026)
    for case in range(40):
        b = int(rs.randint(1, 4))
        h, w = int(rs.randint(1, 40)), int(rs.randint(1, 45))
        cin = int(rs.choice([16, 32, 48, 80, 256]))
        cout = int(rs.choice([7, 16, 33, 64, 130, 256]))
        flags = int(rs.choice([0, ops.CONV_RELU, ops.CONV_OUT_NCHW, ops.CONV_RELU | ops.CONV_OUT_NCHW]))
        pc.check_conv(DEV, b, h, w, cin, cout, flags, seed=case)
        he, we = 2 * int(rs.randint(1, 16)), 2 * int(rs.randint(1, 18))
        pc.check_conv(DEV, b, he, we, cin, cout, ops.CONV_RELU | ops.CONV_POOL2, seed=case)
        pc.check_conv(DEV, b, he, we, cin, cout, ops.CONV_UPSAMPLE2X | (flags & ops.CONV_RELU), seed=case)
        pc.check_conv_transpose3x3(DEV, b, h, w, cin, cout, relu=bool(flags & ops.CONV_RELU), seed=case)
        pc.check_upsample_conv_as_convT(DEV, b, h, w, cin, cout, relu=bool(flags & ops.CONV_RELU), seed=case)
        co4 = int(rs.choice([8, 16, 64, 132, 256]))
        pc.check_wgrad(DEV, b, h, w, cin, co4, k=int(rs.choice([1, 3])), stride=int(rs.choice([1, 2])), seed=case)
        if cin % 32 == 0:
            pc.check_conv_f16x3(DEV, b, max(h, 2), max(w, 2), cin, cout, 3, flags & ops.CONV_RELU, seed=case)


# ---- north-star bounds on the structured (blob-like, magnitude-1) fixtures generated by the reference -------------------
@pytest.mark.parametrize("arch", sorted(cases.STRUCTURED_CASES))
def test_structured_fixture_absolute_tolerance(arch):
    err, perr = pc.check_structured(DEV, arch)
    print("structured %s fp32: max |map error| %.2e, max keypoint error %.2e px" % (arch, err, perr))


@pytest.mark.parametrize("case,repeat", [("vgg_q_400", 64), ("resnet_h", 8), ("resnet_f", 32)])
def test_structured_fixture_at_headline_batch(case, repeat):
    """The north-star bounds on the configurations bench.py times (dream/network.py:503-590): the reference's structured fixture tiled
    to the BASELINE batch -- vgg_q 128 x 400 x 400 (configs[1]), resnet_h 16 frames, resnet_f 32 frames (one GPU's share of configs[3] /
    [4]) -- with the DEFAULT algorithm selection (ops.winograd_tile by batch: F(4x4,3x3) on the XCD-pinned grids at 128 frames; the
    2-frame fixtures run F(2x2) unless forced).  Every copy: maps within an ABSOLUTE 1e-4 of the reference's golden maps, identical
    detection / rejection decisions, keypoints within 1e-3 px."""
    assert ops._WINOGRAD_TILE_FORCED == 0
    err, perr = pc.check_structured(DEV, case, repeat=repeat)
    print("structured %s x %d, default algorithms: max |map error| %.2e, max keypoint error %.2e px" % (case, repeat, err, perr))


@pytest.mark.parametrize("arch", ["vgg_q", "vgg_q_400", "vgg_f", "vgg_f_recipe", "resnet_h"])
def test_structured_fixture_absolute_tolerance_winograd4(arch):
    """The same north-star bounds with Winograd F(4x4,3x3) on every layer the kernel takes (at batch 128 the default; at the
    fixtures' 1-2 frames the layers would fall back to F(2x2,3x3) for lack of tiles)."""
    ops.set_winograd_tile(4)
    try:
        err, perr = pc.check_structured(DEV, arch)
    finally:
        ops.set_winograd_tile(0)
    print("structured %s fp32, F(4x4,3x3) forced: max |map error| %.2e, max keypoint error %.2e px" % (arch, err, perr))


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_train_steps_golden_winograd4(opt):
    ops.set_winograd_tile(4)
    try:
        res = pc.check_train_steps(DEV, opt, steps=3)
    finally:
        ops.set_winograd_tile(0)
    print("train golden %s, F(4x4,3x3) forced: fraction of tight parameter samples %.4f, worst %.2e" % ((opt,) + tuple(res)))


@pytest.mark.parametrize("arch", sorted(cases.STRUCTURED_CASES))
def test_structured_fixture_absolute_tolerance_split_precision(arch):
    err, perr = pc.check_structured(DEV, arch, precision="fp16x3")
    print("structured %s fp16x3: max |map error| %.2e, max keypoint error %.2e px" % (arch, err, perr))


# ---- full-size training (BASELINE configs[2] and one GPU's share of configs[3]) ------------------------------------------
def _grads_of(net, x, target):
    for p in net.model.parameters():
        p.grad = None
    loss = net.loss([x], target)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.item()), {k: p.grad.detach().clone() for k, p in net.model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("arch,batch", [("vgg_q", 128), ("resnet_h", 16)])
def test_full_size_training_batch_replication(arch, batch):
    """Replicating a 2-frame batch batch/2 times changes neither the mean loss nor any gradient (nor, for ResNet, the batch
    statistics): the full-size step (vgg_q: 128 x 400 x 400, split-K over 20.5 M positions) must reproduce the 2-frame step
    up to fp32 summation order.  The 2-frame step itself is pinned to the reference by the golden training tests.
    Bounds: the loss to 2e-6; every gradient's direction (cosine) and norm; the element-wise difference relative to the
    gradient norm for all layers but the first (whose 20 M-term, strongly cancelling sums are checked against fp64 in
    test_first_conv_wgrad_full_size_vs_fp64).  ResNet: train-mode BatchNorm through 100 layers amplifies the 1e-7 relative
    change of the re-summed batch statistics (tests/parity_checks.py::check_resnet_train_step), so only direction and norm
    are bounded there."""
    net = pc.build_network(arch, DEV, weights=om.recipe_weights(om.build_model(arch, 7).state_dict(), cases.TRAIN_FINAL_KEYS
                                                                   if arch == "vgg_q" else ("upsample.12.weight", "upsample.12.bias"),
                                                                   cases.TRAIN_FINAL_SCALE))
    net.enable_training()
    ow, oh = net.trained_net_output_resolution()
    x2 = torch.from_numpy(cases.image_batch(2, 400, 400, seed=17)).to(DEV)
    t2 = torch.from_numpy(cases.target_batch(2, 7, (ow, oh), seed=17)).to(DEV)
    loss2, g2 = _grads_of(net, x2, t2)
    rep = batch // 2
    lossn, gn = _grads_of(net, x2.repeat(rep, 1, 1, 1), t2.repeat(rep, 1, 1, 1))
    assert np.isfinite(loss2) and abs(lossn - loss2) <= 2e-6 * abs(loss2), (loss2, lossn)
    assert set(g2) == set(gn) and len(g2) == len(list(net.model.parameters()))
    gmax = max(float(v.double().norm()) for v in g2.values())
    rows = []
    for k in g2:
        a, b = g2[k].double().flatten(), gn[k].double().flatten()
        if float(a.norm()) < 1e-6 * gmax:                # conv biases in front of a BatchNorm: the true gradient is 0
            assert float(b.norm()) < 1e-4 * gmax, k
            continue
        rows.append((float((a - b).norm() / a.norm()), float((a * b).sum() / (a.norm() * b.norm())),
                     float(b.norm() / a.norm()), k))
    rows.sort(reverse=True)
    print("%s b=%d vs b=2: loss %.9g vs %.9g; relative gradient difference: worst %s, median %.2e" % (
        arch, batch, lossn, loss2, ", ".join("%s %.1e" % (k.replace("module.", ""), r) for r, _, _, k in rows[:4]),
        rows[len(rows) // 2][0]))
    first = {"vgg_q": "module.layer_0_1_down.0.", "resnet_h": "module.conv1."}[arch]
    for rel, cos, ratio, k in rows:
        if arch == "vgg_q":
            assert cos >= 1 - 1e-5 and abs(ratio - 1) <= 1e-3, (k, cos, ratio)
            # measured: first conv 1.6e-3, the 64-channel 400x400 layers 3-5e-4, median 1e-4 (the first-conv kernel itself
            # is exact to 5e-10 of sum|terms|: the differences are the upstream gradients' summation order, amplified by the
            # cancellation in sums over 20 M positions)
            assert rel <= (5e-3 if k.startswith(first) else 1.5e-3), (k, rel)
        else:
            assert cos >= 0.98 and abs(ratio - 1) <= 0.05, (k, cos, ratio)
    assert rows[len(rows) // 2][0] <= (3e-4 if arch == "vgg_q" else 1.5e-1)       # measured 9.6e-5 / 5.1e-2


def test_first_conv_wgrad_full_size_vs_fp64():
    """Weight / bias gradient of the first conv (3 -> 64 channels) at 128 x 400 x 400: sums of 20.5 M products.  Sampled
    entries against a float64 evaluation of the same sums on the device: error relative to sum |terms| at fp32 round-off
    level for a blocked summation (<= 2e-6), i.e. the kernel loses nothing beyond the order of summation."""
    g = torch.Generator(device="cpu").manual_seed(5)
    b, h, w = 128, 400, 400
    x = torch.from_numpy(cases.image_batch(2, h, w, seed=5)).to(DEV).repeat(b // 2, 1, 1, 1) \
        * torch.linspace(0.5, 1.5, b, device=DEV).view(b, 1, 1, 1)
    dy = torch.randn(b, h, w, 64, generator=g).to(DEV) * 1e-3
    dw, db = ops.conv3x3_first_wgrad(x.contiguous(), dy)
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1)).double()
    worst = 0.0
    for (o, c, ky, kx) in [(0, 0, 0, 0), (63, 2, 2, 2), (17, 1, 1, 1), (40, 0, 2, 1), (5, 2, 0, 2)]:
        terms = dy[..., o].double() * xp[:, c, ky:ky + h, kx:kx + w]
        ref, mag = float(terms.sum()), float(terms.abs().sum())
        worst = max(worst, abs(float(dw[o, c, ky, kx]) - ref) / mag)
    for o in (0, 31, 63):
        col = dy[..., o].double()
        worst = max(worst, abs(float(db[o]) - float(col.sum())) / float(col.abs().sum()))
    print("first-conv wgrad at b=128: worst |error| / sum|terms| = %.2e" % worst)
    assert worst <= 2e-6, worst


# ---- checkpoint I/O (dream/network.py:29-63,592-632) -----------------------------------------------
@pytest.mark.parametrize("arch", ["vgg_q", "resnet_h"])
def test_checkpoint_save_load_identical_inference(arch, tmp_path):
    """save_network -> create_network_from_config_file(yaml, pth) -> bit-identical belief maps and keypoints, and the
    verification tool accepts the pair (manifest, round trip, inference twice)."""
    import os
    import sys
    import dream_amd
    net = pc.build_network(arch, DEV)
    net.enable_evaluation()
    x = torch.from_numpy(cases.image_batch(2, 128, 160, seed=23)).to(DEV)
    with torch.no_grad():
        maps, kps = net.inference(x)
    net.save_network(str(tmp_path / "ckpt"), "net")
    yaml_path, pth_path = str(tmp_path / "ckpt" / "net.yaml"), str(tmp_path / "ckpt" / "net.pth")
    sd = torch.load(pth_path)
    assert all(k.startswith("module.") for k in sd) and all(v.device.type in ("cuda", "cpu") for v in sd.values())
    net2 = dream_amd.create_network_from_config_file(yaml_path, pth_path)
    net2.enable_evaluation()
    with torch.no_grad():
        maps2, kps2 = net2.inference(x)
    assert torch.equal(maps, maps2) and torch.equal(kps, kps2)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import verify_checkpoint as vc
    lines = []
    assert vc.verify(yaml_path, pth_path, out=lines.append) == 0, lines
    assert lines[-1] == "OK"


# ---- Winograd F(2x2,3x3) conv kernel ---------------------------------------------------------------------------------------
WINO_CASES = [
    (1, 8, 8, 32, 16, 0, {}), (2, 13, 25, 32, 64, 1, {}), (1, 25, 25, 48, 96, 1, {}), (3, 5, 3, 32, 7, 0, {}),
    (2, 12, 20, 32, 80, 1 | 16, {}), (2, 13, 9, 32, 64, 1 | 16, {}), (1, 399, 201, 64, 64, 1 | 16, {}), (1, 10, 14, 64, 32, 1, {"with_scale": True, "residual": "add"}),
    (1, 9, 11, 32, 48, 32, {"residual": "mask"}), (2, 7, 9, 32, 64, 0, {"mode": 1}),
    (2, 400, 400, 64, 64, 1 | 16, {}), (2, 200, 200, 128, 128, 1, {}), (4, 100, 100, 256, 256, 1, {}),
    (4, 50, 50, 512, 512, 1, {}), (8, 25, 25, 512, 512, 1, {}), (3, 13, 13, 512, 512, 1, {"with_scale": True}),
    (2, 133, 101, 64, 128, 1, {}), (2, 200, 200, 128, 128, 32, {"residual": "mask", "mode": 1}),
    (3, 100, 100, 256, 64, 1, {"with_scale": True, "residual": "add"}), (2, 101, 99, 48, 80, 1 | 16, {}),
]


@pytest.mark.parametrize("b,h,w,cin,cout,flags,kw", WINO_CASES)
def test_conv_winograd(b, h, w, cin, cout, flags, kw):
    err = pc.check_conv_winograd(DEV, b, h, w, cin, cout, flags, seed=h + cin, **kw)
    print("winograd %dx%dx%d %d->%d flags %d: rel err %.2e" % (b, h, w, cin, cout, flags, err))


@pytest.mark.parametrize("b,h,w,cin,cout", [(2, 13, 9, 16, 64), (2, 12, 20, 32, 144), (2, 13, 9, 32, 128), (2, 25, 25, 512, 512),
                                            (2, 400, 400, 64, 64), (2, 200, 200, 128, 128), (4, 100, 100, 256, 256), (4, 50, 50, 512, 512)])
def test_conv_winograd4_pool_both(b, h, w, cin, cout):
    """MODE 4 of the F(4x4) kernel (both workgroup shapes, odd extents, the four pooled vgg_q layers): un-pooled + pooled tensor from one
    launch, bit for bit the plain launch and a max-pool over it."""
    pc.check_conv_winograd4_pool_both(DEV, b, h, w, cin, cout, seed=b + h)


def test_hourglass_pool_in_the_training_conv_same_bits(monkeypatch):
    """DreamHourglass training forward with the pooled tensors stored by the convs' own launches (default) against the stand-alone
    max-pool passes (DREAM_POOL_IN_TRAINING_CONV=0): three Adam steps, losses and parameters bit for bit."""
    x = torch.from_numpy(cases.image_batch(8, 64, 96, seed=45)).to(DEV)

    def run(flag):
        monkeypatch.setenv("DREAM_POOL_IN_TRAINING_CONV", flag)
        net = _dp_network("vgg_q", [0], optimizer="adam", lr=1e-5, in_res=(96, 64))
        net.enable_training()
        ow, oh = net.trained_net_output_resolution()
        t = torch.from_numpy(cases.target_batch(8, 7, (ow, oh), in_wh=(96, 64), seed=45)).to(DEV)
        return net, [net.train([x], t).item() for _ in range(3)]

    a, la = run("1")
    b, lb = run("0")
    assert a.model.module.pool_in_training_conv and not b.model.module.pool_in_training_conv
    assert la == lb, (la, lb)
    for (k, pa), (_, pb) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(pa, pb), k


@pytest.mark.parametrize("b,h,w,cin,cout,flags,kw", [
    # narrow workgroup shape (up to 64 output channels)
    (1, 8, 8, 32, 16, 0, {}), (2, 13, 25, 32, 64, ops.CONV_RELU, {}), (3, 5, 3, 48, 7, 0, {}),
    (2, 13, 9, 16, 64, ops.CONV_RELU | ops.CONV_POOL2, {}),
    (1, 10, 14, 64, 32, ops.CONV_RELU, dict(with_scale=True, residual="add")), (1, 9, 11, 32, 48, ops.CONV_RELUMASK, dict(residual="mask")),
    (2, 7, 9, 32, 64, 0, dict(mode=1)),
    # wide shape
    (1, 8, 8, 32, 80, 0, {}), (2, 13, 25, 32, 128, ops.CONV_RELU, {}), (3, 5, 3, 64, 71, 0, {}),
    (2, 12, 20, 32, 144, ops.CONV_RELU | ops.CONV_POOL2, {}), (2, 13, 9, 32, 128, ops.CONV_RELU | ops.CONV_POOL2, {}),
    (1, 10, 14, 64, 96, ops.CONV_RELU, dict(with_scale=True, residual="add")), (1, 9, 11, 32, 112, ops.CONV_RELUMASK, dict(residual="mask")),
    (2, 7, 9, 32, 128, 0, dict(mode=1)),
    # the vgg_q layers F(4x4,3x3) serves (batch 2; the data gradients of the same layers through mode 1 / the mask)
    (2, 400, 400, 64, 64, ops.CONV_RELU | ops.CONV_POOL2, {}), (2, 400, 400, 64, 64, ops.CONV_RELUMASK, dict(mode=1, residual="mask")),
    (2, 200, 200, 128, 64, ops.CONV_RELUMASK, dict(mode=1, residual="mask")), (4, 100, 100, 64, 64, ops.CONV_RELU, {}),
    (2, 200, 200, 64, 128, ops.CONV_RELU, {}), (2, 200, 200, 128, 128, ops.CONV_RELU | ops.CONV_POOL2, {}),
    (2, 100, 100, 128, 256, ops.CONV_RELU, {}), (2, 100, 100, 256, 256, ops.CONV_RELU, {}), (4, 50, 50, 256, 512, ops.CONV_RELU, {}),
    (4, 50, 50, 512, 512, ops.CONV_RELU, {}), (8, 25, 25, 512, 512, ops.CONV_RELU, {}), (4, 50, 50, 256, 256, 0, {}),
    (2, 100, 100, 256, 128, ops.CONV_RELUMASK, dict(mode=1, residual="mask")), (16, 13, 13, 512, 512, 0, {})])
def test_conv_winograd4(b, h, w, cin, cout, flags, kw):
    err = pc.check_conv_winograd4(DEV, b, h, w, cin, cout, flags, seed=b + h, max_workgroups=(8, 24), **kw)
    print("winograd F(4x4) %dx%dx%d %d->%d flags %d: rel err %.2e" % (b, h, w, cin, cout, flags, err))


# ---- single-process data parallelism behind gpu_ids (dream_amd/data_parallel.py; reference network.py:244-256) ------------
@pytest.mark.parametrize("b,h,w,cin,cout", [(1, 6, 6, 128, 32), (2, 13, 9, 96, 48), (1, 20, 22, 256, 32), (4, 13, 13, 2048, 256),
                                            (4, 104, 104, 256, 256)])
def test_conv4x4s2_winograd(b, h, w, cin, cout):
    """Data gradient of the decoder's transposed convs on the Winograd kernel (four phase convs on stride-2 views, summed)."""
    err = pc.check_conv4x4s2_winograd(DEV, b, h, w, cin, cout, seed=h + cin)
    print("conv4x4s2 winograd %dx%dx%d %d<-%d: rel err %.2e" % (b, h, w, cin, cout, err))


@pytest.mark.parametrize("b,h,w,cin,cout", [(1, 8, 8, 128, 32), (2, 13, 9, 96, 64), (1, 20, 22, 256, 32), (4, 104, 104, 256, 256),
                                            (2, 100, 100, 256, 256)])
def test_conv4x4s2_winograd4(b, h, w, cin, cout):
    """The same data gradient on the F(4x4,3x3) kernel's 25-position phase patterns."""
    err = pc.check_conv4x4s2_winograd(DEV, b, h, w, cin, cout, seed=h + cin, tile=4)
    print("conv4x4s2 winograd F(4x4) %dx%dx%d %d<-%d: rel err %.2e" % (b, h, w, cin, cout, err))


@pytest.mark.parametrize("b,h,w,cin,cout,flags,kw", [
    (1, 6, 6, 32, 128, 0, {}), (2, 13, 9, 48, 96, 1, {"with_scale": True}), (1, 26, 26, 32, 256, 1, {}),
    (4, 13, 13, 2048, 256, 1, {"with_scale": True}), (4, 104, 104, 256, 256, 1, {"with_scale": True}), (2, 208, 208, 256, 256, 1, {})])
def test_conv_transpose4x4_winograd(b, h, w, cin, cout, flags, kw, monkeypatch):
    """The ResNet decoder's ConvTranspose2d(k4,s2,p1) (dream/models.py:37-136) by minimal filtering on the Winograd kernel; small grids
    on four-wavefront workgroups (round 5) and, forced, on eight-wavefront ones."""
    err = pc.check_convT4x4_winograd(DEV, b, h, w, cin, cout, flags, seed=h + cin, **kw)
    if b * ((h + 1) // 2) * ((w + 1) // 2) // 32 * ((cout + 127) // 128) < 72:
        monkeypatch.setenv("DREAM_WINO_SMALL_GRID", "0")
        err = max(err, pc.check_convT4x4_winograd(DEV, b, h, w, cin, cout, flags, seed=h + cin, **kw))
    print("convT4x4 winograd %dx%dx%d %d->%d flags %d: rel err %.2e" % (b, h, w, cin, cout, flags, err))


@pytest.mark.parametrize("b,h,w,cin,cout,flags,kw", [
    (1, 8, 8, 32, 128, 0, {}), (2, 13, 9, 64, 96, 1, {"with_scale": True}), (1, 26, 26, 32, 256, 1, {}),
    (4, 13, 13, 2048, 256, 1, {"with_scale": True}), (4, 104, 104, 256, 256, 1, {"with_scale": True}), (2, 208, 208, 256, 256, 1, {}),
    (2, 100, 100, 256, 256, 1, {})])
def test_conv_transpose4x4_winograd4(b, h, w, cin, cout, flags, kw):
    """The same transposed conv on the F(4x4,3x3) kernel with the 25-position phase patterns (F(4x4,2x2) minimal filtering)."""
    err = pc.check_convT4x4_winograd(DEV, b, h, w, cin, cout, flags, seed=h + cin, max_workgroups=(8, 24), tile=4, **kw)
    print("convT4x4 winograd F(4x4) %dx%dx%d %d->%d flags %d: rel err %.2e" % (b, h, w, cin, cout, flags, err))


@pytest.mark.parametrize("b,h,w,cin,cout,flags,kw", [
    (1, 8, 8, 64, 64, 0, {}), (2, 5, 7, 128, 36, 1, {"with_scale": True}), (1, 13, 13, 256, 192, 1, {"residual": True}),
    (3, 4, 3, 64, 128, 0, {"mode": 1, "residual": True}), (1, 9, 9, 160, 64, 1, {}),
    (16, 100, 100, 64, 256, 1, {"with_scale": True, "residual": True}), (16, 100, 100, 256, 64, 1, {"with_scale": True}),
    (16, 25, 25, 1024, 256, 0, {}), (16, 25, 25, 256, 1024, 0, {"mode": 1, "residual": True}), (16, 13, 13, 2048, 512, 1, {}),
    (128, 50, 50, 512, 128, 1, {"with_scale": True})])
def test_conv1x1_gemm(b, h, w, cin, cout, flags, kw):
    err = pc.check_conv1x1(DEV, b, h, w, cin, cout, flags, seed=h + cin, **kw)
    print("conv1x1 gemm %dx%dx%d %d->%d flags %d: rel err %.2e" % (b, h, w, cin, cout, flags, err))


@pytest.mark.parametrize("b,h,w,cin,cout,pad", [(1, 8, 8, 64, 64, 0), (2, 5, 7, 128, 36, 0), (1, 33, 31, 64, 128, 0), (3, 4, 3, 192, 64, 16),
                                                (16, 100, 100, 64, 256, 0), (16, 25, 25, 1024, 256, 0), (16, 13, 13, 512, 2048, 0),
                                                (128, 25, 25, 256, 1024, 0)])
def test_conv1x1_wgrad_gemm(b, h, w, cin, cout, pad):
    err = pc.check_conv1x1_wgrad(DEV, b, h, w, cin, cout, seed=h + cin, pad_dy=pad)
    print("conv1x1 wgrad %dx%dx%d %d->%d: err / sum|terms| %.2e" % (b, h, w, cin, cout, err))


def test_resnet_batchnorm_paths_agree_at_the_benchmark_shape(monkeypatch):
    """One GPU's share of configs[3] (resnet_h, 16 frames of 400x400): a training step with BatchNorm folded into its neighbours
    (round 4: statistics finished by the ticket tree inside 2 500-row launches, BN + ReLU in the 1x1 convs' loaders, reductions in the
    data-gradient epilogues) against the three-launch kernels of rounds 1-3 -- two correct fp32 evaluations of the same step: the
    loss agrees to 1e-5, the BatchNorm running statistics to 1e-5 of their scale, the gradient in direction (the 101 train-mode
    BatchNorms amplify summation-order differences; parity_checks.check_resnet_train_step holds each path against the fp64 oracle).
    The fused step repeated gives the same bits (the tree's fixed summation order)."""
    k = 7
    wts = om.recipe_weights(om.build_model("resnet_h", k).state_dict(), cases.TRAIN_FINAL_KEYS, cases.TRAIN_FINAL_SCALE)
    x = torch.from_numpy(cases.image_batch(16, 400, 400, seed=8)).to(DEV)
    runs = {}
    for tag, env in (("fused", "1"), ("fused_again", "1"), ("three_launch", "0")):
        monkeypatch.setenv("DREAM_BN_FUSION", env)
        net = pc.build_network("resnet_h", DEV, weights=wts, optimizer="sgd", lr=1e-5, in_res=(400, 400))
        assert net.model.module.bn_fusion == (env == "1")
        net.enable_training()
        ow, oh = net.trained_net_output_resolution()
        t = torch.from_numpy(cases.target_batch(16, k, (ow, oh), in_wh=(400, 400), seed=8)).to(DEV)
        net.optimizer.zero_grad()
        loss = net.loss([x], t)
        loss.backward()
        runs[tag] = (float(loss.detach()), {n: p.grad.detach().clone() for n, p in net.model.named_parameters()},
                     {n: b.detach().clone() for n, b in net.model.named_buffers() if n.endswith(("running_mean", "running_var"))})
        del net
    assert runs["fused"][0] == runs["fused_again"][0]
    assert all(torch.equal(runs["fused"][1][n], runs["fused_again"][1][n]) for n in runs["fused"][1])
    la, lb = runs["fused"][0], runs["three_launch"][0]
    assert abs(la - lb) <= 1e-5 * abs(lb), (la, lb)
    for n, b in runs["three_launch"][2].items():
        assert float((runs["fused"][2][n] - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max())), n
    ga, gb = runs["fused"][1], runs["three_launch"][1]
    names = [n for n in ga if not (n.startswith("module.upsample") and n.endswith(".bias") and n != "module.upsample.12.bias")]
    dot = sum(float((ga[n].double() * gb[n].double()).sum()) for n in names)
    na = sum(float(ga[n].double().pow(2).sum()) for n in names) ** 0.5
    nb = sum(float(gb[n].double().pow(2).sum()) for n in names) ** 0.5
    print("fused vs three-launch BatchNorm at 16x400x400: loss %.7f / %.7f, gradient cosine %.6f, norm ratio %.5f" % (la, lb, dot / (na * nb), na / nb))
    assert dot / (na * nb) >= 0.99 and abs(na / nb - 1.0) <= 0.02


def test_resnet_conv1x1_algorithms_agree():
    """ResnetSimple with the 1x1 convs on the GEMM kernel vs on the direct conv kernel: evaluation maps agree to fp32
    round-off; one training step's gradient agrees in direction (cosine >= 0.99) -- the two kernels sum in different orders;
    the gradients of the biases that feed a BatchNorm are pure round-off (exactly zero in exact arithmetic) and are excluded."""
    k = 7
    wts = om.recipe_weights(om.build_model("resnet_h", k).state_dict(), cases.TRAIN_FINAL_KEYS, cases.TRAIN_FINAL_SCALE)
    x = torch.from_numpy(cases.image_batch(4, 256, 320, seed=5)).to(DEV)
    outs, grads = [], []
    for alg in ("gemm", "direct"):
        net = pc.build_network("resnet_h", DEV, weights=wts, optimizer="sgd", lr=1e-5, in_res=(320, 256))
        net.model.module.conv1x1_algorithm = alg
        net.enable_evaluation()
        with torch.no_grad():
            outs.append(net.inference(x)[0].clone())
        net.enable_training()
        ow, oh = net.trained_net_output_resolution()
        t = torch.from_numpy(cases.target_batch(4, k, (ow, oh), in_wh=(320, 256), seed=5)).to(DEV)
        net.optimizer.zero_grad()
        net.loss([x], t).backward()
        grads.append({n: p.grad.detach().double().clone() for n, p in net.model.named_parameters()})
    scale = max(1.0, float(outs[1].abs().max()))
    map_err = float((outs[0] - outs[1]).abs().max()) / scale
    names = [n for n in grads[0] if not (n.startswith("module.upsample") and n.endswith(".bias") and grads[1][n].dim() == 1
                                         and n.split(".")[-2] in ("0", "3", "6", "9", "12") and n != "module.upsample.12.bias")]
    total = sum(float(grads[1][n].pow(2).sum()) for n in names) ** 0.5
    diff = sum(float((grads[0][n] - grads[1][n]).pow(2).sum()) for n in names) ** 0.5
    rel = {n: float((grads[0][n] - grads[1][n]).norm()) / max(float(grads[1][n].norm()), 1e-30) for n in names if n.endswith("weight")}
    worst = sorted(rel.items(), key=lambda kv: -kv[1])[:3]
    print("gemm vs direct 1x1 convs: maps differ by %.2e of the maximum; whole gradient by %.2e (relative L2); weight tensors: worst %s, "
          "median %.2e" % (map_err, diff / total, ", ".join("%s %.1e" % kv for kv in worst), float(np.median(list(rel.values())))))
    assert map_err <= 2e-5
    # train-mode BatchNorm of a randomly initialised 101-layer trunk is ill-conditioned: two correct fp32 implementations
    # differ by percents in every gradient tensor (parity_checks.check_resnet_train_step measures both kernels against the fp64
    # oracle); what a wiring error would break is the DIRECTION of the gradient
    dot = sum(float((grads[0][n] * grads[1][n]).sum()) for n in names)
    norm0 = sum(float(grads[0][n].pow(2).sum()) for n in names) ** 0.5
    assert dot / (norm0 * total) >= 0.99 and diff / total <= 0.15, (dot / (norm0 * total), diff / total)


def _dp_network(arch, gpu_ids, optimizer="adam", lr=1e-5, in_res=(96, 64), weights=None):
    import contextlib
    import io
    import dream_amd
    cfg = dream_amd.default_network_config(arch, "panda", optimizer=optimizer, learning_rate=lr)
    cfg["training"]["config"]["net_input_resolution"] = list(in_res)
    cfg["training"]["platform"]["gpu_ids"] = list(gpu_ids)
    with contextlib.redirect_stdout(io.StringIO()):
        net = dream_amd.create_network_from_config_data(cfg)
    if weights is None:
        weights = om.recipe_weights(om.build_model(arch, 7).state_dict(), cases.TRAIN_FINAL_KEYS, cases.TRAIN_FINAL_SCALE)
    net.model.load_state_dict({"module." + k: v for k, v in weights.items()})
    return net


def test_single_process_data_parallel_two_replicas_on_one_gpu():
    """gpu_ids = [0, 0]: two persistent replicas (threads, scatter, per-replica peak extraction, flat gradient reduce, flat
    parameter refresh) on the one GPU this box has.  Inference: bit-identical to the single-replica network, in order;
    training: two SGD steps equal the single-replica steps on the whole batch."""
    x = torch.from_numpy(cases.image_batch(5, 64, 96, seed=31)).to(DEV)
    t = torch.from_numpy(cases.target_batch(5, 7, (24, 16), in_wh=(96, 64), seed=31)).to(DEV)
    # SGD: parameter differences are lr x gradient differences (Adam's g / sqrt(v) turns a 1e-9 difference of a near-zero
    # gradient into a full lr-sized step; the single-launch Adam path is checked by the CPU suite)
    dp, one = _dp_network("vgg_q", [0, 0], "sgd", 1e-4), _dp_network("vgg_q", [0], "sgd", 1e-4)
    dp.enable_evaluation()
    one.enable_evaluation()
    with torch.no_grad():
        m2, k2 = dp.inference(x)
        m1, k1 = one.inference(x)
    assert len(dp.model.devices()) == 2 and len(dp.model._replicas) == 1 and len(one.model.devices()) == 1
    assert torch.equal(m2, m1) and torch.equal(k2, k1) and m2.device == x.device
    dp.enable_training()
    one.enable_training()
    l2 = [dp.train([x], t).item() for _ in range(2)]
    l1 = [one.train([x], t).item() for _ in range(2)]
    assert np.allclose(l2, l1, rtol=2e-6), (l2, l1)
    for (k, a), (_, b) in zip(dp.model.named_parameters(), one.model.named_parameters()):
        assert float((a - b).abs().max()) <= 1e-7 + 1e-5 * float(b.abs().max()), k
    grads = [p.grad for p in dp.model.parameters()]
    assert all(g.untyped_storage().data_ptr() == grads[0].untyped_storage().data_ptr() for g in grads)
    dp.model._sync_replicas(2)
    torch.cuda.synchronize()
    for a, b in zip(dp.model.module.parameters(), dp.model._replicas[0].parameters()):
        assert torch.equal(a, b)


def test_single_process_data_parallel_on_two_physical_gpus():
    """gpu_ids = [0, 1] on a node with more than one MI355X (skipped on the one-GPU test box, so that the first multi-GPU driver
    run is a TEST of the never-executed parts -- ncclCommInitAll over distinct devices, peer scatter / gather, one capture thread
    per device -- rather than a discovery): inference equals the one-GPU result bit for bit and in order, two SGD steps equal the
    one-GPU steps on the whole batch, the exchange is RCCL, the replicas stay identical without a parameter copy."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two physical GPUs")
    x = torch.from_numpy(cases.image_batch(6, 64, 96, seed=37)).to(DEV)
    t = torch.from_numpy(cases.target_batch(6, 7, (24, 16), in_wh=(96, 64), seed=37)).to(DEV)
    dev0 = torch.cuda.current_device()
    ids = [dev0, (dev0 + 1) % torch.cuda.device_count()]
    assert ops.allreduce_uses_rccl(ids)
    dp, one = _dp_network("vgg_q", ids, "sgd", 1e-4), _dp_network("vgg_q", [dev0], "sgd", 1e-4)
    dp.enable_evaluation()
    one.enable_evaluation()
    with torch.no_grad():
        m2, k2 = dp.inference(x)
        m1, k1 = one.inference(x)
    devs = dp.model.devices()
    assert [d.index for d in devs] == ids and len(dp.model._replicas) == 1 and len(one.model.devices()) == 1
    assert next(dp.model._replicas[0].parameters()).device == devs[1]
    assert torch.equal(m2, m1) and torch.equal(k2, k1) and m2.device == x.device
    dp.enable_training()
    one.enable_training()
    l2 = [dp.train([x], t).item() for _ in range(3)]          # eager, capture + replay, replay
    l1 = [one.train([x], t).item() for _ in range(3)]
    assert np.allclose(l2, l1, rtol=2e-6), (l2, l1)
    for (k, a), (_, b) in zip(dp.model.named_parameters(), one.model.named_parameters()):
        assert float((a - b).abs().max()) <= 1e-7 + 1e-5 * float(b.abs().max()), k
    assert dp.model.stats["replica_steps"] == 3 and dp.model.stats["param_copies"] == 1
    for d in devs:
        torch.cuda.synchronize(d)
    rep = dp.model._replicas[0]
    assert torch.equal(rep._dream_flat["params"].to(devs[0]), dp.model.module._dream_flat["params"])


def _bench_line(args, env=None, timeout=900):
    """Run bench.py (a subprocess, as the driver does) and return its JSON line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e.update(env or {})
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, cwd=root, env=e, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert lines, "bench.py printed no JSON line (rc %d)\n%s\n%s" % (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    return json.loads(lines[-1]), out.returncode


def test_bench_two_ranks_over_rccl_on_two_physical_gpus():
    """The torchrun twin of the test above (skipped on the one-GPU test box): `bench.py --gpus 2` launches its own two RCCL ranks, as
    the driver's SCALE run does.  After 3 Adam steps both ranks hold the same parameters, and the per-step loss averaged over the
    ranks equals the loss of ONE GPU on the concatenated batch within 1e-5 -- to tolerance, not bit for bit: the conv algorithm
    depends on the per-GPU batch (dream_amd/ops.py winograd_tile), see INTEGRATION.md."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two physical GPUs")
    common = ["--mode", "train", "--arch", "vgg_q", "--res", "128", "--steps", "3", "--warmup", "0", "--dp-check", "--no-secondary", "--no-cpu-baseline"]
    two, rc2 = _bench_line(["--gpus", "2", "--batch", "4"] + common)
    assert rc2 == 0 and "error" not in two, two
    one, rc1 = _bench_line(["--gpus", "1", "--batch", "4", "--concat-ranks", "2"] + common)
    assert rc1 == 0 and "error" not in one, one
    assert two["rccl_ranks"] == 2 and two["n_gpus"] == 2 and two["dp_check"]["ranks"] == 2
    assert two["dp_check"]["param_spread_between_ranks"] == 0.0, two["dp_check"]
    l2, l1 = np.array(two["dp_check"]["losses"]), np.array(one["dp_check"]["losses"])
    assert l2.shape == l1.shape == (3,) and np.allclose(l2, l1, rtol=1e-5, atol=1e-7), (l2, l1)
    assert abs(two["dp_check"]["param_l2"] - one["dp_check"]["param_l2"]) <= 1e-5 * one["dp_check"]["param_l2"]


def test_bench_dp_check_and_error_line_on_one_gpu():
    """What the twin above needs and a one-GPU box can exercise: --dp-check / --concat-ranks on one rank (losses recorded, zero spread),
    and the `error` field -- `--gpus 64` on this box must leave ONE diagnosable JSON line and a non-zero exit status, not a traceback."""
    common = ["--mode", "train", "--arch", "vgg_q", "--res", "64", "--steps", "2", "--warmup", "0", "--dp-check", "--no-secondary", "--no-cpu-baseline"]
    a, rc = _bench_line(["--gpus", "1", "--batch", "2", "--concat-ranks", "2"] + common)
    assert rc == 0 and a["dp_check"]["ranks"] == 1 and len(a["dp_check"]["losses"]) == 2 and a["dp_check"]["param_spread_between_ranks"] == 0.0
    assert a["dp_check"]["losses"][1] != a["dp_check"]["losses"][0]
    bad, rc = _bench_line(["--gpus", "64"] + common)
    assert rc != 0 and bad["value"] is None and "only" in bad["error"] and bad["n_gpus"] == 64, bad


def test_single_process_data_parallel_resnet_batchnorm_semantics():
    """ResNet under gpu_ids = [0, 0]: per-replica batch statistics (as nn.DataParallel), running statistics of replica 0 kept
    in the master module: one training step on 4 frames = the average of the gradients of two independent 2-frame steps."""
    wts = om.recipe_weights(om.build_model("resnet_h", 7).state_dict(), ("upsample.12.weight", "upsample.12.bias"), 0.1)
    x = torch.from_numpy(cases.image_batch(4, 64, 64, seed=33)).to(DEV)
    dp = _dp_network("resnet_h", [0, 0], optimizer="sgd", lr=0.0, in_res=(64, 64), weights=wts)
    dp.enable_training()
    ow, oh = dp.trained_net_output_resolution()
    t = torch.from_numpy(cases.target_batch(4, 7, (ow, oh), in_wh=(64, 64), seed=33)).to(DEV)
    loss = dp.train([x], t).item()
    halves = []
    for sl in (slice(0, 2), slice(2, 4)):
        one = _dp_network("resnet_h", [0], optimizer="sgd", lr=0.0, in_res=(64, 64), weights=wts)
        one.enable_training()
        halves.append((one.train([x[sl]], t[sl]).item(), [p.grad.clone() for p in one.model.parameters()], one))
    assert abs(loss - 0.5 * (halves[0][0] + halves[1][0])) <= 1e-6 * abs(loss)
    gmax = max(float(p.grad.norm()) for p in dp.model.parameters())
    for p, ga, gb in zip(dp.model.parameters(), halves[0][1], halves[1][1]):
        ref = 0.5 * (ga + gb)
        assert float((p.grad - ref).norm()) <= 1e-4 * max(float(ref.norm()), 1e-6 * gmax)
    # running statistics: replica 0's (the first chunk), as DataParallel keeps them
    assert torch.equal(dp.model.module.bn1.running_mean, halves[0][2].model.module.bn1.running_mean)


@pytest.mark.parametrize("split", ["", "0", "8"])
def test_single_process_data_parallel_graph_replay_equals_eager(monkeypatch, split):
    """gpu_ids = [0, 0, 0, 0]: from the second sighting of a shape every replica's forward and backward run as hipGraph
    replays (dream_amd/data_parallel.py).  Three ResNet training steps (eager, capture + replay, replay) must equal the same
    steps with DREAM_DP_GRAPHS=0 bit for bit -- same kernels, same order --, the replicas must stay identical to the master
    without a parameter copy, and a replayed step must hold the host (the GIL) for a fraction of an eager step's enqueue time.
    ``split`` = DREAM_TRAIN_GRAPH_SPLIT: "" = the default (round 6: also for multi-device steps every replica's backward is a sequence of
    graphs, 12 leaves per segment, its leaf segments on the device's second stream -- data_parallel._SplitCapture, captured from four threads), "8" = eight leaves per segment, "0" = one backward graph per replica."""
    import time
    monkeypatch.setenv("DREAM_TRAIN_GRAPH_SPLIT", split)
    wts = om.recipe_weights(om.build_model("resnet_h", 7).state_dict(), ("upsample.12.weight", "upsample.12.bias"), 0.1)
    x = torch.from_numpy(cases.image_batch(8, 64, 64, seed=41)).to(DEV)

    def run(graphs):
        monkeypatch.setenv("DREAM_DP_GRAPHS", "1" if graphs else "0")
        net = _dp_network("resnet_h", [0, 0, 0, 0], optimizer="adam", lr=1e-5, in_res=(64, 64), weights=wts)
        net.enable_training()
        ow, oh = net.trained_net_output_resolution()
        t = torch.from_numpy(cases.target_batch(8, 7, (ow, oh), in_wh=(64, 64), seed=41)).to(DEV)
        losses, host = [], []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = net.train([x], t)
            host.append(time.perf_counter() - t0)          # enqueue time: nothing waits for the GPU inside train()
            losses.append(loss.item())
        torch.cuda.synchronize()
        return net, losses, host

    g, lg, hg = run(True)
    e, le, he = run(False)
    dp = g.model
    assert len(dp._replicas) == 3 and dp.stats["captures"] == 8, dp.stats           # 4 replicas x (forward + backward)
    assert dp.stats["replays"] == 4 * 2 * 3 and dp.stats["param_copies"] == 3 and dp.stats["replica_steps"] == 3 * 4
    assert e.model.stats["replays"] == 0
    plans = [getattr(v["bwd"], "plan", None) for v in dp._graphs.values() if v["bwd"] is not None]
    assert len(plans) == 4 and all((p is not None and sum(op[0] == "side" for op in p) >= 3) if split != "0" else p is None for p in plans)
    if split != "0":
        # every replica replays its leaf segments to the device's one live second stream (more busy streams than hardware queues lose
        # the order between replayed segments on this runtime: tools/dp_exchange_probe.py) and none of them CAPTURES on it (another
        # replica's thread may be replaying to it at that moment)
        sides = [v["bwd"].side for v in dp._graphs.values() if v["bwd"] is not None]
        assert len({s.cuda_stream for s in sides}) == 1
        assert all(v["bwd"].capture_side.cuda_stream != sides[0].cuda_stream for v in dp._graphs.values() if v["bwd"] is not None)
    # the exchange (round 6): two pieces per step -- the early bucket (layer3 and up) behind each replica's event, then the rest -- wherever
    # the backward is a sequence of graphs or eager; ONE piece per step behind a single backward graph
    assert dp.stats.get("exchanges") == (8 if split != "0" else 2 + 3), dp.stats
    assert e.model.stats.get("exchanges") == 8, e.model.stats
    assert lg == le, (lg, le)
    for (k, a), (_, b) in zip(g.model.named_parameters(), e.model.named_parameters()):
        assert torch.equal(a, b), k
    for rep in dp._replicas:
        assert torch.equal(rep._dream_flat["params"], dp.module._dream_flat["params"])
    assert torch.equal(g.model.module.bn1.running_mean, e.model.module.bn1.running_mean)
    print("host seconds per step: graphs %s, eager %s" % (["%.4f" % v for v in hg], ["%.4f" % v for v in he]))
    assert hg[3] < 0.5 * he[3], (hg, he)
    # evaluation after training: graphs are keyed on the parameter versions, results equal the eager path
    g.enable_evaluation()
    e.enable_evaluation()
    with torch.no_grad():
        outs = [g.inference(x) for _ in range(3)]
        ref = e.inference(x)
    for m, k in outs:
        assert torch.equal(m, ref[0]) and torch.equal(k, ref[1])


@pytest.mark.parametrize("where", ["backward_end", "exchange_begin"])
def test_replayed_steps_do_not_depend_on_a_device_synchronisation(monkeypatch, where):
    """tools/dp_exchange_probe.py as a test: a device-wide synchronisation inside the replayed steps (DREAM_DP_PROBE_SYNC) changes the
    timing and nothing else -- five ResNet training steps with gpu_ids=[0, 0, 0, 0] must reproduce the eager steps' losses bit for bit.
    Until round 6 they did not: the memset NODES that hipMemsetAsync left in the captured graphs were not reliably ordered with the
    kernel nodes around them on this runtime (the stride-2 1x1 data gradient then read uninitialised memory: gradients of 1e20 from
    layer4.0 down); the library zeroes with kernels now (csrc/common.h)."""
    wts = om.recipe_weights(om.build_model("resnet_h", 7).state_dict(), ("upsample.12.weight", "upsample.12.bias"), 0.1)
    x = torch.from_numpy(cases.image_batch(8, 64, 64, seed=41)).to(DEV)

    def run(graphs, sync):
        monkeypatch.setenv("DREAM_DP_GRAPHS", "1" if graphs else "0")
        monkeypatch.setenv("DREAM_DP_PROBE_SYNC", sync)
        net = _dp_network("resnet_h", [0, 0, 0, 0], optimizer="adam", lr=1e-5, in_res=(64, 64), weights=wts)
        net.enable_training()
        ow, oh = net.trained_net_output_resolution()
        t = torch.from_numpy(cases.target_batch(8, 7, (ow, oh), in_wh=(64, 64), seed=41)).to(DEV)
        losses = [net.train([x], t).item() for _ in range(5)]
        torch.cuda.synchronize()
        return losses, net

    ref, _ = run(False, "")
    got, net = run(True, where)
    assert net.model.stats["replays"] == 4 * 2 * 4, net.model.stats
    assert got == ref, (got, ref)


def test_strided_data_gradient_zeroes_its_output_inside_a_graph():
    """The stride-2 1x1 data gradient (the downsample convs of ResNet-101) writes the even positions of dx and zeroes the rest -- with a
    KERNEL (round 6: a hipGraph memset node was not reliably ordered on this runtime).  Captured, then replayed over poisoned memory
    with a device synchronisation in between: the odd positions are zero every time."""
    torch.manual_seed(5)
    cin, cout = 64, 128
    w = torch.randn(cout, cin, 1, 1, device=DEV)
    dy = torch.randn(2, 3, 3, cout, device=DEV)
    packed_t, rows, _ = ops.pack_conv_weight(w, 1)
    ref = ops.conv2d_bwd_data(dy, packed_t, cin, 1, 2, (6, 6)).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        dx = ops.conv2d_bwd_data(dy, packed_t, cin, 1, 2, (6, 6))
        graph.capture_end()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(4):
        dx.fill_(1e20)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dx, ref)
    assert float(ref[:, 1::2].abs().max()) == 0.0 and float(ref[:, :, 1::2].abs().max()) == 0.0 and float(ref.abs().max()) > 0.0


def test_peaks_fused_row_pass_and_scan_same_bits():
    """csrc/peaks.hip, round 6: the second Gaussian pass fused with the peak scan against the three-kernel form -- keypoints and counts bit
    for bit, up to the 416 x 416 maps of DREAM-resnet-F."""
    pc.check_peaks_fused_equals_three_kernels(DEV, sizes=((1, 7, 5, 9), (2, 3, 37, 45), (1, 2, 64, 64), (2, 7, 100, 100), (1, 2, 130, 71), (2, 17, 416, 416)))


def test_clone_by_kernel_any_length_and_alignment():
    """ops.clone (dream_copy_f32: the kernel that stands where ATen would leave a memcpy node in a captured graph): every length, and
    sources / destinations that are not 16-byte aligned (views that start one element into their storage)."""
    torch.manual_seed(9)
    for n in (1, 3, 4, 5, 255, 1024, 4097, (1 << 20) + 3):
        base = torch.randn(n + 1, device=DEV)
        for src in (base[:n], base[1:]):
            out = ops.clone(src)
            assert out.data_ptr() != src.data_ptr() and torch.equal(out, src)
    graph = torch.cuda.CUDAGraph()
    src = torch.randn(3, 5, 7, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph.capture_begin()
        out = ops.clone(src)
        graph.capture_end()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        src.normal_()
        out.fill_(7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, src)


def test_bucketed_exchange_through_rccl_on_one_device(monkeypatch):
    """DREAM_FORCE_RCCL=1 (round 6): a one-device step runs the gradient exchange of the single-process multi-GPU path THROUGH RCCL (a
    one-rank communicator: dlopen, ncclCommInitAll, group calls) -- in two pieces per step: the early bucket on the exchange stream behind
    the replica's event, the rest behind the backward pass (dream/network.py:244-256,335).  At least two RCCL calls per step, the early
    one over everything from layer3 up; the training run equals the one without the forced exchange bit for bit (a sum over one rank)."""
    wts = om.recipe_weights(om.build_model("resnet_h", 7).state_dict(), ("upsample.12.weight", "upsample.12.bias"), 0.1)
    x = torch.from_numpy(cases.image_batch(4, 64, 64, seed=43)).to(DEV)

    def run(force):
        monkeypatch.setenv("DREAM_FORCE_RCCL", "1" if force else "0")
        net = _dp_network("resnet_h", [0], optimizer="adam", lr=1e-5, in_res=(64, 64), weights=wts)
        net.hip_graph_train = True
        net.enable_training()
        ow, oh = net.trained_net_output_resolution()
        t = torch.from_numpy(cases.target_batch(4, 7, (ow, oh), in_wh=(64, 64), seed=43)).to(DEV)
        calls = []
        orig = ops.allreduce_sum_
        monkeypatch.setattr(ops, "allreduce_sum_", lambda flats, streams=None: calls.append((int(flats[0].numel()), streams is not None,
                                                                                              ops.allreduce_uses_rccl([0]))) or orig(flats, streams))
        losses = [net.train([x], t).item() for _ in range(4)]
        torch.cuda.synchronize()
        monkeypatch.setattr(ops, "allreduce_sum_", orig)
        return net, losses, calls

    f, lf, cf = run(True)
    p, lp, cp = run(False)
    assert cp == [] and len(cf) == 8, (len(cp), cf)                       # two pieces per step, none without the switch
    total = int(f.model.module._dream_flat["params"].numel())
    for early, late in zip(cf[0::2], cf[1::2]):
        assert early[1] and late[1] and early[2] and late[2]              # on the exchange stream, through RCCL
        assert early[0] + late[0] == total and early[0] > 0.9 * total     # layer3 and up: 97 % of ResNet-101's parameters
    assert lf == lp, (lf, lp)
    for (k, a), (_, b) in zip(f.model.named_parameters(), p.model.named_parameters()):
        assert torch.equal(a, b), k


def test_conv3x3_bn_fused_ops():
    """The 3x3 convs' train-mode BatchNorm inside the Winograd F(2x2) kernel's launches (csrc/conv_wino.hip WINO_STAT), small shapes
    and the two benchmark shapes of ResNet-101 at 16 frames (256 producer rows: both levels of the ticket tree; 64 channels: the
    4-wave kernel), against the unfused launches bit for bit where the arithmetic is the same and against torch on CPU."""
    pc.check_conv3x3_bn_fused(DEV)
    pc.check_conv3x3_bn_fused(DEV, cases=[(16, 25, 25, 256, 256), (8, 100, 100, 64, 64)])


def test_resnet_training_with_batchnorm_in_the_3x3_kernels(monkeypatch):
    """DREAM_BN_FUSION_3X3=1 (opt-in): the reference goldens hold, and two runs give the same bits (fixed summation order)."""
    monkeypatch.setenv("DREAM_BN_FUSION_3X3", "1")
    pc.check_resnet_train_step(DEV, "resnet_h", (2, 64, 64))
    wts = om.recipe_weights(om.build_model("resnet_h", 7).state_dict(), ("upsample.12.weight", "upsample.12.bias"), 0.1)
    x = torch.from_numpy(cases.image_batch(4, 64, 96, seed=51)).to(DEV)
    runs = []
    for _ in range(2):
        net = _dp_network("resnet_h", [0], optimizer="sgd", lr=0.0, in_res=(96, 64), weights=wts)
        net.enable_training()
        assert net.model.module.bn_fusion_3x3
        ow, oh = net.trained_net_output_resolution()
        t = torch.from_numpy(cases.target_batch(4, 7, (ow, oh), in_wh=(96, 64), seed=51)).to(DEV)
        loss = net.train([x], t).item()
        runs.append((loss, [p.grad.clone() for p in net.model.parameters()]))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("arch,res,split", [("resnet_h", (64, 64), 0), ("vgg_q", (64, 48), 0),
                                            ("resnet_h", (64, 64), 7), ("resnet_h", (64, 64), 1000), ("vgg_q", (64, 48), 3)])
def test_one_device_training_step_as_graph_replay_equals_eager(arch, res, split):
    """DreamNetwork.hip_graph_train on a training network with ONE device: from the second step of a batch shape train() is two
    hipGraph replays (forward, backward) + the loss and the optimizer launch.  Four Adam steps must equal the eager steps bit for
    bit (losses, parameters, BatchNorm running statistics), the host must spend clearly less than the eager enqueue time on a replayed
    step, and switching the flag off again returns to the eager path on the same parameters.  ``split`` > 0: the backward as a
    SEQUENCE of graphs (data_parallel._SplitCapture), the weight-gradient leaves in segments of their own on a live second stream."""
    import time
    wts = om.recipe_weights(om.build_model(arch, 7).state_dict(), ("upsample.12.weight", "upsample.12.bias"), 0.1) if arch == "resnet_h" \
        else None                                          # _dp_network's default recipe
    x = torch.from_numpy(cases.image_batch(4, res[1], res[0], seed=47)).to(DEV)        # res = (width, height)

    def run(graph):
        net = _dp_network(arch, [0], optimizer="adam", lr=1e-5, in_res=res, weights=wts)
        net.enable_training()
        net.hip_graph_train = graph
        net.model.graph_split_leaves = split               # > 0: the backward as a sequence of graphs, `split` leaves per segment
        ow, oh = net.trained_net_output_resolution()
        t = torch.from_numpy(cases.target_batch(4, 7, (ow, oh), in_wh=res, seed=47)).to(DEV)
        losses, host = [], []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = net.train([x], t)
            host.append(time.perf_counter() - t0)
            losses.append(loss.item())
        torch.cuda.synchronize()
        return net, losses, host, t

    g, lg, hg, t = run(True)
    e, le, he, _ = run(False)
    st = g.model.stats
    assert st["captures"] == 2 and st["replays"] == 2 * 3 and e.model.stats["replays"] == 0, st
    if split:
        plans = [v["bwd"].plan for v in g.model._graphs.values() if v["bwd"] is not None]
        kinds = [op[0] for op in plans[0]]
        assert len(plans) == 1 and kinds[0] == "main" and kinds[-2:] == ["join", "main"], kinds
        assert kinds.count("join") == 1 and kinds.count("side") >= (1 if split == 1000 else 3), kinds     # 1000: only the tapered tail
        print(arch, "split", split, "->", kinds.count("main"), "main and", kinds.count("side"), "leaf segments")
    assert lg == le, (lg, le)
    for (k, a), (_, b) in zip(g.model.state_dict().items(), e.model.state_dict().items()):
        assert torch.equal(a, b), k
    print("%s host seconds per step: graph %s, eager %s" % (arch, ["%.4f" % v for v in hg], ["%.4f" % v for v in he]))
    assert hg[3] < (0.7 if not split else 0.9) * he[3], (hg, he)     # measured: resnet_h 8 ms against 25, vgg_q 1.6 against 3.9
    g.hip_graph_train = False                              # back to the eager path, same parameters, same optimizer state
    assert g.train([x], t).item() == e.train([x], t).item()
    assert st["replays"] == 2 * 3


def test_resnet_batched_packing_equals_lazy_packing(monkeypatch):
    """ResnetSimple._repack_weights: from the second training step on the packed weight copies are refreshed by ONE launch
    (dream_pack_weights_batched).  Four Adam steps and an evaluation in between must equal the same with DREAM_PACK_BATCHED=0
    (one launch per tensor, on demand), bit for bit."""
    wts = om.recipe_weights(om.build_model("resnet_h", 7).state_dict(), ("upsample.12.weight", "upsample.12.bias"), 0.1)
    x = torch.from_numpy(cases.image_batch(4, 64, 96, seed=43)).to(DEV)

    def run(flag):
        monkeypatch.setenv("DREAM_PACK_BATCHED", flag)
        monkeypatch.setenv("DREAM_PACK_SPLIT", "1")          # the opt-in two-launch form (late copies on the second stream) is the one under test
        net = _dp_network("resnet_h", [0], optimizer="adam", lr=1e-5, in_res=(96, 64), weights=wts)
        net.enable_training()
        ow, oh = net.trained_net_output_resolution()
        t = torch.from_numpy(cases.target_batch(4, 7, (ow, oh), in_wh=(96, 64), seed=43)).to(DEV)
        losses = [net.train([x], t).item() for _ in range(3)]
        net.enable_evaluation()
        with torch.no_grad():
            maps = net.inference(x)[0].clone()             # evaluation re-packs (folded BatchNorm) outside the graph ...
        net.enable_training()
        losses.append(net.train([x], t).item())            # ... and the next training step must not use those copies
        return net, losses, maps

    a, la, ma = run("1")
    b, lb, mb = run("0")
    st = a.model.module._packs.view()
    assert st.table_built and st.jobs >= 190 and b.model.module._packs.view().idle, st.jobs
    # round 6 (opt-in): the re-pack as two launches -- the copies layer3 and everything behind it read are rewritten on the second stream
    assert st.split is not None and 0 < st.split[0] < st.split[1] and not st.pending
    assert la == lb and torch.equal(ma, mb), (la, lb)
    for (k, pa), (_, pb) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(pa, pb), k


def test_allreduce_entry_point(monkeypatch):
    """dream_allreduce_sum_f32: buffers that share the one GPU of this box are summed locally; with DREAM_FORCE_RCCL=1 a
    one-device list goes through RCCL itself (dlopen, ncclCommInitAll, group call) -- the sequence an 8-GPU node runs."""
    a = torch.arange(1000, dtype=torch.float32, device=DEV)
    bufs = [a.clone(), 2 * a, 3 * a + 1]
    assert not ops.allreduce_uses_rccl([0, 0, 0]) and ops.allreduce_uses_rccl([0, 1, 2])
    ops.allreduce_sum_(bufs)
    torch.cuda.synchronize()
    for b in bufs:
        assert torch.equal(b, 6 * a + 1)
    monkeypatch.setenv("DREAM_FORCE_RCCL", "1")
    assert ops.allreduce_uses_rccl([0])
    one = [a.clone()]
    ops.allreduce_sum_(one)
    torch.cuda.synchronize()
    assert torch.equal(one[0], a)


# ---- Winograd-domain weight gradient -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,h,w,cin,cout,pad", [(1, 8, 8, 64, 16, 0), (2, 13, 9, 64, 32, 0), (3, 6, 10, 128, 48, 0), (2, 5, 3, 64, 16, 16),
                                                 (4, 400, 400, 64, 64, 0), (4, 100, 100, 256, 256, 0), (8, 25, 25, 512, 512, 0),
                                                 (2, 133, 101, 128, 64, 0), (16, 13, 13, 512, 512, 0)])
def test_wgrad_winograd(b, h, w, cin, cout, pad):
    err = pc.check_wgrad_winograd(DEV, b, h, w, cin, cout, seed=h + cin, pad_dy=pad)
    print("winograd wgrad %dx%dx%d %d->%d: err / sum|terms| %.2e" % (b, h, w, cin, cout, err))


@pytest.mark.parametrize("b,h,w,cin,cout", [(2, 12, 10, 64, 64), (1, 26, 26, 128, 64), (8, 100, 100, 256, 128), (16, 50, 50, 512, 256)])
def test_wgrad_winograd_fused_upsample(b, h, w, cin, cout):
    """The decoder convs that follow nn.Upsample(2) (dream/models.py:691-710): x at half resolution, upsample fused into the loads."""
    err = pc.check_wgrad_winograd(DEV, b, h, w, cin, cout, seed=h + cin, ups=True)
    print("winograd wgrad after upsample %dx%dx%d %d->%d: err / sum|terms| %.2e" % (b, h, w, cin, cout, err))


@pytest.mark.parametrize("algorithm", ["winograd", "direct"])
def test_skip_connections_fold_into_the_producing_conv(monkeypatch, algorithm):
    """K13 (dream/models.py:774-799): in inference the skip-connection sums x + x_0_k_d are made by the producing conv's epilogue
    (DREAM_CONV_RES_AFTER_RELU) -- no stand-alone add launch -- and the reference's golden maps still hold; training keeps the add."""
    monkeypatch.setenv("DREAM_CONV_ALGORITHM", algorithm)
    adds = []
    real = ops.add
    monkeypatch.setattr(ops, "add", lambda *a, **k: (adds.append(1), real(*a, **k))[1])
    for name in ("vgg_q_skip", "vgg_f_skip"):
        pc.check_variant(DEV, name, train=False)
    assert not adds
