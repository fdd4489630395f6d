"""Whole training steps at resolutions that no pool and no stride divides, shared by the emulator suite
(test_ragged_training_emulated.py) and the GPU suite (test_gpu_ragged_training.py).

Every kernel has odd-extent parity cases of its own (check_backward_ops, check_resnet_training_ops, check_pool_and_layouts); what those
cannot see is an extent that models.py hands over wrongly -- a swapped (h, w), a floor where the reference takes the ceiling, an ``in_hw``
of the wrong level -- because such an extent may well stay inside the allocation.  At an even shape every such mistake is invisible
(floor == ceiling, and most test shapes are square or nearly so); here every level of every network has an odd side.

The yardsticks are the project's own, unchanged: parity_checks.check_vgg_train_grads (loss 1e-5 relative, per-tensor cosine >= 0.9999,
worst element 2 % of the tensor's maximum, against torch autograd on the CPU oracle) and parity_checks.check_resnet_train_step (as close
to the fp64 oracle as torch's own fp32 path, factor 3 + a floor); for the fp16 training modes the 3 E_p of their modules, E_p measured on
a CPU reference that rounds where the device rounds.  Each fp32 case also asserts which entry points were launched, so that a case
cannot silently run the default plan.

Shapes (B, H, W) -- the smallest that put an odd extent on every level:

* HOURGLASS_SHAPES[0] = (2, 37, 50): the four 2x2 pools see H 37 -> 18 -> 9 -> 4 -> 2 and W 50 -> 25 -> 12 -> 6 -> 3: a leftover row at
  pools 1 and 3, a leftover column at pool 2;
* HOURGLASS_SHAPES[1] = (1, 35, 45): H 35 -> 17 -> 8 -> 4 -> 2, W 45 -> 22 -> 11 -> 5 -> 2: the complementary pattern (rows at pools 1
  and 2, columns at pools 1, 3 and 4), and a one-frame backward;
* RESNET_H_SHAPE = (2, 75, 101): stem (7x7 s2 p3) 38 x 51, max-pool (3x3 s2 p1) 19 x 26, layer2..4 (3x3 s2 p1) 10 x 13, 5 x 7, 3 x 4:
  an odd side into the max-pool and into each of the three stride-2 blocks (ceiling semantics: 19 -> 10, 13 -> 7, 5 -> 3, 7 -> 4);
* RESNET_F_SHAPE = (2, 33, 47): 17 x 24, 9 x 12, 5 x 6, 3 x 3, 2 x 2.

What cannot run at these shapes: a multi-stage hourglass concatenates the image with the (x4 upsampled) maps of the previous stage, and
a deconv decoder with skip connections adds 2 * floor(n / 2) rows to n rows, so vgg_ms2 and vgg_f_ms2_skip take inputs whose sides are
multiples of 16 only -- the reference raises at (2, 37, 50) (torch.cat / the skip sum), and so must this project, before any launch that
would read past a tensor: check_variant_refused."""
import collections
import contextlib
import os

import torch

import cases
import parity_checks as pc
from dream_amd import ops
from oracle import models as om

HOURGLASS_SHAPES = ((2, 37, 50), (1, 35, 45))
RESNET_H_SHAPE = (2, 75, 101)
RESNET_F_SHAPE = (2, 33, 47)

W2, W4 = "dream_conv3x3_winograd_nhwc_f32", "dream_conv3x3_winograd4_nhwc_f32"
DS_GEMM_FORMS = ("dream_subsample2_nhwc_f32", "dream_scatter2_nhwc_f32", "dream_im2col3s2_nhwc_f32", "dream_col2im3s2_nhwc_f32")

# name -> (check, arch, shape, environment, forced Winograd tile, entry points that must have been launched, name parts that must not)
FP32_CASES = {
    "vgg_q-2x37x50": ("vgg", "vgg_q", HOURGLASS_SHAPES[0], {}, 0, (W2, "dream_maxpool2_relu_bwd_nhwc_f32", "dream_conv4x4s2_winograd_nhwc_f32"), ()),
    "vgg_q-1x35x45": ("vgg", "vgg_q", HOURGLASS_SHAPES[1], {}, 0, (W2, "dream_maxpool2_relu_bwd_nhwc_f32", "dream_conv4x4s2_winograd_nhwc_f32"), ()),
    "vgg_f-2x37x50": ("vgg", "vgg_f", HOURGLASS_SHAPES[0], {}, 0, (W2, "dream_maxpool2_relu_bwd_nhwc_f32", "dream_conv_transpose3x3s2_nhwc_f32"), ()),
    "vgg_f-1x35x45": ("vgg", "vgg_f", HOURGLASS_SHAPES[1], {}, 0, (W2, "dream_maxpool2_relu_bwd_nhwc_f32", "dream_conv_transpose3x3s2_nhwc_f32"), ()),
    # F(4x4) wherever it applies: with it the pool fused into the training conv (CONV_POOL2 floors, both tensors written by one launch)
    "vgg_f-2x37x50-tile4": ("vgg", "vgg_f", HOURGLASS_SHAPES[0], {}, 4, (W4, "dream_conv3x3_winograd4_pool_both_nhwc_f32"), ()),
    "vgg_f-2x37x50-direct": ("vgg", "vgg_f", HOURGLASS_SHAPES[0], {"DREAM_CONV_ALGORITHM": "direct"}, 0, ("dream_conv3x3_nhwc_f32", "dream_maxpool2_nhwc_f32"), ("winograd",)),
    "vgg_q_skip-2x37x50": ("vgg", "vgg_q_skip", HOURGLASS_SHAPES[0], {}, 0, (W2, "dream_add_f32"), ()),
    "resnet_h-2x75x101": ("resnet", "resnet_h", RESNET_H_SHAPE, {}, 0,
                          DS_GEMM_FORMS + ("dream_maxpool3s2_idx_bwd_nhwc_f32", "dream_conv1x1_bnstats_nhwc_f32", "dream_col2im4s2_nhwc_f32"), ()),
    "resnet_f-2x33x47": ("resnet", "resnet_f", RESNET_F_SHAPE, {}, 0, DS_GEMM_FORMS + ("dream_maxpool3s2_idx_bwd_nhwc_f32",), ()),
    # direct strided convs, their strided data gradients (in_hw) and the Winograd transposed convs of the decoder
    "resnet_h-2x75x101-ds_gemm0": ("resnet", "resnet_h", RESNET_H_SHAPE, {"DREAM_DS_GEMM": "0"}, 0,
                                   ("dream_conv2d_s2_bwd_data_nhwc_f32", "dream_conv_transpose4x4s2_winograd_nhwc_f32", "dream_conv2d_nhwc_f32"),
                                   ("subsample2", "scatter2", "im2col3s2", "col2im3s2")),
    "resnet_h-2x75x101-bn_fusion0": ("resnet", "resnet_h", RESNET_H_SHAPE, {"DREAM_BN_FUSION": "0"}, 0,
                                     ("dream_bn_train_fwd_nhwc_f32", "dream_bn_train_bwd_nhwc_f32", "dream_maxpool3s2_bwd_nhwc_f32"),
                                     ("dream_conv1x1_bnstats_", "_bnmask_", "dream_conv1x1_pre_")),
    "resnet_h-2x75x101-bn_fusion_3x3": ("resnet", "resnet_h", RESNET_H_SHAPE, {"DREAM_BN_FUSION_3X3": "1"}, 0,
                                        ("dream_conv3x3_winograd_bnstats_nhwc_f32", "dream_conv3x3_winograd_bwd_bnmask_nhwc_f32"), ()),
    "resnet_h-2x75x101-tile4": ("resnet", "resnet_h", RESNET_H_SHAPE, {}, 4, (W4, "dream_conv4x4s2_winograd4_nhwc_f32"), ()),
}
# the cases of the default CPU suite (10, 14 and 82 s under the emulator); the rest behind DREAM_EMU_FULL=1
EMULATED_ALWAYS = ("vgg_f-1x35x45", "vgg_f-2x37x50", "resnet_h-2x75x101")
REFUSED_VARIANTS = ("vgg_ms2", "vgg_f_ms2_skip")


@contextlib.contextmanager
def recorded_launches():
    """Counts, per entry point, of what goes through ``ops.call`` while the block runs (launch_trace.Recorder's place, passing through)."""
    real, seen = ops.call, collections.Counter()

    def call(name, *args):
        seen[name] += 1
        return real(name, *args)

    ops.call = call
    try:
        yield seen
    finally:
        ops.call = real


@contextlib.contextmanager
def environment(values):
    """The DREAM_* switches that a network reads when it is constructed."""
    saved = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def winograd_tile(tile):
    forced = ops._WINOGRAD_TILE_FORCED
    ops.set_winograd_tile(tile)
    try:
        yield
    finally:
        ops.set_winograd_tile(forced)


def check_fp32_step(dev, name):
    """One fp32 training step of FP32_CASES[name] against the oracle, by the unchanged check of parity_checks, and the launches."""
    kind, arch, shape, env, tile, must, must_not = FP32_CASES[name]
    with environment(env), winograd_tile(tile), recorded_launches() as seen:
        if kind == "vgg":
            pc.check_vgg_train_grads(dev, arch, shape, k=7)
        else:
            pc.check_resnet_train_step(dev, arch, shape)
    missing = [n for n in must if not seen[n]]
    present = sorted(n for n in seen for part in must_not if part in n)
    assert not missing and not present, (name, "never launched: %s" % missing, "launched: %s" % present)
    return seen


def check_variant_refused(dev, name, shape=HOURGLASS_SHAPES[0]):
    """vgg_ms2 / vgg_f_ms2_skip at a shape whose sides are no multiples of 16: the reference raises, and the network raises a RuntimeError
    about the two sizes -- it neither crops silently nor launches a kernel on mismatched tensors -- and leaves the parameters alone."""
    b, h, w = shape
    x = torch.from_numpy(cases.image_batch(b, h, w, seed=3))
    ref = om.build_model(name, 7)
    try:
        ref(x)
    except RuntimeError:
        pass
    else:
        raise AssertionError("the oracle accepts %s at %s: hold it with check_vgg_train_grads instead" % (name, shape))
    net = pc.build_network(name, dev, optimizer="sgd", lr=0.0, in_res=(w, h))
    net.enable_training()
    ow, oh = net.trained_net_output_resolution()
    t = torch.from_numpy(cases.target_batch(b, 7, (ow, oh), in_wh=(w, h), seed=3))
    before = [p.detach().cpu().clone() for p in net.model.parameters()]
    try:
        net.train([pc.to(dev, x)], pc.to(dev, t))
    except RuntimeError as e:
        message = str(e)
    else:
        raise AssertionError("%s trained at %s, where the reference raises" % (name, shape))
    print("%s at %s refused: %s" % (name, shape, message))
    assert "size" in message.lower() and "must match" in message, message      # a refusal of the two shapes, as the reference's
    assert all(torch.equal(a, p.detach().cpu()) for a, p in zip(before, net.model.parameters()))


# ---- two Adam steps twice, graph replay (GPU only) --------------------------------------------------------------------------------
def _adam_network(dev, arch, shape, weights, graph=False, split=0):
    b, h, w = shape
    net = pc.build_network(arch, dev, weights=weights, optimizer="adam", lr=1e-5, in_res=(w, h))
    net.enable_training()
    if graph:
        net.hip_graph_train = True
        net.model.graph_split_leaves = split
    ow, oh = net.trained_net_output_resolution()
    x = pc.to(dev, torch.from_numpy(cases.image_batch(b, h, w, seed=3)))
    t = pc.to(dev, torch.from_numpy(cases.target_batch(b, 7, (ow, oh), in_wh=(w, h), seed=3)))
    return net, x, t


def _weights(arch):
    final = cases.RESNET_TRAIN_CASES[arch][4] if arch in cases.RESNET_TRAIN_CASES else cases.TRAIN_FINAL_KEYS
    return om.recipe_weights(om.build_model(arch, 7).state_dict(), final, cases.TRAIN_FINAL_SCALE)


def check_deterministic(dev, arch, shape, steps=2):
    """test_training_is_deterministic's property at a ragged shape: the same Adam steps from the same weights, run twice, give the same
    losses, parameters and BatchNorm buffers, bit for bit."""
    runs = []
    for _ in range(2):
        net, x, t = _adam_network(dev, arch, shape, _weights(arch))
        losses = [net.train([x], t).item() for _ in range(steps)]
        assert all(l == l and abs(l) < float("inf") for l in losses), losses
        runs.append((losses, {k: v.detach().clone() for k, v in net.model.state_dict().items()}))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert len(runs[0][1]) == len(runs[1][1]) > 0
    for k, a in runs[0][1].items():
        assert torch.equal(a, runs[1][1][k]), k
    print("deterministic %s %s: losses %s" % (arch, shape, ["%.9g" % l for l in runs[0][0]]))


def check_graph_replay(dev, arch, shape, split, steps=4):
    """The body of test_one_device_training_step_as_graph_replay_equals_eager at a ragged shape, without its host-time assertion: four
    Adam steps as hipGraph replays equal the eager steps bit for bit (losses, state_dict), and the graphs were really replayed."""
    wts = _weights(arch)
    g, x, t = _adam_network(dev, arch, shape, wts, graph=True, split=split)
    lg = [g.train([x], t).item() for _ in range(steps)]
    e, x, t = _adam_network(dev, arch, shape, wts)
    le = [e.train([x], t).item() for _ in range(steps)]
    st = g.model.stats
    assert st["captures"] == 2 and st["replays"] == 2 * (steps - 1) and e.model.stats["replays"] == 0, st
    if split:
        plans = [v["bwd"].plan for v in g.model._graphs.values() if v["bwd"] is not None]
        kinds = [op[0] for op in plans[0]]
        assert len(plans) == 1 and kinds[0] == "main" and kinds[-2:] == ["join", "main"] and kinds.count("side") >= 3, kinds
    assert lg == le, (lg, le)
    for (k, a), (_, b) in zip(g.model.state_dict().items(), e.model.state_dict().items()):
        assert torch.equal(a, b), k
    g.hip_graph_train = False                              # back to the eager path, same parameters, same optimizer state
    assert g.train([x], t).item() == e.train([x], t).item()
    assert st["replays"] == 2 * (steps - 1)
    print("graph replay %s %s split %d: losses %s" % (arch, shape, split, ["%.9g" % l for l in lg]))


# ---- the fp16 training modes, held by their own modules -------------------------------------------------------------------------------
# E_p of the rounded CPU reference (fp16_resnet_step_checks.step_yardstick) at RESNET_H_SHAPE: upsample.12.bias 1.79e-3, upsample.10.weight
# 1.01e-2, upsample.12.weight 1.02e-2, upsample.10.bias 1.11e-2 -- then upsample.7.bias 9.3e-2, upsample.7.weight 0.111, upsample.9.weight
# 0.114 and up to order one in the trunk: the rule E_p <= 0.05 selects the same four tensors as at 2 x 64 x 64 (check_step asserts it);
# the rounded reference moves the loss by 1.42e-3.  With the decoder rounded as well (fp16_resnet_decoder_checks.step_yardstick) the four
# lie between 5.7e-6 and 5.6e-4.
RESNET_CONDITIONED = ("upsample.10.weight", "upsample.10.bias", "upsample.12.weight", "upsample.12.bias")
FP16_CASES = ("train_precision", "train_activation_storage", "train_gradient_storage", "resnet_gemm", "resnet_decoder", "resnet_both")


def check_fp16_step(dev, mode):
    """One training step of an fp16 mode at a ragged shape by the check_training_step / check_step of its module: every parameter
    (ResnetSimple: the loss and the conditioned tensors) within 3 E_p of the fp32 step, E_p from the CPU reference at that shape."""
    if mode == "train_precision":
        import fp16_train_checks as m
        m.check_training_step(dev, HOURGLASS_SHAPES[0])
    elif mode == "train_activation_storage":
        import fp16_train_storage_checks as m
        m.check_training_step(dev, HOURGLASS_SHAPES[0])
    elif mode == "train_gradient_storage":
        import fp16_grad_storage_checks as m
        m.check_training_step(dev, HOURGLASS_SHAPES[0])
    elif mode == "resnet_gemm":
        import fp16_resnet_step_checks as m
        m.check_step(dev, RESNET_H_SHAPE, RESNET_CONDITIONED)
    else:
        import fp16_resnet_decoder_checks as m                # (CONVT_GEMM_MAX_PIXELS = 0 in both arms: the stages are transposed convs)
        m.check_step(dev, mode == "resnet_both", RESNET_H_SHAPE, RESNET_CONDITIONED)
