"""DreamHourglass issues a static list of C-ABI calls: this pins that list, launch by launch, without a GPU.

``ops.call`` / ``ops.ptr`` / ``ops.stream`` are replaced by recorders and the network is driven with tensors on the ``meta`` device, so
every host-side decision (which kernel, which tile, which fusion, which flags, which sizes) runs for real and no kernel does.  Host-side
size queries go to the built library, which needs no GPU.  Per launch the entry-point name and every scalar argument are recorded
(pointers dropped), per training pass also the shapes of the saved (input, output) pair of every plan entry (a half tensor's marked ``f16``).

tests/golden/hourglass_launch_trace.json holds the full traces (one table of distinct launches, one index list per case).  The lazy
weight-packing launches are compared as a multiset, everything else as an exact ordered sequence.  Its "switch_matrix" entry holds,
for every setting of the six precision switches, whether a pass runs or what it raises (switch_matrix()).

    python tests/test_hourglass_launch_trace.py --record

rewrites the fixture from the tree it runs in; a change that is meant to keep the launch list is checked against a fixture written
by the commit before it.
"""
import collections
import itertools
import json
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import launch_trace as lt  # noqa: E402
from dream_amd import data_parallel, models, ops  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "hourglass_launch_trace.json")
KEYPOINTS = 7
VARIANTS = {
    "vgg_q": {},
    "vgg_q_skip": dict(skip_connections=True),
    "vgg_f": dict(deconv_decoder=True),
    "vgg_f_skip": dict(deconv_decoder=True, skip_connections=True),
    "vgg_q_full": dict(full_output=True),
    "wide": dict(n_image_input_channels=10),             # the first conv of a later stage: image + previous maps
}

def _base_cases():
    """(variant, (B, H, W), pass, options) before the conv_algorithm x tile product."""
    out = [("vgg_q", (128, 400, 400), p, {}) for p in ("inference", "training")]
    out.append(("vgg_q", (128, 400, 400), "training", dict(pool_in_training_conv=False)))
    out += [("vgg_q", (8, 400, 400), p, dict(first_subbatch=2)) for p in ("inference", "training")]
    out += [(v, (16, 400, 400), p, {}) for v in ("vgg_q_skip", "vgg_f", "vgg_f_skip", "vgg_q_full") for p in ("inference", "training")]
    out += [(v, (2, 70, 93), p, {}) for v in ("vgg_q", "vgg_f") for p in ("inference", "training")]
    out += [("vgg_q", (1, 320, 320), p, {}) for p in ("inference", "training")]
    out += [(v, (2, 70, 93), p, dict(raises=True)) for v in ("vgg_q_skip", "vgg_f_skip") for p in ("inference", "training")]
    out += [("wide", (4, 64, 96), "training", dict(need_input_grad=True)),
            ("wide", (4, 64, 96), "inference", {}), ("wide", (4, 64, 96), "inference", dict(x_is_nhwc=True))]
    for shape in ((4, 64, 96), (16, 400, 400)):
        out += [(v, shape, "inference", dict(precision="fp16x3")) for v in ("vgg_q", "vgg_q_skip", "vgg_f_skip", "wide")]
        out.append(("wide", shape, "inference", dict(precision="fp16x3", x_is_nhwc=True)))
    shapes = ((4, 64, 96), (16, 400, 400))
    every = ("vgg_q", "vgg_q_skip", "vgg_f", "vgg_f_skip", "vgg_q_full")
    # the opt-in modes, appended so that the indices of the cases above stay what they were
    for shape in shapes:
        out += [(v, shape, "inference", dict(precision="fp16")) for v in ("vgg_q", "vgg_q_skip", "vgg_f_skip", "wide")]
        out.append(("wide", shape, "inference", dict(precision="fp16", x_is_nhwc=True)))
    act16 = dict(precision="fp16", activation_storage="fp16")
    out += [(v, shape, "inference", dict(act16)) for shape in shapes for v in every]
    out += [("vgg_q", (b, 400, 400), "inference", dict(act16, conv_ksplit="auto")) for b in (1, 8, 16)]
    out.append(("vgg_f_skip", (1, 400, 400), "inference", dict(act16, conv_ksplit="auto")))
    ladder = [dict(train_precision="fp16")]
    ladder.append(dict(ladder[-1], train_activation_storage="fp16"))
    ladder.append(dict(ladder[-1], train_gradient_storage="fp16"))
    for rung in ladder:
        for shape in shapes:
            out += [(v, shape, "training", dict(rung)) for v in every]
            out.append(("wide", shape, "training", dict(rung, need_input_grad=True)))
    out.append(("vgg_q", (128, 400, 400), "training", dict(ladder[-1])))          # the measured workload
    return out


def _cases():
    out = {}
    for n, (variant, shape, which, opts) in enumerate(_base_cases()):
        for algo in ("winograd", "direct"):
            for tile in ((0, 4, 2) if n == 0 else (0, 4)):
                name = "-".join([variant, "%dx%dx%d" % shape, which] + ["%s=%s" % kv for kv in sorted(opts.items())] + [algo, "tile%d" % tile])
                out[name] = dict(variant=variant, shape=shape, training=which == "training", algo=algo, tile=tile, **opts)
    return out


CASES = _cases()
# the six precision switches with their defaults, and their valid values
SWITCHES = (("precision", "fp32"), ("activation_storage", "fp32"), ("conv_ksplit", "off"),
            ("train_precision", "fp32"), ("train_activation_storage", "fp32"), ("train_gradient_storage", "fp32"))
SWITCH_VALUES = (("precision", ("fp32", "fp16x3", "fp16")), ("activation_storage", ("fp32", "fp16")), ("conv_ksplit", ("off", "auto")),
                 ("train_precision", ("fp32", "fp16")), ("train_activation_storage", ("fp32", "fp16")),
                 ("train_gradient_storage", ("fp32", "fp16")))
KSPLIT_ENTRY = "dream_conv2d_f16_ksplit_nhwc_f16"
_nets = {}


def _net(variant):
    """One network per variant on the meta device (the cases reset its switches and its packed-weight caches)."""
    if variant not in _nets:
        with pytest.MonkeyPatch.context() as mp, warnings.catch_warnings():
            mp.setenv("DREAM_VGG19_WEIGHTS", os.path.join(ROOT, "tests", "golden", "no-such-weights.pth"))   # default initialisation, no lookup
            warnings.simplefilter("ignore")
            net = models.DreamHourglass(KEYPOINTS, internalize_spatial_softmax=False, **VARIANTS[variant])
        _nets[variant] = net.to("meta")
    return _nets[variant]


def run_case(case, mp):
    """-> {"seq": launches in order, "packs": sorted weight-pack launches, "saved": shapes per plan entry, "error": text or None}."""
    net = _net(case["variant"])
    for switch, default in SWITCHES:                      # the nets are shared: no case inherits the previous one's switches
        setattr(net, switch, case.get(switch, default))
    net.conv_algorithm = case["algo"]
    net.pool_in_training_conv = case.get("pool_in_training_conv", True)
    data_parallel.reset_weight_caches(net)
    rec = lt.Recorder()
    rec.install(mp, ops)
    mp.setenv("DREAM_FIRST_SUBBATCH", str(case.get("first_subbatch", 0)))
    b, h, w = case["shape"]
    nhwc = case.get("x_is_nhwc", False)
    x = torch.empty((b, h, w, net.input_channel_pad()) if nhwc else (b, net.n_image_input_channels, h, w), device="meta")
    amax = torch.empty((1,), dtype=torch.int32, device="meta") if nhwc and net.precision != "fp32" else None
    params = [p.detach() for p in net.plan_parameters()]
    saved, error = [], None
    forced = ops._WINOGRAD_TILE_FORCED
    ops.set_winograd_tile(case["tile"])
    try:
        out, saved = net.run_forward(x, params, case["training"], x_is_nhwc=nhwc, x_amax=amax)
        assert tuple(out.shape) == (b, KEYPOINTS) + tuple(net.output_resolution((w, h)))[::-1]
        if case["training"]:
            assert len(saved) == len(net.plan_layers())
            need = case.get("need_input_grad", False)
            grads = net.run_backward(saved, torch.empty(out.shape, device="meta"), need_input_grad=need)
            if need:
                grads, g_input = grads
                assert tuple(g_input.shape[:3]) == (b, h, w)
            assert [tuple(g.shape) for g in grads] == [tuple(p.shape) for p in params]
    except RuntimeError as e:
        if not case.get("raises"):
            raise
        error = str(e)
    finally:
        ops.set_winograd_tile(forced)
    assert (error is not None) == bool(case.get("raises"))
    return dict(seq=[l for l in rec.launches if not lt.is_pack(l)], packs=sorted(l for l in rec.launches if lt.is_pack(l)),
                saved=["saved %s %s" % (_shape(i), _shape(o)) for i, o in saved], error=error)


def _shape(t):
    """A float32 tensor's shape; a half tensor's is marked."""
    return lt.shape(t) + (" f16" if t.dtype == torch.float16 else "")


def switch_matrix(mp):
    """Which setting of the six switches raises what, in which pass -> {"<the six values> <pass>": "ok" | "<exception type>: <message>"}:
    every combination of their valid values, and each switch alone at an unknown value, in an inference and in a training pass of
    vgg_q at 1 x 3 x 32 x 32."""
    net = _net("vgg_q")
    net.conv_algorithm, net.pool_in_training_conv = "winograd", True
    data_parallel.reset_weight_caches(net)
    lt.Recorder().install(mp, ops)
    x = torch.empty((1, 3, 32, 32), device="meta")
    params = [p.detach() for p in net.plan_parameters()]
    settings = list(itertools.product(*(values for _, values in SWITCH_VALUES)))
    defaults = [default for _, default in SWITCHES]
    settings += [defaults[:k] + ["bf16"] + defaults[k + 1:] for k in range(len(SWITCHES))]
    out = {}
    for setting in settings:
        for (switch, _), value in zip(SWITCHES, setting):
            setattr(net, switch, value)
        for training in (False, True):
            try:
                y, saved = net.run_forward(x, params, training)
                if training:
                    net.run_backward(saved, torch.empty(y.shape, device="meta"))
                result = "ok"
            except Exception as e:                        # noqa: BLE001 (the type is what is recorded)
                result = "%s: %s" % (type(e).__name__, e)
            out["%s %s" % ("/".join(setting), "training" if training else "inference")] = result
    for switch, default in SWITCHES:
        setattr(net, switch, default)
    return out


def check_properties(name, case, trace):
    """What the paths must show whatever the fixture says."""
    unforced_wino = case["algo"] == "winograd" and case["tile"] == 0
    if case["variant"] == "vgg_q" and case["shape"] == (128, 400, 400) and unforced_wino:
        assert lt.count(trace, "dream_conv3x3_winograd_nhwc_f32") == 0, name              # every Winograd conv picks F(4x4) on its own
        if case.get("train_precision", "fp32") == "fp16":
            pass                                         # (a half-precision training conv folds no pool: _group)
        elif case["training"] and case.get("pool_in_training_conv", True):
            assert lt.count(trace, "dream_conv3x3_winograd4_pool_both_nhwc_f32") == 4 and lt.count(trace, "dream_maxpool2_nhwc_f32") == 0, name
        elif case["training"]:
            assert lt.count(trace, "dream_conv3x3_winograd4_pool_both_nhwc_f32") == 0 and lt.count(trace, "dream_maxpool2_nhwc_f32") == 4, name
    if "first_subbatch" in case:
        sub = case["algo"] == "winograd" and case["tile"] != 2 and not case["training"]
        assert lt.count(trace, "dream_conv3x3_first_nchw_f32") == (4 if sub else 1), name
    if case["variant"].endswith("_skip") and not case.get("raises"):
        adds = lt.count(trace, "dream_add_f16" if case.get("activation_storage") == "fp16" else "dream_add_f32")
        folded = not case["training"] and case.get("precision", "fp32") == "fp32"
        assert (adds == 0) if folded else (adds >= 2), name
    if case.get("conv_ksplit") == "auto" and case["shape"] == (1, 400, 400):
        assert lt.count(trace, KSPLIT_ENTRY) >= 1, name                                   # a grid that cannot fill the chip is split ...
    elif case.get("conv_ksplit", "off") == "off":
        assert lt.count(trace, KSPLIT_ENTRY) == 0, name                                   # ... and with "off" nothing is
    if case.get("raises"):
        assert trace["error"].startswith("The size of tensor a (") and "must match the size of tensor b (" in trace["error"], name


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_exactly_the_cases(fixture):
    assert sorted(fixture["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_trace(name, fixture, monkeypatch):
    case = CASES[name]
    got = run_case(case, monkeypatch)
    check_properties(name, case, got)
    want = lt.decode(fixture, name)
    assert got["error"] == want["error"]
    assert got["seq"] == want["seq"], lt.first_difference(want["seq"], got["seq"])
    assert collections.Counter(got["packs"]) == collections.Counter(want["packs"])
    assert got["saved"] == want["saved"], lt.first_difference(want["saved"], got["saved"])


def test_switch_matrix(fixture, monkeypatch):
    got, want = switch_matrix(monkeypatch), fixture["switch_matrix"]
    assert sorted(got) == sorted(want)
    assert not {k: (want[k], got[k]) for k in want if got[k] != want[k]}


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_hourglass_launch_trace.py --record")
    traces = {}
    for case_name, case_ in CASES.items():
        with pytest.MonkeyPatch.context() as patch:
            traces[case_name] = run_case(case_, patch)
        check_properties(case_name, case_, traces[case_name])
    with pytest.MonkeyPatch.context() as patch:
        matrix = switch_matrix(patch)
    lt.write(dict(lt.encode(traces), switch_matrix=matrix), FIXTURE)
    print("wrote %s: %d cases, %d distinct launches, %d bytes" % (FIXTURE, len(traces), len(lt.encode(traces)["launches"]), os.path.getsize(FIXTURE)))
