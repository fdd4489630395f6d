"""ResnetSimple issues a static list of C-ABI calls per (shape, switches): this pins that list, launch by launch, without a GPU.

The harness of test_hourglass_launch_trace.py (launch_trace.py): the network runs on the ``meta`` device with ``ops.call`` / ``ops.ptr`` /
``ops.stream`` replaced by a recorder.  A training case pins three more things the launch list alone does not show while there is no
second stream:

* the weight-gradient leaves -- ``models._on_side`` is replaced, so each leaf appears in the sequence as ``leaf <shapes of its inputs>``
  ... ``end`` (the inputs are what _SideStream keeps alive or record_stream()s; _DeferredSide cuts graph segments by leaf count);
* the gradient hand-over -- ``run_backward`` gets a recording reducer: ``grad <shape>`` per assignment, ``pack_early <n>`` and
  ``mark_early`` where the early bucket is packed (the overlapped all-reduce and the early bucket depend on this order);
* the returned dict: one gradient of the parameter's shape for every parameter.

tests/golden/resnet_launch_trace.json holds the traces.  The lazy weight-pack launches are compared as a multiset, everything else as an
exact ordered sequence.

    python tests/test_resnet_launch_trace.py --record

rewrites the fixture from the tree it runs in; a change that is meant to keep the launch list is checked against a fixture written by the
commit before it.
"""
import collections
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import launch_trace as lt  # noqa: E402
from dream_amd import data_parallel, models, ops  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "resnet_launch_trace.json")
NETWORKS = {"h": dict(n_keypoints=7, full=False), "f": dict(n_keypoints=17, full=True)}
SWITCHES = dict(precision="fp32", conv_algorithm="winograd", conv1x1_algorithm="gemm", convT_algorithm="winograd", bn_fusion=True,
                bn_fusion_3x3=True, bn_fusion_head=True, stem_on_gemm=True, ds_on_gemm=True, train_gemm_precision="fp32",
                inference_activation_storage="fp32")
ONE_AT_A_TIME = [dict(bn_fusion=False), dict(bn_fusion_3x3=False), dict(bn_fusion_head=False), dict(stem_on_gemm=False), dict(ds_on_gemm=False),
                 dict(conv_algorithm="direct"), dict(conv1x1_algorithm="direct"), dict(convT_algorithm="direct")]
BIG, SMALL = (16, 400, 400), (2, 70, 93)
HALF_STORED = dict(precision="fp16", inference_activation_storage="fp16")


def _base_cases():
    """(network, (B, H, W), pass, options).  128 and 256 frames are limits of the kernels: above 69 frames of 400x400 the stem leaves the
    GEMM, above 47 the head leaves the BatchNorm loader, above 209 dz3_fits fails in layer1."""
    out = [(n, s, p, {}) for n in ("h", "f") for s in (BIG, SMALL) for p in ("inference", "training")]
    out += [("h", s, p, {}) for s in ((128, 400, 400), (1, 320, 320)) for p in ("inference", "training")]
    out.append(("h", (256, 400, 400), "training", {}))
    for sw in ONE_AT_A_TIME:
        out += [("h", BIG, "training", sw), ("h", (4, 128, 128), "training", sw), ("h", BIG, "inference", sw)]
    out.append(("f", (4, 128, 128), "training", dict(bn_fusion=False)))
    out.append(("h", BIG, "training", dict(env_DREAM_CONVT_WGRAD="direct")))
    out.append(("h", BIG, "training", dict(tile=4)))
    out += [("h", s, "training", dict(tile=2)) for s in (BIG, (128, 400, 400))]
    out.append(("h", BIG, "inference", dict(tile=4)))
    out += [("h", BIG, "inference", dict(precision="fp16x3")), ("f", SMALL, "inference", dict(precision="fp16x3"))]
    out += [("h", BIG, "inference", dict(precision="fp16")), ("f", SMALL, "inference", dict(precision="fp16"))]
    out += [(n, s, "inference", HALF_STORED) for n, s in (("h", BIG), ("f", SMALL), ("h", (1, 320, 320)))]
    out += [(n, s, "training", dict(train_gemm_precision="fp16")) for n, s in (("h", BIG), ("h", (4, 128, 128)), ("f", SMALL))]
    return out


def _cases():
    out = {}
    for net, shape, which, opts in _base_cases():
        name = "-".join([net, "%dx%dx%d" % shape, which] + ["%s=%s" % kv for kv in sorted(opts.items())])
        assert name not in out
        out[name] = dict(net=net, shape=shape, training=which == "training", opts=opts)
    return out


CASES = _cases()
_nets = {}


def _net(name):
    """One network per variant on the meta device (the cases set its switches and reset its packed-weight caches)."""
    if name not in _nets:
        _nets[name] = models.ResnetSimple(pretrained=False, **NETWORKS[name]).to("meta")
    return _nets[name]


class _Reducer:
    """What run_backward hands over, in order, into the recorder's sequence."""
    early_marker = "layer3.0"

    def __init__(self, launches):
        self.launches = launches

    def add(self, g):
        self.launches.append("grad " + lt.shape(g))

    def pack_early(self, grads):
        self.launches.append("pack_early %d" % len(grads))

    def mark_early(self, stream):
        self.launches.append("mark_early")


def run_case(case, mp):
    """-> {"seq": launches, leaves and gradient hand-overs in order, "packs": sorted weight-pack launches}."""
    net = _net(case["net"])
    opts = case["opts"]
    for name, default in SWITCHES.items():
        setattr(net, name, opts.get(name, default))
    net.train(case["training"])
    data_parallel.reset_weight_caches(net)
    rec = lt.Recorder()
    rec.install(mp, ops)
    for key, value in opts.items():
        if key.startswith("env_"):
            mp.setenv(key[4:], value)

    def on_side(side, fn, *inputs):
        assert side is None
        rec.launches.append(" ".join(["leaf"] + [lt.shape(t) for t in inputs]))
        out = fn()
        rec.launches.append("end")
        return out

    mp.setattr(models, "_on_side", on_side)
    b, h, w = case["shape"]
    x = torch.empty((b, 3, h, w), device="meta")
    want_shape = (b, NETWORKS[case["net"]]["n_keypoints"]) + tuple(net.output_resolution((w, h)))[::-1]
    forced = ops._WINOGRAD_TILE_FORCED
    ops.set_winograd_tile(opts.get("tile", 0))
    try:
        with torch.no_grad():
            if case["training"]:
                out, tape = net.run_forward_train(x)
                assert tuple(out.shape) == want_shape
                grads = net.run_backward(tape, torch.empty(out.shape, device="meta"), reducer=_Reducer(rec.launches))
                params = list(net.parameters())
                assert len(grads) == len(params)
                assert [tuple(grads[p].shape) for p in params] == [tuple(p.shape) for p in params]
            else:
                assert tuple(net.run_forward(x).shape) == want_shape
    finally:
        ops.set_winograd_tile(forced)
    return dict(seq=[l for l in rec.launches if not lt.is_pack(l)], packs=sorted(l for l in rec.launches if lt.is_pack(l)))


def _count_prefix(trace, prefix):
    return sum(1 for l in trace["seq"] if l.startswith(prefix))


def _count_infix(trace, infix):
    return sum(1 for l in trace["seq"] if infix in l.split(" ", 1)[0])


def check_properties(name, case, trace):
    """What the paths must show whatever the fixture says."""
    seq, opts = trace["seq"], case["opts"]
    fused = opts.get("bn_fusion", True)
    if case["training"]:
        # every BatchNorm of the network gets its backward: 104 in the trunk + the decoder's 4 (5)
        bn_bwd = _count_prefix(trace, "dream_bn_bwd_apply_" if fused else "dream_bn_train_bwd_")
        assert bn_bwd == {"h": 108, "f": 109}[case["net"]], name
        # the early bucket: packed exactly once, by the first leaf after the leaves of layer3.0 (its downsample conv's is the last of them),
        # with every parameter from layer3 on, and marked behind that leaf
        assert seq.count("mark_early") == 1 and _count_prefix(trace, "pack_early ") == 1, name
        at = seq.index("mark_early")
        n_early = len(list(_net(case["net"]).parameters())) - _net(case["net"]).dp_early_bucket()[0]
        assert seq[at - 3:at] == ["leaf", "pack_early %d" % n_early, "end"], name
        leaves = [i for i, l in enumerate(seq[:at - 3]) if l == "leaf" or l.startswith("leaf ")]
        blocks = list(_net(case["net"])._trunk())
        behind = sum(3 + hasattr(blk, "downsample") for n, blk in blocks[[n for n, _ in blocks].index("layer3.0"):])
        assert len(leaves) == behind + len(list(_net(case["net"])._decoder())), name          # one leaf per conv from layer3.0 on
        assert seq.count("end") == _count_prefix(trace, "leaf"), name
    else:
        assert not any(l.startswith(("leaf", "grad ", "pack_early", "mark_early")) for l in seq), name
    if case["net"] == "h" and case["shape"] == BIG and case["training"] and not opts:
        assert _count_prefix(trace, "dream_conv1x1_bwd_bnmask_") == 66, name
        assert _count_prefix(trace, "dream_conv3x3_winograd_bnstats_") == 30, name
        assert _count_prefix(trace, "dream_conv3x3_winograd_bwd_bnmask_") == 30, name
        assert _count_prefix(trace, "dream_bn_train_fwd_") == 0, name
    if case["net"] == "h" and case["shape"] == BIG and opts == dict(train_gemm_precision="fp16"):
        # the covered data gradients: of the 66 fused 1x1 GEMM ones of the fp32 trace (above) all but one run on the fp16 matrix cores
        # (the one left: the head conv's behind the last decoder BatchNorm, a "final" record -- _half_unit covers "conv" records only)
        assert _count_prefix(trace, "dream_conv1x1_bwd_bnmask_") == 66 and _count_prefix(trace, "dream_conv1x1_bwd_bnmask_f16") == 65, name
    if opts.get("inference_activation_storage") == "fp16":
        # the rule of test_fp16_resnet_storage_emulated.py (test_every_launch_between_the_ends_is_half_storage): behind the stem's im2col
        # every launch reads and writes half NHWC -- no fp32 conv between the image and the head, which writes the fp32 maps
        names = [l.split(" ", 1)[0] for l in seq if not l.startswith("dream_bn_fold_f32")]
        assert names[0] == "dream_im2col_nchw_f16" and names[-1] == "dream_conv2d_f16_nhwc_f16", name
        assert all(n.endswith("_nhwc_f16") for n in names[1:]) and not any(n.endswith("_nhwc_f32") for n in names), name
    if not fused:
        assert _count_infix(trace, "_bnstats_") == 0 and _count_infix(trace, "_bnmask_") == 0, name
        assert _count_prefix(trace, "dream_conv1x1_pre_") == 0, name


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
    assert got["seq"] == want["seq"], lt.first_difference(want["seq"], got["seq"])
    assert collections.Counter(got["packs"]) == collections.Counter(want["packs"])


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_resnet_launch_trace.py --record")
    traces = {}
    for case_name, case_ in CASES.items():
        with pytest.MonkeyPatch.context() as patch:
            traces[case_name] = run_case(case_, patch)
        check_properties(case_name, case_, traces[case_name])
    lt.write(lt.encode(traces), FIXTURE)
    print("wrote %s: %d cases, %d launches, %d distinct, %d bytes" % (
        FIXTURE, len(traces), sum(len(t["seq"]) + len(t["packs"]) for t in traces.values()), len(lt.encode(traces)["launches"]),
        os.path.getsize(FIXTURE)))
