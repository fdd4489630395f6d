"""The launch list of ResnetSimple with inference_head_fusion, pinned without a GPU (the harness of test_resnet_launch_trace.py: the
network runs on the ``meta`` device with ``ops.call`` / ``ops.ptr`` / ``ops.stream`` replaced by a recorder; the predicate and the
ksplit rule are the product library's host functions, so the branch a trace shows is the branch a GPU run takes).

* "off", and the attribute as the constructor left it, reproduce the half-stored cases of tests/golden/resnet_launch_trace.json and,
  with inference_conv_ksplit="auto", every case of tests/golden/resnet_ksplit_launch_trace.json: today's traces;
* "on": the trace is the "off" trace with its last two lines -- the last decoder stage and the head -- replaced by ONE line of
  dream_conv_transpose4x4s2_head_f16_nhwc_f16 that carries their scalars; every other line, and the weight packs, unchanged.  No fixture
  of its own: the expected trace is written down from the "off" one;
* with inference_conv_ksplit="auto" the same holds where the rule leaves the last stage in one slice, and where it splits that stage
  the "on" trace IS the "auto" trace."""
import collections
import json

import pytest

import launch_trace as lt
import test_resnet_ksplit_launch_trace as tk
import test_resnet_launch_trace as tr
from dream_amd import models, ops

FUSED = "dream_conv_transpose4x4s2_head_f16_nhwc_f16"
STAGE, CONV = "dream_conv_transpose4x4s2_f16_nhwc_f16", "dream_conv2d_f16_nhwc_f16"
HALF_CASES = sorted(n for n, c in tr.CASES.items() if c["opts"] == tr.HALF_STORED)
ON_CASES = {"h-128x400x400": ("h", (128, 400, 400)), "f-32x400x400": ("f", (32, 400, 400)), "h-16x400x400": ("h", (16, 400, 400)),
            "f-2x70x93": ("f", (2, 70, 93)), "h-1x320x320": ("h", (1, 320, 320))}


@pytest.fixture(autouse=True)
def _switches_off_afterwards():
    """The meta networks are shared with the other suites of this process: none of them leaves here with a switch on."""
    yield
    for name in tr._nets:
        tr._nets[name].inference_head_fusion = "off"
        tr._nets[name].inference_conv_ksplit = "off"


def _run(net, shape, fusion, ksplit, mp):
    module = tr._net(net)
    module.inference_head_fusion, module.inference_conv_ksplit = fusion, ksplit
    try:
        return tr.run_case(dict(net=net, shape=shape, training=False, opts=dict(tr.HALF_STORED)), mp)
    finally:
        module.inference_head_fusion, module.inference_conv_ksplit = "off", "off"


def fused_line(stage_line, head_line):
    """The one launch that stands for an "off" trace's last stage and head."""
    name, *s = stage_line.split(" ")
    assert name == STAGE
    b, h, w, cin, cmid, cmid_pad, flags = (int(v) for v in s)
    name, *c = head_line.split(" ")
    assert name == CONV
    b2, h2, w2, cin2, k, k_pad, ksize, stride, head_flags = (int(v) for v in c)
    assert (b2, h2, w2, cin2, ksize, stride, head_flags) == (b, 2 * h, 2 * w, cmid, 1, 1, ops.CONV_OUT_NCHW)
    return " ".join([FUSED] + [repr(v) for v in (b, h, w, cin, cmid, cmid_pad, k, k_pad, flags)])


def check_on_against_off(name, off, on):
    assert collections.Counter(on["packs"]) == collections.Counter(off["packs"]), name
    want = off["seq"][:-2] + [fused_line(off["seq"][-2], off["seq"][-1])]
    assert on["seq"] == want, lt.first_difference(want, on["seq"])
    assert lt.count(on, FUSED) == 1 and lt.count(on, STAGE) == lt.count(off, STAGE) - 1 and lt.count(on, CONV) == lt.count(off, CONV) - 1, name


@pytest.fixture(scope="module")
def parent_fixture():
    with open(tr.FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ksplit_fixture():
    with open(tk.FIXTURE) as f:
        return json.load(f)


_fresh = {}


@pytest.mark.parametrize("how", ["off", "never set"])
@pytest.mark.parametrize("name", HALF_CASES)
def test_off_is_the_pinned_launch_list(name, how, parent_fixture, monkeypatch):
    assert len(HALF_CASES) == 3
    case = tr.CASES[name]
    if how == "never set":                                   # a network on which nothing ever assigned the attribute
        if case["net"] not in _fresh:
            _fresh[case["net"]] = models.ResnetSimple(pretrained=False, **tr.NETWORKS[case["net"]]).to("meta")
        monkeypatch.setitem(tr._nets, case["net"], _fresh[case["net"]])
    else:
        tr._net(case["net"]).inference_head_fusion = "off"
    got = tr.run_case(case, monkeypatch)
    want = lt.decode(parent_fixture, name)
    assert got["seq"] == want["seq"], lt.first_difference(want["seq"], got["seq"])
    assert collections.Counter(got["packs"]) == collections.Counter(want["packs"])
    assert lt.count(got, FUSED) == 0


@pytest.mark.parametrize("name", sorted(tk.AUTO_CASES))
def test_off_with_ksplit_is_the_pinned_launch_list(name, ksplit_fixture, monkeypatch):
    net, shape = tk.AUTO_CASES[name]
    got = _run(net, shape, "off", "auto", monkeypatch)
    want = lt.decode(ksplit_fixture, name)
    assert got["seq"] == want["seq"], lt.first_difference(want["seq"], got["seq"])
    assert collections.Counter(got["packs"]) == collections.Counter(want["packs"])


@pytest.mark.parametrize("name", sorted(ON_CASES))
def test_on_replaces_the_last_stage_and_the_head_by_one_launch(name, monkeypatch):
    net, shape = ON_CASES[name]
    off = _run(net, shape, "off", "off", monkeypatch)
    on = _run(net, shape, "on", "off", monkeypatch)
    check_on_against_off(name, off, on)
    b, h, w, cin, cmid, cmid_pad, k, k_pad, flags = (int(v) for v in on["seq"][-1].split(" ")[1:])
    assert (b, cin, cmid, cmid_pad, k, flags) == (shape[0], 256, 256, 256, tr.NETWORKS[net]["n_keypoints"], ops.CONV_RELU) and k_pad % 32 == 0
    assert (2 * h, 2 * w) == tuple(tr._net(net).output_resolution((shape[2], shape[1])))[::-1]


@pytest.mark.parametrize("name", sorted(tk.AUTO_CASES))
def test_on_with_ksplit_yields_where_the_rule_splits_the_last_stage(name, monkeypatch):
    net, shape = tk.AUTO_CASES[name]
    auto = _run(net, shape, "off", "auto", monkeypatch)
    on = _run(net, shape, "on", "auto", monkeypatch)
    last = auto["seq"][-2].split(" ")
    if last[0] == STAGE:                                      # the rule left the last stage in one slice: the fusion applies
        b, h, w, cin, cmid = (int(v) for v in last[1:6])
        assert ops.conv_transpose4x4s2_f16_ksplit(b, h, w, cin, cmid) == 1
        check_on_against_off(name, auto, on)
    else:                                                     # it split that stage: the fusion yields
        assert tk.SPLIT.get(last[0]) == STAGE, last[0]
        assert on["seq"] == auto["seq"] and lt.count(on, FUSED) == 0, name


def test_on_with_a_split_last_stage_is_the_auto_trace(monkeypatch):
    """Two slices forced: every covered launch is split, the last stage too, and the fusion yields."""
    import fp16_ksplit_checks as kc
    with kc.forced_ksplit(2):
        auto = _run("h", (1, 320, 320), "off", "auto", monkeypatch)
        on = _run("h", (1, 320, 320), "on", "auto", monkeypatch)
    assert auto["seq"][-2].split(" ")[0] == "dream_conv_transpose4x4s2_f16_ksplit_nhwc_f16"
    assert on["seq"] == auto["seq"] and lt.count(on, FUSED) == 0
    assert collections.Counter(on["packs"]) == collections.Counter(auto["packs"])


def test_33_keypoints_keep_the_unfused_launches(monkeypatch):
    monkeypatch.setitem(tr.NETWORKS, "k33", dict(n_keypoints=33, full=False))
    try:
        off = _run("k33", (2, 70, 93), "off", "off", monkeypatch)
        on = _run("k33", (2, 70, 93), "on", "off", monkeypatch)
    finally:
        tr._nets.pop("k33", None)
    assert on["seq"] == off["seq"] and lt.count(on, FUSED) == 0 and on["seq"][-1].startswith(CONV + " ")
