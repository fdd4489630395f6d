"""The launch list of ResnetSimple with inference_conv_ksplit, pinned without a GPU (the harness of test_resnet_launch_trace.py: the
network runs on the ``meta`` device with ``ops.call`` / ``ops.ptr`` / ``ops.stream`` replaced by a recorder; the rule is the product
library's host function, so the slices in a trace are the slices a GPU run gets).

* "off", and the attribute as the constructor left it, reproduce every case of tests/golden/resnet_launch_trace.json;
* "auto": tests/golden/resnet_ksplit_launch_trace.json pins the traces of resnet_h at 1, 8, 16 and 128 frames of 400 x 400 and of
  resnet_f at (1, 200, 200) and (32, 400, 400) -- and whatever the fixture says: split entries stand only where a covered launch stood,
  the stem, the head and the 33 residual launches are the "off" launches with their arguments, every other launch is the "off" launch
  or its split sibling with S in front, and where the rule says 1 everywhere the trace IS the "off" trace.

    python tests/test_resnet_ksplit_launch_trace.py --record

rewrites the fixture from the tree it runs in."""
import collections
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import launch_trace as lt  # noqa: E402
import test_resnet_launch_trace as tr  # noqa: E402
from dream_amd import models, ops  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "resnet_ksplit_launch_trace.json")
SPLIT = {"dream_conv2d_f16_ksplit_nhwc_f16": "dream_conv2d_f16_nhwc_f16",
         "dream_conv_transpose4x4s2_f16_ksplit_nhwc_f16": "dream_conv_transpose4x4s2_f16_nhwc_f16"}
RESIDUAL, PLAIN = "dream_conv2d_f16_res16_nhwc_f16", "dream_conv2d_f16_nhwc_f16"
AUTO_CASES = {"h-%dx400x400" % b: ("h", (b, 400, 400)) for b in (1, 8, 16, 128)}
AUTO_CASES.update({"f-1x200x200": ("f", (1, 200, 200)), "f-32x400x400": ("f", (32, 400, 400))})


def _run(net, shape, ksplit, mp):
    case = dict(net=net, shape=shape, training=False, opts=dict(tr.HALF_STORED))
    module = tr._net(net)
    module.inference_conv_ksplit = ksplit
    try:
        return tr.run_case(case, mp)
    finally:
        module.inference_conv_ksplit = "off"


def _slices_by_the_rule(line):
    """S the rule answers for the launch an "off" line records (1 for a launch that is not covered)."""
    name, *args = line.split(" ")
    if name == PLAIN:
        b, h, w, cin, cout, _, k, _, flags = (int(v) for v in args)
        return ops.conv2d_f16_ksplit_resnet(b, h, w, cin, cout, k, flags)
    if name == SPLIT["dream_conv_transpose4x4s2_f16_ksplit_nhwc_f16"]:
        b, h, w, cin, cout, _, _ = (int(v) for v in args)
        return ops.conv_transpose4x4s2_f16_ksplit(b, h, w, cin, cout)
    return 1


def check_properties(name, off, auto):
    seq_off, seq_auto = off["seq"], auto["seq"]
    assert len(seq_off) == len(seq_auto), name
    assert collections.Counter(off["packs"]) == collections.Counter(auto["packs"]), name
    convs = [i for i, l in enumerate(seq_off) if l.startswith(PLAIN + " ")]
    stem, head = convs[0], convs[-1]
    assert head == len(seq_off) - 1 and sum(1 for l in seq_off if l.startswith(RESIDUAL + " ")) == 33, name
    nsplit = 0
    for i, (o, a) in enumerate(zip(seq_off, seq_auto)):
        s = 1 if i in (stem, head) else _slices_by_the_rule(o)
        if s == 1:
            assert a == o, (name, i, o, a)
            continue
        # the split sibling: the same scalars with S in front
        entry, rest = a.split(" ", 1)
        assert SPLIT.get(entry) == o.split(" ", 1)[0] and rest == "%d %s" % (s, o.split(" ", 1)[1]), (name, i, o, a)
        nsplit += 1
    assert seq_auto[stem] == seq_off[stem] and seq_auto[head] == seq_off[head], name
    assert [l for l in seq_auto if l.startswith(RESIDUAL + " ")] == [l for l in seq_off if l.startswith(RESIDUAL + " ")], name
    assert (nsplit == 0) == (seq_auto == seq_off), name
    return nsplit


@pytest.fixture(scope="module")
def parent_fixture():
    with open(tr.FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


_fresh = {}


@pytest.mark.parametrize("how", ["off", "never set"])
@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_off_is_the_pinned_launch_list(name, how, parent_fixture, monkeypatch):
    case = tr.CASES[name]
    if how == "never set":                                   # a network on which nothing ever assigned the attribute
        if case["net"] not in _fresh:
            _fresh[case["net"]] = models.ResnetSimple(pretrained=False, **tr.NETWORKS[case["net"]]).to("meta")
        monkeypatch.setitem(tr._nets, case["net"], _fresh[case["net"]])
    else:
        tr._net(case["net"]).inference_conv_ksplit = "off"
    got = tr.run_case(case, monkeypatch)
    want = lt.decode(parent_fixture, name)
    assert got["seq"] == want["seq"], lt.first_difference(want["seq"], got["seq"])
    assert collections.Counter(got["packs"]) == collections.Counter(want["packs"])
    assert not [l for l in got["seq"] if l.split(" ", 1)[0] in SPLIT]


def test_fixture_covers_exactly_the_cases(fixture):
    assert sorted(fixture["cases"]) == sorted(AUTO_CASES)


@pytest.mark.parametrize("name", sorted(AUTO_CASES))
def test_auto_launch_trace(name, fixture, monkeypatch):
    net, shape = AUTO_CASES[name]
    off = _run(net, shape, "off", monkeypatch)
    auto = _run(net, shape, "auto", monkeypatch)
    nsplit = check_properties(name, off, auto)
    want = lt.decode(fixture, name)
    assert auto["seq"] == want["seq"], lt.first_difference(want["seq"], auto["seq"])
    assert collections.Counter(auto["packs"]) == collections.Counter(want["packs"])
    assert nsplit == fixture["split_launches"][name]


def test_one_frame_splits_and_128_frames_do_not(fixture):
    assert fixture["split_launches"]["h-1x400x400"] >= 10 and fixture["split_launches"]["f-1x200x200"] >= 10
    assert fixture["split_launches"]["h-128x400x400"] == 0


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_resnet_ksplit_launch_trace.py --record")
    traces, counts = {}, {}
    for case_name, (net_, shape_) in AUTO_CASES.items():
        with pytest.MonkeyPatch.context() as patch:
            off_ = _run(net_, shape_, "off", patch)
            traces[case_name] = _run(net_, shape_, "auto", patch)
        counts[case_name] = check_properties(case_name, off_, traces[case_name])
    enc = lt.encode(traces)
    enc["split_launches"] = counts
    lt.write(enc, FIXTURE)
    print("wrote %s: %d cases, split launches %s, %d bytes" % (FIXTURE, len(traces), counts, os.path.getsize(FIXTURE)))
