"""The launch list of a DreamHourglass training pass with train_upsample_precision="fp16", pinned without a GPU (the recorder and the driver
of test_hourglass_launch_trace.py, on the ``meta`` device): vgg_q with train_precision="fp16" alone and with the two storage switches on
top, and a full_output network.  tests/golden/hourglass_upsample_launch_trace.json holds the traces;

    python tests/test_hourglass_upsample_launch_trace.py --record

rewrites it from the tree it runs in.  Whatever the fixture says, each trace is compared with the same pass with the switch off: exactly the
rule's entries changed their three launches -- forward, data gradient, weight gradient (+ the bias sum) --, an amax pass may come or go beside
them (the forward now publishes the amax the conv behind it used to measure; the data gradient scales by the amax it is handed), and nothing
else moved.
"""
import collections
import difflib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import launch_trace as lt  # noqa: E402
import test_hourglass_launch_trace as ht  # noqa: E402
from fp16_upsample_train_checks import is_covered  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "hourglass_upsample_launch_trace.json")
_STORED = dict(train_activation_storage="fp16", train_gradient_storage="fp16")
CASES = {
    "vgg_q-16x400x400": dict(variant="vgg_q", shape=(16, 400, 400)),
    "vgg_q-128x400x400-half-stored": dict(variant="vgg_q", shape=(128, 400, 400), **_STORED),
    "vgg_q-2x70x93": dict(variant="vgg_q", shape=(2, 70, 93)),
    "vgg_q_full-16x400x400": dict(variant="vgg_q_full", shape=(16, 400, 400)),
    "vgg_q_full-4x64x96-half-stored": dict(variant="vgg_q_full", shape=(4, 64, 96), **_STORED),
}
for _case in CASES.values():
    _case.update(training=True, algo="winograd", tile=0, train_precision="fp16")
# the launches of a covered entry with the switch on ...
NEW = ("dream_conv_transpose4x4s2_f16_nhwc_f32", "dream_conv_transpose4x4s2_dgrad_f16_nhwc_f32", "dream_upsample_conv3x3_wgrad_f16_nhwc_f32",
       "dream_channel_sum_nhwc_f32")
# ... and what the fp32 path may launch for it: forward, data gradient (one launch, or the 3x3 form + the upsample's backward), weight gradient
OLD = ("dream_conv_transpose4x4s2_winograd_nhwc_f32", "dream_conv_transpose4x4s2_winograd4_nhwc_f32", "dream_conv_transpose4x4s2_nhwc_f32",
       "dream_conv4x4s2_winograd_nhwc_f32", "dream_conv4x4s2_winograd4_nhwc_f32", "dream_conv3x3_winograd_nhwc_f32",
       "dream_conv3x3_winograd4_nhwc_f32", "dream_conv3x3_nhwc_f32", "dream_conv2d_nhwc_f32", "dream_upsample2_bwd_nhwc_f32",
       "dream_conv3x3_wgrad_winograd_bias_nhwc_f32", "dream_conv3x3_wgrad_winograd_nhwc_f32", "dream_conv3x3_wgrad_nhwc_f32",
       "dream_unpack_conv3x3_weight", "dream_channel_sum_nhwc_f32")
AMAX = "dream_absmax_f32"


def run(case, mode, mp):
    net = ht._net(case["variant"])
    net.train_upsample_precision = mode
    try:
        return ht.run_case(case, mp)
    finally:
        net.train_upsample_precision = "fp32"


def _name(launch):
    return launch.split(" ", 1)[0]


def check_properties(name, case, on, off):
    net = ht._net(case["variant"])
    ncov = sum(is_covered(kind, mod, flags) for kind, mod, flags in net.plan_layers())
    assert ncov == (4 if case["variant"] == "vgg_q_full" else 2), name
    for entry in NEW[:3]:
        assert lt.count(on, entry) == ncov and lt.count(off, entry) == 0, (name, entry)
    assert lt.count(on, NEW[3]) >= ncov, name                             # the bias gradient: the channel sum of the unrounded dz
    assert on["saved"] == off["saved"] and on["error"] is None and off["error"] is None, name        # fp32 in and out: no tensor changed its storage
    blocks = [op for op in difflib.SequenceMatcher(None, off["seq"], on["seq"], autojunk=False).get_opcodes() if op[0] != "equal"]
    gone, come = [], []
    for _, i1, i2, j1, j2 in blocks:
        gone += off["seq"][i1:i2]
        come += on["seq"][j1:j2]
    assert all(_name(l) in OLD + (AMAX,) for l in gone), (name, [l for l in gone if _name(l) not in OLD + (AMAX,)])
    assert all(_name(l) in NEW + (AMAX,) for l in come), (name, [l for l in come if _name(l) not in NEW + (AMAX,)])
    assert sum(_name(l) in NEW[:3] for l in come) == 3 * ncov, name
    # per covered entry at most one amax pass comes (its gradient's, where the launch behind published none) ...
    assert sum(_name(l) == AMAX for l in come) <= 2 * ncov and len(blocks) <= 2 * ncov, name
    # ... and the packs that moved are the covered weights' own
    moved = collections.Counter(on["packs"])
    moved.subtract(collections.Counter(off["packs"]))
    for launch, n in moved.items():
        if n:
            assert _name(launch) in ("dream_pack_convT4x4_weight_f16x3", "dream_pack_conv_weight_f16x3", "dream_pack_conv3x3_weight",
                                     "dream_pack_conv_weight", "dream_pack_convT4x4_weight", "dream_pack_convT4x4_winograd_weight",
                                     "dream_pack_convT4x4_winograd4_weight", "dream_pack_conv3x3_winograd_weight",
                                     "dream_pack_conv3x3_winograd4_weight") + lt.PACK_LAUNCHES, (name, launch, n)
    assert sum(n for launch, n in moved.items() if n > 0 and _name(launch).endswith("_f16x3")) == 2 * ncov, name


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_exactly_the_cases(fixture):
    assert sorted(fixture["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_trace(name, fixture, monkeypatch):
    case = CASES[name]
    on = run(case, "fp16", monkeypatch)
    off = run(case, "fp32", monkeypatch)
    check_properties(name, case, on, off)
    want = lt.decode(fixture, name)
    assert on["seq"] == want["seq"], lt.first_difference(want["seq"], on["seq"])
    assert collections.Counter(on["packs"]) == collections.Counter(want["packs"])
    assert on["saved"] == want["saved"], lt.first_difference(want["saved"], on["saved"])


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_hourglass_upsample_launch_trace.py --record")
    traces = {}
    for case_name, case_ in CASES.items():
        with pytest.MonkeyPatch.context() as patch:
            traces[case_name] = run(case_, "fp16", patch)
            check_properties(case_name, case_, traces[case_name], run(case_, "fp32", patch))
    lt.write(lt.encode(traces), FIXTURE)
    print("wrote %s: %d cases, %d distinct launches, %d bytes" % (FIXTURE, len(traces), len(lt.encode(traces)["launches"]), os.path.getsize(FIXTURE)))
