"""The launch list of a ResnetSimple training step with train_decoder_precision, pinned without a GPU (the harness of
test_resnet_launch_trace.py: the network runs on the ``meta`` device with ``ops.call`` / ``ops.ptr`` / ``ops.stream`` replaced by a recorder).

* "fp32", and the attribute as the constructor left it, reproduce the training cases of tests/golden/resnet_launch_trace.json;
* "fp16" changes, per covered "convT" record, exactly its three products -- the forward launch, the data-gradient launch, the weight-gradient
  leaf (one fp16 launch + its unpack; the bias gradient leaves the Winograd-domain launch and becomes the fp32 channel sum) -- plus the amax
  form of that record's BatchNorm apply pass and the packs of its two half planes; every other launch is the "fp32" launch with its
  arguments, in its place, and no ``absmax`` launch appears.  Covered: every decoder stage that did not take the small-map GEMM form
  (at 16 frames of 400 x 400 the first stage is a GEMM + col2im4s2 and stays; at 128 frames it is covered)."""
import collections
import json

import pytest

import launch_trace as lt
import test_resnet_launch_trace as tr
from dream_amd import models

FWD32 = ("dream_conv_transpose4x4s2_winograd_nhwc_f32", "dream_conv_transpose4x4s2_winograd4_nhwc_f32", "dream_conv_transpose4x4s2_nhwc_f32")
FWD16 = "dream_conv_transpose4x4s2_f16_sat_nhwc_f32"
DGRAD32 = ("dream_conv4x4s2_winograd_nhwc_f32", "dream_conv4x4s2_winograd4_nhwc_f32", "dream_conv4x4s2_nhwc_f32")
DGRAD16 = "dream_conv_transpose4x4s2_dgrad_f16_nhwc_f32"
WGRAD32 = ("dream_convT4x4_wgrad_winograd_nhwc_f32", "dream_convT4x4_wgrad_nhwc_f32")
WGRAD16 = "dream_convT4x4_wgrad_f16_nhwc_f32"
APPLY32, APPLY16 = "dream_bn_bwd_apply_nhwc_f32", "dream_bn_bwd_apply_amax_nhwc_f32"
# case -> covered decoder stages; LOSERS: those of them whose weight gradient keeps the fp32 launch (ops.convT4x4_wgrad_f16_pays: the
# 2048 -> 256 stage, a transposed conv only from 128 frames on)
CASES = {"h-16x400x400-training": 3, "h-128x400x400-training": 4, "f-16x400x400-training": 4, "h-2x70x93-training": 0,
         "h-16x400x400-training-train_gemm_precision=fp16": 3}
SMALL_MAPS = "h-2x70x93-training"             # every stage is a small-map GEMM: nothing is covered, the trace is the fp32 one
LOSERS = {"h-128x400x400-training": 1}


def _name(line):
    return line.split(" ", 1)[0]


def _run(case_name, mode, mp, fresh=False):
    case = tr.CASES[case_name]
    if fresh:
        mp.setitem(tr._nets, case["net"], models.ResnetSimple(pretrained=False, **tr.NETWORKS[case["net"]]).to("meta"))
    else:
        tr._net(case["net"]).train_decoder_precision = mode
    try:
        return tr.run_case(case, mp)
    finally:
        tr._net(case["net"]).train_decoder_precision = "fp32"


def _canonical(seq):
    """The sequence with the launches of a decoder stage's three products written form-independently: FWD / DGRAD by the input grid of the
    transposed conv, a weight-gradient leaf as WGRAD + its sorted hand-overs, the apply pass under its fp32 name."""
    out, i = [], 0
    while i < len(seq):
        line = seq[i]
        name, args = _name(line), line.split(" ")[1:]
        if name in FWD32 or name == FWD16:
            out.append("FWD " + " ".join(args[:5]))
        elif name in DGRAD32:
            out.append("DGRAD " + " ".join(args[:3]))
        elif name == DGRAD16:
            out.append("DGRAD %s %d %d" % (args[0], int(args[1]) // 2, int(args[2]) // 2))
        elif name == APPLY16:
            out.append(" ".join([APPLY32] + args))
        elif line.startswith("leaf ") and _name(seq[i + 1]) in WGRAD32 + (WGRAD16,):
            end = seq.index("end", i)
            out.append(line)
            out.append("WGRAD")
            out.extend(sorted(l for l in seq[i + 1:end] if l.startswith("grad ")))
            launches = [_name(l) for l in seq[i + 1:end] if not l.startswith("grad ")]
            if launches[0] == WGRAD16:
                assert launches == [WGRAD16, "dream_unpack_conv_weight", "dream_channel_sum_nhwc_f32"], launches
            out.append("end")
            i = end
        else:
            out.append(line)
        i += 1
    return out


@pytest.fixture(scope="module")
def parent_fixture():
    with open(tr.FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("how", ["fp32", "never set"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_off_is_the_pinned_launch_list(name, how, parent_fixture, monkeypatch):
    got = _run(name, "fp32", monkeypatch, fresh=how == "never set")
    want = lt.decode(parent_fixture, name)
    assert got["seq"] == want["seq"], lt.first_difference(want["seq"], got["seq"])
    assert collections.Counter(got["packs"]) == collections.Counter(want["packs"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_on_changes_exactly_the_covered_records(name, parent_fixture, monkeypatch):
    off = lt.decode(parent_fixture, name)
    on = _run(name, "fp16", monkeypatch)
    tr.check_properties(name, tr.CASES[name], on)
    covered = CASES[name]
    n_on = collections.Counter(_name(l) for l in on["seq"])
    n_off = collections.Counter(_name(l) for l in off["seq"])
    assert not any("absmax" in n for n in n_on)
    assert n_on[FWD16] == n_on[DGRAD16] == covered and n_on[WGRAD16] == covered - LOSERS.get(name, 0), n_on
    assert [l.split(" ")[4:6] for l in on["seq"] if _name(l) == WGRAD16] == [["256", "256"]] * n_on[WGRAD16]
    assert n_on[APPLY16] - n_off[APPLY16] == covered and n_off[APPLY32] - n_on[APPLY32] == covered
    # the stages the rule leaves alone keep their launches (the small-map GEMM form: col2im4s2 forward)
    assert n_on["dream_col2im4s2_nhwc_f32"] == n_off["dream_col2im4s2_nhwc_f32"] == 4 + (tr.CASES[name]["net"] == "f") - sum(n_off[n] for n in FWD32)
    assert sum(n_off[n] for n in FWD32) - sum(n_on[n] for n in FWD32) == covered
    # launch for launch: everything else is identical, in place, arguments included
    assert _canonical(on["seq"]) == _canonical(off["seq"]), lt.first_difference(_canonical(off["seq"]), _canonical(on["seq"]))
    if covered == 0:
        assert on["seq"] == off["seq"]
        # ... although the pass did resolve the switch: the decision was taped, and it was "no" for every stage
        net = tr._net(tr.CASES[name]["net"])
        net.train_decoder_precision = "fp16"
        try:
            assert net._resolve_switches(True).dec16
        finally:
            net.train_decoder_precision = "fp32"
    if "train_gemm_precision=fp16" in name:               # both switches: the fp16 GEMM launches stand beside the decoder's
        assert n_on["dream_conv1x1_bnstats_f16_nhwc_f32"] == n_off["dream_conv1x1_bnstats_f16_nhwc_f32"] > 0
    # the packs: two half planes per covered record come, packs of convT forms only go
    came = collections.Counter(on["packs"]) - collections.Counter(off["packs"])
    went = collections.Counter(off["packs"]) - collections.Counter(on["packs"])
    names = collections.Counter(_name(l) for l in came.elements())
    assert names == collections.Counter({"dream_pack_convT4x4_weight_f16x3": covered, "dream_pack_conv_weight_f16x3": covered}) or covered == 0, came
    assert all(" 16 " in l for l in came if _name(l) == "dream_pack_conv_weight_f16x3")           # the 16-slice transposed plane
    assert all(_name(l).startswith("dream_pack_convT4x4_") or "16" in l.split(" ")[3:4] for l in went.elements()), went
