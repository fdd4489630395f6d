"""ResnetSimple's packed-weight store (dream_amd/packed_weights.py) as a state machine, without a GPU: which weight-pack launches each
step of a sequence issues -- record on step 1, table on step 2, one launch from then on, start over after a reset or a moved buffer.

The harness of test_resnet_launch_trace.py: network ``h`` on the ``meta`` device, ``lt.Recorder`` installed, ``models._on_side`` replaced,
shape (2, 70, 93), and DREAM_PACK_BATCHED_ON_CPU=1 so that the re-pack runs off the GPU.  ``ops.pack_job_table`` / ``ops.pack_span_table``
write host pointers, which the recorder does not have: stand-ins append ``table <n>`` / ``spans <n>`` to the record and return a meta
tensor.  Every parameter is bumped (``p.add_(0)``) after each training step, as an optimizer step would.  Per step only the pack-class
lines are kept, in order (``lt.is_pack`` plus the two stand-ins); the ordered rest of the launches is pinned by test_resnet_launch_trace.py.

On ``meta`` every ``data_ptr()`` is 0, so the rule "batchable iff every pack build() made reads one of the key's tensors itself" accepts
derived copies too: 217 records and 229 jobs HERE are not the device's numbers (test_gpu_parity.py asserts >= 190 jobs there).  The split
form (DREAM_PACK_SPLIT) and the fp16 re-pack return early off the GPU: they stay with test_gpu_parity.py::
test_resnet_batched_packing_equals_lazy_packing and test_gpu_fp16_resnet_train.py::test_later_steps_repack_in_one_batch.

tests/golden/resnet_repack_trace.json holds the traces, written by the commit named in its ``recorded_by`` entry -- the parent of the
commit that introduced the store -- with

    python tests/test_resnet_repack_trace.py --record <commit>

The second half of the file tests the store alone, on CPU tensors of a few elements.
"""
import copy
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import launch_trace as lt  # noqa: E402
import test_resnet_launch_trace as rt  # noqa: E402
from dream_amd import data_parallel, models, ops  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "resnet_repack_trace.json")
SHAPE = (2, 70, 93)
MOVED_TO = 4096               # the first parameter's data_ptr() after the simulated move (0 on meta before it)
# sequence -> (environment, steps).  "train": forward + backward, then every parameter bumped; "eval": an evaluation forward (no bump: what
# it re-packed lazily carries the current versions, and the next training step must still not use those copies); "reset":
# data_parallel.reset_weight_caches; "move": the first parameter reports another data_ptr() from here on -- what the store sees when the
# flat parameter buffer was reallocated (the other parameters' tags on a device move with it; on meta only this one can).
SEQUENCES = {
    "three_steps": ({}, ["train", "train", "train"]),
    "eval_between": ({}, ["train", "train", "eval", "train"]),
    "reset_between": ({}, ["train", "train", "reset", "train", "train"]),
    "all_lazy": ({"DREAM_PACK_BATCHED": "0"}, ["train", "train", "train"]),
    "no_spans": ({"DREAM_PACK_SPANS": "0"}, ["train", "train", "train"]),
    "storage_moved": ({}, ["train", "train", "move", "train", "train"]),
}


def run_sequence(name, mp):
    """-> per step the pack-class lines, in order."""
    env, steps = SEQUENCES[name]
    net = rt._net("h")
    for switch, default in rt.SWITCHES.items():
        setattr(net, switch, default)
    data_parallel.reset_weight_caches(net)
    rec = lt.Recorder()
    rec.install(mp, ops)
    for key in ("DREAM_PACK_BATCHED", "DREAM_PACK_SPANS", "DREAM_PACK_SPLIT"):
        mp.delenv(key, raising=False)
    mp.setenv("DREAM_PACK_BATCHED_ON_CPU", "1")
    for key, value in env.items():
        mp.setenv(key, value)

    def job_table(descs, device):
        rec.launches.append("table %d" % len(descs))
        return torch.empty((0,), dtype=torch.uint8, device="meta")

    def span_table(descs, device):
        rec.launches.append("spans %d" % len(descs))
        return torch.empty((0,), dtype=torch.uint8, device="meta"), len(descs)

    mp.setattr(ops, "pack_job_table", job_table)
    mp.setattr(ops, "pack_span_table", span_table)
    mp.setattr(models, "_on_side", lambda side, fn, *inputs: fn())
    x = torch.empty((SHAPE[0], 3) + SHAPE[1:], device="meta")
    first = next(net.parameters())
    out = []
    try:
        for step in steps:
            rec.launches.clear()
            with torch.no_grad():
                if step == "train":
                    net.train(True)
                    maps, tape = net.run_forward_train(x)
                    net.run_backward(tape, torch.empty(maps.shape, device="meta"))
                    for p in net.parameters():
                        p.add_(0)
                elif step == "eval":
                    net.train(False)
                    net.run_forward(x)
                elif step == "reset":
                    data_parallel.reset_weight_caches(net)
                else:
                    assert step == "move" and first.data_ptr() == 0
                    first.data_ptr = lambda: MOVED_TO
            out.append([l for l in rec.launches if lt.is_pack(l) or l.startswith(("table ", "spans "))])
    finally:
        first.__dict__.pop("data_ptr", None)
        data_parallel.reset_weight_caches(net)
    return out


def check_properties(name, steps):
    """What the machine must show whatever the fixture says."""
    lazy = [[l for l in s if not l.startswith(("table ", "spans ", "dream_pack_weights_"))] for s in steps]
    if name == "three_steps":
        assert len(lazy[0]) == len(steps[0]) > 200
        njobs = int(steps[1][0].split()[1])
        assert steps[1] == ["table %d" % njobs, "spans %d" % njobs, "dream_pack_weights_spans %d" % njobs]
        assert steps[2] == steps[1][2:]
    if name == "eval_between":                  # evaluation packs lazily and only what it needs; the step behind it is the one launch
        assert 0 < len(lazy[2]) == len(steps[2]) < len(steps[0]) and steps[3] == steps[1][2:]
    if name == "reset_between":                 # the machine starts over
        assert steps[2] == [] and steps[3:] == steps[:2]
    if name == "all_lazy":
        assert lazy == steps and steps[0] == steps[1] == steps[2]
    if name == "no_spans":
        assert not any(l.startswith("spans ") for s in steps for l in s)
        assert steps[2] == [steps[1][-1]] and steps[1][-1].startswith("dream_pack_weights_batched ")
    if name == "storage_moved":                 # a new stamp: record again, build a new table
        assert steps[2] == [] and len(lazy[3]) == len(steps[3]) == len(steps[0]) and steps[4][0].startswith("table ")


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_exactly_the_sequences(fixture):
    assert sorted(fixture["cases"]) == sorted(SEQUENCES) and fixture["recorded_by"]["commit"]


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_repack_trace(name, fixture, monkeypatch):
    got = run_sequence(name, monkeypatch)
    check_properties(name, got)
    want = lt.decode(fixture, name)
    assert len(got) == want["steps"]
    for i, step in enumerate(got):
        assert step == want["step%d" % i], "step %d: %s" % (i, lt.first_difference(want["step%d" % i], step))


# ---- the store alone ------------------------------------------------------------------------------------------------------------------
def _store():
    from dream_amd.packed_weights import PackedWeights
    return PackedWeights()


class _Build:
    """A counting build(): returns a fresh tensor per call."""

    def __init__(self, fn=None):
        self.calls, self.fn = 0, fn

    def __call__(self):
        self.calls += 1
        return self.fn() if self.fn else torch.zeros(2)


def test_hit_is_identical_until_version_or_storage_changes():
    store, w, build = _store(), torch.ones(3), _Build()
    a = store.get(("w", "x"), [w], build)
    assert store.get(("w", "x"), [w], build) is a and build.calls == 1
    w.add_(1)                                              # _version
    b = store.get(("w", "x"), [w], build)
    assert b is not a and build.calls == 2 and store.get(("w", "x"), [w], build) is b
    w.data = torch.ones(3)                                 # data_ptr (the version stays)
    assert store.get(("w", "x"), [w], build) is not b and build.calls == 3
    assert store.get(("w", "y"), [w], build) is not store.get(("w", "x"), [w], build) and build.calls == 4


def _recording_store(monkeypatch, first):
    monkeypatch.setenv("DREAM_PACK_BATCHED_ON_CPU", "1")
    monkeypatch.delenv("DREAM_PACK_BATCHED", raising=False)
    store = _store()
    store.begin_step(first, split=False, half=False)       # step 1: records
    return store


def _pack_of(src):
    """A build() whose one pack launch reads ``src`` (the record_packs() descriptor of ops' packers: kind, source, copy, cout, cin, mode)."""
    def build():
        out = torch.zeros(4)
        ops._log_pack(ops.PACK_CONV1X1, src, out, 2, 2, 0)
        return out
    return build


def test_bn_keys_are_never_recorded_and_derived_copies_are_not_batchable(monkeypatch):
    w = torch.ones(4)
    store = _recording_store(monkeypatch, w)
    derived = w.reshape(2, 2).t().contiguous()
    store.get(("g0", "a"), [w], _pack_of(w))               # reads the parameter itself
    store.get(("g0", "b"), [w], _pack_of(derived))         # reads a derived copy
    store.get(("g0", "c"), [w], _Build())                  # launches no pack of the table's kinds
    store.get(("bn", "a"), [w], _pack_of(w))               # folded BatchNorm: never recorded
    assert store.view().recorded == 1
    assert not store.view().table_built and store.view().jobs == 0


def test_reset_joins_a_pending_repack_before_dropping(monkeypatch):
    store, w, order = _store(), torch.ones(3), []
    store.get(("w", "x"), [w], _Build())

    class _Stream:                                         # the main stream: what join() makes wait for the late launch's event
        @staticmethod
        def wait_event(event):
            order.append((event, store.view().copies))

    # (only a split re-pack on a GPU leaves a launch pending: its state is set by hand here)
    store._pending = ("the late launch's event", frozenset())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: _Stream)
    assert store.view().pending and not store.view().idle
    store.reset()
    assert order == [("the late launch's event", 1)]       # joined while the copies were still there
    v = store.view()
    assert not v.pending and v.copies == 0 and not v.table_built and not v.half_table_built


def test_deepcopy_of_a_store_is_empty_and_shares_nothing(monkeypatch):
    w = torch.ones(4)
    store = _recording_store(monkeypatch, w)
    store.get(("g0", "a"), [w], _pack_of(w))
    store.half_source(("g0f16", "a"), w, 0)
    twin = copy.deepcopy(store)
    v = twin.view()
    assert (v.copies, v.recorded, v.table_built, v.half_table_built, v.pending, v.split) == (0, 0, False, False, False, None)
    twin.get(("g0", "z"), [w], _Build())
    assert store.view().copies == 1 and twin.view().copies == 1 and twin.view().recorded == 0
    cache = models._PackedCache()
    cache._store["k"] = 1
    assert copy.deepcopy(cache)._store == {} and cache._store == {"k": 1}
    cache.reset()
    assert cache._store == {}


def test_deepcopy_of_the_network_keeps_state_dict_and_empties_the_store(monkeypatch):
    net = rt._net("h")
    data_parallel.reset_weight_caches(net)
    rec = lt.Recorder()
    rec.install(monkeypatch, ops)
    net.train(False)
    with torch.no_grad():
        net.run_forward(torch.empty((1, 3, 64, 64), device="meta"))
    assert net._packs.view().copies > 100
    try:
        twin = copy.deepcopy(net)
    finally:
        data_parallel.reset_weight_caches(net)
    assert twin._packs is not net._packs and twin._packs.view().copies == 0
    a, b = net.state_dict(), twin.state_dict()
    assert list(a) == list(b) and [tuple(v.shape) for v in a.values()] == [tuple(v.shape) for v in b.values()]
    assert not any(k.startswith("_packs") for k in a)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_resnet_repack_trace.py --record <commit the tree is at>")
    traces = {}
    for seq_name in SEQUENCES:
        with pytest.MonkeyPatch.context() as patch:
            steps_ = run_sequence(seq_name, patch)
        check_properties(seq_name, steps_)
        traces[seq_name] = dict({"step%d" % i: s for i, s in enumerate(steps_)}, steps=len(steps_))
    encoded = lt.encode(traces)
    encoded["recorded_by"] = {"commit": sys.argv[2], "shape": "%dx%dx%d" % SHAPE, "device": "meta"}
    lt.write(encoded, FIXTURE)
    print("wrote %s: %s, %d bytes" % (FIXTURE, {n: [len(t["step%d" % i]) for i in range(t["steps"])] for n, t in traces.items()},
                                      os.path.getsize(FIXTURE)))
