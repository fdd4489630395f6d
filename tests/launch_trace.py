"""What the launch-trace tests share (test_hourglass_launch_trace.py, test_resnet_launch_trace.py): a recorder that stands in for
``ops.call`` / ``ops.ptr`` / ``ops.stream`` while a network runs on the ``meta`` device, the rule that tells the lazy weight-pack
launches from the rest, and the fixture format -- one table of distinct lines, per case the indices into it."""
import json

PACK_LAUNCHES = ("dream_upsample_conv3x3_weight_as_convT4x4", "dream_convT4x4_phase_weights")


def is_pack(launch):
    """The lazy weight-pack launches: compared as a multiset, everything else as an exact ordered sequence."""
    name = launch.split(" ", 1)[0]
    return name.startswith("dream_pack_") or name in PACK_LAUNCHES


class Recorder:
    """Per launch the entry-point name and every scalar argument (pointers dropped), in order, in ``launches``."""

    def __init__(self):
        self.launches = []

    def call(self, name, *args):
        self.launches.append(" ".join([name] + [repr(a) for a in args if type(a) in (int, float, bool)]))

    @staticmethod
    def ptr(t):
        if t is not None and not t.is_contiguous():
            raise RuntimeError("non-contiguous tensor passed to the HIP library")
        return None if t is None else Recorder                  # neither int nor float: dropped from the record

    @staticmethod
    def stream():
        return None

    def install(self, mp, ops):
        for name in ("call", "ptr", "stream"):
            mp.setattr(ops, name, getattr(self, name))


def shape(t):
    return "x".join(str(int(v)) for v in t.shape)


def count(trace, name):
    return sum(1 for l in trace["seq"] if l.split(" ", 1)[0] == name)


# ---- fixture: one table of distinct lines, per case the indices into it (list-valued entries of a trace; others are kept as they are) --
def encode(traces):
    table = {}

    def enc(v):
        return [table.setdefault(s, len(table)) for s in v] if isinstance(v, list) else v

    cases = {name: {k: enc(v) for k, v in t.items()} for name, t in traces.items()}
    return dict(launches=list(table), cases=cases)


def decode(fixture, name):
    return {k: [fixture["launches"][i] for i in v] if isinstance(v, list) else v for k, v in fixture["cases"][name].items()}


def write(fixture, path):
    with open(path, "w") as f:
        f.write('{"launches": [\n' + ",\n".join(json.dumps(s) for s in fixture["launches"]) + '\n],\n"cases": {\n')
        f.write(",\n".join("%s: %s" % (json.dumps(n), json.dumps(c, separators=(",", ":"))) for n, c in fixture["cases"].items()))
        for key in sorted(set(fixture) - {"launches", "cases"}):           # further entries: one mapping each, a line per item
            f.write("\n},\n%s: {\n" % json.dumps(key) + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in fixture[key].items()))
        f.write("\n}}\n")


def first_difference(want, got):
    n = next((i for i, (a, b) in enumerate(zip(want, got)) if a != b), min(len(want), len(got)))
    return "launch %d of %d (recorded) / %d (now):\n  recorded: %s\n  now:      %s\n  after:    %s" % (
        n, len(want), len(got), want[n] if n < len(want) else "<end>", got[n] if n < len(got) else "<end>", want[max(0, n - 3):n])
