"""The packed and folded copies of the weights that the kernels read, and the code that keeps them fresh.

``_PackedCache`` is DreamHourglass's: one copy per (weight, form, direction, tile), packed lazily.  ``PackedWeights`` is ResnetSimple's:
copies under the keys of RESNET_FORMS, packed lazily in evaluation and re-packed by ONE launch per training step (record -> table ->
stamp -> invalidate: begin_step).  Neither is an ``nn.Module``: a store is not in ``state_dict()``, ``reset()`` drops all it holds, and a
deep copy is a fresh, empty store -- a data-parallel replica builds its own copies on its own device.
"""
import collections
import contextlib
import os
import types

import torch

from . import ops


class _PackedCache:
    """Packed copies of conv weights for the MFMA kernels, one per (weight, form, direction, tile), refreshed when the parameter
    changes (optimizer step / load_state_dict bump ``_version``).  direction 0 / 1: the forward / the data-gradient operator
    (transposed, flipped taps); tile 4 / 2: the Winograd kernel the operand is for (0 where the form has no tile)."""

    def __init__(self):
        self._store = {}

    def reset(self):
        self._store = {}

    def __deepcopy__(self, memo):
        return type(self)()

    def get(self, weight, form, direction=0, tile=0):
        key = (id(weight), form, direction, tile)
        tag = (weight._version, weight.data_ptr(), weight.device)
        hit = self._store.get(key)
        if hit is None or hit[0] != tag:
            with torch.no_grad():
                hit = (tag, self._pack(weight.detach(), form, direction, tile))
            self._store[key] = hit
        return hit[1]

    @staticmethod
    def _pack(w, form, direction, tile):
        if form == "direct":                      # tap-major packing of the implicit-GEMM kernel
            return ops.pack_weight(w, direction)
        if form == "winograd":                    # transformed weights of the F(2x2,3x3) / F(4x4,3x3) kernel
            return ops.pack_weight_winograd_tile(w, direction, tile)
        if form == "ups":                         # the conv that follows a nearest x2 upsample, as the equivalent 4x4 transposed conv
            return ops.pack_convT4x4_weight(ops.upsample_conv_weight(w))               # (sub-pixel phase packing)
        if form == "ups_winograd":                # ... and that transposed conv by minimal filtering (9- / 25-position phase patterns)
            return ops.pack_convT4x4_winograd_weight_tile(ops.upsample_conv_weight(w), tile, direction)
        if form == "stride2":                     # a [Cin_T,Cout_T,3,3] ConvTranspose weight as the stride-2 conv that is its data gradient
            return ops.pack_conv_weight(w, 0)
        if form == "f16x3":                       # split precision: two fp16 planes of the tap-major packing
            return ops.pack_conv_weight_f16x3(w, direction)
        if form == "ups_f16x3":
            return ops.pack_convT4x4_weight_f16x3(ops.upsample_conv_weight(w))
        if form == "f16":                         # half precision: the `hi` plane and the exponent only
            return ops.pack_conv_weight_f16(w, direction)
        if form == "ups_f16":
            return ops.pack_convT4x4_weight_f16(ops.upsample_conv_weight(w))
        if form == "ups_f16b":                    # ... and the 16-slice plane its data gradient reads (train_upsample_precision="fp16")
            return ops.pack_upsample_conv_dgrad_weight_f16(w)
        raise ValueError("unknown packed form %r" % (form,))


def _col3(w):               # a 3x3 conv that runs on its patch rows (ops.im2col3s2): the GEMM weight [Cout][t Cin + c] = w[co][c][ky][kx]
    return w.permute(0, 2, 3, 1).reshape(int(w.shape[0]), -1, 1, 1).contiguous()


def _head_rows(w, rows):     # the head's [K, Cin, 1, 1] weight, its K output channels zero-padded to ``rows``
    w2 = w.reshape(int(w.shape[0]), int(w.shape[1]))
    return torch.cat([w2, w2.new_zeros((rows - int(w2.shape[0]), int(w2.shape[1])))]).reshape(rows, int(w2.shape[1]), 1, 1)


def _stem_cols(w, cols):     # the 7x7 stem's weight for its im2col rows: 147 taps, zero-padded to ``cols`` columns
    return torch.cat([w.reshape(64, 147), w.new_zeros((64, cols - 147))], dim=1).reshape(64, cols, 1, 1)


# ResnetSimple's packed forms: form -> (kind of the cache key, (the detached parameter, ``arg``) -> the copy).  The key is (kind, name), for
# the forms of TILED (kind, name, tile).  A trailing "T": the form of a ConvTranspose2d(k4,s2,p1) weight; a leading "stem_": of the 7x7 stem
# for its im2col rows (147 taps, ``arg`` columns); "col3": of a 3x3 conv on its patch rows; 0 / 1: forward / data-gradient operator.  The
# keys are visible in the re-pack records and in the early / late split of begin_step, so two forms may share a kind (the names differ) and
# one copy has two kinds: "w" and "w0" are both pack_conv_weight(w, 0) -- a follow-up may merge them, which changes what a train -> eval ->
# train sequence launches.
RESNET_FORMS = {
    "w": ("w", lambda w, _: ops.pack_conv_weight(w, 0)),                      # the direct kernel in evaluation -> (packed, rows, _)
    "w0": ("w0", lambda w, _: ops.pack_conv_weight(w, 0)),                    # ... in training, and
    "w1": ("w1", lambda w, _: ops.pack_conv_weight(w, 1)),                    # its data gradient
    "wT": ("w", lambda w, _: ops.pack_convT4x4_weight(w)),                    # sub-pixel phases -> (packed, rows)
    "wTb": ("wTb", lambda w, _: ops.pack_convT4x4_bwd_weight(w)),
    "wu4": ("wu4", lambda w, tile: ops.pack_convT4x4_winograd_weight_tile(w, tile)),        # ... by minimal filtering -> (u4, rows)
    "wu4b": ("wu4b", lambda w, tile: ops.pack_convT4x4_winograd_weight_tile(w, tile, 1)),
    "wino": ("wino", lambda w, tile: ops.pack_weight_winograd_tile(w, 0, tile)),            # stride-1 3x3 convs -> (u, rows)
    "wino1": ("wino1", lambda w, tile: ops.pack_weight_winograd_tile(w, 1, tile)),
    "g0": ("g0", lambda w, _: ops.pack_conv1x1_weight(w, 0)),                 # the 1x1 GEMM -> (packed, rows)
    "g1": ("g1", lambda w, _: ops.pack_conv1x1_weight(w, 1)),
    "g0col3": ("g0", lambda w, _: ops.pack_conv1x1_weight(_col3(w), 0)),
    "g1col3": ("g1", lambda w, _: ops.pack_conv1x1_weight(_col3(w), 1)),
    "g0T": ("g0T", lambda w, _: ops.pack_conv1x1_weight(                      # a transposed conv as one GEMM with N = 16 Cout
        w.permute(2, 3, 1, 0).reshape(16 * int(w.shape[1]), -1, 1, 1).contiguous(), 0)),
    "g0h": ("g0h", lambda w, rows: ops.pack_conv1x1_weight(_head_rows(w, rows), 0)[0]),     # the head conv, its K output
    "g1h": ("g1h", lambda w, rows: ops.pack_conv1x1_weight(_head_rows(w, rows), 1)[0]),     # channels zero-padded to ``rows``
    "g0hb": ("g0hb", lambda b, rows: torch.cat([b, b.new_zeros((rows - int(b.shape[0]),))])),             # ... and its bias
    "g0f16": ("g0f16", lambda w, _: ops.pack_conv1x1_weight_f16(w, 0)),       # the fp16 GEMM -> (halfs, e_w, rows)
    "g1f16": ("g1f16", lambda w, _: ops.pack_conv1x1_weight_f16(w, 1)),
    "g0f16col3": ("g0f16", lambda w, _: ops.pack_conv1x1_weight_f16(_col3(w), 0)),
    "g1f16col3": ("g1f16", lambda w, _: ops.pack_conv1x1_weight_f16(_col3(w), 1)),
    "stem_w": ("w", lambda w, cols: ops.pack_matrix_weight(w.reshape(64, 147), cols)[0]),                 # the 1-tap direct kernel
    "stem_g0e": ("g0e", lambda w, cols: ops.pack_conv1x1_weight(_stem_cols(w, cols), 0)[0]),             # the 1x1 GEMM in evaluation
    "stem_g0": ("g0", lambda w, cols: ops.pack_conv1x1_weight(_stem_cols(w, cols), 0)[0]),               # ... in training
    # train_decoder_precision="fp16": the half planes of a decoder stage -- sub-pixel phases (forward) and the 16-slice transposed plane
    # (data gradient) -> (halfs, None, e_w, rows); keys of their own: the evaluation copy "wf16T" is not shared.  Both join the batched
    # fp16 re-pack from the second step on (HALF_SOURCES modes 2 / 3)
    "wT16": ("wT16", lambda w, _: ops.pack_convT4x4_weight_f16(w)),
    "wT16b": ("wT16b", lambda w, _: ops.pack_convT4x4_dgrad_weight_f16(w)),
    "wf16col3": ("wf16col3", lambda w, _: ops.pack_conv_weight_f16(_col3(w), 0)),
    # eval-mode BatchNorm (+ the conv's bias) folded to (scale, shift): the one form of several tensors
    "bn": ("bn", lambda t, eps: ops.bn_fold(t[0], t[1], t[2], t[3], eps, t[4] if len(t) > 4 else None)),
}
for _sfx in ("f16x3", "f16"):                     # the split- / half-precision conv kernels (models._HALF_OPS): the same three forms each
    RESNET_FORMS["w" + _sfx] = ("w" + _sfx, lambda w, _, pack=getattr(ops, "pack_conv_weight_" + _sfx): pack(w, 0))
    RESNET_FORMS["w" + _sfx + "T"] = ("w" + _sfx, lambda w, _, pack=getattr(ops, "pack_convT4x4_weight_" + _sfx): pack(w))
    RESNET_FORMS["stem_w" + _sfx] = ("w" + _sfx, lambda w, _, pack=getattr(ops, "pack_conv_weight_" + _sfx): pack(w.reshape(64, 147, 1, 1), 0))
TILED = frozenset(("wino", "wino1", "wu4", "wu4b"))
HALF_SOURCES = {"g0f16": 0, "g1f16": 1, "wT16": 2, "wT16b": 3}           # packed from the parameter itself: batchable (PackedWeights.half_source)

# What a test may ask of a store: copies held; keys recorded for the fp32 table, is it built, its jobs; (early keys, all keys) of a split
# re-pack or None; is its late launch still pending; is the fp16 table built; idle: no re-pack state at all (every pack so far was lazy).
PackView = collections.namedtuple("PackView", "copies recorded table_built jobs split pending half_table_built idle")
_NOT_RECORDING = contextlib.nullcontext(())


class PackedWeights:
    """ResnetSimple's store (the module docstring has its life cycle).  It also owns the two per-replica pools of device words that are
    handed out per launch and restart with every training forward pass: the BatchNorm ticket words and the amax words."""

    def __init__(self):
        self._copies = {}                 # key -> (tag, copy)
        self._recording = None            # the records of the recording step (the table's), else None
        self._table = None                # the fp32 re-pack of one flat parameter buffer (_repack)
        self._pending = None              # (event of the late launch on the second stream, the early keys) of a split re-pack
        self._half = {}                   # key -> (parameter, mode) of the fp16 GEMM copies packed from a parameter itself
        self._table16 = None              # (stamp, table, scratch)
        self._tickets = self._amax = None
        self._ticket_pos = self._amax_pos = 0

    def reset(self):
        """Drops every copy, table, record and pool -- behind a pending re-pack on the second stream, which still writes into the copies."""
        self.join()
        self.__init__()

    def __deepcopy__(self, memo):
        return type(self)()

    def view(self):
        t = self._table
        return PackView(len(self._copies), len(t.records) if t else 0, bool(t) and t.table is not None, t.njobs if t else 0,
                        t.split and (len(t.split[2]), len(t.keys)) if t else None, self._pending is not None, self._table16 is not None,
                        t is None and self._table16 is None and self._pending is None)

    def get(self, key, tensors, build):
        """The copy under ``key``, (re)built by ``build()`` under no_grad when the (_version, data_ptr) of any of ``tensors`` changed."""
        rec = self._recording if key[0] != "bn" else None
        if self._pending is not None and key not in self._pending[1]:
            self.join()                              # the late part of the step's re-pack runs on the second stream (begin_step)
        tag = tuple((t._version, t.data_ptr()) for t in tensors)
        hit = self._copies.get(key)
        if hit is None or hit[0] != tag:
            with torch.no_grad(), (_NOT_RECORDING if rec is None else ops.record_packs()) as descs:
                out = build()
            self._copies[key] = hit = (tag, out)
            # batchable: everything build() launched was one of the table's kinds, reading the parameter itself (not a derived copy)
            if descs and all(any(d[1].data_ptr() == t.data_ptr() for t in tensors) for d in descs):
                rec[key] = (tensors, out, list(descs))
        return hit[1]

    def form(self, form, name, source, arg=None):
        """The copy of RESNET_FORMS form ``form`` of ``source`` (a parameter; for "bn" the list of tensors) of the layer ``name``."""
        kind, build = RESNET_FORMS[form]
        key = (kind, name, arg) if form in TILED else (kind, name)
        if form in HALF_SOURCES:
            self.half_source(key, source, HALF_SOURCES[form])
        if isinstance(source, list):
            return self.get(key, source, lambda: build([t.detach() for t in source], arg))
        return self.get(key, [source], lambda: build(source.detach(), arg))

    def half_source(self, key, weight, mode):
        """``key`` holds an fp16 GEMM copy packed from ``weight`` itself: the batched fp16 re-pack may rewrite it (_repack_half)."""
        self._half[key] = (weight, mode)

    def join(self):
        """The main stream waits for the late part of this step's re-pack (second stream); a no-op when none is pending."""
        pend, self._pending = self._pending, None
        if pend is not None:
            torch.cuda.current_stream().wait_event(pend[0])

    def restart_pools(self):
        self._ticket_pos = self._amax_pos = 0

    def tickets(self, device):
        """Allocator of zero ticket words for the BatchNorm launches of this replica (ops.bn_counter_buffer: every launch takes its own
        slice of one persistent buffer and leaves it zero; the cursor restarts with every forward pass)."""
        buf = self._tickets
        if buf is None or buf.device != device:
            buf = self._tickets = ops.bn_counter_buffer(device)
            self._ticket_pos = 0

        def take(n):
            if n > buf.numel():                     # a short slice would let the kernel's ticket atomics run past the buffer
                raise RuntimeError("dream_amd: a BatchNorm launch needs %d ticket words, the replica's buffer holds %d" % (n, buf.numel()))
            if self._ticket_pos + n > buf.numel():
                self._ticket_pos = 0
            self._ticket_pos += n
            return buf[self._ticket_pos - n:self._ticket_pos]
        return take

    def amax_word(self, device):
        """One zero-initialised amax word per covered unit and step (ops.bn_bwd_apply_amax zeroes it again before it publishes), from a
        persistent pool beside the ticket words; the cursor restarts with every forward pass."""
        buf = self._amax
        if buf is None or buf.device != device:
            buf = self._amax = torch.zeros((1024,), dtype=torch.int32, device=device)
            self._amax_pos = 0
        self._amax_pos = self._amax_pos % buf.numel() + 1
        return buf[self._amax_pos - 1:self._amax_pos]

    # ---- training: all packed weight copies of a step refreshed by ONE launch ------------------------------------------------------
    def begin_step(self, first, split=False, half=False):
        """A training step re-packs every conv weight (the optimizer changed them all): 216 launches of 2-10 us, 6.8 % of a
        step at 16 frames (profiles/r02_layer_profile_resnet_h_train16.txt).  The first training step records which packed copies
        it builds from which parameter; from the second step on ONE launch (dream_pack_weights_batched: a device-resident job
        table, blockIdx.y = job) rewrites all of them in place at the start of the step and the entries are stamped with
        the parameters' new versions.  The few packs the table does not cover (tap-major copies for the direct kernel, the
        transposed convs' phase kernels) stay lazy.  Skipped while a hipGraph capture is under way (the data-parallel replicas
        capture their whole step, packing included).  ``first``: the module's first parameter, whose data_ptr stamps the table."""
        self.join()
        if first.is_cuda or os.environ.get("DREAM_PACK_BATCHED_ON_CPU"):
            if (first.is_cuda and torch.cuda.is_current_stream_capturing()) or os.environ.get("DREAM_PACK_BATCHED", "1") == "0":
                self._recording = None
            else:
                self._repack(first, split)
        if half and first.is_cuda and not torch.cuda.is_current_stream_capturing():
            self._repack_half(first)

    def _repack(self, first, split):
        st = self._table
        if st is None or st.stamp != first.data_ptr():                # records: key -> (tensors, copy, its pack descriptors)
            st = self._table = types.SimpleNamespace(stamp=first.data_ptr(), records={}, steps=0, table=None, njobs=0, keys=[], spans=None, split=None)
        if st.table is None:
            st.steps += 1
            if st.steps == 1 or not st.records:
                self._recording = st.records                 # record this step's packs
                return
            self._recording = None
            st.keys = list(st.records.items())
            descs = [d for _, (_, _, ds) in st.keys for d in ds]
            st.table, st.njobs = ops.pack_job_table(descs, first.device), len(descs)
            # the launch's workgroups by job size (round 6): the decoder's 2048 -> 256 transposed conv is 19 M packed floats, a 64 x 64 1x1 conv
            # 4 K -- with 16 workgroups each the large jobs set the launch's length (0.50 ms; DREAM_PACK_SPANS=0 restores that)
            st.spans = ops.pack_span_table(descs, first.device) if os.environ.get("DREAM_PACK_SPANS", "1") != "0" else None
            # Round 6, measured and NOT adopted (DREAM_PACK_SPLIT=1 opts in; DESIGN.md 4.9, profiles/r06_ab_pack_split.txt): the copies the stem,
            # layer1 and layer2 read are rewritten on the main stream, the rest on the SECOND stream, which is idle during a forward pass; the
            # main stream waits for it at the first use of a late copy (get -> join)
            if split and first.is_cuda and st.spans is not None and os.environ.get("DREAM_PACK_SPLIT", "0") == "1":
                early = [str(key[1]).startswith(("conv1", "layer1.", "layer2.")) for key, _ in st.keys]
                parts = []
                for want in (True, False):
                    ds = [d for (_, (_, _, dd)), e in zip(st.keys, early) if e == want for d in dd]
                    parts.append((ops.pack_job_table(ds, first.device), ops.pack_span_table(ds, first.device)) if ds else None)
                if parts[0] is not None and parts[1] is not None:
                    st.split = (parts[0], parts[1], frozenset(key for (key, _), e in zip(st.keys, early) if e))
        tags = {key: tuple((t._version, t.data_ptr()) for t in tensors) for key, (tensors, _, _) in st.keys}
        if any(self._copies.get(key, (None,))[0] != tag or self._copies[key][1] is not st.records[key][1] for key, tag in tags.items()):
            if split and st.split is not None:
                from .models import _SideStream
                (t0, s0), (t1, s1), early_keys = st.split
                ops.pack_weights_spans(t0, s0[0], s0[1])
                main, side = torch.cuda.current_stream(), _SideStream.live_stream(first.device)
                side.wait_stream(main)                   # behind the optimizer step and the previous backward's reads of the old copies
                with torch.cuda.stream(side):
                    ops.pack_weights_spans(t1, s1[0], s1[1])
                    self._pending = (side.record_event(), early_keys)
            elif st.spans is not None:
                ops.pack_weights_spans(st.table, st.spans[0], st.spans[1])
            else:
                ops.pack_weights_batched(st.table, st.njobs)
            for key, tag in tags.items():
                self._copies[key] = (tag, st.records[key][1])

    def _repack_half(self, first):
        """train_gemm_precision="fp16" / train_decoder_precision="fp16": the half copies that earlier steps built from a parameter itself (HALF_SOURCES; not the patch-row
        forms) are rewritten in place by ONE batched pack at the start of the step (three launches) and their entries stamped with the
        parameters' new versions -- packed one by one, three launches per copy, they cost a 16-frame step more than the fp16 GEMMs save
        (profiles/microbench_resnet_train_precision.txt).  Skipped on the first step (nothing is held yet), off the GPU and during a
        hipGraph capture; what the table does not hold stays lazy."""
        live = {key: src for key, src in self._half.items() if key in self._copies}
        if not live:
            return
        stamp = tuple((key,) + tuple(t.data_ptr() for t in ops.half_planes(self._copies[key][1])) + (src[0].data_ptr(),) for key, src in live.items())
        if self._table16 is None or self._table16[0] != stamp:
            entries = [(w.detach(), self._copies[key][1], mode) for key, (w, mode) in live.items()]
            # workgroups per job: 16 for the GEMM copies (4.8j's measured launch); with a decoder plane in the table one per 32 K halfs of
            # the largest plane, at most 256 -- the 2048 -> 256 planes of the 128-frame step are 8.4 M halfs each
            planes = [int(self._copies[key][1][0].numel()) for key, (_, mode) in live.items() if mode >= 2]
            wgs = min(256, max(16, max(planes) >> 15)) if planes else 16
            self._table16 = (stamp,) + ops.pack16_job_table(entries, first.device) + (wgs,)
        tags = {key: ((w._version, w.data_ptr()),) for key, (w, _) in live.items()}
        if any(self._copies[key][0] != tag for key, tag in tags.items()):
            ops.pack_conv1x1_weights_f16_batched(self._table16[1], self._table16[2], workgroups_per_job=self._table16[3])
            for key, tag in tags.items():
                self._copies[key] = (tag, self._copies[key][1])
