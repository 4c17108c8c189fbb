#!/usr/bin/env python
"""Records what the Python layer LAUNCHES, for tests/test_launch_trace.py (development tool, NO GPU: it refuses to run
with one).  Usage, on a checkout of the commit whose behaviour is to be pinned:

    python tools/record_launch_trace.py | gzip -9n > tests/golden/launch_trace.json.gz

(690 KB of JSON, one row per line: stored compressed, 45 KB; `zcat` shows it, and two recordings compare with `zcmp`.)

Under tools/dry_run.py the planning entry points of the real library run and every launching one is a stub; the stub's
hook notes a ROW per call: the entry point, every non-pointer argument and descriptor field (floats as bit patterns) and
a LABEL per pointer -- 0 for NULL, `w:<key>[:i]` for a tensor of the network's weight dictionary (this tells the fp32,
f16, s16 and fused packs of one layer apart), `scratch:conv_ws`, `scratch:f16:<slot>`, `scratch:gn:<field>` for the
long-lived scratch buffers, `x` for anything else (`+<bytes>` behind a label: an address inside that buffer).  Planning
queries are not part of a trace.

Modes: the engine modes of dry_run.engine_modes (the eight of tools/record_conv_plans.py plus the celeba `Model` on the
all-fp32 engine) at the batch sizes of BATCHES, one pass each; then one pass per mode with a `KernelTimer` installed,
whose (variant, flops, shape) records are stored (and whose launches must equal the untimed pass).  Direct cases
(direct_cases()): ops.conv2d / ops.conv16 calls on paths no network reaches -- the module switches, `one_tile=`,
`tile=`, `out_hw=`, `out_nchw=` beside a residual, the two ValueErrors, a refused descriptor per entry point -- at the
smallest shapes that qualify, with the exception (type, message) where one is raised.

Distinct rows are stored once ("rows"); a mode or case is a list of indices.
"""
import bisect
import ctypes
import json
import os
import struct
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dry_run  # noqa: E402
from ddnm_amd import _lib, ops  # noqa: E402

BATCHES = (8, 1)


def _bits(v):
    return struct.unpack("<i", struct.pack("<f", v))[0]


def _pointee(t):
    """The pointee class of a POINTER(...) parameter type, None for a scalar (or raw address) parameter."""
    return t._type_ if isinstance(getattr(t, "_type_", None), type) else None


def signature(name):
    """Field names of a row of entry point `name` (behind the name itself)."""
    out = []
    for i, t in enumerate(_lib.PROTOTYPES[name][1]):
        st = _pointee(t)
        if st is not None and issubclass(st, ctypes.Structure):
            out += [f"{st.__name__}.{n}" for n, _ in st._fields_]
        else:
            out.append(f"arg{i}")
    return out


class Tracer:
    """The hook of dry_run.DryLib: `rows` grows by one row per launching call; `net` (anything with a weight dictionary
    `w` and, optionally, a GroupNorm workspace `_ws`) names the pointers."""

    def __init__(self):
        self.rows, self.net, self._index = [], None, None

    def _weights(self):
        w = getattr(self.net, "w", None) or {}
        if self._index is None or self._index[0] is not w or self._index[1] != len(w):
            spans = []

            def add(label, v):
                if isinstance(v, torch.Tensor) and v.numel():
                    spans.append((v.data_ptr(), v.data_ptr() + v.numel() * v.element_size(), label))
                elif isinstance(v, (tuple, list)):
                    for i, e in enumerate(v):
                        add(f"{label}:{i}", e)
            for k, v in w.items():
                add(f"w:{k}", v)
            spans.sort(key=lambda s: s[0])
            self._index = (w, len(w), [s[0] for s in spans], spans)
        return self._index[2], self._index[3]

    def label(self, p):
        if not p:
            return 0
        scratch = [("scratch:conv_ws", t) for t in ops._conv_ws.values()]
        scratch += [(f"scratch:f16:{k[1]}", t) for k, t in ops._f16_scratch_buf.items()]
        gn = getattr(self.net, "_ws", None)
        if gn is not None:
            scratch += [(f"scratch:gn:{f}", getattr(gn, f)) for f in ("partial", "scale", "shift")]
        for name, t in scratch:
            if t.data_ptr() <= p < t.data_ptr() + t.numel() * t.element_size():
                return name + (f"+{p - t.data_ptr()}" if p != t.data_ptr() else "")
        starts, spans = self._weights()
        i = bisect.bisect_right(starts, p) - 1
        if i >= 0 and p < spans[i][1]:
            return spans[i][2] + (f"+{p - spans[i][0]}" if p != spans[i][0] else "")
        return "x"

    def _value(self, v, t):
        if t is ctypes.c_void_p:
            return self.label(v)
        if t is ctypes.c_float:
            return _bits(v)
        return int(v)

    def __call__(self, name, args):
        row = [name]
        for a, t in zip(args, _lib.PROTOTYPES[name][1]):
            st = _pointee(t)
            if st is not None and issubclass(st, ctypes.Structure):
                row += [self._value(getattr(a._obj, n), ft) for n, ft in st._fields_]
            elif st is not None:                             # a small host array (POINTER(c_float))
                row.append(0 if a is None else [_bits(x) for x in a])
            else:
                row.append(self._value(a, t))
        self.rows.append(row)

    def take(self, net, fn):
        """(rows, exception as [type, message] or None) of `fn()` with `net` naming the pointers."""
        self.rows, self.net, self._index = [], net, None
        ops._conv_ws.clear()               # grown on demand, and a descriptor carries its size: every pass starts without
        ops._f16_scratch_buf.clear()
        err = None
        try:
            fn()
        except (ValueError, _lib.DDNMHipError) as e:
            err = [type(e).__name__, str(e)]
        return self.rows, err


class _Event:
    """torch.cuda.Event of the timed pass (the real one needs a device)."""

    def __init__(self, enable_timing=False):
        pass

    def record(self):
        pass


def timed(tracer, net, fn):
    """(rows, [(variant, flops, shape), ...]) of `fn()` with a KernelTimer installed."""
    timer, event = ops.KernelTimer(), torch.cuda.Event
    torch.cuda.Event = _Event
    ops.set_kernel_timer(timer)
    try:
        rows, err = tracer.take(net, fn)
    finally:
        ops.set_kernel_timer(None)
        torch.cuda.Event = event
    assert err is None, err
    return rows, [[r[0], r[1], list(s)] for r, s in zip(timer.records, timer.shapes)]


# ---------------------------------------------------------------------------------------------- direct calls
class _Net:
    def __init__(self, w):
        self.w = w


def direct_cases(dry):
    """[(name, weight dictionary, call, switches)]: `switches` = module attributes of ops set for the call.  B = 1, 16 x 16,
    128 channels is the smallest shape the MFMA families accept (the sub-pixel form: a 32 x 32 input, 64 channels)."""
    C, H = 128, 16
    e = torch.empty
    w3, w1 = torch.full((C, C, 3, 3), 0.01), torch.full((C, C, 1, 1), 0.02)
    wo, wu = torch.full((3, C, 3, 3), 0.01), torch.full((64, 64, 3, 3), 0.01)
    s3, s1, s31 = ops.s16_weight_scale(w3), ops.s16_weight_scale(w1), ops.s16_weight_scale(w3, w1)
    w = {"w3": ops.pack_conv_weight(w3), "w3.s16": (ops.pack_conv_weight_s16(w3, s3), s3, None),
         "w3.f16": ops.pack_conv_weight_f16(w3), "w3.h16": ops.pack_conv_weight16(w3),
         "w3.s16+skip": (ops.pack_conv_weight_s16(w3, s31), s31, ops.pack_conv_weight_s16(w1, s31)),
         "w1": ops.pack_conv_weight(w1), "w1.s16": (ops.pack_conv_weight_s16(w1, s1), s1, None),
         "skip": ops.pack_skip_weight(w1), "skip.f16": ops.pack_skip_weight(w1, f16=True), "wo": ops.pack_conv_weight(wo),
         "wu": ops.pack_conv_weight(wu), "wu.s16_subpixel": ops.upsample_weight_s16(wu), "bias": e(C)}
    x, x16, gn = e(1, H, H, C), e(1, H, H, C, dtype=torch.float16), (e(C), e(C))
    x32 = e(1, 32, 32, C)               # (the small-Cout kernel walks 8 x 32 tiles)

    def s16(**kw):
        return ops.conv2d(x, w["w3"], C, 3, gn=gn, emit_stats=True, weight_s16=w["w3.s16"], **kw)

    def f16(**kw):
        return ops.conv2d(x, w["w3"], C, 3, gn=gn, weight_f16=w["w3.f16"], **kw)

    def refused_conv2d():
        # the real launcher answers: it must never see an accepted descriptor where there is a device
        assert not torch.cuda.is_available(), "conv2d_refused: host-only machines"
        dry.real = ("ddnm_conv2d_f32",)
        try:
            ops.conv2d(e(1, H, H, 20), w["w3"], C, 3, emit_stats=True)        # Cin = 20: no planner or launcher takes it
        finally:
            dry.real = ()
    cases = [
        ("s16", s16, {}),
        ("s16_one_tile", lambda: s16(one_tile=True), {}),
        ("s16_force_one_tile", s16, {"FORCE_ONE_TILE": True}),
        ("s16_no_fused_gn", s16, {"_NO_FUSED_GN": True}),
        ("s16_fused_skip", lambda: ops.conv2d(x, w["w3"], C, 3, gn=gn, skip=(x, None), skip_weight=w["skip"], emit_stats=True,
                                              weight_s16=w["w3.s16+skip"]), {}),
        ("gather_1x1", lambda: ops.conv2d(x, w["w1"], C, 1, weight_s16=w["w1.s16"], emit_stats=True), {}),
        ("gather_1x1_no_s16_gather", lambda: ops.conv2d(x, w["w1"], C, 1, weight_s16=w["w1.s16"], emit_stats=True),
         {"_NO_S16_GATHER": True}),
        ("f32_no_fused_gn", lambda: ops.conv2d(x, w["w3"], C, 3, gn=gn, emit_stats=True), {"_NO_FUSED_GN": True}),
        ("f32_tile_2", lambda: ops.conv2d(x, w["w3"], C, 3, bias=w["bias"], tile=2), {}),
        ("f32_stride_2_out_hw", lambda: ops.conv2d(x, w["w3"], C, 3, bias=w["bias"], stride=2, pad=0, out_hw=(H // 2, H // 2),
                                                   tile=1), {}),
        ("s16_stride_2_out_hw", lambda: ops.conv2d(x, w["w3"], C, 3, stride=2, pad=0, out_hw=(H // 2, H // 2), emit_stats=True,
                                                   weight_s16=w["w3.s16"]), {}),
        ("small_cout_out_nchw", lambda: ops.conv2d(x32, w["wo"], 3, 3, gn=gn, bias=w["bias"], out_nchw=True), {}),
        ("out_nchw_with_residual", lambda: ops.conv2d(x32, w["wo"], 3, 3, gn=gn, bias=w["bias"], out_nchw=True,
                                                      res=e(1, 3, 32, 32)), {}),
        ("f16", f16, {}),
        ("f16_prepass_min_cout_0", f16, {"_F16_PREPASS_MIN_COUT": 0}),
        ("f16_fused_skip", lambda: f16(skip=(x, None), skip_weight=w["skip"], skip_weight_f16=w["skip.f16"]), {}),
        ("f16_fused_skip_without_f16_pack", lambda: f16(skip=(x, None), skip_weight=w["skip"]), {}),
        ("ups_subpixel", lambda: ops.conv2d(e(1, 32, 32, 64), w["wu"], 64, 3, ups=True, weight_s16=w["wu.s16_subpixel"],
                                            ups_subpixel=True, emit_stats=True), {}),
        ("ups_subpixel_not_qualifying", lambda: ops.conv2d(e(1, H, H, 64), w["wu"], 64, 3, ups=True,
                                                           weight_s16=w["wu.s16_subpixel"], ups_subpixel=True), {}),
        ("conv16", lambda: ops.conv16(x16, w["w3.h16"], C, 3, gn=gn), {}),
        ("conv16_out", lambda: ops.conv16_out(x16, w["w3.h16"], 3, bias=w["bias"], gn=gn), {}),
        ("conv16_refused", lambda: ops.conv16(e(1, H, H, 20, dtype=torch.float16), w["w3.h16"], C, 3), {}),
        ("conv2d_refused", refused_conv2d, {}),
    ]
    return [(name, w, fn, sw) for name, fn, sw in cases]


def run_direct(tracer, case):
    name, w, fn, switches = case
    saved = {k: getattr(ops, k) for k in switches}
    for k, v in switches.items():
        setattr(ops, k, v)
    try:
        return tracer.take(_Net(w), fn)
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def install():
    """(dry library, tracer) with the tracer hooked into every launching entry point."""
    dry = dry_run.install()
    dry_run.stub_device_queries()
    dry.on_launch = Tracer()
    return dry, dry.on_launch


def modes(tracer):
    """Yields (mode name, rows of the untimed pass, records of the timed pass or None).  The timed pass runs once per
    network configuration (at BATCHES[0]; both batch sizes of the celeba `Model`, whose variants differ)."""
    for name, net, run in dry_run.engine_modes(BATCHES, mfma32=True):
        rows, err = tracer.take(net, run)
        assert err is None, (name, err)
        records = None
        if name.startswith("celeba") or name.endswith(f"_b{BATCHES[0]}"):
            again, records = timed(tracer, net, run)
            diff = [(a, b) for a, b in zip(again, rows) if a != b][:1]
            assert again == rows, f"{name}: the timed pass launches differently ({len(again)} / {len(rows)} rows): {diff}"
        yield name, rows, records


class Table:
    """Distinct items stored once, in order of first appearance."""

    def __init__(self):
        self.items, self._at = [], {}

    def index(self, item):
        key = json.dumps(item)
        if key not in self._at:
            self._at[key] = len(self.items)
            self.items.append(item)
        return self._at[key]


if __name__ == "__main__":
    # --replay (tests/test_launch_trace.py): also where there is a device, without the one case that needs its absence
    if torch.cuda.is_available() and "--replay" not in sys.argv[1:]:
        sys.exit("record_launch_trace.py: record on a machine without a GPU (the conv2d_refused case asks the real launcher)")
    dry, tracer = install()
    rows, records = Table(), Table()
    out_modes, out_timed, out_direct = {}, {}, {}
    for name, trace, recs in modes(tracer):
        out_modes[name] = [rows.index(r) for r in trace]
        if recs is not None:
            out_timed[name] = [records.index(r) for r in recs]
        print(f"{name}: {len(trace)} launches", file=sys.stderr)
    for case in direct_cases(dry):
        if case[0] == "conv2d_refused" and torch.cuda.is_available():
            continue
        trace, err = run_direct(tracer, case)
        out_direct[case[0]] = {"rows": [rows.index(r) for r in trace], "error": err}
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(["git", "status", "--porcelain", "ddnm_amd"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    print(f"{len(rows.items)} distinct rows, {len(records.items)} distinct timer records", file=sys.stderr)

    def lines(items):         # one item per line: a later re-record shows up row by row
        return "[\n" + ",\n".join(json.dumps(i, separators=(",", ":")) for i in items) + "\n]"

    def block(d):
        return "{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}" for k, v in d.items()) + "\n}"
    used = sorted({r[0] for r in rows.items})
    sys.stdout.write(f'{{"recorded_at":{json.dumps(commit + (" (ddnm_amd modified)" if dirty else ""))},\n'
                     f'"entry_points":{block({n: signature(n) for n in used})},\n"rows":{lines(rows.items)},\n'
                     f'"records":{lines(records.items)},\n"modes":{block(out_modes)},\n"timed":{block(out_timed)},\n'
                     f'"direct":{block(out_direct)}}}\n')
