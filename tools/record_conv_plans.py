#!/usr/bin/env python
"""Records what the C++ host layer answers, for tests/test_conv_host_plans.py (development tool, NO GPU: it refuses to
run with one).  Usage, on a checkout of the commit whose behaviour is to be pinned:

    python tools/record_conv_plans.py > tests/golden/conv_host_plans.json

Convolution part.  Corpus = every distinct ddnm_conv_desc (non-pointer fields, pointers as NULL / non-NULL) that reaches
the library in the eight modes of profiles/host_scaffold_launch_lists.md under tools/dry_run.py at the batch sizes of
BATCHES, plus the explicit edge grid below.  (B = 1, 4, 8, 32 give 2420 mode rows and a 450 KB table; BATCHES is thinned
to batch 1, where the plans split K most, and the benchmark's batch 8.  The edge grid is not thinned.)  Per row: the planning queries of all four families (QUERIES), and the refusal code of each
of the five LAUNCHERS for the row as it is and for its "statistics without scratch" variant (stats_out set, workspace
NULL); equal answer triples are stored once ("answers") and a row ends in the index of its triple.  A launcher that does not refuse cannot launch here (no device: the HIP runtime returns an error, a positive
number) and is stored as 0; the test never passes such a row to that launcher.

Step part.  For the 16 sampler-step entry points that exist per noise source: every argument mutation listed in
step_cases(), alone and together with a missing / misaligned noise source, with the refusal code (0 as above).

Integers only: acc_scale travels as its bit pattern.
"""
import ctypes
import json
import os
import struct
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ddnm_amd import _lib  # noqa: E402
from ddnm_amd._lib import ConvDesc, StepScalars  # noqa: E402

POINTERS = [n for n, t in ConvDesc._fields_ if t is ctypes.c_void_p]
FIELDS = [n for n, t in ConvDesc._fields_ if t is not ctypes.c_void_p]         # acc_scale: as bits
QUERIES = [f"ddnm_{fam}_{q}" for fam in ("conv2d_f32", "conv3x3_f16", "conv3x3_s16", "conv_gather_s16", "conv1x1_f16")
           for q in ("supported", "workspace_floats", "stats_tiles") if (fam, q) != ("conv2d_f32", "supported")] + \
          ["ddnm_conv2d_f32_tile_n", "ddnm_conv2d_f32_fuses_skip", "ddnm_conv3x3_s16_persistent",
           "ddnm_conv3x3_s16_ups_subpixel_supported"]
LAUNCHERS = ["ddnm_conv2d_f32", "ddnm_conv3x3_f16_f32", "ddnm_conv3x3_s16_f32", "ddnm_conv_gather_s16_f32", "ddnm_conv1x1_f16_f32"]
BATCHES = (8, 1)
DUMMY = 4096          # a non-null, 16-byte aligned address that is never dereferenced


def desc_key(d):
    vals = [struct.unpack("<i", struct.pack("<f", d.acc_scale))[0] if n == "acc_scale" else int(getattr(d, n)) for n in FIELDS]
    return tuple(vals) + (sum(1 << i for i, n in enumerate(POINTERS) if getattr(d, n)),)


def desc_of(key):
    d = ConvDesc()
    for n, v in zip(FIELDS, key):
        setattr(d, n, struct.unpack("<f", struct.pack("<i", v))[0] if n == "acc_scale" else v)
    for i, n in enumerate(POINTERS):
        setattr(d, n, DUMMY * (i + 1) if key[-1] >> i & 1 else None)
    return d


def conv_answers(L, key):
    """(query results, launcher codes of the row, launcher codes of its statistics-without-scratch variant)"""
    d = desc_of(key)
    q = [int(getattr(L, n)(ctypes.byref(d))) for n in QUERIES]

    def codes(d):
        return [min(int(getattr(L, n)(ctypes.byref(d), None)), 0) for n in LAUNCHERS]
    as_is = codes(d)
    d.stats_out, d.workspace, d.workspace_floats = DUMMY, None, 0
    return q, as_is, codes(d)


# ---------------------------------------------------------------------------------------------- corpus: the eight modes
class Capture:
    """Sits in front of tools/dry_run.py's library object and notes every ddnm_conv_desc that passes."""

    def __init__(self, inner, seen):
        self._inner, self._seen = inner, seen

    def __getattr__(self, name):
        fn = getattr(self._inner, name)
        args = _lib.PROTOTYPES.get(name, (None, []))[1]
        if not args or args[0] is not ctypes.POINTER(ConvDesc):
            return fn

        def call(d, *rest):
            self._seen[desc_key(d._obj)] = None
            return fn(d, *rest)
        return call


def mode_descs(seen):
    import dry_run
    dry = dry_run.install()
    _lib._lib = Capture(dry, seen)
    for _, _, run in dry_run.engine_modes(BATCHES):
        run()


# ---------------------------------------------------------------------------------------------- corpus: the edge grid
def edge_descs(seen):
    def add(B=2, H=32, C0=128, Cout=128, k=3, stride=1, pad=None, ptrs=("src0", "weight", "out", "gn_scale", "gn_shift", "amax_in"),
            **kw):
        d = ConvDesc()
        d.B, d.Hin, d.Win, d.C0, d.Cout, d.ksize, d.stride = B, H, H, C0, Cout, k, stride
        d.pad = k // 2 if pad is None else pad
        d.Ho = d.Wo = H // stride
        d.acc_scale = 1.0
        for n in ptrs:
            setattr(d, n, DUMMY)
        for n, v in kw.items():
            setattr(d, n, v)
        seen[desc_key(d)] = None
    for k in (3, 1):
        for B, H, C0, Cout in ((2, 32, 128, 128), (1, 16, 128, 128), (8, 64, 256, 256), (4, 8, 512, 512), (1, 10, 64, 64)):
            add(B, H, C0, Cout, k)                                              # (1, 10, ..): Ho * Wo = 100
            for tile in (1, 2, 3):
                add(B, H, C0, Cout, k, tile=tile)
            add(B, H, C0, Cout, k, stride=2)
            add(B, H, C0, Cout, k, flags=1)
            add(B, H, C0, Cout, k, ups=1, flags=2)
            add(B, H, C0, Cout, k, src_f16=1, ptrs=("src0", "weight", "out"))
            add(B, H, C0, Cout, k, src_f16=1)                                   # src_f16 with a GroupNorm prologue
            add(B, H, C0, Cout, k, ptrs=("src0", "weight", "out"))              # raw operand, no bound
            add(B, H, C0, Cout, k, ptrs=("src0", "weight", "out", "gn_scale"))  # gn_scale without gn_shift
            add(B, H, C0, Cout, k, acc_scale=0.0)
            add(B, H, C0, Cout, k, C1=64)                                       # C1 > 0, src1 missing
            add(B, H, C0, Cout, k, C1=64, src1=DUMMY)
            add(B, H, C0, Cout, k, res=DUMMY, res_ups=1)
            add(B, H, C0, Cout, k, badd=DUMMY, badd_stride=Cout)
            for ptrs in (("weight", "out"), ("src0", "out"), ("src0", "weight")):
                add(B, H, C0, Cout, k, ptrs=ptrs)
    for Cout in (3, 6):
        add(2, 32, 128, Cout, 3, out_nchw=1)
        add(2, 32, 128, Cout, 3, out_nchw=1, res=DUMMY)
    add(2, 32, 128, 128, 3, out_nchw=1)
    add(2, 33, 128, 128, 3, ups=1)                                              # ups with odd Hin
    add(2, 33, 128, 128, 3, ups=1, flags=2)
    add(2, 33, 128, 128, 3, res=DUMMY, res_ups=1)                               # res_ups with odd Ho
    add(2, 33, 128, 128, 1, res=DUMMY, res_ups=1)
    for sc0, sc1 in ((128, 0), (48, 0), (128, 64), (128, 48)):                  # skips: SC0 % 32 != 0, SC1 > 0
        for s1 in (None, DUMMY):
            add(2, 32, 128, 128, 3, skip0=DUMMY, skip1=s1, skip_weight=DUMMY, SC0=sc0, SC1=sc1)
        add(2, 32, 128, 128, 3, skip0=DUMMY, SC0=sc0, SC1=sc1)                  # no skip_weight
        add(2, 32, 128, 128, 3, skip0=DUMMY, skip_weight=DUMMY, SC0=sc0, SC1=sc1, ups=1)
    add(2, 32, 200, 128, 3)                                                     # Cin = 200
    add(2, 32, 200, 128, 1)
    add(2, 32, 128, 128, 3, pad=0)                                              # pad 0 on a 3x3
    add(2, 512, 128, 128, 3, ups=1, flags=2)                                    # a sub-pixel launch of many tiles
    add(8, 256, 128, 128, 3)                                                    # persistent form
    add(8, 256, 128, 128, 3, flags=1)
    add(256, 256, 128, 128, 3)                                                  # 2^31 output elements exactly
    add(256, 256, 128, 128, 1)


# ---------------------------------------------------------------------------------------------- step entry points
STEP_ARGS = {
    "combine": "x0 proj apy noise et et_bstride xt_next B chw s",
    "sr_avgpool": "xt et et_bstride noise y x0 xt_next B H W r s",
    "color": "xt et et_bstride noise y x0 xt_next B HW w3_host s",
    "inpaint": "xt et et_bstride noise y rank n_kept x0 xt_next B HW s",
    "inpaint_pi": "xt et et_bstride noise y y_stride rank n_kept_max x0 xt_next B HW s",
    "denoise": "xt et et_bstride noise y x0 xt_next B chw s",
    "plus_spectral": "xt_hat et_hat y_hat gains gains_cstride noise out_hat B C plane sigma_y sigma_t eta s",
    "plus_cs_pre": "xt et et_bstride noise aty x0_out xt_next w B C D ps a_lambda d1n d2n dd1 dd2 s",
}
STEP_GOOD = dict(et_bstride=3072, B=2, chw=3072, H=32, W=32, r=4, HW=1024, n_kept=100, n_kept_max=100, y_stride=300,
                 gains_cstride=1024, C=3, plane=1024, D=32, ps=8, sigma_y=0.1, sigma_t=0.5, eta=0.85, a_lambda=0.5, d1n=0.1,
                 d2n=0.2, dd1=0.3, dd2=0.4)
STEP_BAD = [("B", 0), ("chw", 0), ("chw", 6), ("HW", 0), ("HW", 6), ("H", 6), ("W", 6), ("et_bstride", 2), ("r", 2),
            ("y_stride", 302), ("y_stride", 296), ("n_kept_max", 0), ("C", 0), ("plane", 0), ("plane", 6), ("gains_cstride", 2),
            ("gains_cstride", -4), ("D", 0), ("D", 30), ("ps", 0), ("ps", 6)]


def step_cases():
    """[(entry point, {argument: value}), ...]: the mutations of an otherwise valid call; pointers are "null" / "odd"."""
    out = []
    for base, names in STEP_ARGS.items():
        names = names.split()
        for keyed in (False, True):
            fn = f"ddnm_step_{base}{'_keyed' if keyed else ''}_f32"
            ptrs = [n for n, t in zip(names, _lib.PROTOTYPES[fn][1]) if t is ctypes.c_void_p or n in ("s", "w3_host")]
            src_bad = [{"noise": "odd"}, {"noise": "null"}] if keyed else [{"noise": "null", "rng_on": 0}]
            muts = [{p: "null"} for p in ptrs if p != "noise"] + [{n: v} for n, v in STEP_BAD if n in names]
            if base == "plus_cs_pre":       # no output may alias an input or another output
                muts += [{"alias": [a, b]} for a, b in (("xt_next", "xt"), ("w", "aty"), ("x0_out", "et"), ("w", "xt_next"))]
            out += [(fn, m) for m in src_bad + muts] + [(fn, {**m, **sb}) for sb in src_bad for m in muts]
            if not keyed:
                out.append((fn, {"noise": "null"}))      # rng_on = 1: the in-kernel draw, accepted
    return out


def step_call(L, fn, mut):
    base = fn[len("ddnm_step_"):-len("_f32")].replace("_keyed", "")
    names = STEP_ARGS[base].split()
    sc = StepScalars(0.5, 0.8, 0.9, 0.1, 0.2, 1.0, mut.get("rng_on", 1), 1, 2, 3, 0, 0)
    args = []
    for i, (n, t) in enumerate(zip(names, _lib.PROTOTYPES[fn][1])):
        if n == "s":
            v = None if mut.get(n) == "null" else ctypes.byref(sc)
        elif n == "w3_host":
            v = None if mut.get(n) == "null" else (ctypes.c_float * 3)(0.3, 0.4, 0.3)
        elif t is ctypes.c_void_p:
            v = {"null": None, "odd": DUMMY * (i + 1) + 4}.get(mut.get(n), DUMMY * (i + 1))
            if mut.get("alias", [None])[0] == n:
                v = DUMMY * (names.index(mut["alias"][1]) + 1)
        else:
            v = mut.get(n, STEP_GOOD[n])
        args.append(v)
    return min(int(getattr(L, fn)(*args, None)), 0)


if __name__ == "__main__":
    if torch.cuda.is_available():
        sys.exit("record_conv_plans.py: run this on a machine without a GPU (accepted descriptors would launch on dummy pointers)")
    L = _lib.lib()
    seen = {}
    edge_descs(seen)
    n_edge = len(seen)
    mode_descs(seen)
    _lib._lib = L
    answers, rows = {}, []
    for k in seen:
        rows.append(list(k) + [answers.setdefault(json.dumps(conv_answers(L, k)), len(answers))])
    steps = [[fn, mut, step_call(L, fn, mut)] for fn, mut in step_cases()]
    print(f"{n_edge} edge rows, {len(rows) - n_edge} rows from the eight modes, {len(steps)} step calls", file=sys.stderr)
    def lines(items):         # one item per line: a later re-record shows up row by row
        return "[\n" + ",\n".join(json.dumps(i, separators=(",", ":")) for i in items) + "\n]"
    head = {"fields": FIELDS + ["pointer_mask", "answer"], "pointers": POINTERS, "queries": QUERIES, "launchers": LAUNCHERS}
    sys.stdout.write("{" + ",\n".join(f'"{k}":{json.dumps(v, separators=(",", ":"))}' for k, v in head.items()) +
                     f',\n"answers":{lines(json.loads(a) for a in answers)},\n"conv_rows":{lines(rows)},\n"step_rows":{lines(steps)}}}\n')
