"""The Python layer launches what it launched when tests/golden/launch_trace.json.gz was recorded
(tools/record_launch_trace.py): per engine mode the ordered list of launching library calls -- entry point, every
non-pointer argument and descriptor field, a label per pointer that tells a layer's weight packs and the scratch buffers
apart -- the `KernelTimer` records of a timed pass, and direct ops.conv2d / ops.conv16 calls on the paths no network
reaches.  No GPU needed: the launching entry points are stubs (tools/dry_run.py), the planners are the real host code.
The recorder runs in a process of its own (it replaces the library object and several module attributes).  A refactor
of the host Python must leave this file and the table alone."""
import gzip
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_launch_trace as rec  # noqa: E402


def _load(path):
    with (gzip.open if str(path).endswith(".gz") else open)(path, "rt") as f:
        t = json.load(f)
    # a mode or case as its rows themselves (the file stores distinct rows once)
    t["modes"] = {m: [t["rows"][i] for i in idx] for m, idx in t["modes"].items()}
    t["timed"] = {m: [t["records"][i] for i in idx] for m, idx in t["timed"].items()}
    for c in t["direct"].values():
        c["rows"] = [t["rows"][i] for i in c["rows"]]
    return t


@pytest.fixture(scope="module")
def table():
    return _load(os.path.join(ROOT, "tests", "golden", "launch_trace.json.gz"))


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    from ddnm_amd import build
    build.build()
    out = tmp_path_factory.mktemp("launch_trace") / "replay.json"
    with open(out, "w") as f:
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "record_launch_trace.py"), "--replay"], stdout=f,
                       stderr=subprocess.PIPE, check=True, cwd=ROOT)
    return _load(out)


def _first_difference(table, got, want):
    """The first differing row of two traces, field by field."""
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            if g[0] != w[0]:
                return f"launch {i}: {g[0]}, recorded {w[0]}"
            names = table["entry_points"][w[0]]
            return f"launch {i} ({w[0]}): " + ", ".join(f"{n} = {a!r}, recorded {b!r}" for n, a, b in zip(names, g[1:], w[1:])
                                                        if a != b)
    return f"{len(got)} launches, recorded {len(want)}"


def test_every_mode_launches_what_was_recorded(table, replay):
    assert list(replay["modes"]) == list(table["modes"])
    for mode, want in table["modes"].items():
        got = replay["modes"][mode]
        assert got == want, f"{mode}: {_first_difference(table, got, want)}"


def test_timed_passes_record_what_was_recorded(table, replay):
    """(variant, flops, shape tuple) of every `KernelTimer` record: what bench.py reports."""
    assert list(replay["timed"]) == list(table["timed"])
    for mode, want in table["timed"].items():
        got = replay["timed"][mode]
        diff = [f"record {i}: {g}, recorded {w}" for i, (g, w) in enumerate(zip(got, want)) if g != w][:1]
        assert got == want, f"{mode}: {diff or (len(got), len(want))}"


def test_direct_calls_launch_and_raise_what_was_recorded(table, replay):
    # conv2d_refused asks the REAL launcher, which must never see a descriptor it accepts where there is a device
    skipped = {"conv2d_refused"} if torch.cuda.is_available() else set()
    assert set(table["direct"]) - set(replay["direct"]) == skipped
    for case, want in table["direct"].items():
        if case in skipped:
            continue
        got = replay["direct"][case]
        assert got["error"] == want["error"], case
        assert got["rows"] == want["rows"], f"{case}: {_first_difference(table, got['rows'], want['rows'])}"


def test_table_covers_every_family_and_path(table):
    """The table itself reaches every kernel family of ops.CONV_FAMILIES, both first-generation pre-passes, all three
    `flags` values and a fused shortcut in the f32, f16 and s16 families."""
    from ddnm_amd import ops
    sig = table["entry_points"]
    launched = [r for rows in list(table["modes"].values()) + [c["rows"] for c in table["direct"].values()] for r in rows]

    def field(r, name):
        names = sig[r[0]]
        return r[1 + names.index(name)] if name in names else None

    def rows_of(entry, **fields):
        return [r for r in launched if r[0] == entry and all(field(r, "ConvDesc." + k) == v for k, v in fields.items())]
    is_family = {
        "small_cout": lambda r: True, "s16_subpixel": lambda r: field(r, "ConvDesc.flags") == 2,
        "s16": lambda r: field(r, "ConvDesc.flags") != 2, "s16_gather": lambda r: True, "f16_3x3": lambda r: True,
        "f16_1x1": lambda r: True, "f32": lambda r: True, "conv16": lambda r: field(r, "Conv16Desc.out_nchw_f32") == 0,
        "conv16_out": lambda r: field(r, "Conv16Desc.out_nchw_f32") == 1,
    }
    assert set(is_family) == set(ops.CONV_FAMILIES)
    for name, fam in ops.CONV_FAMILIES.items():
        assert any(r[0] == fam.run and is_family[name](r) for r in launched), f"no launch of family {name}"
    assert {r[0] for r in launched} >= {"ddnm_im2col3x3_f16", "ddnm_gn_apply_f16", "ddnm_conv16"}
    assert rows_of("ddnm_conv1x1_f16_f32", src0="scratch:f16:1") and rows_of("ddnm_conv3x3_f16_f32", src0="scratch:f16:0")
    for flags in (0, 1, 2):
        assert rows_of("ddnm_conv3x3_s16_f32", flags=flags), f"no split-fp16 launch with flags = {flags}"
    for entry in ("ddnm_conv2d_f32", "ddnm_conv3x3_f16_f32", "ddnm_conv3x3_s16_f32"):
        assert any(field(r, "ConvDesc.skip_weight") != 0 for r in rows_of(entry)), f"{entry}: no fused shortcut"


def test_recorder_still_generates_the_recorded_cases(table):
    """The table's direct cases are the ones the committed recorder lists (a recorder edit needs a re-record)."""
    assert [c[0] for c in rec.direct_cases(None)] == list(table["direct"])
    assert all(m.rsplit("_b", 1)[1] in {str(b) for b in rec.BATCHES} for m in table["modes"])
