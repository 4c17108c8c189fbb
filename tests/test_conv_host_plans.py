"""The C++ host layer answers what it answered when tests/golden/conv_host_plans.json was recorded
(tools/record_conv_plans.py): plans of the four convolution families over every descriptor of the eight engine modes
and an edge grid, and the refusal codes of the convolution launchers and the 16 sampler-step entry points.  Host code
only: no GPU needed.  A refactor of csrc's host side must leave this file and the table alone."""
import ctypes
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_conv_plans as rec  # noqa: E402

# an accepted descriptor would LAUNCH on its dummy pointers where there is a device: the refusal half runs without one
no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="refusal codes are replayed on dummy pointers: host-only machines")


@pytest.fixture(scope="module")
def lib():
    from ddnm_amd import _lib, build
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(ROOT, "tests", "golden", "conv_host_plans.json")) as f:
        t = json.load(f)
    assert t["fields"] == rec.FIELDS + ["pointer_mask", "answer"] and t["pointers"] == rec.POINTERS
    assert t["queries"] == rec.QUERIES and t["launchers"] == rec.LAUNCHERS
    assert len(t["conv_rows"]) > 1400 and len(t["step_rows"]) > 400
    # a row = the descriptor key + the index of its answers [queries, launcher codes, codes with stats_out and no workspace]
    t["conv_rows"] = [[r[:-1]] + t["answers"][r[-1]] for r in t["conv_rows"]]
    return t


def _show(t, key):
    return ", ".join(f"{n}={v}" for n, v in zip(t["fields"], key) if v)


def test_planning_queries_match_the_recorded_table(lib, table):
    bad = []
    for i, (key, want, _, _) in enumerate(table["conv_rows"]):
        d = rec.desc_of(key)
        for name, w in zip(table["queries"], want):
            got = int(getattr(lib, name)(ctypes.byref(d)))
            if got != w:
                bad.append(f"row {i} ({_show(table, key)}): {name} = {got}, recorded {w}")
    assert not bad, f"{len(bad)} answers differ:\n" + "\n".join(bad[:20])


@no_device
def test_conv_launchers_refuse_with_the_recorded_codes(lib, table):
    bad, n = [], 0
    for i, (key, _, as_is, no_scratch) in enumerate(table["conv_rows"]):
        for variant, want in (("as recorded", as_is), ("stats_out set, no workspace", no_scratch)):
            d = rec.desc_of(key)
            if variant != "as recorded":
                d.stats_out, d.workspace, d.workspace_floats = rec.DUMMY, None, 0
            for name, w in zip(table["launchers"], want):
                if w == 0:
                    continue                    # the recorded commit accepts this row: never launched
                n += 1
                got = getattr(lib, name)(ctypes.byref(d), None)
                if got != w:
                    bad.append(f"row {i} ({_show(table, key)}; {variant}): {name} = {got}, recorded {w}")
    assert n > 5000
    assert not bad, f"{len(bad)} refusal codes differ:\n" + "\n".join(bad[:20])


@no_device
def test_step_entry_points_refuse_with_the_recorded_codes(lib, table):
    assert {fn for fn, _, _ in table["step_rows"]} == {f"ddnm_step_{b}{k}_f32" for b in rec.STEP_ARGS for k in ("", "_keyed")}
    bad = []
    for fn, mut, want in table["step_rows"]:
        if want == 0:
            continue
        got = rec.step_call(lib, fn, mut)
        if got != want:
            bad.append(f"{fn} with {mut}: {got}, recorded {want}")
    assert not bad, f"{len(bad)} refusal codes differ:\n" + "\n".join(bad[:20])


def test_recorder_still_generates_the_recorded_cases(table):
    """The table's step cases and edge rows are the ones the committed recorder lists (a recorder edit needs a re-record)."""
    assert [[fn, mut] for fn, mut in rec.step_cases()] == [[fn, mut] for fn, mut, _ in table["step_rows"]]
    seen = {}
    rec.edge_descs(seen)
    assert [list(k) for k in seen] == [r[0] for r in table["conv_rows"][:len(seen)]]
