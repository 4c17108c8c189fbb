"""The degradation operators launch what they launched when tests/golden/operator_trace.json.gz was recorded
(tools/record_operator_trace.py): per case -- one method of one operator of ddnm_amd/functions/svd_operators.py, at image
size 64 -- the ordered list of launching library calls (entry point, every scalar argument bit for bit, every descriptor
field, a label per pointer that tells the caller's tensors, the returned one and the operator's own tables apart), the
exception's type and message where the call raises, and the shape and dtype of what it returns.  No GPU needed: the
launching entry points are stubs (tools/dry_run.py) and the tensors live on the CPU.  The recorder runs in a process of its
own (it replaces the library object, torch.svd and several module attributes).  What the table cannot see is which
scratch buffer feeds which launch: the GPU tests of the operators hold that.  A refactor of the operator layer must leave
this file and the table alone."""
import gzip
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(path):
    with (gzip.open if str(path).endswith(".gz") else open)(path, "rt") as f:
        t = json.load(f)
    for c in t["cases"].values():          # a case as its rows themselves (the file stores distinct rows once)
        c["rows"] = [t["rows"][i] for i in c["rows"]]
    return t


@pytest.fixture(scope="module")
def table():
    return _load(os.path.join(ROOT, "tests", "golden", "operator_trace.json.gz"))


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    from ddnm_amd import build
    build.build()
    out = tmp_path_factory.mktemp("operator_trace") / "replay.json"
    with open(out, "w") as f:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "record_operator_trace.py"), "--replay"], stdout=f,
                           stderr=subprocess.PIPE, text=True, cwd=ROOT)
    assert r.returncode == 0, "the recorder stopped (an exception no case expects):\n" + r.stderr[-3000:]
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


def test_recorder_still_generates_the_recorded_cases(table, replay):
    """The committed recorder lists the table's cases, in the table's order (a recorder edit needs a re-record)."""
    assert list(replay["cases"]) == list(table["cases"])


def test_every_case_launches_raises_and_returns_what_was_recorded(table, replay):
    wrong = []
    for case, want in table["cases"].items():
        got = replay["cases"].get(case)
        if got is None:
            wrong.append(f"{case}: not replayed")
        elif got["error"] != want["error"]:
            wrong.append(f"{case}: raised {got['error']}, recorded {want['error']}")
        elif got["rows"] != want["rows"]:
            wrong.append(f"{case}: {_first_difference(table, got['rows'], want['rows'])}")
        elif got["returned"] != want["returned"]:
            wrong.append(f"{case}: returned {got['returned']}, recorded {want['returned']}")
    assert not wrong, f"{len(wrong)} of {len(table['cases'])} cases differ:\n" + "\n".join(wrong[:20])


def test_table_covers_the_operator_layer(table):
    """The table itself reaches every operator entry point the module names, keyed and unkeyed fused steps, both GEMM
    operand orders, the fused `D` epilogue, the `ldc` write into wider planes, and every outcome of the coefficient rule."""
    cases = table["cases"]
    launched = {r[0] for c in cases.values() for r in c["rows"]}
    for step in ("denoise", "sr_avgpool", "color", "inpaint", "inpaint_pi", "combine", "plus_spectral", "plus_cs_pre"):
        assert {f"ddnm_step_{step}_f32", f"ddnm_step_{step}_keyed_f32"} <= launched, step
    assert launched >= {"ddnm_axpby_f32", "ddnm_mask_mix_f32", "ddnm_site_spectral_f32", "ddnm_gather_scale_f32",
                        "ddnm_site_matmul_f32", "ddnm_op_avgpool_f32", "ddnm_op_upsample_f32", "ddnm_op_color_A_f32",
                        "ddnm_op_color_pinv_f32", "ddnm_op_inpaint_A_f32", "ddnm_op_inpaint_pinv_f32",
                        "ddnm_op_inpaint_A_pi_f32", "ddnm_op_inpaint_pinv_pi_f32", "ddnm_fwht2d_f32", "ddnm_fwht2d_masked_f32",
                        "ddnm_wh_gather_f32", "ddnm_wh_scatter_f32", "ddnm_patchify_f32", "ddnm_mul_planes_f32",
                        "ddnm_spectral_mix_f32", "ddnm_step_plus_cs_post_f32", "ddnm_fill_f32", "ddnm_step_x0_f32"}
    sig = table["entry_points"]["ddnm_bgemm_f32"]
    gemms = [dict(zip(sig, r[1:])) for c in cases.values() for r in c["rows"] if r[0] == "ddnm_bgemm_f32"]
    assert {g["GemmDesc.transb"] for g in gemms} == {0, 1}
    assert any(g["GemmDesc.D"] != 0 and g["GemmDesc.beta"] != 0 for g in gemms)
    assert any(g["GemmDesc.ldc"] > g["GemmDesc.N"] for g in gemms)
    assert any(g["GemmDesc.inner"] > 1 for g in gemms)                      # et read through its strides
    assert any(g["GemmDesc.M"] == 64 * 3 * 2 and g["GemmDesc.K"] == 64 for g in gemms)     # _site_matmul, 64 entries per site
    # Lambda_noise at the three coefficient points: (d1, 0) below and above the threshold with different d1, (d1, d2) at 0
    sig = table["entry_points"]["ddnm_mask_mix_f32"]
    mix = {p: dict(zip(sig, cases[f"inpainting.Lambda_noise_{p}"]["rows"][0][1:])) for p in ("below", "above", "sigma_y_0")}
    assert mix["below"]["arg9"] == 0 and mix["above"]["arg9"] == 0 and mix["sigma_y_0"]["arg9"] != 0
    assert mix["below"]["arg7"] != mix["above"]["arg7"]
    errors = {c["error"][1] for c in cases.values() if c["error"]}
    assert {"ddnm_plus_step needs begin_plus_run(y) for this batch first", "et must be channel-contiguous NCHW",
            "per-image mask banks need the SVD path", "img_dim must be a multiple of 32"} <= errors
