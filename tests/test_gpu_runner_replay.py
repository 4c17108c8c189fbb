"""The CLI runner against a recorded replay of itself (tests/golden/runner_runs.json, written by
tools/record_runner_runs.py at the commit before the runner's three tails -- plain, fused, K-sample -- became one
sampler-call path).  The other runner tests compare the modes with each other, so a change that moves all modes together
passes them; this one pins every mode to what it wrote before: the model's batch sizes per call, the PSNR / SSIM /
K-sample lines and totals string for string, and every PNG by the SHA-256 of its pixels.  The same tensors go to the same
kernels, so equality is exact; both runs reproduce the table bit for bit on the MI355X."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_runner_runs as rec  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, "tests", "golden", "runner_runs.json")) as f:
    TABLE = json.load(f)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("replay"))
    rec.prepare_root(root)
    return root


def test_table_holds_the_cases_of_the_recorder():
    assert list(TABLE) == [c["name"] for c in rec.CASES]
    for case in rec.CASES:
        assert TABLE[case["name"]]["argv"] == case["argv"] and TABLE[case["name"]]["env"] == case["env"], case["name"]


@pytest.mark.parametrize("case", rec.CASES, ids=[c["name"] for c in rec.CASES])
def test_runner_replays_the_recorded_run(hip, workdir, case):
    want = TABLE[case["name"]]
    got = rec.run_case(case, workdir)
    assert got["calls"] == want["calls"]
    assert got["lines"] == want["lines"]
    assert sorted(got["png"]) == sorted(want["png"])
    assert [n for n in want["png"] if got["png"][n] != want["png"][n]] == []
