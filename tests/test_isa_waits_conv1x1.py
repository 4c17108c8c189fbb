"""The counted `s_waitcnt vmcnt(N)` waits of the GEMM-form 1x1 convolution (ddnm_amd/csrc/conv1x1_s16.hip), checked against the
issue order in the gfx950 ISA that hipcc emits (tools/isa_waits.analyse replays the request stream of the main loop, as for the
gather kernel in tests/test_isa_waits.py).  CPU only (hipcc cross-compiles)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_waits  # noqa: E402

KS = 2                                       # conv1x1_s16.hip: G1_KS
AR, BR = 2, 2                                # G1_AR, G1_BR of the 64 x 64 tile


REQ_A, REQ_W = KS * (AR + 2), KS * BR        # requests per wave of one A step (gathers + 2 GroupNorm vectors per sub-row) / W step


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return isa_waits.compile_isa(os.path.join(isa_waits.CSRC, "conv1x1_s16.hip"), str(tmp_path_factory.mktemp("isa") / "g1.s"))


@pytest.fixture(scope="module")
def loop(asm):
    # the main loop holds three steps (one per A register set) of two barriers each; W(s) is the third DMA group back from its
    # wait: W(s+2) and W(s+1) were requested behind it
    res = isa_waits.analyse(asm, r"conv1x1_s16_kernel", min_barriers=6, depth=3)
    assert len(res) == 1, list(res)
    (r,) = res.values()
    return r


def test_every_counted_wait_matches_the_issue_order(loop):
    assert loop["barriers"] == 6 and len(loop["waits"]) == 3, loop
    for n, behind in loop["waits"]:
        # behind W(s): A(s+1) W(s+1) A(s+2) W(s+2) A(s+3)
        assert n == behind == 3 * REQ_A + 2 * REQ_W and n < 64, loop
    assert set(loop["groups"]) == {REQ_W}, loop      # the weight groups are whole steps


def test_the_steps_behind_the_loop_wait_alike_on_every_path(asm):
    """The one or two steps behind the three-step loop issue clamped requests whose data nobody reads; were the compiler to
    delete them, those steps' waits would count requests that were never issued (tools/isa_waits.analyse_cfg walks back from
    every counted wait along every path of the kernel: three in the loop, two behind it)."""
    res = isa_waits.analyse_cfg(asm, r"conv1x1_s16_kernel", depth=3, group_size=REQ_W)
    (waits,) = res.values()
    assert len(waits) == 5, waits
    for n, found, line in waits:
        assert found == [n] and n == 3 * REQ_A + 2 * REQ_W, f"wait vmcnt({n}) at line {line}: requests behind W(s) = {found}"
