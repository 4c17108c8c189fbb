"""The counted `s_waitcnt vmcnt(N)` waits of the sub-pixel upsample convolution (ddnm_amd/csrc/conv_s16_subpixel.hip), checked
against the issue order in the gfx950 ISA on every path of the kernel's control-flow graph (tools/isa_waits.analyse_cfg, as for
the persistent 3x3 kernel in tests/test_isa_waits.py).  CPU only (hipcc cross-compiles)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_waits  # noqa: E402

MID, LAST, FIRST = 0, 1, 2
BR, HR, NOUT = 2, 6, 64


def _first_of(s):
    return (0, 22, 43, NOUT)[s] if s < 4 else NOUT


def _q_extra(kind, s):
    """Python restatement of conv_s16_subpixel.hip::q_extra: requests of step s in front of its weight-tile DMA."""
    n = HR if s == 0 else 0                                          # the next chunk's halo
    if kind == FIRST:
        n += _first_of(s + 1) - _first_of(s) + (1 if s == 0 else 0)  # deferred stores (+ the statistics store)
    if kind == LAST and s == 0:
        n += 3                                                       # 2 bias loads + the next tile's operand bound
    return n


def _q_wait(kind, s):
    """conv_s16_subpixel.hip::q_wait: W(s) is the last request of step s - 2, behind it lies the whole block of step s - 1."""
    return BR + _q_extra(kind, (s - 1) % 4)


@pytest.fixture(scope="module")
def waits(tmp_path_factory):
    asm = isa_waits.compile_isa(os.path.join(isa_waits.CSRC, "conv_s16_subpixel.hip"), str(tmp_path_factory.mktemp("isa") / "q.s"))
    res = isa_waits.analyse_cfg(asm, r"conv2x2x4_s16_subpixel_kernel", depth=2, group_size=BR)
    assert len(res) == 1, list(res)
    (w,) = res.values()
    return w


def test_every_counted_wait_matches_the_issue_order_on_every_path(waits):
    assert len(waits) == 3 * 4, len(waits)                           # 3 chunk kinds x 4 steps, each exactly once in the code
    for n, found, line in waits:
        assert found == [n], f"wait vmcnt({n}) at line {line}: requests behind the awaited tile on the paths = {found}"


def test_the_immediates_are_the_source_table(waits):
    assert all(_q_extra(kind, 3) == 0 for kind in (MID, LAST, FIRST))      # what makes a chunk's table independent of its neighbours
    want = sorted(_q_wait(kind, s) for kind in (MID, LAST, FIRST) for s in range(4))
    assert max(want) < 64
    assert sorted(n for n, _, _ in waits) == want, (sorted(n for n, _, _ in waits), want)
