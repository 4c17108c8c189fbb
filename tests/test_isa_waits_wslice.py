"""The request pipeline of the slices-on-waves 3x3 convolution (ddnm_amd/csrc/conv_s16_wslice.hip) in the gfx950 ISA that hipcc
emits.  Every request of that kernel has a register destination, so the `s_waitcnt vmcnt(N)` are the compiler's own and cannot
be wrong; what nothing else pins is that they stay COUNTED: the weight rows of a step are requested two steps ahead only because
scheduling fences keep the requests where the source puts them, and a compiler that moved them, or drained the queue in front of
a step (`vmcnt(0)`), would leave a correct kernel with every memory latency exposed.  Also pinned: the budgets the kernel is
built on -- no scratch, registers within the 256 of a 512-thread workgroup's wave, LDS within one CU's.
CPU only (hipcc cross-compiles)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_waits  # noqa: E402

TAPS, MFMA_PER_TAP, BR = 9, 12, 4            # 2 x 1 MFMA tiles x 2 k-steps x 3 products; WS_BR requests of 8 rows per weight tile
AHEAD = 2                                    # WS_NB - 1: steps a weight request runs ahead of its products


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return isa_waits.compile_isa(os.path.join(isa_waits.CSRC, "conv_s16_wslice.hip"), str(tmp_path_factory.mktemp("isa") / "ws.s"))


@pytest.fixture(scope="module")
def body(asm):
    ks = {n: b for n, b in isa_waits.kernels(asm).items() if "conv_s16_wslice_kernel" in n}
    assert len(ks) == 1, list(ks)
    (b,) = ks.values()
    return b


def _taps(body):
    """The instruction lines of the nine taps of a chunk: from the first MFMA of the kernel to its last (all of them sit in the
    unrolled tap sequence), cut into taps behind every twelfth MFMA."""
    idx = [i for i, line in enumerate(body) if line.startswith("\tv_mfma_f32_32x32x16_f16")]
    assert len(idx) == TAPS * MFMA_PER_TAP, len(idx)
    taps, start = [], idx[0]
    for t in range(TAPS):
        end = idx[(t + 1) * MFMA_PER_TAP - 1] + 1
        taps.append(body[start:end])
        start = end
    return taps


def test_no_tap_drains_the_request_queue(body):
    for t, lines in enumerate(_taps(body)):
        waits = [int(m.group(1)) for line in lines for m in [re.search(r"s_waitcnt.*vmcnt\((\d+)\)", line)] if m]
        assert 0 not in waits, (t, waits)
        if t == 0:
            continue                         # (its requests and waits sit in front of the first MFMA, outside the cut)
        # the tap requests the weight rows of tap + 2, then waits for its own: the requests of tap + 1 and tap + 2 stay in flight
        loads = [i for i, line in enumerate(lines) if line.startswith("\tbuffer_load_dwordx4")]
        assert len(loads) == BR, (t, len(loads))
        assert all(w >= AHEAD * BR for w in waits), (t, waits)
        if t >= 2:                           # (tap 0 waits behind a branch, for the tile of tap 1 too: tap 1 has nothing to wait for)
            assert waits and min(waits) == AHEAD * BR, (t, waits)


def test_budgets(asm):
    seg = asm[asm.index("conv_s16_wslice_kernel"):]
    vgpr = int(re.search(r"; TotalNumVgprs: (\d+)", seg).group(1))
    scratch = int(re.search(r"; ScratchSize: (\d+)", seg).group(1))
    lds = int(re.search(r"; LDSByteSize: (\d+)", seg).group(1))
    assert scratch == 0
    assert vgpr <= 256, vgpr                 # 8 waves per workgroup = 2 per SIMD of 512 registers
    assert lds == 8 * (100 * 144 + 4096) and lds <= 160 * 1024, lds      # 8 halos | 8 weight tiles (the slabs lie over them)
