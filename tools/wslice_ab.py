#!/usr/bin/env python
"""Per-launch A/B of the 3x3 convolutions of the 8 x 8 level of the celeba `Model`: the slices-on-waves form
(csrc/conv_s16_wslice.hip) against the gather kernel plus its split-K reduction launch (`one_tile=True` keeps a launch on that
route), on the same inputs.

    python tools/wslice_ab.py [out.md]

HIP events around 10 launches (enqueued behind ~3 ms of other GPU work, so that the kernels run back to back), median of 7 rounds
alternating the two forms; B = 8, 4, 2, 1; GroupNorm + swish prologue, residual, statistics (a ResBlock's conv2).
Prints a markdown table (profiles/wslice_ab.md).  A row whose `routed` column says 0 runs the gather route both times (the plan
has more slices than the workgroup has waves): its two columns measure the same kernels.  A shape wins when the [min..max] ranges
of its 7 rounds do not overlap."""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddnm_amd import _lib, ops  # noqa: E402

DEV = "cuda"
# layer: C0, C1, Cout, H
LAYERS = [("3x3 @8², 512 -> 512", 512, 0, 512, 8),
          ("3x3 @8², 512 + 512 -> 512", 512, 512, 512, 8)]
# below the network's shapes: the ones tests/test_gpu_s16_wslice.py runs
SMALL = [("3x3 @8², 256 -> 64", 256, 0, 64, 8),
         ("3x3 @8², 64 + 32 -> 64", 64, 32, 64, 8)]
LAUNCHES, ROUNDS = 10, 7


def routed(B, C0, C1, Cout, H):
    d = _lib.ConvDesc()
    d.B, d.Hin, d.Win, d.C0, d.C1, d.Cout = B, H, H, C0, C1, Cout
    d.ksize, d.stride, d.pad, d.Ho, d.Wo = 3, 1, 1, H, H
    d.stats_out = 16
    return _lib.lib().ddnm_conv_gather_s16_wslice(ctypes.byref(d))


def main(out=None):
    g = torch.Generator(device=DEV).manual_seed(5)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    busy = torch.ones(1 << 28, device=DEV)
    lines = ["| B | layer | routed | gather route us [min..max] | slices on waves us [min..max] | ratio | bit-equal | ranges apart |",
             "|---:|---|---:|---:|---:|---:|---|---|"]
    for B, layers in ((8, LAYERS), (4, LAYERS), (2, LAYERS), (1, LAYERS), (2, SMALL)):
        for name, C0, C1, Cout, H in layers:
            cin = C0 + C1
            a, b = rn(B, H, H, C0), (rn(B, H, H, C1) if C1 else None)
            w = rn(Cout, cin, 3, 3) / (3 * cin ** 0.5)
            s = ops.s16_weight_scale(w)
            w32, s16, bias = ops.pack_conv_weight(w), (ops.pack_conv_weight_s16(w, s), s, None), rn(Cout)
            gnp = (rn(B, cin) * 0.3 + 1.0, rn(B, cin) * 0.3)
            r = rn(B, H, H, Cout)
            o = torch.empty(B, H, H, Cout, device=DEV)

            def launch(one_tile):
                return ops.conv2d(a, w32, Cout, 3, src1=b, bias=bias, res=r, gn=gnp, gn_silu=True, emit_stats=True,
                                  weight_s16=s16, one_tile=one_tile, out=o)

            def timed(one_tile):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(6):                             # ~3 ms of GPU work: the host enqueues the launches behind it,
                    busy.mul_(1.0)                             # so the events time the kernels, not the Python call rate
                e0.record()
                for _ in range(LAUNCHES):
                    launch(one_tile)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3 / LAUNCHES

            outs = {}
            for ot in (True, False):
                act = launch(ot)
                outs[ot] = (o.clone(), act.stats.clone())
                timed(ot)                                      # warm-up
            t = {True: [], False: []}
            for _ in range(ROUNDS):
                for ot in (True, False):
                    t[ot].append(timed(ot))
            old, new = statistics.median(t[True]), statistics.median(t[False])
            equal = torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])
            lines.append(f"| {B} | {name} | {routed(B, C0, C1, Cout, H)} | {old:.1f} [{min(t[True]):.1f}..{max(t[True]):.1f}] | "
                         f"{new:.1f} [{min(t[False]):.1f}..{max(t[False]):.1f}] | {new / old:.3f} | {'yes' if equal else 'NO'} | "
                         f"{'yes' if max(t[False]) < min(t[True]) else 'no'} |")
    text = "\n".join(lines) + "\n"
    if out:
        open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
