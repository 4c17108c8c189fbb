#!/usr/bin/env python
"""Per-launch A/B of the 1x1 convolutions of the celeba `Model`: the GEMM form (csrc/conv1x1_s16.hip) against the gather kernel
plus its split-K reduction launch (`one_tile=True` keeps a launch on that route), on the same inputs.

    python tools/conv1x1_ab.py [out.md]

HIP events around 10 launches (enqueued behind ~3 ms of other GPU work, so that the kernels run back to back), median of 7 rounds alternating the two forms; B = 8, 4, 2, 1; operand bound precomputed.
Prints a markdown table (profiles/conv1x1_s16_ab.md) with the rel-L2 distance of the two routes' outputs; the routing rule in
csrc/conv1x1_s16.hip::conv1x1_s16_routes is read off its last column."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddnm_amd import _lib, ops  # noqa: E402

DEV = "cuda"
# layer: C0, C1, Cout, H, GroupNorm affine, residual + statistics
LAYERS = [("qkv @16²", 512, 0, 1536, 16, True, False),
          ("proj_out @16²", 512, 0, 512, 16, False, True),
          ("qkv @8²", 512, 0, 1536, 8, True, False),
          ("proj_out @8²", 512, 0, 512, 8, False, True),
          ("nin_shortcut @8²", 512, 512, 512, 8, False, False)]
# below the network's shapes: the ones tests/test_gpu_s16_conv1x1.py runs (ragged K, concat, 64 ... 192 output channels), B = 2
SMALL = [("qkv form @8²", 96, 0, 192, 8, True, False),
         ("proj_out form @16²", 64, 0, 64, 16, False, True),
         ("proj_out form @8²", 64, 0, 64, 8, False, True),
         ("shortcut form @16²", 96, 32, 64, 16, False, False)]
LAUNCHES, ROUNDS = 10, 7
BAR = 0.8                                   # routing bar: GEMM form at most this fraction of the gather route


def force_gemm_form():
    """Every gather-family launch of this process carries DDNM_CONV_GEMM1X1 (include/ddnm_hip.h): the GEMM form wherever the
    kernel has one, whatever the routing rule says.  ops.conv2d does not expose the bit (DDNM_CONV_ONE_TILE still wins)."""
    L = _lib.lib()
    run = L.ddnm_conv_gather_s16_f32

    def forced(dref, stream):
        dref._obj.flags |= 4
        return run(dref, stream)
    L.ddnm_conv_gather_s16_f32 = forced


def main(out=None):
    force_gemm_form()
    g = torch.Generator(device=DEV).manual_seed(5)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    busy = torch.ones(1 << 28, device=DEV)
    lines = ["| B | layer | workgroups | gather route us [min..max] | GEMM form us [min..max] | ratio | rel-L2 | meets the bar |",
             "|---:|---|---:|---:|---:|---:|---:|---|"]
    for B, layers in ((8, LAYERS), (4, LAYERS), (2, LAYERS), (1, LAYERS), (2, SMALL)):
        for name, C0, C1, Cout, H, gn, res in layers:
            cin = C0 + C1
            a, b = rn(B, H, H, C0), (rn(B, H, H, C1) if C1 else None)
            w = rn(Cout, cin, 1, 1) / cin ** 0.5
            s = ops.s16_weight_scale(w)
            w32, s16, bias = ops.pack_conv_weight(w), (ops.pack_conv_weight_s16(w, s), s, None), rn(Cout)
            gnp = (rn(B, cin) * 0.3 + 1.0, rn(B, cin) * 0.3) if gn else None
            r = rn(B, H, H, Cout) if res else None
            amax = None if gn else ops.amax_bound(a, b)
            o = torch.empty(B, H, H, Cout, device=DEV)

            def launch(one_tile):
                return ops.conv2d(a, w32, Cout, 1, src1=b, bias=bias, res=r, gn=gnp, gn_silu=False, emit_stats=res,
                                  weight_s16=s16, raw_amax=amax, one_tile=one_tile, out=o)

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
                launch(ot)
                outs[ot] = o.clone().double()
                timed(ot)                                      # warm-up
            t = {True: [], False: []}
            for _ in range(ROUNDS):
                for ot in (True, False):
                    t[ot].append(timed(ot))
            old, new = statistics.median(t[True]), statistics.median(t[False])
            rel = ((outs[False] - outs[True]).norm() / outs[True].norm()).item()
            lines.append(f"| {B} | {name}, {cin} -> {Cout} | {B * H * H // 64 * (Cout // 64)} | {old:.1f} [{min(t[True]):.1f}..{max(t[True]):.1f}] | "
                         f"{new:.1f} [{min(t[False]):.1f}..{max(t[False]):.1f}] | {new / old:.3f} | {rel:.1e} | "
                         f"{'yes' if new <= BAR * old else 'no'} |")
    text = "\n".join(lines) + "\n"
    if out:
        open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
