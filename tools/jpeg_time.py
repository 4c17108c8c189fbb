"""Stream times of the JPEG step on one MI355X: the fused `ddnm_step_jpeg_f32` against the same step
composed from the `ddnm_op_jpeg_T_f32` / `_pinv_f32` entry points, the generic step kernels and elementwise torch ops, and
the three operator launches with their `torch.empty`.

B = 8, 3 x 256 x 256, Q = 50, in-kernel Philox noise, x0 written.  By the method of DESIGN.md 1.10 / 1.11: HIP events on the
launch stream, `--reps` launches after `--warmup` warm-up ones; the minimum and median of an event pair around ONE
host-issued launch, then the mean of `--reps` back-to-back launches.  Both include launch overhead; device-only kernel
time is not measured here.  The byte floor counts xt, et, x0 and xt_next once each and y once.

    python tools/jpeg_time.py [--sites 2x2,2x1,1x1] [--out profiles/jpeg_time.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12          # measured float4 copy rate of the MI355X
B, D, QUALITY, BOX, ETA = 8, 256, 50, 0.98, 0.85


def measure(fn, reps, warmup):
    import torch

    def timed(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k          # us per call

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    single = sorted(timed(1) for _ in range(reps))
    return {"single_launch_us": {"min": single[0], "median": statistics.median(single)}, "back_to_back_mean_us": timed(reps)}


def site_times(rw, rh, reps, warmup):
    import torch
    from ddnm_amd import ops
    from ddnm_amd.functions import svd_operators as E
    op = E.JPEG(3, D, QUALITY, rw, rh, "cuda", box=BOX)
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(B, 3, D, D, generator=g) * 2 - 1).cuda()
    et6 = torch.randn(B, 6, D, D, generator=g).cuda()
    et = et6[:, :3]
    xt = ((x + 0.1 * torch.randn(B, 3, D, D, generator=g).cuda()) * 0.45 ** 0.5 + et * 0.55 ** 0.5).contiguous()
    y = op.A(x)
    s = ops.PhiloxNoise(1234).stamp(ops.step_scalars(torch.tensor(0.45), torch.tensor(0.6), ETA), 3)
    x0, out, x0c, outc = (torch.empty_like(xt) for _ in range(4))
    h = (op._q_row * (BOX / 2)).float().to("cuda")

    def fused():
        op.ddnm_step(xt, et, None, y, s, x0, out)

    def composed():
        ops.step_x0(xt, et, s, out=x0c)
        c = op.A_linear(x0c)
        proj = op.A_pinv(c - torch.minimum(torch.maximum(c, y - h), y + h)).reshape(xt.shape)
        ops.step_combine(x0c, proj, None, None, et, s, out=outc)

    fused()
    composed()
    torch.cuda.synchronize()
    agree = float(((out - outc).double().norm() / outc.double().norm()).item())
    res = {"fused_step": measure(fused, reps, warmup), "composed_step": measure(composed, reps, warmup),
           "op_T": measure(lambda: op.A_linear(x), reps, warmup), "op_A": measure(lambda: op.A(x), reps, warmup),
           "op_pinv": measure(lambda: op.A_pinv(y), reps, warmup)}
    nbytes = 4 * xt.numel() * 4 + y.numel() * 4
    res.update(fused_vs_composed_rel_l2=agree, workgroups=op.workgroups(B), bytes=nbytes, byte_floor_us=nbytes / HBM_BYTES_PER_S * 1e6)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sites", default="2x2")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/jpeg_time.py needs the MI355X: a time is not measured on the CPU")
    res = {"device": torch.cuda.get_device_name(0), "shape": {"B": B, "d": D, "quality": QUALITY, "box": BOX},
           "reps": opts.reps, "warmup": opts.warmup}
    for site in opts.sites.split(","):
        rw, rh = (int(v) for v in site.split("x"))
        res[site] = site_times(rw, rh, opts.reps, opts.warmup)
        print(json.dumps({site: res[site]}), flush=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
