"""Stream time of `ddnm_ssim_f32` (tile kernel + per-image sum) on one MI355X, next to its byte floor.

HIP events around host-issued launches at B = 8, 3 x 256 x 256 (random [-1, 1] inputs, transform on): the median of `--reps`
single launches after `--warmup` launches, and the time per call of a back-to-back train of 100.  Both include launch
overhead; device time alone needs a kernel trace.  The byte floor is two image reads plus the workspace written and read.

    python tools/ssim_time.py [--reps 300] [--warmup 50] [--out profiles/ssim_time.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12          # measured float4 copy rate of the MI355X


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--shape", type=int, nargs=4, default=[8, 3, 256, 256], metavar=("B", "C", "H", "W"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from ddnm_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("tools/ssim_time.py needs the MI355X: a time is not measured on the CPU")
    torch.manual_seed(0)
    B, C, H, W = args.shape
    x = torch.rand(B, C, H, W, device="cuda") * 2 - 1
    y = torch.rand(B, C, H, W, device="cuda") * 2 - 1
    lib = _lib.lib()
    n = lib.ddnm_ssim_workspace_elems(B, C, H, W)
    work = torch.empty(n, dtype=torch.float64, device="cuda")
    out = torch.empty(B, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.check(lib.ddnm_ssim_f32(x.data_ptr(), y.data_ptr(), out.data_ptr(), work.data_ptr(), n, B, C, H, W, 1, stream),
                   "ddnm_ssim_f32")

    def timed(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            launch()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k          # us per call

    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    single = sorted(timed(1) for _ in range(args.reps))
    train = sorted(timed(100) for _ in range(5))
    nbytes = 2 * B * C * H * W * 4 + 2 * n * 8 + B * 8
    res = {"shape": [B, C, H, W], "workgroups": n, "reps": args.reps, "warmup": args.warmup,
           "single_launch_us": {"median": statistics.median(single), "min": single[0], "p90": single[int(0.9 * len(single))]},
           "back_to_back_us_per_call": {"median": statistics.median(train), "min": train[0], "max": train[-1]},
           "bytes": nbytes, "byte_floor_us": nbytes / HBM_BYTES_PER_S * 1e6, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
