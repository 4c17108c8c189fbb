"""Restorations/s of the CLI runner drawing K samples per measurement in one engine batch (DDNM_SAMPLES=K) against K
plain runs with K seeds, A/B in one process on one MI355X -- and the stream time of the statistics kernel behind it.

Runner: `celeba_hq.yml`, sr_bicubic 4x, T = 100, loader batches of one image, two synthetic images, random weights.
Setting A is ONE run with DDNM_SAMPLES=8; setting B is eight plain runs of the same two images under the noise seeds
seed ... seed + 7, which is what a user does without the switch (minus seven process starts and model loads, which are
not timed here: the model is built once and shared).  Both restore 16 images.  One warm-up of each setting (code
objects, hipGraph capture at B = 1, launch plans at B = 8), then `--reps` times each, alternating; every run is the whole
runner (`Diffusion.svd_based_ddnm_plus`: loader, y = A x, Apy PNGs, sampler, PSNR, statistics, PNGs) timed on the host
clock and ended by a device synchronise.

Kernel: `ddnm_sample_stats_f32` at B = K = 8, 3 x 256 x 256, as tools/ssim_time.py times the SSIM: HIP events around
host-issued launches, the median of `--kernel-reps` single launches and the time per call of back-to-back trains of
100; both include launch overhead.  The byte floor is K reads, one read of the original and two writes per element.

    python tools/samples_time.py [--reps 2] [--out profiles/samples_time.json]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12          # measured float4 copy rate of the MI355X
K, IMAGES, SEED = 8, 2, 1234


def _runner(seed, exp):
    """A runner under noise seed `seed` whose loader keeps the images and their order of the base seed."""
    import main
    from ddnm_amd.guided_diffusion.diffusion import Diffusion
    args, config = main.parse_args_and_config(["--ni", "--config", "celeba_hq.yml", "--exp", exp, "--path_y",
                                                f"synthetic:{IMAGES}", "--eta", "0.85", "--deg", "sr_bicubic",
                                                "--deg_scale", "4", "--sigma_y", "0.", "-i", "samples_time", "--seed",
                                                str(seed)])
    runner = Diffusion(args, config)
    loader = runner._loader

    def pinned():
        keep, runner.args.seed = runner.args.seed, SEED
        try:
            return loader()
        finally:
            runner.args.seed = keep

    runner._loader = pinned
    return runner


def time_runner(reps):
    import torch
    os.environ["DDNM_RANDOM_WEIGHTS"] = "1"
    times = {"samples": [], "plain": []}
    with tempfile.TemporaryDirectory() as exp:
        first = _runner(SEED, exp)
        with contextlib.redirect_stdout(io.StringIO()):
            model = first._build_model()
        model.auto_graphs(int(os.environ.get("DDNM_GRAPH_MAX_BATCH", "2")))     # as Diffusion.sample does

        def timed(seeds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for seed in seeds:
                runner = _runner(seed, exp)            # fresh args: the runner rescales sigma_y in place
                with contextlib.redirect_stdout(io.StringIO()):
                    runner.svd_based_ddnm_plus(model, None)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        for rep in range(reps + 1):                    # rep 0 = warm-up
            for setting in ("samples", "plain"):
                if setting == "samples":
                    os.environ["DDNM_SAMPLES"] = str(K)
                    dt = timed([SEED])
                else:
                    os.environ.pop("DDNM_SAMPLES", None)
                    dt = timed(range(SEED, SEED + K))
                if rep > 0:
                    times[setting].append(dt)
        os.environ.pop("DDNM_SAMPLES", None)
    best = {k: min(v) for k, v in times.items()}
    n = K * IMAGES
    return {"config": "celeba_hq.yml", "deg": "sr_bicubic 4x", "T_sampling": 100, "loader_batch": 1, "images": IMAGES,
            "samples_per_image": K, "restorations": n, "restorations_per_s_one_run_of_K_samples": n / best["samples"],
            "restorations_per_s_K_plain_runs": n / best["plain"], "speedup": best["plain"] / best["samples"], "runs_s": times}


def time_kernel(reps, warmup):
    import torch
    from ddnm_amd import _lib
    B, chw = 8, 3 * 256 * 256
    torch.manual_seed(0)
    x = torch.randn(K * B, chw, device="cuda") * 0.8
    xo = torch.rand(B, chw, device="cuda") * 2 - 1
    lib = _lib.lib()
    n = lib.ddnm_sample_stats_workspace_elems(B, chw)
    work = torch.empty(n, dtype=torch.float64, device="cuda")
    mean, std = torch.empty(B, chw, device="cuda"), torch.empty(B, chw, device="cuda")
    sse, std_mean = (torch.empty(B, dtype=torch.float64, device="cuda") for _ in range(2))
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for layout, (si, ss) in (("samples_major", (chw, B * chw)), ("images_major", (K * chw, chw))):
        def launch():
            _lib.check(lib.ddnm_sample_stats_f32(x.data_ptr(), si, ss, xo.data_ptr(), mean.data_ptr(), std.data_ptr(),
                                                 sse.data_ptr(), std_mean.data_ptr(), work.data_ptr(), n, B, K, chw, stream),
                       "ddnm_sample_stats_f32")

        def timed(k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                launch()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / k          # us per call

        for _ in range(warmup):
            launch()
        torch.cuda.synchronize()
        single = sorted(timed(1) for _ in range(reps))
        train = sorted(timed(100) for _ in range(5))
        out[layout] = {"single_launch_us": {"median": statistics.median(single), "min": single[0],
                                            "p90": single[int(0.9 * len(single))]},
                       "back_to_back_us_per_call": {"median": statistics.median(train), "min": train[0], "max": train[-1]}}
    nbytes = (K + 1 + 2) * B * chw * 4 + 2 * n * 8 + 2 * B * 8
    return {"shape": {"B": B, "K": K, "chw": chw}, "workgroups": n // 2, "reps": reps, "warmup": warmup, "bytes": nbytes,
            "byte_floor_us": nbytes / HBM_BYTES_PER_S * 1e6, **out}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=300)
    ap.add_argument("--kernel-warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/samples_time.py needs the MI355X: a time is not measured on the CPU")
    kernel = time_kernel(opts.kernel_reps, opts.kernel_warmup)
    print(json.dumps({"stats_kernel": kernel}), flush=True)
    runner = time_runner(opts.reps)
    res = {"device": torch.cuda.get_device_name(0), "runner": runner, "stats_kernel": kernel}
    print(json.dumps(res))
    if opts.out:
        with open(opts.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
