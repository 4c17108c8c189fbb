"""Images/s of the CLI runner with and without batch fusing (DDNM_FUSE_BATCHES), A/B in one process on one MI355X.

The shipped configurations restore one image per loader batch.  For each workload below the runner
(`Diffusion.svd_based_ddnm_plus`: loader, y = A x, Apy PNGs, sampler, PSNR, PNGs) runs once per setting as warm-up
(code objects, hipGraph capture at B = 1, launch plans of the fused batch), then `--reps` times per setting, alternating
K = 1 and K = fused; each run is timed on the host clock and ends in a device synchronise.  Random weights
(DDNM_RANDOM_WEIGHTS=1) of the shipped architectures, synthetic inputs.

    python tools/fuse_time.py [--reps 2] [--out profiles/fuse_time.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [
    # name, config, images, --deg, --deg_scale, fused K
    ("celeba_sr_bicubic4", "celeba_hq.yml", 16, "sr_bicubic", "4", 8),
    ("adm_colorization", "imagenet_256.yml", 8, "colorization", "0", 4),
]


def _runner(cfg, n, deg, scale, exp):
    import main
    from ddnm_amd.guided_diffusion.diffusion import Diffusion
    args, config = main.parse_args_and_config(["--ni", "--config", cfg, "--exp", exp, "--path_y", f"synthetic:{n}",
                                                "--eta", "0.85", "--deg", deg, "--deg_scale", scale, "--sigma_y", "0.",
                                                "-i", "fuse_time"])
    return Diffusion(args, config)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    import contextlib
    import io
    import torch
    os.environ["DDNM_RANDOM_WEIGHTS"] = "1"
    results = []
    with tempfile.TemporaryDirectory() as exp:
        for name, cfg, n, deg, scale, kf in WORKLOADS:
            first = _runner(cfg, n, deg, scale, exp)
            with contextlib.redirect_stdout(io.StringIO()):
                model = first._build_model()
            model.auto_graphs(int(os.environ.get("DDNM_GRAPH_MAX_BATCH", "2")))     # as Diffusion.sample does
            cls_fn = getattr(first, "_cls_fn", None)
            times = {1: [], kf: []}
            for rep in range(opts.reps + 1):                # rep 0 = warm-up
                for k in (1, kf):
                    os.environ["DDNM_FUSE_BATCHES"] = str(k)
                    runner = _runner(cfg, n, deg, scale, exp)          # fresh args: the runner rescales sigma_y in place
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with contextlib.redirect_stdout(io.StringIO()):
                        runner.svd_based_ddnm_plus(model, cls_fn)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if rep > 0:
                        times[k].append(dt)
            os.environ.pop("DDNM_FUSE_BATCHES", None)
            best = {k: min(v) for k, v in times.items()}
            r = {"workload": name, "config": cfg, "images": n, "deg": deg, "T_sampling": 100, "fused_K": kf,
                 "images_per_s_unfused": n / best[1], "images_per_s_fused": n / best[kf],
                 "speedup": best[1] / best[kf], "runs_s": {str(k): v for k, v in times.items()}}
            results.append(r)
            print(f"{name}: K=1 {r['images_per_s_unfused']:.2f} images/s, K={kf} {r['images_per_s_fused']:.2f} images/s "
                  f"({r['speedup']:.2f}x; best of {opts.reps}, runs {json.dumps(r['runs_s'])})", flush=True)
    line = {"device": torch.cuda.get_device_name(0), "results": results}
    print(json.dumps(line))
    if opts.out:
        with open(opts.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
