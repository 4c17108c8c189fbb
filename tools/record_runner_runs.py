#!/usr/bin/env python
"""Records what the CLI runner prints and writes, for tests/test_gpu_runner_replay.py (development tool, needs the
MI355X).  Usage, on a checkout of the commit whose behaviour is to be pinned:

    python tools/record_runner_runs.py > tests/golden/runner_runs.json

Every case of CASES is one `main.main([...])` run of the mini configuration of the runner tests (`configs/celeba_hq.yml`
with image_size 64, ch_mult [1, 1, 2], T_sampling 4; synthetic images, DDNM_RANDOM_WEIGHTS=1, --seed 1234) in a scratch
directory.  Per case the table holds the argv and the environment switches, the model's batch sizes per call (repeats
dropped), the stdout lines that start with one of HEADS, and the PNG paths with a SHA-256 of their decoded pixels.  The
two-rank case runs as one `torch.distributed.run` child (gloo, both ranks on this GPU): stdout and PNGs only.

Run it twice and diff the outputs before committing a table: a case that does not reproduce cannot be pinned exactly.
"""
import contextlib
import hashlib
import io
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWITCHES = ("DDNM_FUSE_BATCHES", "DDNM_SAMPLES", "DDNM_NOISE", "DDNM_METRICS", "DDNM_SAVE_Y")       # unset unless the case sets them
HEADS = ("PSNR:", "SSIM:", "Mean-of-K", "Sample PSNR:", "Std:", "Total Average", "Number of samples:",
         "Samples per image:")
SEED = 1234
SR = ["--deg", "sr_averagepooling", "--deg_scale", "4", "--sigma_y", "0."]
INP = ["--deg", "inpainting", "--sigma_y", "0."]


def _case(name, batch, n, deg, env=None, bank=False, ranks=1):
    argv = ["--ni", "--config", f"mini_b{batch}.yml", "--seed", str(SEED), "--path_y", f"synthetic:{n}", "--eta", "0.85"]
    return dict(name=name, argv=argv + deg + ["-i", name], env=dict(env or {}), bank=bank, ranks=ranks)


CASES = [
    _case("plain", 1, 3, SR),
    _case("ragged", 2, 3, SR),
    _case("fused", 1, 6, SR, {"DDNM_FUSE_BATCHES": "4"}),
    _case("samples", 1, 3, SR, {"DDNM_SAMPLES": "3"}),
    _case("samples_fused_ragged", 2, 5, SR, {"DDNM_SAMPLES": "2", "DDNM_FUSE_BATCHES": "2"}),
    _case("plain_torch", 1, 3, SR, {"DDNM_NOISE": "torch"}),
    _case("fused_torch", 1, 6, SR, {"DDNM_FUSE_BATCHES": "4", "DDNM_NOISE": "torch"}),
    _case("samples_torch", 1, 3, SR, {"DDNM_SAMPLES": "3", "DDNM_NOISE": "torch"}),
    _case("bank", 2, 4, INP, bank=True),
    _case("bank_fused_samples", 2, 4, INP, {"DDNM_FUSE_BATCHES": "2", "DDNM_SAMPLES": "2"}, bank=True),
    _case("plus_samples_fused", 1, 3, ["--deg", "sr_bicubic", "--deg_scale", "4", "--sigma_y", "0.05", "--add_noise"],
          {"DDNM_SAMPLES": "2", "DDNM_FUSE_BATCHES": "2"}),
    _case("samples_ssim", 1, 3, SR, {"DDNM_SAMPLES": "3", "DDNM_METRICS": "ssim"}),
    _case("two_ranks_split_bank_samples", 2, 3, INP, {"DDNM_SAMPLES": "2"}, bank=True, ranks=2),
]


def prepare_root(root):
    """The scratch directory of the runs: configs/mini_b{1,2}.yml and the three-mask bank of the mask tests."""
    import numpy as np
    import yaml
    from tests.test_inpaint_masks_host import bank_masks
    with open(os.path.join(ROOT, "configs", "celeba_hq.yml")) as f:
        cfg = yaml.safe_load(f)
    cfg["time_travel"]["T_sampling"] = 4
    cfg["data"]["image_size"] = 64
    cfg["model"]["ch_mult"] = [1, 1, 2]
    os.makedirs(os.path.join(root, "configs"), exist_ok=True)
    for batch in (1, 2):
        cfg["sampling"]["batch_size"] = batch
        with open(os.path.join(root, "configs", f"mini_b{batch}.yml"), "w") as f:
            yaml.safe_dump(cfg, f)
    np.save(os.path.join(root, "bank_masks.npy"), bank_masks(64))


def _set_mask(root, case):
    """exp/inp_masks/mask.npy is the bank for a bank case and absent otherwise."""
    import shutil
    path = os.path.join(root, "exp", "inp_masks", "mask.npy")
    if case["bank"]:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        shutil.copyfile(os.path.join(root, "bank_masks.npy"), path)
    elif os.path.exists(path):
        os.remove(path)


def _pngs(folder):
    import numpy as np
    from PIL import Image
    table = {}
    for d, _, files in os.walk(folder):
        for f in files:
            if f.endswith(".png"):
                px = np.ascontiguousarray(np.asarray(Image.open(os.path.join(d, f))))
                digest = hashlib.sha256(repr((px.shape, str(px.dtype))).encode() + px.tobytes()).hexdigest()
                table[os.path.relpath(os.path.join(d, f), folder)] = digest
    return dict(sorted(table.items()))


def _lines(out):
    return [line for line in out.splitlines() if line.startswith(HEADS)]


def _environment(case):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    return dict(env, DDNM_RANDOM_WEIGHTS="1", DDNM_GPUS="1", **case["env"])       # DDNM_GPUS=1: no self-launch


def run_case(case, root):
    """One run in `root` (prepare_root): {"calls": [...] or None for the two-rank case, "lines": [...], "png": {...}}."""
    _set_mask(root, case)
    folder = os.path.join(root, "exp", "image_samples", case["name"])
    if case["ranks"] > 1:
        import socket
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={case['ranks']}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "main.py")] + case["argv"]
        r = subprocess.run(cmd, cwd=root, env=dict(_environment(case), DDNM_DIST_BACKEND="gloo", PYTHONPATH=ROOT),
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"{case['name']}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        return dict(calls=None, lines=_lines(r.stdout), png=_pngs(folder))
    import main
    from ddnm_amd.guided_diffusion.models import Model
    calls, orig_call = [], Model.__call__

    def call(self, x, t):
        calls.append(int(x.shape[0]))
        return orig_call(self, x, t)

    buf, cwd, env = io.StringIO(), os.getcwd(), dict(os.environ)
    Model.__call__ = call
    os.environ.clear()
    os.environ.update(_environment(case))
    os.chdir(root)
    try:
        with contextlib.redirect_stdout(buf):
            rc = main.main(case["argv"])
    finally:
        os.chdir(cwd)
        os.environ.clear()
        os.environ.update(env)
        Model.__call__ = orig_call
    out = buf.getvalue()
    if rc != 0 or "Number of samples:" not in out:          # main logs an exception of the run and still returns 0
        raise RuntimeError(f"{case['name']}: the run did not finish\n{out[-3000:]}")
    return dict(calls=[c for i, c in enumerate(calls) if i == 0 or c != calls[i - 1]], lines=_lines(out), png=_pngs(folder))


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", action="append", help="record this case alone (repeatable), e.g. under a kernel trace")
    opts = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/record_runner_runs.py needs the MI355X: the table holds what the GPU run writes")
    table = {}
    with tempfile.TemporaryDirectory() as root:
        prepare_root(root)
        for case in CASES:
            if opts.case and case["name"] not in opts.case:
                continue
            table[case["name"]] = dict(argv=case["argv"], env=case["env"], **run_case(case, root))
            print(f"[record] {case['name']}: calls {table[case['name']]['calls']}, {len(table[case['name']]['lines'])} lines, "
                  f"{len(table[case['name']]['png'])} PNGs", file=sys.stderr, flush=True)
    json.dump(table, sys.stdout, indent=1)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
