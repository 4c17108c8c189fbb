"""PSNR and SSIM of an image folder the runner wrote: `python -m ddnm_amd.evaluate <image_folder>
[--against restored|Apy|mean] [--sample k] [--json FILE]`.

`restored` (default) pairs `Apy/orig_{i}.png` with the restoration `{i}_0.png` -- `{i}_{k}.png` with `--sample k`, the
k-th restoration of a DDNM_SAMPLES run; `Apy` pairs it with `Apy/Apy_{i}.png`, the A^+ y baseline row of the paper's
tables; `mean` pairs it with `mean/mean_{i}.png`, the posterior mean of a DDNM_SAMPLES run.  The 8-bit PNGs are loaded
with PIL and evaluated on the GPU by the kernels the runner reports with: PSNR by `ops.finalize_psnr` on 2v - 1, SSIM by `ops.ssim(..., transform=False)`.
One `index PSNR SSIM` row per image, then the averages.  Indices present on one side only are listed and skipped.

(`--simplified` runs name the restoration of image i `{i - 1}_0.png`, like the reference; rename them before pairing.)
"""
import argparse
import json
import os
import re
import sys

import numpy as np

AGAINST = ("restored", "Apy", "mean")
BATCH = 32          # images of one size evaluated per launch


def _indexed(folder, pattern):
    """{i: path} of the files of `folder` whose name matches `pattern` (one group: the index)."""
    if not os.path.isdir(folder):
        return {}
    found = {}
    for name in os.listdir(folder):
        m = re.fullmatch(pattern, name)
        if m:
            found[int(m.group(1))] = os.path.join(folder, name)
    return found


def pair_files(image_folder, against="restored", sample=0):
    """(pairs, missing): pairs = [(i, path of orig_i, path of the image compared with it)] sorted by i; missing =
    {"orig": [...], against: [...]} = the indices that have the other file only.  `sample` picks the restoration
    `{i}_{sample}.png` of a DDNM_SAMPLES run (against="restored" only).  Touches file names only."""
    if against not in AGAINST:
        raise ValueError(f"--against: unknown choice {against!r}; accepted values: {', '.join(AGAINST)}")
    sample = int(sample)
    if sample < 0 or (sample and against != "restored"):
        raise ValueError(f"--sample {sample}: a sample index >= 0, with --against restored only")
    apy = os.path.join(image_folder, "Apy")
    orig = _indexed(apy, r"orig_(\d+)\.png")
    if against == "restored":
        other = _indexed(image_folder, r"(\d+)_%d\.png" % sample)
    elif against == "mean":
        other = _indexed(os.path.join(image_folder, "mean"), r"mean_(\d+)\.png")
    else:
        other = _indexed(apy, r"Apy_(\d+)\.png")
    pairs = [(i, orig[i], other[i]) for i in sorted(orig.keys() & other.keys())]
    missing = {"orig": sorted(other.keys() - orig.keys()), against: sorted(orig.keys() - other.keys())}
    if not pairs:
        raise FileNotFoundError(f"{image_folder}: no Apy/orig_<i>.png has a partner for --against {against}" +
                                (f" --sample {sample}" if sample else ""))
    return pairs, missing


def load_image(path):
    """8-bit RGB PNG -> float32 [3, H, W] in [0, 1] (v = u / 255, divided on the host)."""
    from PIL import Image
    with Image.open(path) as im:
        u = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return np.ascontiguousarray((u.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))


def evaluate(pairs, device="cuda"):
    """[(i, psnr, ssim)] in the order of `pairs`; images are batched per equal size."""
    import torch

    from . import ops
    by_shape, rows = {}, {}
    for i, a, b in pairs:
        ref, img = load_image(a), load_image(b)
        if ref.shape != img.shape:
            raise ValueError(f"index {i}: {a} is {ref.shape[1:]} but {b} is {img.shape[1:]}")
        by_shape.setdefault(ref.shape, []).append((i, ref, img))
    for items in by_shape.values():
        for lo in range(0, len(items), BATCH):
            chunk = items[lo:lo + BATCH]
            ref = torch.from_numpy(np.stack([c[1] for c in chunk])).to(device)
            img = torch.from_numpy(np.stack([c[2] for c in chunk])).to(device)
            _, psnr = ops.finalize_psnr((2 * img - 1).contiguous(), (2 * ref - 1).contiguous(), want_img=False)
            ssim = ops.ssim(img, ref, transform=False)
            for (i, _, _), p, s in zip(chunk, psnr.cpu().tolist(), ssim.cpu().tolist()):
                rows[i] = (i, p, s)
    return [rows[i] for i, _, _ in pairs]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m ddnm_amd.evaluate", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("image_folder", help="<exp>/image_samples/<-i> of a finished run")
    ap.add_argument("--against", choices=AGAINST, default="restored", help="what Apy/orig_<i>.png is compared with")
    ap.add_argument("--sample", type=int, default=0, metavar="k",
                    help="with --against restored: compare the k-th restoration <i>_<k>.png of a DDNM_SAMPLES run")
    ap.add_argument("--json", metavar="FILE", help="also write the rows and averages as JSON")
    args = ap.parse_args(argv)
    pairs, missing = pair_files(args.image_folder, args.against, args.sample)
    for side, idx in missing.items():
        if idx:
            print(f"skipped (no {side} file): {' '.join(map(str, idx))}")
    rows = evaluate(pairs)
    for i, p, s in rows:
        print("%d %.2f %.4f" % (i, p, s))
    psnr, ssim = sum(r[1] for r in rows) / len(rows), sum(r[2] for r in rows) / len(rows)
    print("Average PSNR: %.2f" % psnr)
    print("Average SSIM: %.4f" % ssim)
    print("Number of images: %d" % len(rows))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"image_folder": args.image_folder, "against": args.against, "missing": missing,
                       "images": [{"index": i, "psnr": p, "ssim": s} for i, p, s in rows],
                       "psnr": psnr, "ssim": ssim, "n": len(rows)}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
