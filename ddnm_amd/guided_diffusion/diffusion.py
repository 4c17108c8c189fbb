"""Runner of the DDNM CLI on MI355X: `Diffusion(args, config).sample(simplified)`.

Same seam as the reference's `guided_diffusion/diffusion.py::Diffusion` (:79-610): it is built
from the argparse namespace + YAML namespace of `main.py`, constructs the noise predictor and the
degradation operator for `--deg`, forms `y = A(x_orig)`, draws `x_T`, runs the reverse loop and
reports PSNR.  The hot path underneath is ours: `ddnm_amd.guided_diffusion.models.Model`,
`ddnm_amd.functions.svd_operators.*`, `ddnm_amd.functions.svd_ddnm.ddnm_diffusion`.

Deliberate differences at the boundary (not in the results):
  * checkpoints are never downloaded (no network): `exp/logs/celeba/celeba_hq.ckpt` must exist,
    or `DDNM_RANDOM_WEIGHTS=1` selects seeded random weights of the same architecture;
  * images are read/written with PIL (torchvision is not required);
  * multi-GPU is one process per GPU (ddnm_amd.dist), not `torch.nn.DataParallel` (:140,164): every rank sees the
    same batches, restores the images [lo, hi) of each batch (its slice of x_T and of the per-step noise, both drawn
    for the WHOLE batch from a per-batch generator so the result does not depend on the number of ranks), and the
    restored shards meet in ONE RCCL all_gather per batch; rank 0 writes the PNGs and reports the PSNR;
  * DDNM_FUSE_BATCHES=K (default 1) restores up to K consecutive loader batches of a rank in one sampler call, each image
    with the noise it gets alone (per-image Philox keys, ops.KeyedPhiloxNoise): the shipped configs' batch of one image
    leaves most of the chip idle.  Files, PSNR lines and totals are those of the unfused run;
  * `--deg inpainting` with a 3-D `exp/inp_masks/mask.npy` [N, S, S] restores every image with its own hole: the image
    written as `{i}_0.png` uses mask i % N (`restored_images`), in every sharding and fusing mode.  The reference holds
    one mask per run; a 2-D file behaves as there;
  * DDNM_METRICS=ssim adds the SSIM column of the paper's tables: an `SSIM: %.4f` line (running mean) after every
    `PSNR:` line and `Total Average SSIM: %.4f` after the total (ops.ssim, csrc/metrics.hip).  Unset, nothing changes.
    The averages and, with the switch, this rank's per-image values stay on the runner as `last_metrics`;
  * DDNM_SAMPLES=K (default 1) restores every measurement K times in ONE sampler call, sample k with the noise of a run
    under `--seed seed + k` (sample_sources) and all K with the one measurement y of the run's own seed: `{i}_{k}.png` for
    every k (the reference hard-wires the 0), `mean/mean_{i}.png` (the posterior mean) and `std/std_{i}.png` (the
    per-pixel standard deviation, ops.sample_stats, csrc/metrics.hip).  The PSNR / SSIM lines stay those of sample 0;
  * measurements leave and enter the process: DDNM_SAVE_Y=1 writes the rows the sampler is given to `y/y_{i}.npy` (+
    `y/measurements.json`, settings only), and `--path_y measurements:DIR` restores the .npy rows or pictures lying in DIR
    (MeasurementFolder) instead of degrading a ground truth: no `orig_{i}.png`, no PSNR / SSIM.  With the same seed and
    settings the second run writes the first run's PNGs byte for byte (not under DDNM_NOISE=torch, not for the two CS
    operators, whose matrices come from the global generators);
  * DDNM_METRICS=cons reports the data consistency of every restoration, the one figure of merit that needs no ground
    truth (and the one a run over given measurements reports unasked): `Cons: %.3e`, the running mean of
    sum |A x^ - y| / (2 n) over the n valid entries of an image's measurement ([0, 1] scale), `Total Average Cons` and
    `Max Cons`, the largest max |A x^ - y| / 2 of the run (ops.consistency, csrc/metrics.hip);
  * `--deg demosaic_rggb | demosaic_bggr | demosaic_grbg | demosaic_gbrg | demosaic_xtrans` (and `--deg demosaic` with
    the pattern of `exp/cfa/pattern.npy`) restores a raw sensor frame, one colour sample per pixel (svd_operators.Mosaic):
    the reference's Inpainting over single entries, so every switch above applies; its measurement is a one-channel
    S x S picture, and `Apy_{i}.png` shows the coloured mosaic;
  * `--deg mask_color_sr` (the 2-D mask of `exp/inp_masks/mask.npy`, grey, average pool by `--deg_scale` 1 | 2 | 4 | 8) and
    `--deg sr_color` (the same without a mask) restore an old photo on the SVD path too (svd_operators.MaskColorSR: the
    exact pseudo-inverse, one fused step kernel for DDNM and one for DDNM+), so every switch above applies; the measurement
    is a one-channel S/r x S/r picture and `Apy_{i}.png` shows A^+ y.  `--simplified --deg mask_color_sr | diy` keeps the
    reference's Composition and its chained inverse;
  * `--deg chroma_420 | chroma_422 | chroma_411` (chroma sites of 2 x 2, 2 x 1, 4 x 1 pixels; `--deg_scale` is not read) and
    `--deg chroma_sub --deg_scale 2 | 4 | 8` (square sites) restore a picture stored as Y'CbCr with subsampled chroma:
    full-resolution luma, one Cb and one Cr sample per site (svd_operators.ChromaSubsample, full-range BT.601: the exact
    pseudo-inverse, one fused step kernel for DDNM and one for DDNM+), so every switch above applies; a measurement is the
    three planes in a row, S^2 + 2 S^2 / n values, which no picture holds (`.npy` rows), and `Apy_{i}.png` shows A^+ y;
  * `--deg jpeg_444 | jpeg_422 | jpeg_420 --deg_scale Q` (the quality, an integer in 1..100) restores a JPEG file
    (svd_operators.JPEG): the measurement is the dequantised 8 x 8 block-DCT coefficients of those planes, the step pulls
    T x0 back into every coefficient's quantisation cell (share `--jpeg_box`, default 0.98) in one fused launch, so the
    restoration re-encodes to the same file (`Cons` is 0 exactly then); `Apy_{i}.png` is the decoded JPEG picture.
    Noise-free only: `--sigma_y > 0`, `--sigma_y_shot`, `--sigma_y_map` and `--simplified` are refused (check_jpeg_flags).

All of these run through ONE path of `Diffusion.svd_based_ddnm_plus`: the plan (`fuse_groups`: which loader batches this
rank restores, grouped into sampler calls; `restored_images` is the same plan as image indices), `prepare` (a loader batch
-> a `Part`: y, Apy files, x_T and one noise source per sample), `restore` (a group of parts -> one sampler call, the only
one) and `finish` (one part's rows -> gather in split mode, PNGs, metric lines, K-sample statistics).  The plain run is
the case of one part per call and one sample per image.
"""
import collections
import os
import random

import numpy as np
import torch
import torch.utils.data as data

from .. import dist as ddist
from .. import ops
from ..functions.svd_ddnm import (_AtenNoise, _reverse_loop, _TapeNoise, ddnm_diffusion, ddnm_plus_diffusion,
                                  get_schedule_jump)
from ..functions.svd_operators import (DEMOSAIC, HN_OPERATORS, JPEG_NAMES, Colorization, Denoising, Inpainting, InpaintingBank,
                                      NoiseModel, SuperResolution, build_operator, jpeg_quality_of, mask_color_sr,
                                      missing_indices_of_mask)
from .models import Model


def get_beta_schedule(beta_schedule, *, beta_start, beta_end, num_diffusion_timesteps):
    """float64 schedules of diffusion.py:46-76."""
    n = num_diffusion_timesteps
    if beta_schedule == "quad":
        betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=np.float64) ** 2
    elif beta_schedule == "linear":
        betas = np.linspace(beta_start, beta_end, n, dtype=np.float64)
    elif beta_schedule == "const":
        betas = beta_end * np.ones(n, dtype=np.float64)
    elif beta_schedule == "jsd":
        betas = 1.0 / np.linspace(n, 1, n, dtype=np.float64)
    elif beta_schedule == "sigmoid":
        s = np.linspace(-6, 6, n)
        betas = 1 / (np.exp(-s) + 1) * (beta_end - beta_start) + beta_start
    else:
        raise NotImplementedError(beta_schedule)
    assert betas.shape == (n,)
    return betas


IMG_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".webp")


class ImageFolder(data.Dataset):
    """torchvision.datasets.ImageFolder + ToTensor: classes = sorted sub-directories, files sorted inside each.
    transform "resize": Resize([S,S]) bilinear (datasets/__init__.py:138-150, CelebA_HQ / FFHQ);
    transform "center_crop_arr": the guided-diffusion crop (`out_of_dist` LSUN / ImageNet folders, :113-119,177-183)."""

    def __init__(self, root, image_size, transform="resize"):
        from PIL import Image  # noqa: F401
        self.size, self.transform = image_size, transform
        self.items = []
        classes = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
        for ci, c in enumerate(classes):
            for dirpath, _, files in sorted(os.walk(os.path.join(root, c))):
                for f in sorted(files):
                    if f.lower().endswith(IMG_EXT):
                        self.items.append((os.path.join(dirpath, f), ci))
        if not self.items:
            raise FileNotFoundError(f"no images under {root}")

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        from PIL import Image
        path, cls = self.items[i]
        img = Image.open(path).convert("RGB")
        if self.transform == "center_crop_arr":
            arr = center_crop_arr(img, self.size)
        else:
            arr = np.asarray(img.resize((self.size, self.size), Image.BILINEAR), dtype=np.uint8)
        x = torch.from_numpy(arr.copy()).permute(2, 0, 1).float().div(255.0)
        return x, cls


def center_crop_arr(pil_image, image_size=256):
    """datasets/__init__.py:29-44 (from openai/guided-diffusion): box-downsample while >= 2x, bicubic to the
    short side, centre crop."""
    from PIL import Image
    while min(*pil_image.size) >= 2 * image_size:
        pil_image = pil_image.resize(tuple(x // 2 for x in pil_image.size), resample=Image.BOX)
    scale = image_size / min(*pil_image.size)
    pil_image = pil_image.resize(tuple(round(x * scale) for x in pil_image.size), resample=Image.BICUBIC)
    arr = np.array(pil_image)
    cy, cx = (arr.shape[0] - image_size) // 2, (arr.shape[1] - image_size) // 2
    return arr[cy:cy + image_size, cx:cx + image_size]


def center_crop_long_edge(pil_image):
    """datasets/imagenet_subset.py:5-23 (`CenterCropLongEdge`): torchvision's center_crop to min(w, h) -- the offsets
    are int(round((dim - s) / 2.0)) like torchvision.transforms.functional.center_crop."""
    w, h = pil_image.size
    s = min(w, h)
    left, top = int(round((w - s) / 2.0)), int(round((h - s) / 2.0))
    return pil_image.crop((left, top, left + s, top + s))


class ImageList(data.Dataset):
    """datasets/imagenet_subset.py::ImageDataset(normalize=False) (:48-103), what `subset_1k: true` of the ImageNet
    configs selects (datasets/__init__.py:169-175): list file of '<name> <label>' (label -1 when absent),
    CenterCropLongEdge + Resize(image_size) (bilinear) + ToTensor."""

    def __init__(self, root, list_file, image_size):
        self.root, self.size = root, image_size
        self.items = []
        with open(list_file) as f:
            for line in f:
                parts = line.rstrip().split()
                if parts:
                    self.items.append((parts[0], int(parts[1]) if len(parts) == 2 else -1))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        from PIL import Image
        name, label = self.items[i]
        with open(self.root + "/" + name, "rb") as f:
            img = Image.open(f).convert("RGB")
        img = center_crop_long_edge(img).resize((self.size, self.size), Image.BILINEAR)
        x = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255.0)
        return x, label


class SyntheticImages(data.Dataset):
    """Seeded U[0,1] images (BASELINE metric inputs; `--path_y synthetic:N`)."""

    def __init__(self, n, image_size, seed):
        self.n, self.size, self.seed = n, image_size, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 100003 + i)
        return torch.rand(3, self.size, self.size, generator=g), 0


MEASUREMENTS = "measurements:"                      # --path_y measurements:DIR: restore the measurements lying in DIR
MEASUREMENT_EXT = (".npy", ".png", ".jpg", ".jpeg")
MEASUREMENT_SETTINGS = "measurements.json"          # what DDNM_SAVE_Y=1 writes next to the y_{i}.npy: settings only
MEASUREMENT_PINNED = ("deg", "deg_scale", "image_size", "channels")      # a folder's settings a run must agree with
# ... and, where the folder records them (a run under --sigma_y_shot / --sigma_y_map), the per-entry noise model
MEASUREMENT_NOISE_KEYS = ("sigma_y_shot", "sigma_y_map_sha256", "sigma_y_map_len")


def measurement_dir(path_y, exp):
    """DIR of `--path_y measurements:DIR` (absolute, or below <exp>/datasets/), None for every other --path_y."""
    path_y = str(path_y)
    if not path_y.startswith(MEASUREMENTS):
        return None
    d = path_y[len(MEASUREMENTS):]
    if not d:
        raise ValueError(f"--path_y {path_y}: name the folder of measurements after the colon")
    return d if os.path.isabs(d) else os.path.join(exp, "datasets", d)


# DDNM_SAVE_Y=1: the SVD-path runner writes the measurement rows it restores from to <image_folder>/y/ (default: off)
def save_y():
    v = os.environ.get("DDNM_SAVE_Y", "")
    if v not in ("", "0", "1"):
        raise ValueError(f"DDNM_SAVE_Y must be 0 or 1, got {v!r}")
    return v == "1"


def run_settings(args, config, sigma_y, noise_model=None):
    """The settings a saved measurement depends on (`sigma_y` on the command line's [0, 1] scale); a per-entry
    `noise_model` (shot + read noise, a noise map) adds its shot gain and the map's SHA-256 and length."""
    out = {"deg": args.deg, "deg_scale": float(args.deg_scale), "image_size": int(config.data.image_size),
           "channels": int(config.data.channels), "sigma_y": float(sigma_y), "add_noise": bool(args.add_noise),
           "seed": int(args.seed)}
    if noise_model is not None and not noise_model.is_scalar:
        out.update(noise_model.settings())
    return out


def noise_model_of(args, op=None):
    """The NoiseModel of the command line (--sigma_y, --sigma_y_shot, --sigma_y_map; [0, 1] scale) for operator `op`:
    the scalar form unless one of the two new flags is given; a per-entry form needs an operator with the hook."""
    shot, path = float(getattr(args, "sigma_y_shot", 0.0) or 0.0), getattr(args, "sigma_y_map", None)
    nm = NoiseModel.from_options(args.sigma_y, shot, path, op)
    if not nm.is_scalar and not hasattr(op, "ddnm_plus_step_hn"):
        raise ValueError(f"--sigma_y_shot / --sigma_y_map: per-entry measurement noise is supported by {HN_OPERATORS}, "
                         f"not by --deg {args.deg} ({type(op).__name__})")
    return nm


def check_noise_flags(args, simplified):
    """--sigma_y_shot / --sigma_y_map belong to the SVD path's DDNM+ loop."""
    if simplified and (float(getattr(args, "sigma_y_shot", 0.0) or 0.0) != 0.0 or getattr(args, "sigma_y_map", None)):
        raise ValueError("--simplified with --sigma_y_shot / --sigma_y_map: the simplified loop knows one sigma_y; "
                         "per-entry measurement noise runs on the SVD path only")


def check_jpeg_flags(args, simplified):
    """What `--deg jpeg_444 | jpeg_422 | jpeg_420` cannot be combined with, and `--jpeg_box` under any other --deg."""
    box = getattr(args, "jpeg_box", None)
    if args.deg not in JPEG_NAMES:
        if box is not None:
            raise ValueError(f"--jpeg_box is the cell share of --deg {' | '.join(JPEG_NAMES)}; --deg {args.deg} does not read it")
        return
    jpeg_quality_of(args.deg, args.deg_scale)
    if box is not None and not 0.0 <= box <= 1.0:
        raise ValueError(f"--jpeg_box is a share of the quantisation cell, in [0, 1]: got {box!r}")
    why = ("the quantisation error of a JPEG file is bounded, not Gaussian, and its cell is the exact model: the step "
           "projects into the cell and there is no DDNM+ form")
    if float(args.sigma_y) > 0.0:
        raise ValueError(f"--deg {args.deg} with --sigma_y {args.sigma_y}: {why}")
    if float(getattr(args, "sigma_y_shot", 0.0) or 0.0) != 0.0:
        raise ValueError(f"--deg {args.deg} with --sigma_y_shot: {why}")
    if getattr(args, "sigma_y_map", None):
        raise ValueError(f"--deg {args.deg} with --sigma_y_map: {why}")
    if simplified:
        raise ValueError(f"--simplified with --deg {args.deg}: the simplified loop corrects with A^+(A x0 - y) onto one "
                         "value; the cell projection is a fused step of the SVD path only")


def check_measurements(args, simplified):
    """What a run over given measurements (`--path_y measurements:DIR`) cannot do, said before its first image is loaded."""
    if measurement_dir(args.path_y, args.exp) is None:
        return
    if args.add_noise:
        raise ValueError("--add_noise with --path_y measurements:DIR: the measurement is given, there is nothing to add "
                         "noise to (--sigma_y alone states its noise level and selects DDNM+)")
    if "ssim" in extra_metrics():
        raise ValueError("DDNM_METRICS=ssim with --path_y measurements:DIR: SSIM compares with the ground truth, and a "
                         "run over given measurements has none (Cons is reported instead)")
    if simplified:
        raise ValueError("--simplified with --path_y measurements:DIR: measurements are read by the SVD path only")


def _last_int_key(name):
    """Sort key of a measurement file: the last integer of its stem, then the name (y_2 before y_10); stems without a
    digit follow, by name."""
    stem = os.path.splitext(name)[0]
    digits = ""
    for ch in reversed(stem):
        if ch.isdigit():
            digits = ch + digits
        elif digits:
            break
    return (0, int(digits), name) if digits else (1, 0, name)


class MeasurementFolder(data.Dataset):
    """The measurements of `--path_y measurements:DIR`: the .npy / .png / .jpg / .jpeg files of DIR (not
    measurements.json), ordered by the last integer of the stem, then by name; position p is image --subset_start + p.
    `bind(op, config, start)` names the operator the rows belong to and checks every file against it (element count of
    an .npy, pixel size of a picture) before anything is restored.  An item is (tensor, is_picture): an .npy gives its
    row as it is -- any shape with `measurement_size` elements, cast to fp32, zero padded to a mask bank's y_dim --, a
    picture gives [c, h, w] of `measurement_image_shape()` on the engine's [-1, 1] scale (the runner flattens it, or
    applies A for inpainting).  Nothing is resized, cropped or shuffled."""

    def __init__(self, root, limit=None):
        if not os.path.isdir(root):
            raise FileNotFoundError(f"no folder of measurements at {root}")
        names = [f for f in os.listdir(root)
                 if f.lower().endswith(MEASUREMENT_EXT) and os.path.isfile(os.path.join(root, f))]
        names.sort(key=_last_int_key)
        stems = {}
        for f in names:
            stem = os.path.splitext(f)[0]
            if stem in stems:
                raise ValueError(f"{root}: {stems[stem]} and {f} share the stem {stem!r}: one measurement per image")
            stems[stem] = f
        if not names:
            raise FileNotFoundError(f"no measurements (.npy, .png, .jpg, .jpeg) in {root}")
        self.root, self.names = root, names[:limit]
        self.op = self.config = None
        self.start = 0

    def settings(self):
        """The folder's measurements.json as a dict, None without the file."""
        import json
        path = os.path.join(self.root, MEASUREMENT_SETTINGS)
        if not os.path.exists(path):
            return None
        with open(path) as f:
            return json.load(f)

    def check_settings(self, run):
        """`run` (run_settings) against the folder's measurements.json: the operator must be the one y was formed with."""
        have = self.settings()
        for key in MEASUREMENT_PINNED if have else ():
            if key in have and have[key] != run[key]:
                raise ValueError(f"{os.path.join(self.root, MEASUREMENT_SETTINGS)}: the measurements were formed with "
                                 f"{key} = {have[key]!r}, this run has {key} = {run[key]!r}")

    def check_noise_settings(self, run):
        """The per-entry noise model the folder records (MEASUREMENT_NOISE_KEYS of its measurements.json) against this
        run's: another shot gain, another map or none is refused; a folder that records none leaves the run free."""
        have = self.settings() or {}
        for key in MEASUREMENT_NOISE_KEYS:
            if key in have and have[key] != run.get(key, 0.0 if key == "sigma_y_shot" else None):
                raise ValueError(f"{os.path.join(self.root, MEASUREMENT_SETTINGS)}: the measurements were formed with "
                                 f"{key} = {have[key]!r}, this run has {key} = {run.get(key)!r}")

    def __len__(self):
        return len(self.names)

    def _expected(self, p):
        """(valid entries, row length) of the measurement at position p."""
        if hasattr(self.op, "for_images"):                     # a mask bank: image i uses mask i % N
            return self.op.measurement_size(self.start + p), self.op.y_dim
        n = self.op.measurement_size()
        return n, n

    def bind(self, op, config, start=0):
        self.op, self.config, self.start = op, config, start
        shape = op.measurement_image_shape()
        for p, f in enumerate(self.names):
            path, n = os.path.join(self.root, f), self._expected(p)[0]
            if f.lower().endswith(".npy"):
                arr = np.load(path, mmap_mode="r", allow_pickle=False)
                if arr.size != n:
                    raise ValueError(f"{path} holds {arr.size} values (shape {tuple(arr.shape)}), the operator's measurement "
                                     f"of image {start + p} has {n}")
            elif shape is None:
                raise ValueError(f"{path} is a picture, but a measurement of this operator is no picture: it takes .npy "
                                 f"files of {n} values")
            elif shape[0] not in (1, 3):
                raise ValueError(f"{path}: pictures hold 1 or 3 channels, the operator's measurement has {shape[0]}")
            else:
                from PIL import Image
                with Image.open(path) as img:
                    (w, h), bands = img.size, img.getbands()
                if shape[0] == 1 and len(bands) != 1:
                    # (a luminance conversion is no operator's measurement: a grey frame is taken as it is, nothing else)
                    raise ValueError(f"{path} holds {len(bands)} channels ({''.join(bands)}), the operator's measurement "
                                     f"has 1: nothing is converted")
                if (h, w) != tuple(shape[1:]):
                    raise ValueError(f"{path} is {w} x {h} pixels (width x height), the operator's measurement is "
                                     f"{shape[2]} x {shape[1]}: nothing is resized or cropped")
        return self

    def __getitem__(self, p):
        if self.op is None:
            raise RuntimeError("MeasurementFolder.bind(operator, config) comes first")
        f = self.names[p]
        path = os.path.join(self.root, f)
        if f.lower().endswith(".npy"):
            n, width = self._expected(p)
            row = torch.zeros(width, dtype=torch.float32)
            row[:n] = torch.from_numpy(np.load(path, allow_pickle=False).astype(np.float32).reshape(-1))
            return row, False
        from PIL import Image
        c = self.op.measurement_image_shape()[0]
        with Image.open(path) as img:
            arr = np.asarray(img.convert("L" if c == 1 else "RGB"), dtype=np.uint8)
        x = torch.from_numpy(arr.reshape(arr.shape[0], arr.shape[1], c).copy()).permute(2, 0, 1).float().div(255.0)
        return data_transform(self.config, x).contiguous(), True


def save_image(x, path):
    """torchvision.utils.save_image for one [3,H,W] image in [0,1]."""
    from PIL import Image
    arr = x.detach().float().cpu().mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
    Image.fromarray(arr).save(path)


def data_transform(config, X):
    """datasets/__init__.py:201-216 for the configs on the hot path (rescaled: 2x - 1)."""
    if getattr(config.data, "uniform_dequantization", False) or getattr(config.data, "gaussian_dequantization", False):
        raise NotImplementedError("dequantization transforms are training-time options")
    if config.data.rescaled:
        return 2 * X - 1.0
    raise NotImplementedError("only rescaled data is on the DDNM hot path")


# functions/ckpt_util.py:15-24 (EMA checkpoints of the DDIM authors; `church_outdoor` -> `church`, :56-57)
LSUN_CKPT = {"bedroom": "ema_diffusion_lsun_bedroom_model/model-2388000.ckpt",
             "cat": "ema_diffusion_lsun_cat_model/model-1761000.ckpt",
             "church": "ema_diffusion_lsun_church_model/model-4432000.ckpt"}


def simple_checkpoint_path(config, exp):
    """Checkpoint of a `model.type: simple` config (guided_diffusion/diffusion.py:115-136): celeba_hq ->
    exp/logs/celeba/celeba_hq.ckpt; LSUN category -> the `ema_lsun_<category>` file get_ckpt_path resolves under
    $XDG_CACHE_HOME or exp/logs/ + diffusion_models_converted/ (ckpt_util.py:55-66).  Nothing is downloaded here."""
    ds = config.data.dataset
    if ds == "CelebA_HQ":
        return os.path.join(exp, "logs/celeba/celeba_hq.ckpt")
    if ds == "LSUN":
        cat = str(config.data.category).replace("church_outdoor", "church")
        if cat not in LSUN_CKPT:
            raise ValueError(f"no checkpoint known for LSUN category {config.data.category!r}")
        cachedir = os.environ.get("XDG_CACHE_HOME", os.path.join(exp, "logs/"))
        return os.path.join(cachedir, "diffusion_models_converted", LSUN_CKPT[cat])
    raise ValueError(f"no checkpoint family for dataset {ds!r} with model.type=simple")   # CIFAR10 is not a DDNM config


def _mix64(seed, k):
    """64-bit key of (run seed, batch index): splitmix64 finaliser, so that neighbouring seeds / batches share no key bits."""
    z = (int(seed) * 0x9E3779B97F4A7C15 + int(k) * 0xBF58476D1CE4E5B9 + 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


class BatchNoise:
    """Noise of one loader batch, independent of how the batch is sharded: x_T and the tensor of loop iteration k are
    drawn for ALL `n` images from a generator seeded by (seed, batch index) -- in a fixed order -- and sliced to
    [lo, hi).  Indexing is sequential (`tape[k]` for k = 0, 1, ...), which is how `ddnm_diffusion(noise=...)` reads it."""

    def __init__(self, seed, batch_index, n, shape, lo, hi, device):
        self.g = torch.Generator(device=device)
        self.g.manual_seed((int(seed) * 1000003 + int(batch_index)) % (2 ** 63 - 1))
        self.full, self.lo, self.hi, self.device = (n,) + tuple(shape), lo, hi, device
        self.next_k = 0

    def draw(self, shape=None):
        return torch.randn(self.full if shape is None else shape, generator=self.g, device=self.device)

    def x_T(self):
        return self.draw()[self.lo:self.hi].contiguous()

    def __getitem__(self, k):
        if k != self.next_k:
            raise IndexError(f"BatchNoise is a sequential tape: asked for {k}, expected {self.next_k}")
        self.next_k += 1
        return self.draw()[self.lo:self.hi].contiguous()


def measurement_noise(key, like):
    """N(0, I) of `--add_noise` for y viewed as [b, n] (Philox key `key`, image counter = index in the batch): the
    unkeyed draw when n % 4 == 0, else the keyed one, which takes any n (inpainting's y has 3 * n_kept entries) and gives
    the same values on the whole blocks of four."""
    src = ops.PhiloxNoise(key, 0)
    if like.shape[1] % 4 == 0:
        return src.tensor(0, like)
    return ops.KeyedPhiloxNoise.from_sources([(src, i) for i in range(like.shape[0])]).tensor(0, like)


class FusedTape:
    """Noise tape of a fused sampler call: `tape[k]` = the concatenation of each loader batch's own draw k (BatchNoise
    tapes, or per-image lists of the simplified path), so every part keeps the sequence it has when restored alone."""

    def __init__(self, parts):
        self.parts = list(parts)

    def __getitem__(self, k):
        return torch.cat([p[k] for p in self.parts], 0)


# DDNM_FUSE_BATCHES=K: restore up to K consecutive loader batches of this rank in ONE sampler call (default 1 = off)
def fuse_batches():
    k = int(os.environ.get("DDNM_FUSE_BATCHES", "1"))
    if k < 1:
        raise ValueError(f"DDNM_FUSE_BATCHES must be >= 1, got {k}")
    return k


# DDNM_SAMPLES=K: K restorations of every measurement in ONE sampler call (default 1 = off)
def samples():
    k = int(os.environ.get("DDNM_SAMPLES", "1"))
    if k < 1:
        raise ValueError(f"DDNM_SAMPLES must be >= 1, got {k}")
    return k


def check_samples(k, simplified):
    """What a run with DDNM_SAMPLES=k cannot do, said before its first image is loaded."""
    if k > 1 and simplified:
        raise ValueError(f"DDNM_SAMPLES={k} needs the SVD path: the --simplified loop draws its noise from ATen's global "
                         "generator, which has no per-sample key")


def sample_sources(seed, bi, k, lo):
    """Philox sources of the `k` samples of loader batch `bi` for a rank whose slice of the batch starts at image `lo`:
    sample s draws what the batch draws in a run under `--seed seed + s` (sample 0: today's source)."""
    return [ops.PhiloxNoise(_mix64(seed + s, bi), image_base=lo) for s in range(k)]


def sample_rows(images, sizes, k):
    """Image of every row of a sampler call over `k` samples: `images` lists the call's images batch after batch,
    `sizes` the number of images of each batch; the rows run batch-major, then sample, then image."""
    if sum(sizes) != len(images):
        raise ValueError(f"sample_rows: {len(images)} images for batches of {list(sizes)}")
    rows, off = [], 0
    for n in sizes:
        rows += list(images[off:off + n]) * k
        off += n
    return rows


STD_DISPLAY_GAIN = 4.0      # std/std_{i}.png holds clamp(gain * s, 0, 1): a display choice, s itself rarely exceeds 0.25


# DDNM_METRICS: comma-separated metrics reported NEXT TO the PSNR (unset / empty = PSNR alone, today's output)
METRICS = ("ssim", "cons")
SSIM_MIN_SIZE = 11          # the 11x11 window needs one valid position


def extra_metrics(image_size=None):
    """The metrics DDNM_METRICS asks for, as a tuple of names out of METRICS; `image_size` (when given) is checked against
    what they need, so that a run that cannot report fails before its first image."""
    names = tuple(t.strip() for t in os.environ.get("DDNM_METRICS", "").split(",") if t.strip())
    for t in names:
        if t not in METRICS:
            raise ValueError(f"DDNM_METRICS: unknown metric {t!r}; accepted values: {', '.join(METRICS)}")
    if "ssim" in names and image_size is not None and image_size < SSIM_MIN_SIZE:
        raise ValueError(f"DDNM_METRICS=ssim needs images of at least {SSIM_MIN_SIZE} x {SSIM_MIN_SIZE} pixels, "
                         f"got image_size {image_size}")
    return names


class MetricLog:
    """PSNR (always) and SSIM (DDNM_METRICS=ssim) of the images one rank finishes: running sums for the printed means
    and, with the switch set, per-image values in the order the images were finished.  `index` names the IMAGE (the i
    of `Apy/orig_{i}.png`); the simplified runner writes that image's restoration as `{i - 1}_0.png`, like the
    reference."""

    def __init__(self, image_size, samples=1, ground_truth=True):
        names = extra_metrics(image_size)
        self.with_ssim = "ssim" in names
        # Cons (DDNM_METRICS=cons, and unasked in a run without ground truth, whose only figure of merit it is): per image
        # l1 / (2 n), the mean absolute residual of A x^ - y on the [0, 1] scale, and ConsMax = maxabs / 2 (add_cons)
        self.ground_truth = ground_truth
        self.with_cons = "cons" in names or not ground_truth
        self.cons_sum, self.all_cons_sum, self.cons_max, self.cons = 0.0, 0.0, 0.0, []
        self.psnr_sum, self.ssim_sum, self.n = 0.0, 0.0, 0
        self.index, self.psnr, self.ssim = [], [], []
        # DDNM_SAMPLES=K > 1: the posterior-mean image, all K samples, the mean standard deviation (add_samples)
        self.samples = samples
        self.mean_psnr_sum, self.all_psnr_sum, self.std_sum, self.mean_ssim_sum = 0.0, 0.0, 0.0, 0.0

    def add(self, x, x_orig, psnr, idx0):
        """One finished loader batch: x, x_orig on the [-1, 1] scale, `psnr` from ops.finalize_psnr; prints the lines."""
        b = x_orig.shape[0]
        self.psnr_sum += float(psnr.sum())
        self.n += b
        print("PSNR: %.2f" % (self.psnr_sum / self.n))
        if self.with_ssim:
            self.index += range(idx0, idx0 + b)
            self.psnr += psnr.double().cpu().tolist()
            s = ops.ssim(x, x_orig)
            self.ssim_sum += float(s.sum())
            self.ssim += s.cpu().tolist()
            print("SSIM: %.4f" % (self.ssim_sum / self.n))
        elif self.with_cons:
            self.index += range(idx0, idx0 + b)

    def count(self, b, idx0):
        """One finished loader batch of a run without ground truth: no PSNR / SSIM line, the images are counted."""
        self.n += b
        self.index += range(idx0, idx0 + b)

    def add_cons(self, l1, maxabs, sizes, sample):
        """ops.consistency's `l1`, `maxabs` [b] of sample `sample` of the loader batch `add` / `count` has just counted;
        `sizes` [b]: valid entries of each measurement row.  Sample 0 prints the `Cons:` line (running mean)."""
        cons = l1.double().cpu() / (2.0 * torch.tensor([float(n) for n in sizes], dtype=torch.float64))
        self.all_cons_sum += float(cons.sum())
        self.cons_max = max(self.cons_max, float(maxabs.max()) / 2.0)
        if sample == 0:
            self.cons_sum += float(cons.sum())
            self.cons += cons.tolist()
            print("Cons: %.3e" % (self.cons_sum / self.n))
        if self.samples > 1 and sample == self.samples - 1:
            print("Sample Cons: %.3e" % (self.all_cons_sum / (self.n * self.samples)))

    def add_samples(self, psnr_mean, psnr_all, std_mean, mean_img, x_orig):
        """The K-sample figures of the loader batch `add` has just counted (sample 0): `psnr_mean`, `std_mean` [b] and
        `mean_img` ([0, 1] scale) from ops.sample_stats, `psnr_all` [K, b] of every sample, x_orig on the [-1, 1] scale."""
        self.std_sum += float(std_mean.sum())
        if not self.ground_truth:                # no x_orig: the spread of the samples is all there is to say
            print("Std: %.4f" % (self.std_sum / self.n))
            return
        self.mean_psnr_sum += float(psnr_mean.sum())
        self.all_psnr_sum += float(psnr_all.double().sum())
        print("Mean-of-K PSNR: %.2f" % (self.mean_psnr_sum / self.n))
        print("Sample PSNR: %.2f" % (self.all_psnr_sum / (self.n * self.samples)))
        print("Std: %.4f" % (self.std_sum / self.n))
        if self.with_ssim:
            self.mean_ssim_sum += float(ops.ssim(mean_img, ops.finalize_psnr(x_orig)[0], transform=False).sum())
            print("Mean-of-K SSIM: %.4f" % (self.mean_ssim_sum / self.n))

    def total(self, rank, device, reduce):
        """Totals over the ranks (`reduce`: the sums live on several ranks) printed by rank 0; returns last_metrics."""
        if reduce:
            self.psnr_sum, self.n = ddist.reduce_sum(self.psnr_sum, device), int(ddist.reduce_sum(self.n, device))
            if self.with_ssim:
                self.ssim_sum = ddist.reduce_sum(self.ssim_sum, device)
            if self.samples > 1:
                self.mean_psnr_sum = ddist.reduce_sum(self.mean_psnr_sum, device)
                self.all_psnr_sum = ddist.reduce_sum(self.all_psnr_sum, device)
                self.std_sum = ddist.reduce_sum(self.std_sum, device)
                if self.with_ssim:
                    self.mean_ssim_sum = ddist.reduce_sum(self.mean_ssim_sum, device)
        if reduce and self.with_cons:
            self.cons_sum = ddist.reduce_sum(self.cons_sum, device)
            self.all_cons_sum = ddist.reduce_sum(self.all_cons_sum, device)
            self.cons_max = ddist.reduce_scalar(self.cons_max, device, "max")
        n = max(self.n, 1)
        if rank == 0:
            if self.ground_truth:
                print("Total Average PSNR: %.2f" % (self.psnr_sum / n))
            if self.with_ssim:
                print("Total Average SSIM: %.4f" % (self.ssim_sum / n))
            if self.with_cons:
                print("Total Average Cons: %.3e" % (self.cons_sum / n))
                print("Max Cons: %.3e" % self.cons_max)
            if self.samples > 1 and self.ground_truth:
                print("Total Average Mean-of-K PSNR: %.2f" % (self.mean_psnr_sum / n))
                print("Total Average Sample PSNR: %.2f" % (self.all_psnr_sum / (n * self.samples)))
                print("Total Average Std: %.4f" % (self.std_sum / n))
                if self.with_ssim:
                    print("Total Average Mean-of-K SSIM: %.4f" % (self.mean_ssim_sum / n))
            if self.samples > 1 and not self.ground_truth:
                print("Total Average Std: %.4f" % (self.std_sum / n))
            if self.samples > 1 and self.with_cons:
                print("Total Average Sample Cons: %.3e" % (self.all_cons_sum / (n * self.samples)))
            print("Number of samples: %d" % self.n)
            if self.samples > 1:
                print("Samples per image: %d" % self.samples)
        extra = {}
        if self.samples > 1:
            extra = {"samples": self.samples, "psnr_mean_image": self.mean_psnr_sum / n if self.ground_truth else None,
                     "psnr_all_samples": self.all_psnr_sum / (n * self.samples) if self.ground_truth else None,
                     "std": self.std_sum / n}
            if self.with_ssim:
                extra["ssim_mean_image"] = self.mean_ssim_sum / n
        if self.with_cons:      # the keys of a run that reports Cons; the runner's last_metrics holds None for the first two without
            extra.update(cons=self.cons_sum / n, cons_max=self.cons_max, cons_per_image=self.cons)
            if self.samples > 1:
                extra["cons_all_samples"] = self.all_cons_sum / (n * self.samples)
        return {**self._totals(n), **extra}

    def _totals(self, n):
        lists = self.with_ssim or self.with_cons
        return {"psnr": self.psnr_sum / n if self.ground_truth else None,
                "ssim": self.ssim_sum / n if self.with_ssim else None, "n": self.n,
                "index": self.index if lists else None, "psnr_per_image": self.psnr if self.with_ssim else None,
                "ssim_per_image": self.ssim if self.with_ssim else None}


# the simplified path pre-draws x_T and every loop iteration's ATen noise of a fused group (to replay the unfused draw
# order): (n_iter + 1) * K * C * S^2 * 4 bytes, kept under this bound by capping K (celeba / ADM at 256^2, T = 100:
# 79 MB per image, K <= 27)
SIMPLIFIED_TAPE_BYTES = 2 << 30


def fuse_groups(n_items, batch_size, rank, world, k):
    """Loader batches restored by `rank`, grouped into sampler calls: a list of groups, each a list of
    (batch index, index of its first image in the loader order, batch size).  Fusing needs whole loader batches per rank
    -- one rank, or deal mode (batch_size < world: batch bi belongs to rank bi % world) -- and takes up to `k`
    consecutive owned batches per group (the last group may be shorter).  Split mode (batch_size >= world > 1: every
    rank restores a slice of every batch) and k == 1 give one batch per group."""
    sizes = [min(batch_size, n_items - lo) for lo in range(0, n_items, batch_size)]
    starts = [i * batch_size for i in range(len(sizes))]
    deal = world > 1 and batch_size < world
    owned = [(bi, starts[bi], b) for bi, b in enumerate(sizes) if not deal or bi % world == rank]
    step = k if (world == 1 or deal) else 1
    return [owned[i:i + step] for i in range(0, len(owned), step)]


def restored_images(n_items, batch_size, rank, world, k, start=0):
    """Global image indices -- the i of `{i}_0.png`, `start` = --subset_start -- that each sampler call of `rank` restores,
    in call order: the whole batches of a fused group (one rank, deal mode) or this rank's slice [lo, hi) of one batch
    (split mode); a call without images (fewer images than ranks) is left out.  With a mask bank of N masks image i is
    restored with mask i % N, whichever call it lands in."""
    calls = []
    for group in fuse_groups(n_items, batch_size, rank, world, k):
        idx = []
        for _, first, b in group:
            lo, hi = rank_slice(b, batch_size, rank, world)
            idx += range(start + first + lo, start + first + hi)
        if idx:
            calls.append(idx)
    return calls


def rank_slice(b, batch_size, rank, world):
    """[lo, hi) of the `b` images of one loader batch that `rank` restores: its shard in split mode (batch_size >= world
    > 1), the whole batch otherwise (one rank, or deal mode: fuse_groups lists the batches a rank owns)."""
    return ddist.shard_range(b, rank, world) if world > 1 and batch_size >= world else (0, b)


# What one rank restores of one loader batch (Diffusion.svd_based_ddnm_plus): batch index `bi`, global index `idx0` of the
# batch's first image, batch size `b`, this rank's images [lo, hi) of it, `x_orig` [b] on the [-1, 1] scale, the
# measurement rows `y` [hi - lo], `x_T` [NS * (hi - lo)] ordered [sample k][image j], and `noise`: one source per sample
# (ops.PhiloxNoise with image_base = lo, or a BatchNoise tape under DDNM_NOISE=torch)
# For the writer's Cons and y/ files the part also keeps the whole batch: its measurement rows `y_all` [b], its operator `op`
# and the number of valid entries of every row, `valid` [b] (a mask bank pads its rows).  A run over given measurements has
# x_orig None.
Part = collections.namedtuple("Part", "bi idx0 b lo hi x_orig y x_T noise y_all op valid")


def _cat(tensors):
    """torch.cat along the rows that launches nothing for a single tensor."""
    return tensors[0] if len(tensors) == 1 else torch.cat(tensors, 0)


class Diffusion(object):
    def __init__(self, args, config, device=None):
        self.args, self.config = args, config
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("ddnm_amd needs an MI355X: the hot path has no CPU fallback")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.model_var_type = config.model.var_type
        betas = get_beta_schedule(beta_schedule=config.diffusion.beta_schedule, beta_start=config.diffusion.beta_start,
                                  beta_end=config.diffusion.beta_end,
                                  num_diffusion_timesteps=config.diffusion.num_diffusion_timesteps)
        self.betas = torch.from_numpy(betas).float().to(self.device)
        self.num_timesteps = self.betas.shape[0]

    # ------------------------------------------------------------------ model construction
    @staticmethod
    def _load_weights(net, ckpt, random_weights, announce=True):
        """The checkpoint `ckpt` if it exists, else `random_weights()` under DDNM_RANDOM_WEIGHTS=1, else an error
        (`announce=False`, the classifier: no line about the random weights, and the shorter error text)."""
        if os.path.exists(ckpt):
            net.load_state_dict(torch.load(ckpt, map_location="cpu"))
        elif os.environ.get("DDNM_RANDOM_WEIGHTS") == "1":
            if announce:
                print(f"[ddnm_amd] {ckpt} not found; DDNM_RANDOM_WEIGHTS=1 -> seeded random weights")
            net.load_state_dict(random_weights())
        else:
            place = "no network here: place the checkpoint there, or " if announce else ""
            raise FileNotFoundError(f"{ckpt} not found ({place}set DDNM_RANDOM_WEIGHTS=1 for seeded random weights)")

    def _build_model(self):
        cfg = self.config
        if cfg.model.type == "simple":
            model = Model(cfg, device=self.device)
            self._load_weights(model, simple_checkpoint_path(cfg, self.args.exp),
                               lambda: model.random_state_dict(self.args.seed))
            return model
        if cfg.model.type == "openai":
            from .unet import create_model
            model = create_model(**vars(cfg.model))
            model.device = self.device
            if cfg.model.use_fp16:
                model.convert_to_fp16()          # 3x3 torso convolutions on fp16 MFMA operands (unet.py here)
            if cfg.model.class_cond:
                ckpt = os.path.join(self.args.exp, "logs/imagenet/%dx%d_diffusion.pt" % (
                    cfg.data.image_size, cfg.data.image_size))
            else:
                ckpt = os.path.join(self.args.exp, "logs/imagenet/256x256_diffusion_uncond.pt")
            self._load_weights(model, ckpt, lambda: model.random_state_dict(self.args.seed))
            if cfg.model.class_cond:
                # noisy classifier + guidance gradient (diffusion.py:166-191)
                from .classifier import args_to_dict, classifier_defaults, create_classifier, make_cond_fn
                ckpt = os.path.join(self.args.exp, "logs/imagenet/%dx%d_classifier.pt" % (
                    cfg.data.image_size, cfg.data.image_size))
                classifier = create_classifier(**args_to_dict(cfg.classifier, classifier_defaults().keys()))
                classifier.device = self.device

                def random_classifier():
                    g = torch.Generator().manual_seed(self.args.seed + 1)
                    return {k: (torch.randn(v, generator=g) * (1.0 / max(1, int(np.prod(v[1:])))) ** 0.5 if len(v) > 1
                                else (1.0 + 0.1 * torch.randn(v, generator=g) if k.endswith("weight") else
                                      0.05 * torch.randn(v, generator=g)))
                            for k, v in classifier.state_dict_shapes().items()}

                self._load_weights(classifier, ckpt, random_classifier, announce=False)
                if cfg.classifier.classifier_use_fp16:
                    classifier.convert_to_fp16()
                self._cls_fn = make_cond_fn(classifier, cfg.classifier.classifier_scale)
            return model
        raise ValueError(cfg.model.type)

    def sample(self, simplified):
        check_samples(samples(), simplified)
        check_measurements(self.args, simplified)
        check_noise_flags(self.args, simplified)
        check_jpeg_flags(self.args, simplified)
        save_y()
        model = self._build_model()
        # batch sizes of 1 and 2 (the reference's shipped `sampling.batch_size: 1`) replay the forward from a hipGraph:
        # eager, the host needs longer to enqueue a forward's ~250-300 launches than the GPU to run them
        # (DDNM_GRAPH_MAX_BATCH=0 switches it off; bench.py `latency` reports both)
        model.auto_graphs(int(os.environ.get("DDNM_GRAPH_MAX_BATCH", "2")))
        tt = self.config.time_travel
        print(("Run Simplified DDNM, without SVD." if simplified else "Run SVD-based DDNM."),
              f"{tt.T_sampling} sampling steps.", f"travel_length = {tt.travel_length},",
              f"travel_repeat = {tt.travel_repeat}.", f"Task: {self.args.deg}.")
        cls_fn = getattr(self, "_cls_fn", None)
        if simplified:
            self.simplified_ddnm_plus(model, cls_fn)
        else:
            self.svd_based_ddnm_plus(model, cls_fn)

    # ------------------------------------------------------------------ data
    def _loader(self):
        args, config = self.args, self.config
        mdir = measurement_dir(args.path_y, args.exp)
        if mdir is not None:
            return self._measurement_loader(mdir)
        if str(args.path_y).startswith("synthetic"):
            n = int(str(args.path_y).split(":")[1]) if ":" in str(args.path_y) else config.sampling.batch_size
            ds = SyntheticImages(n, config.data.image_size, args.seed)
        elif config.data.dataset in ("CelebA_HQ", "FFHQ"):
            if getattr(config.data, "out_of_dist", False):          # datasets/__init__.py:137-143
                ds = ImageFolder(os.path.join(args.exp, "datasets", "ood_celeba"), config.data.image_size)
            else:
                ds = ImageFolder(os.path.join(args.exp, "datasets", args.path_y), config.data.image_size)
                # datasets/__init__.py:152-167: indices shuffled with numpy seed 2019, all of them are "test"
                idx = list(range(len(ds)))
                state = np.random.get_state()
                np.random.seed(2019)
                np.random.shuffle(idx)
                np.random.set_state(state)
                ds = data.Subset(ds, idx)
        elif config.data.dataset == "LSUN":
            if getattr(config.data, "out_of_dist", False):          # datasets/__init__.py:112-119
                ds = ImageFolder(os.path.join(args.exp, "datasets", f"ood_{config.data.category}"), config.data.image_size,
                                 transform="center_crop_arr")
            else:
                raise NotImplementedError("the LSUN lmdb validation sets (datasets/__init__.py:120-134) need the `lmdb` "
                                          "package; use out_of_dist: true with an image folder exp/datasets/ood_<category>")
        elif config.data.dataset == "ImageNet":
            if getattr(config.data, "subset_1k", False):
                # datasets/__init__.py:169-175: exp/imagenet_val_1k.txt lists "<file> <label>" under exp/datasets/imagenet/imagenet
                ds = ImageList(os.path.join(args.exp, "datasets", "imagenet", "imagenet"),
                               os.path.join(args.exp, "imagenet_val_1k.txt"), config.data.image_size)
            elif getattr(config.data, "out_of_dist", False):        # :176-183
                ds = ImageFolder(os.path.join(args.exp, "datasets", "ood"), config.data.image_size,
                                 transform="center_crop_arr")
            else:
                raise NotImplementedError("torchvision.datasets.ImageNet(split='val') (datasets/__init__.py:184-190) is "
                                          "not rebuilt here; use subset_1k: true or out_of_dist: true")
        else:
            raise NotImplementedError(f"dataset {config.data.dataset}")
        if args.subset_start >= 0 and args.subset_end > 0:
            assert args.subset_end > args.subset_start
            ds = data.Subset(ds, range(args.subset_start, args.subset_end))
        else:
            args.subset_start, args.subset_end = 0, len(ds)
        print(f"Dataset has size {len(ds)}")

        def seed_worker(worker_id):
            s = args.seed % 2 ** 32
            np.random.seed(s)
            random.seed(s)

        g = torch.Generator()
        g.manual_seed(args.seed)
        return data.DataLoader(ds, batch_size=config.sampling.batch_size, shuffle=True, num_workers=0,
                               worker_init_fn=seed_worker, generator=g)

    def _measurement_loader(self, root):
        """The loader of `--path_y measurements:DIR`: the folder's entries in their own order (no celeba index shuffle, no
        loader shuffle), position p = image --subset_start + p, at most --subset_end - --subset_start of them.  A batch
        is the list of its items (rows and pictures do not stack); the operator is bound by the SVD path."""
        args, config = self.args, self.config
        limit = None
        if args.subset_start >= 0 and args.subset_end > 0:
            assert args.subset_end > args.subset_start
            limit = args.subset_end - args.subset_start
        ds = MeasurementFolder(root, limit)
        ds.check_settings(run_settings(args, config, args.sigma_y))
        if limit is None:
            args.subset_start, args.subset_end = 0, len(ds)
        print(f"Dataset has size {len(ds)}")
        return data.DataLoader(ds, batch_size=config.sampling.batch_size, shuffle=False, num_workers=0, collate_fn=list)

    # ------------------------------------------------------------------ SVD path (diffusion.py:419-610)
    def _write_apy(self, A_funcs, y, x_orig, idx0):
        """`Apy/Apy_{i}.png` (A^+ y, or what the reference shows in its place for the task) and `Apy/orig_{i}.png` of one
        loader batch whose first image has the global index `idx0` (`x_orig` None, a run over given measurements: no
        orig file)."""
        args, config = self.args, self.config
        b, C, S = y.shape[0], config.data.channels, config.data.image_size
        Apy = A_funcs.A_pinv(y).view(b, C, S, S)
        if args.deg[:6] == "deblur":
            Apy = y.view(b, C, S, S)
        elif args.deg == "colorization":
            Apy = y.view(b, 1, S, S).repeat(1, 3, 1, 1)
        elif args.deg == "inpainting" or args.deg.startswith(DEMOSAIC):
            # entries that are not measured are shown black (a mosaic: each pixel in the colour it samples)
            Apy = Apy + A_funcs.A_pinv(A_funcs.A(torch.ones_like(Apy))).reshape(*Apy.shape) - 1
        for i in range(b):
            save_image(ops.finalize_psnr(Apy[i:i + 1].contiguous())[0][0],
                       os.path.join(args.image_folder, f"Apy/Apy_{idx0 + i}.png"))
            if x_orig is not None:
                save_image(ops.finalize_psnr(x_orig[i:i + 1])[0][0],
                           os.path.join(args.image_folder, f"Apy/orig_{idx0 + i}.png"))

    def svd_based_ddnm_plus(self, model, cls_fn):
        args, config = self.args, self.config
        loader = self._loader()
        A_funcs = build_operator(args.deg, args.deg_scale, config, self.device, jpeg_box=getattr(args, "jpeg_box", None))
        # --path_y measurements:DIR: y is given, there is no x_orig; every file is checked against the operator here
        measured = isinstance(loader.dataset, MeasurementFolder)
        if measured:
            loader.dataset.bind(A_funcs, config, args.subset_start)
        # --sigma_y_shot / --sigma_y_map: a per-entry NoiseModel in sigma_y's place (scalar: the float, as before)
        noise_model = noise_model_of(args, A_funcs)
        settings = run_settings(args, config, args.sigma_y, noise_model)
        if measured:
            loader.dataset.check_noise_settings(settings)
        args.sigma_y = 2 * args.sigma_y          # scaling to [-1, 1] (:524)
        sigma_y = args.sigma_y
        per_entry = not noise_model.is_scalar
        rank, world = ddist.world_state()      # the INITIALISED group (env-only sharding without a group loses shards)
        print(f"Start from {args.subset_start}")
        C, S, batch_size = config.data.channels, config.data.image_size, config.sampling.batch_size
        # DDNM_SAMPLES=NS: every measurement restored NS times in one sampler call, rows [sample k][image j], sample k with
        # the noise of a run under --seed seed + k and all of them with the one y of this run (NS = 1: the plain run)
        NS = samples()
        log = MetricLog(S, NS, ground_truth=not measured)
        os.makedirs(os.path.join(args.image_folder, "Apy"), exist_ok=True)      # (rank 0 made the image folder before the first barrier)
        # DDNM_SAVE_Y=1: the rows the sampler is given go to y/y_{i}.npy (written by the rank that writes Apy_{i}.png), the
        # settings they were formed with to y/measurements.json (rank 0, once)
        keep_y = save_y()
        if keep_y:
            import json
            os.makedirs(os.path.join(args.image_folder, "y"), exist_ok=True)
            if rank == 0:
                with open(os.path.join(args.image_folder, "y", MEASUREMENT_SETTINGS), "w") as f:
                    json.dump(settings, f, indent=1)
        if NS > 1:
            os.makedirs(os.path.join(args.image_folder, "mean"), exist_ok=True)
            os.makedirs(os.path.join(args.image_folder, "std"), exist_ok=True)
        # Sharding (one process per GPU): a loader batch of at least `world` images is split by image index and gathered once;
        # SMALLER batches -- every shipped config has sampling.batch_size 1 -- are dealt whole, round-robin, each rank writing
        # its own images (file names carry the global image index) and the PSNR reduced at the end (splitting a
        # batch of one left N - 1 GPUs idle).  Either way an image's result does not depend on the rank count: its noise is a
        # function of (seed, batch index, image index in the batch) only.
        deal = world > 1 and batch_size < world
        split = world > 1 and not deal
        writer = rank == 0 or deal
        philox = os.environ.get("DDNM_NOISE") != "torch"      # in-kernel Philox draws (default) | ATen tape (BatchNoise)
        # DDNM_FUSE_BATCHES=K: up to K consecutive loader batches of this rank restored in ONE sampler call (per-image
        # noise keys: each image draws what it draws alone); needs whole batches per rank
        K = fuse_batches()
        if K > 1 and split:
            print(f"[ddnm_amd] DDNM_FUSE_BATCHES={K} ignored: loader batches of {batch_size} images are "
                  f"split over {world} ranks")
        # the plan: the loader batches this rank restores, grouped into sampler calls (restored_images reads the same plan)
        groups = fuse_groups(len(loader.dataset), batch_size, rank, world, K)
        first = {bi: args.subset_start + start for group in groups for bi, start, _ in group}
        ends = {group[-1][0] for group in groups}
        # a mask bank (3-D mask.npy): every operator is built for the images of ITS rows, image i using mask i % N
        bank = A_funcs if isinstance(A_funcs, InpaintingBank) else None

        def given(items, A_batch):
            """The measurement rows [b, m] of a batch of MeasurementFolder items: an .npy row as it is, a picture
            flattened -- or, for inpainting, passed through A, which reads the kept pixels and pads a bank's row."""
            rows = []
            for j, (t, picture) in enumerate(items):
                t = t.to(self.device)
                if picture and args.deg == "inpainting":
                    t = (A_batch if bank is None else A_batch.narrow(j, j + 1)).A(t[None].contiguous())
                rows.append(t.reshape(1, -1))
            return _cat(rows).contiguous()

        def prepare(bi, batch):
            """The Part of loader batch `bi`: y = A x_orig of the whole batch (operators are cheap, and the writer needs
            A^+ y of all: the Apy/ files) -- or the given y of a run over measurements, which has no x_orig --, x_T and
            the noise sources of this rank's images [lo, hi) for every sample."""
            idx0, b = first[bi], len(batch)
            # (split mode: every rank sees the same batch -- same loader seed; rank r restores images [lo, hi) of it)
            x_orig = None if measured else data_transform(config, batch.to(self.device)).contiguous()
            lo, hi = rank_slice(b, batch_size, rank, world)
            if philox:
                # no ATen RNG launch in the loop, nothing drawn for other ranks' images: key = (seed + sample, batch),
                # counter = (element, iteration, image index in the batch); bench.py times this path
                noise = sample_sources(args.seed, bi, NS, lo)
                like = torch.empty(max(hi - lo, 1), C, S, S, device=self.device)
                x_T = _cat([src.tensor(ops.PhiloxNoise.XT_ITER, like)[:hi - lo] for src in noise])
            else:
                noise = [BatchNoise(args.seed + k, bi, b, (C, S, S), lo, hi, self.device) for k in range(NS)]
                x_T = _cat([tape.x_T() for tape in noise])
            A_batch = A_funcs if bank is None else bank.for_images(range(idx0, idx0 + b))
            y = given(batch, A_batch) if measured else A_batch.A(x_orig)
            if args.add_noise:
                # a per-entry model simulates itself: sigma_j of the CLEAN y (shot noise: the clean intensity), same draw
                std = noise_model.std(y.reshape(b, -1)).expand(b, -1).reshape(y.shape) if per_entry else sigma_y
                if philox:
                    y = y + measurement_noise(_mix64(args.seed, bi) ^ 0x5DEECE66D, y.reshape(b, -1)).reshape(y.shape) * std
                else:
                    y = y + noise[0].draw(tuple(y.shape)) * std
                    for tape in noise[1:]:
                        tape.draw(tuple(y.shape))    # the samples share y; each tape still moves as in its own run
            if writer:
                self._write_apy(A_batch, y, x_orig, idx0)
            y_all = y.reshape(b, -1)
            valid = A_batch.measurement_size() if bank is not None else [y_all.shape[1]] * b
            if writer and keep_y:
                rows = y_all.cpu().numpy()
                for j in range(b):
                    np.save(os.path.join(args.image_folder, "y", f"y_{idx0 + j}.npy"), rows[j, :valid[j]])
            return Part(bi, idx0, b, lo, hi, x_orig, y_all[lo:hi].contiguous(), x_T, noise, y_all, A_batch, valid)

        def restore(parts):
            """ONE sampler call for the loader batches `parts` (one batch, or a fused group), rows batch-major, then
            sample, then image (sample_rows); returns the rows of every part."""
            sizes = [p.hi - p.lo for p in parts]
            if not any(sizes):                   # empty shard (fewer images than ranks): takes part in the gather only
                return [p.x_T for p in parts]
            ys = [p.y.repeat(NS, 1) if NS > 1 else p.y for p in parts]      # the samples of an image share its y
            if len(parts) == 1 and NS == 1:      # the batch's own source: the unkeyed step kernels, no torch.cat per step
                noise = parts[0].noise[0]
            elif philox:
                noise = ops.KeyedPhiloxNoise.from_sources([(src, j) for p, n in zip(parts, sizes) for src in p.noise
                                                           for j in range(n)])
            else:
                noise = FusedTape([tape for p in parts for tape in p.noise])
            op = A_funcs
            if bank is not None:
                images = [i for p in parts for i in range(p.idx0 + p.lo, p.idx0 + p.hi)]
                op = bank.for_images(sample_rows(images, sizes, NS))
            x, y = _cat([p.x_T for p in parts]), _cat(ys)
            # noise-free: DDNM (diffusion.py:587-588); noisy: DDNM+, which takes sigma_y after y (:589-590).  classes=None:
            # the samplers take the class from the config, like the reference
            if per_entry:
                sampler, extra = ddnm_plus_diffusion, (noise_model,)
            else:
                sampler, extra = (ddnm_diffusion, ()) if sigma_y == 0.0 else (ddnm_plus_diffusion, (sigma_y,))
            with torch.no_grad():
                xs, _ = sampler(x, model, self.betas, args.eta, op, y, *extra, cls_fn=cls_fn, classes=None, config=config,
                                noise=noise, return_cpu=False)
            return torch.split(xs[0], [NS * n for n in sizes])

        def finish(p, x_rows):
            """The NS * (hi - lo) restorations of part `p`, rows [k][j] as the sampler leaves them: gathered if the batch
            is split over ranks; then every sample's PNG, sample 0's lines and, for NS > 1, the K-sample figures."""
            layout = "samples_major"
            if split:
                # [k][j] -> one row of NS * chw per image, so that the batch meets in ONE collective (the path's single
                # one, once per loader batch); every rank then holds [b][NS][chw]
                n = p.hi - p.lo
                rows = x_rows.reshape(NS, n, C * S * S).transpose(0, 1).reshape(n, NS * C * S * S)
                x_rows, layout = ddist.gather_images(rows, n_total=p.b).reshape(p.b * NS, C, S, S), "images_major"
            if not writer:
                return
            x_rows = x_rows.contiguous()
            xs = x_rows.view(NS, p.b, C, S, S) if layout == "samples_major" else x_rows.view(p.b, NS, C, S, S).transpose(0, 1)
            psnr_all = []
            for k in range(NS):
                x_k = xs[k].contiguous()
                img, psnr = ops.finalize_psnr(x_k, p.x_orig)
                for j in range(p.b):
                    save_image(img[j], os.path.join(args.image_folder, f"{p.idx0 + j}_{k}.png"))
                if k == 0 and measured:
                    log.count(p.b, p.idx0)
                elif k == 0:
                    log.add(x_k, p.x_orig, psnr, p.idx0)
                psnr_all.append(psnr)
                if log.with_cons:
                    # A applied to the sampler's final tensor (unclamped, [-1, 1] scale) against the y it was given
                    l1, _, maxabs = ops.consistency(p.op.A(x_k).reshape(p.b, -1), p.y_all,
                                                    p.valid if bank is not None else None)
                    log.add_cons(l1, maxabs, p.valid, k)
            if NS > 1:
                mean_img, std_img, psnr_mean, std_mean = ops.sample_stats(x_rows, p.b, NS, layout, p.x_orig)
                std_shown = (std_img * STD_DISPLAY_GAIN).clamp_(0.0, 1.0)
                for j in range(p.b):
                    save_image(mean_img[j], os.path.join(args.image_folder, f"mean/mean_{p.idx0 + j}.png"))
                    save_image(std_shown[j], os.path.join(args.image_folder, f"std/std_{p.idx0 + j}.png"))
                log.add_samples(psnr_mean, None if measured else torch.stack(psnr_all), std_mean, mean_img, p.x_orig)

        group = []
        # the batches of the plan: the images of a ground-truth batch, the list of items of a batch of given measurements
        for bi, batch in ((bi, x if measured else x[0]) for bi, x in enumerate(loader) if bi in first):
            group.append(prepare(bi, batch))
            if bi in ends:
                for p, x_rows in zip(group, restore(group)):     # one PSNR line per loader batch, in loader order
                    finish(p, x_rows)
                group = []
        # (cons / cons_max: None unless Cons was reported; psnr: None in a run over given measurements)
        self.last_metrics = {"cons": None, "cons_max": None, **log.total(rank, self.device, reduce=deal)}
        ddist.barrier()
        return self.last_metrics["psnr"]

    # ------------------------------------------------------------------ simplified path (diffusion.py:211-415)
    def _simplified_operator(self):
        args, config = self.args, self.config
        d, dev = config.data.image_size, self.device
        if args.deg == "colorization":
            return Colorization(d, dev, weights=(1 / 3, 1 / 3, 1 / 3))          # color2gray / gray2color :33-42
        if args.deg == "denoising":
            return Denoising(config.data.channels, d, dev)
        if args.deg == "sr_averagepooling":
            return SuperResolution(config.data.channels, d, round(args.deg_scale), dev)   # AdaptiveAvgPool2d / MeanUpsample
        if args.deg == "inpainting":
            mask = np.load("exp/inp_masks/mask.npy")
            if mask.ndim == 3:
                raise ValueError("per-image mask banks need the SVD path")
            return Inpainting(config.data.channels, d, missing_indices_of_mask(mask), dev)      # A = Ap = z * mask
        if args.deg.startswith(DEMOSAIC):                                                # A / Ap of the Mosaic operator
            return build_operator(args.deg, args.deg_scale, config, dev)
        if args.deg in ("mask_color_sr", "diy"):                                         # :260-290
            mask = torch.from_numpy(np.load("exp/inp_masks/mask.npy"))
            return mask_color_sr(config.data.channels, d, mask, round(args.deg_scale), dev)
        raise NotImplementedError("degradation type not supported")

    def simplified_ddnm_plus(self, model, cls_fn):
        args, config = self.args, self.config
        loader = self._loader()
        print("args.deg:", args.deg)
        op = self._simplified_operator()
        args.sigma_y = 2 * args.sigma_y
        sigma_y = args.sigma_y
        rank, world = ddist.world_state()      # the INITIALISED group (env-only sharding without a group loses shards)
        print(f"Start from {args.subset_start}")
        idx_so_far = args.subset_start
        log = MetricLog(config.data.image_size)
        os.makedirs(os.path.join(args.image_folder, "Apy"), exist_ok=True)
        # DDNM_FUSE_BATCHES=K: up to K of this rank's images in one loop.  The loop's noise is ATen's (torch.randn), so the
        # unfused draw order -- per image: x_T, then one draw per loop iteration -- is replayed into a tape up front
        tt = config.time_travel
        n_iter = len(get_schedule_jump(tt.T_sampling, tt.travel_length, tt.travel_repeat)) - 1
        per_image = (n_iter + 1) * config.data.channels * config.data.image_size ** 2 * 4
        K = min(fuse_batches(), max(1, SIMPLIFIED_TAPE_BYTES // per_image))
        group_ends = {g[-1][0] for g in fuse_groups(len(loader.dataset), 1, rank, world, K)} if K > 1 else set()
        pending = []

        def finish(x, x_orig, idx0, y):
            img, psnr = ops.finalize_psnr(x, x_orig)
            # the reference names the file with the stale loop variable j = -1 (:402); reproduced
            save_image(img[0], os.path.join(args.image_folder, f"{idx0 + (-1)}_{0}.png"))
            log.add(x, x_orig, psnr, idx0)
            if log.with_cons:
                y = y.reshape(1, -1).contiguous()
                l1, _, maxabs = ops.consistency(op.A(x).reshape(1, -1).contiguous(), y)
                log.add_cons(l1, maxabs, [y.shape[1]], 0)

        for bi, (x_orig, classes) in enumerate(loader):
            if config.sampling.batch_size != 1:
                raise ValueError("please change the config file to set batch size as 1")
            if bi % world != rank:               # batch size is 1 here (:308-309): whole images are dealt round-robin
                idx_so_far += x_orig.shape[0]
                continue
            x_orig = data_transform(config, x_orig.to(self.device)).contiguous()
            y = op.A(x_orig)
            Apy = op.A_pinv(y).view(*x_orig.shape)
            save_image(ops.finalize_psnr(Apy.contiguous())[0][0], os.path.join(args.image_folder, f"Apy/Apy_{idx_so_far}.png"))
            save_image(ops.finalize_psnr(x_orig)[0][0], os.path.join(args.image_folder, f"Apy/orig_{idx_so_far}.png"))
            x = torch.randn(y.shape[0], config.data.channels, config.data.image_size, config.data.image_size,
                            device=self.device)
            if K > 1:
                tape = [torch.randn_like(x) for _ in range(n_iter)]      # what simplified_loop would draw for this image
                pending.append((x, y.reshape(1, -1), tape, x_orig, idx_so_far))
                if bi in group_ends:
                    xf = simplified_loop(torch.cat([p[0] for p in pending], 0), model, self.betas, args.eta, op,
                                         torch.cat([p[1] for p in pending], 0), sigma_y, config,
                                         noise=FusedTape([p[2] for p in pending]))
                    for j, p in enumerate(pending):
                        finish(xf[j:j + 1].contiguous(), p[3], p[4], p[1])
                    pending = []
            else:
                x = simplified_loop(x, model, self.betas, args.eta, op, y, sigma_y, config)
                finish(x, x_orig, idx_so_far, y)
            idx_so_far += y.shape[0]
        self.last_metrics = {"cons": None, "cons_max": None, **log.total(rank, self.device, reduce=True)}
        return self.last_metrics["psnr"]


def simplified_loop(x, model, betas, eta, op, y, sigma_y, config, noise=None):
    """The loop inlined in the reference at diffusion.py:333-397: Eq. 19 lambda_t / gamma_t with
    sigma_t = sqrt(1 - alpha_bar'^2) (sic, :356) and the whole noise term scaled by gamma_t (:384)."""
    def step(it, xt, et, y, noise, x0_t, out):
        at_next = it.at_next
        sigma_t = (1 - at_next ** 2).sqrt()
        if sigma_t >= at_next * sigma_y:
            lambda_t = 1.0
            gamma_t = float((sigma_t ** 2 - (at_next * sigma_y) ** 2).sqrt())
        else:
            lambda_t = float(sigma_t / (at_next * sigma_y))
            gamma_t = 0.0
        s = ops.step_scalars(it.at, at_next, eta, lam=lambda_t, gamma=gamma_t)
        op.ddnm_step(xt, et, noise.kernel_arg(s, it.k), y, s, x0_t, out)

    # the noise is ATen's here, never the in-kernel draw: the runner replays its draw order into tapes when it fuses
    source = _AtenNoise(x) if noise is None else _TapeNoise(noise, x)
    return _reverse_loop(x, model, betas, y, config, source, step, begin=getattr(op, "begin_run", None))[0]
