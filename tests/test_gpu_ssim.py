"""SSIM on the GPU: ddnm_ssim_f32 against the float64 model of tests/test_ssim_host.py, its independence of the batch,
the transform, the runner's DDNM_METRICS=ssim switch and the folder evaluator."""
import contextlib
import io
import json
import os
import re

import numpy as np
import pytest
import torch

from tests.test_gpu_fuse import _mini_yaml, _run_main
from tests.test_ssim_host import ssim_f64

pytestmark = pytest.mark.gpu

# The kernel accumulates the moments in fp64 from exact fp64 products of the fp32 pixels, so what is left against the model
# is the order of the fp64 sums (rounding residue of the variances against C2 = 9e-4).  Measured on the MI355X over every
# case below (printed by the test): max |ssim_gpu - ssim_f64| = 3.7e-13, at (1, 1, 11, 11) on the near-constant pair; the
# bar is 10x that = 3.7e-12, far below the 1e-5 it may never exceed.
MEASURED = 3.7e-13
BAR = 10 * MEASURED
assert BAR <= 1e-5

# (B, C, H, W): one valid position; 2 x 2 positions; one 32 x 16 tile exactly and a one-pixel second tile in both axes;
# 32 x 32 and 33 x 33 positions; several tiles and images; non-square; the shipped image size
SHAPES = [(1, 1, 11, 11), (2, 3, 12, 12), (1, 3, 26, 42), (1, 3, 27, 43), (1, 3, 42, 42), (1, 3, 43, 43), (3, 3, 64, 64),
          (2, 1, 40, 75)]
KINDS = ["noise", "smooth_1pct", "smooth_10pct", "identical", "const_03_07", "black_white", "flat_09"]


def _smooth(shape):
    B, C, H, W = shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    b, c = np.arange(B).reshape(B, 1, 1, 1), np.arange(C).reshape(1, C, 1, 1)
    return 0.5 + 0.25 * np.sin(0.21 * xx + 0.7 * c + b) + 0.2 * np.cos(0.13 * yy - 0.4 * c)


def make_pair(kind, shape, seed):
    """Two float32 images on the [0, 1] scale."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        x, y = rng.random(shape), rng.random(shape)
    elif kind in ("smooth_1pct", "smooth_10pct"):
        y = _smooth(shape)
        x = np.clip(y + (0.01 if kind == "smooth_1pct" else 0.1) * rng.standard_normal(shape), 0.0, 1.0)
    elif kind == "identical":
        x = y = rng.random(shape)
    elif kind == "const_03_07":
        x, y = np.full(shape, 0.3), np.full(shape, 0.7)
    elif kind == "black_white":
        x, y = np.zeros(shape), np.ones(shape)
    elif kind == "flat_09":
        y = np.full(shape, 0.9)
        x = np.clip(y + 1e-3 * rng.standard_normal(shape), 0.0, 1.0)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)


def _gpu(x, y, transform):
    from ddnm_amd import ops
    return ops.ssim(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), transform=transform).cpu().numpy()


def _errors(kind, shape, seed):
    """|gpu - model| for transform=False on the images and for transform=True on 2v - 1 (the model then sees what the
    kernel sees: clamp((t + 1) / 2, 0, 1) evaluated in fp32), and the GPU values."""
    x, y = make_pair(kind, shape, seed)
    got = _gpu(x, y, False)
    assert got.dtype == np.float64 and got.shape == (shape[0],)
    e0 = np.abs(got - ssim_f64(x, y)).max()
    tx, ty = 2 * x - np.float32(1), 2 * y - np.float32(1)
    back = lambda t: np.clip((t + np.float32(1)) / np.float32(2), 0, 1).astype(np.float32)      # noqa: E731
    got_t = _gpu(tx, ty, True)
    e1 = np.abs(got_t - ssim_f64(back(tx), back(ty))).max()
    return max(e0, e1), got, got_t


def test_kernel_matches_the_float64_model(hip):
    worst, where = 0.0, None
    for si, shape in enumerate(SHAPES):
        for ki, kind in enumerate(KINDS):
            err, got, got_t = _errors(kind, shape, 100 * si + ki)
            if kind == "identical":
                assert np.abs(got - 1).max() <= 1e-6 and np.abs(got_t - 1).max() <= 1e-6, (shape, got, got_t)
            if err > worst:
                worst, where = err, (shape, kind)
    err, _, _ = _errors("smooth_1pct", (1, 3, 256, 256), 999)            # the large shape once
    if err > worst:
        worst, where = err, ((1, 3, 256, 256), "smooth_1pct")
    print(f"ssim kernel vs float64 model: max |diff| = {worst:.3e} at {where} (bar {BAR:.1e})")
    assert worst <= BAR, (worst, where)


def test_flat_images_keep_four_decimals(hip):
    """The pairs whose variance a plain fp32 formulation loses against C2 (1e-4 off): closed forms of the constants."""
    c1 = 0.01 ** 2
    a, b = np.float64(np.float32(0.3)), np.float64(np.float32(0.7))
    x, y = make_pair("const_03_07", (1, 3, 43, 43), 0)
    assert abs(_gpu(x, y, False)[0] - (2 * a * b + c1) / (a * a + b * b + c1)) < 1e-12
    x, y = make_pair("black_white", (1, 3, 43, 43), 0)
    assert abs(_gpu(x, y, False)[0] - c1 / (1 + c1)) < 1e-12


@pytest.mark.parametrize("shape", [(3, 3, 64, 64), (1, 3, 43, 43)])
def test_value_does_not_depend_on_the_batch(hip, shape):
    """Alone, first, last, and after a different first image: the same double, bit for bit."""
    from ddnm_amd import ops
    x, y = (torch.from_numpy(a).cuda() for a in make_pair("smooth_10pct", shape, 7))
    ox, oy = (torch.from_numpy(a).cuda() for a in make_pair("noise", (2,) + shape[1:], 8))
    whole = ops.ssim(x, y, transform=False)
    for i in range(shape[0]):
        xi, yi = x[i:i + 1].contiguous(), y[i:i + 1].contiguous()
        alone = ops.ssim(xi, yi, transform=False)
        first = ops.ssim(torch.cat([xi, ox]), torch.cat([yi, oy]), transform=False)
        last = ops.ssim(torch.cat([ox, xi]), torch.cat([oy, yi]), transform=False)
        other = ops.ssim(torch.cat([ox[1:], xi, ox[:1]]), torch.cat([oy[1:], yi, oy[:1]]), transform=False)
        torch.cuda.synchronize()
        for name, v in (("batch", whole[i]), ("first", first[0]), ("last", last[2]), ("after another", other[1])):
            assert torch.equal(v, alone[0]), (i, name, float(v), float(alone[0]))


def test_transform_is_the_one_of_finalize_psnr(hip):
    from ddnm_amd import ops
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(2, 3, 40, 75, generator=g) * 0.8).cuda()          # part of it outside [-1, 1]: the clamp acts
    xo = (torch.rand(2, 3, 40, 75, generator=g) * 2 - 1).cuda()
    img_x, _ = ops.finalize_psnr(x, xo)
    img_xo, _ = ops.finalize_psnr(xo)
    a, b = ops.ssim(x, xo, transform=True), ops.ssim(img_x, img_xo, transform=False)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and a.dtype == torch.float64 and bool((a.abs() < 1).all())


def test_bad_shapes_raise(hip):
    from ddnm_amd import ops
    from ddnm_amd._lib import DDNMHipError
    z = torch.zeros(1, 3, 10, 32, device="cuda")
    with pytest.raises(DDNMHipError):
        ops.ssim(z, z)
    with pytest.raises(ValueError):
        ops.ssim(torch.zeros(1, 3, 16, 16, device="cuda"), torch.zeros(1, 3, 16, 17, device="cuda"))


# ------------------------------------------------------------------------------------------------ runner and evaluator
ARGV = ["--eta", "0.85", "--sigma_y", "0.", "--deg", "sr_averagepooling", "--deg_scale", "4"]


class _Run:
    def __init__(self, tmp, mp, folder, n, metrics, fuse=None, simplified=False):
        """One in-process `main.main` on synthetic:n at 64 x 64 with T = 4, ops.ssim wrapped to keep its arguments."""
        from ddnm_amd import ops
        self.calls = []
        orig = ops.ssim

        def spy(x, x_orig, transform=True):
            out = orig(x, x_orig, transform)
            self.calls.append((x.detach().clone(), x_orig.detach().clone(), out.cpu()))
            return out

        buf = io.StringIO()
        with mp.context() as m, contextlib.redirect_stdout(buf):
            m.setattr(ops, "ssim", spy)
            if metrics is None:
                m.delenv("DDNM_METRICS", raising=False)
            else:
                m.setenv("DDNM_METRICS", metrics)
            argv = ["--path_y", f"synthetic:{n}"] + ARGV + (["--simplified"] if simplified else [])
            _, self.psnr, self.imgs, self.names, self.apy = _run_main(tmp, mp, folder, argv, fuse)
        self.out = buf.getvalue()
        self.dir = tmp / "exp" / "image_samples" / folder
        self.lines = self.out.splitlines()
        self.psnr_lines = [ln for ln in self.lines if "PSNR" in ln]

    def png_bytes(self):
        files = sorted(self.dir.glob("*.png")) + sorted((self.dir / "Apy").glob("*.png"))
        return {str(p.relative_to(self.dir)): p.read_bytes() for p in files}


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    """The runner once per configuration; the tests below only read what these runs left."""
    tmp = tmp_path_factory.mktemp("ssim_runner")
    mp = pytest.MonkeyPatch()
    try:
        _mini_yaml(tmp)
        mp.chdir(tmp)
        mp.setenv("DDNM_GPUS", "1")              # stay in this process (set before the function-scoped autouse fixture runs)
        yield {"plain": _Run(tmp, mp, "plain", 3, None), "again": _Run(tmp, mp, "again", 3, None),
               "ssim": _Run(tmp, mp, "ssim", 3, "ssim"), "fused": _Run(tmp, mp, "fused", 3, "ssim", fuse=2),
               "simplified": _Run(tmp, mp, "simplified", 2, "ssim", simplified=True)}
    finally:
        mp.undo()


def test_runner_without_the_switch_is_unchanged(runs):
    a, b = runs["plain"], runs["again"]
    assert "SSIM" not in a.out and "SSIM" not in b.out and not a.calls and not b.calls
    assert "Number of samples: 3" in a.out and len(a.psnr_lines) == 4
    assert a.psnr_lines == b.psnr_lines and a.png_bytes() == b.png_bytes() and len(a.png_bytes()) == 9


def test_runner_with_the_switch_adds_the_ssim_lines_only(runs):
    a, s = runs["plain"], runs["ssim"]
    assert s.psnr_lines == a.psnr_lines and s.png_bytes() == a.png_bytes()
    for i, ln in enumerate(s.lines):
        if ln.startswith("PSNR: "):
            assert re.fullmatch(r"SSIM: -?\d\.\d{4}", s.lines[i + 1]), s.lines[i:i + 2]
        if ln.startswith("Total Average PSNR: "):
            assert s.lines[i + 1].startswith("Total Average SSIM: ")
    assert sum(ln.startswith("SSIM: ") for ln in s.lines) == 3 and s.out.count("Total Average SSIM: ") == 1
    # the printed total is the mean of ops.ssim over the restored and original tensors the runner handed over
    from ddnm_amd import ops
    assert len(s.calls) == 3 and torch.equal(torch.cat([c[0] for c in s.calls]), s.imgs)
    values = torch.cat([ops.ssim(x, xo).cpu() for x, xo, _ in s.calls])
    assert torch.equal(values, torch.cat([c[2] for c in s.calls]))
    total = float(s.out.split("Total Average SSIM:")[1].split()[0])
    assert abs(total - float(values.mean())) <= 5e-5
    running = [float(ln.split()[1]) for ln in s.lines if ln.startswith("SSIM: ")]
    for k, r in enumerate(running):
        assert abs(r - float(values[:k + 1].mean())) <= 5e-5


def test_fused_run_reports_the_unfused_ssim_per_image(runs):
    s, f = runs["ssim"], runs["fused"]
    assert f.psnr.shape == s.psnr.shape == (3,) and f.names == s.names
    one, two = torch.cat([c[2] for c in s.calls]), torch.cat([c[2] for c in f.calls])
    assert one.shape == two.shape == (3,)
    print(f"fused K=2 vs unfused per-image SSIM: max |diff| = {float((one - two).abs().max()):.3e}")
    assert (one - two).abs().max() < 1e-3
    assert sum(ln.startswith("SSIM: ") for ln in f.lines) == 3 and f.out.count("Total Average SSIM: ") == 1


def test_simplified_run_with_the_switch(runs):
    r = runs["simplified"]
    assert "Number of samples: 2" in r.out and r.names == ["-1_0.png", "0_0.png"]
    assert sum(ln.startswith("SSIM: ") for ln in r.lines) == 2 and r.out.count("Total Average SSIM: ") == 1
    values = torch.cat([c[2] for c in r.calls])
    total = float(r.out.split("Total Average SSIM:")[1].split()[0])
    assert values.shape == (2,) and abs(total - float(values.mean())) <= 5e-5
    i = r.lines.index(next(ln for ln in r.lines if ln.startswith("Total Average PSNR: ")))
    assert r.lines[i + 1].startswith("Total Average SSIM: ") and r.lines[i + 2] == "Number of samples: 2"


def _png(path):
    from PIL import Image
    u = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
    return (u.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)[None]


def _evaluate(argv):
    from ddnm_amd import evaluate
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert evaluate.main(argv) == 0
    return buf.getvalue().splitlines()


@pytest.mark.parametrize("against", ["restored", "Apy"])
def test_evaluator_on_the_folder_the_runner_wrote(runs, tmp_path, against):
    import shutil
    folder = tmp_path / "run"
    shutil.copytree(runs["ssim"].dir, folder)                             # three images; one side of one index removed
    if against == "restored":
        os.remove(folder / "2_0.png")
        want_idx, skipped = [0, 1], ["skipped (no restored file): 2"]
    else:
        os.remove(folder / "Apy" / "Apy_1.png")
        want_idx, skipped = [0, 2], ["skipped (no Apy file): 1"]
    out = _evaluate([str(folder), "--against", against, "--json", str(tmp_path / "m.json")])
    assert out[:1] == skipped
    rows = [ln.split() for ln in out[1:1 + len(want_idx)]]
    assert [int(r[0]) for r in rows] == want_idx
    doc = json.load(open(tmp_path / "m.json"))
    assert doc["against"] == against and doc["n"] == 2 and [im["index"] for im in doc["images"]] == want_idx
    for r, im in zip(rows, doc["images"]):
        i = im["index"]
        ref = _png(folder / "Apy" / f"orig_{i}.png")
        img = _png(folder / (f"{i}_0.png" if against == "restored" else f"Apy/Apy_{i}.png"))
        assert abs(im["ssim"] - ssim_f64(img, ref)[0]) <= BAR
        mse = np.mean((img.astype(np.float64) - ref.astype(np.float64)) ** 2)
        assert abs(im["psnr"] - 10 * np.log10(1 / mse)) <= 1e-3
        assert r[1] == "%.2f" % im["psnr"] and r[2] == "%.4f" % im["ssim"]
    assert out[-3:] == ["Average PSNR: %.2f" % doc["psnr"], "Average SSIM: %.4f" % doc["ssim"], "Number of images: 2"]
    assert abs(doc["ssim"] - np.mean([im["ssim"] for im in doc["images"]])) < 1e-15
