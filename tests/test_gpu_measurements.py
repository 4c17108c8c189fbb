"""Measurements out and in on the GPU: a ground-truth run under DDNM_SAVE_Y=1 followed by a run over its y/ folder
(`--path_y measurements:DIR`) writes the same PNGs byte for byte -- alone, fused, with K samples and noisy measurements,
with a ragged mask bank --, a run from grey PNGs of one's own, and the Cons lines of DDNM_METRICS=cons against a hook on
ops.consistency.  The mini configuration of tests/test_gpu_fuse.py: random weights, synthetic images, T = 4."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_fuse import _mini_yaml
from tests.test_inpaint_masks_host import bank_masks

pytestmark = pytest.mark.gpu

SWITCHES = ("DDNM_SAVE_Y", "DDNM_FUSE_BATCHES", "DDNM_SAMPLES", "DDNM_METRICS", "DDNM_NOISE")


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    root = tmp_path_factory.mktemp("measurements")
    _mini_yaml(root)
    return str(root)


def _files(folder):
    """{relative path: bytes} of everything below `folder`."""
    out = {}
    for d, _, files in os.walk(folder):
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), folder)] = fh.read()
    return out


def _run(root, folder, argv, **env):
    """main.main([...]) in-process, in `root`, with the switches of `env` set and every other one unset.  Returns a dict:
    `out` (stdout), `files` ({relative path: bytes} of the image folder), `folder`, `cons` (arguments and results of every
    ops.consistency call), `metrics` (the runner's last_metrics)."""
    import main
    from ddnm_amd import ops
    from ddnm_amd.guided_diffusion.diffusion import Diffusion
    cons, runners = [], []
    orig_cons, orig_sample = ops.consistency, Diffusion.sample

    def consistency(ax, y, counts=None):
        res = orig_cons(ax, y, counts)
        cons.append(dict(ax=ax.detach().clone(), y=y.detach().clone(), counts=None if counts is None else list(counts),
                         l1=res[0].clone(), sse=res[1].clone(), maxabs=res[2].clone()))
        return res

    def sample(self, simplified):
        runners.append(self)
        return orig_sample(self, simplified)

    buf = io.StringIO()
    cwd = os.getcwd()
    with pytest.MonkeyPatch.context() as m:
        m.setattr(ops, "consistency", consistency)
        m.setattr(Diffusion, "sample", sample)
        m.setenv("DDNM_RANDOM_WEIGHTS", "1")
        for name in SWITCHES:
            if name in env:
                m.setenv(name, str(env[name]))
            else:
                m.delenv(name, raising=False)
        os.chdir(root)
        try:
            with contextlib.redirect_stdout(buf):
                rc = main.main(["--ni", "--config", "mini.yml", "-i", folder, "--eta", "0.85"] + argv)
        finally:
            os.chdir(cwd)
    out = buf.getvalue()
    assert rc == 0
    assert "Number of samples:" in out, out[-3000:]          # main logs an exception of the run and still returns 0
    path = os.path.join(root, "exp", "image_samples", folder)
    return dict(out=out, files=_files(path), folder=path, cons=cons, metrics=runners[0].last_metrics)


def _round_trip(root, name, argv_truth, argv_given, n, K=1, **env):
    """The ground-truth run under DDNM_SAVE_Y=1, then the run over its y/ folder: byte-equal restorations and Apy files,
    no orig files and no PSNR / SSIM line in the second run.  Returns both runs."""
    truth = _run(root, name + "_truth", ["--path_y", f"synthetic:{n}"] + argv_truth, DDNM_SAVE_Y=1, **env)
    ydir = os.path.join(truth["folder"], "y")
    assert sorted(os.listdir(ydir)) == sorted([f"y_{i}.npy" for i in range(n)] + ["measurements.json"])
    given = _run(root, name + "_given", ["--path_y", f"measurements:{ydir}"] + argv_given, **env)
    same = [f"{i}_{k}.png" for i in range(n) for k in range(K)] + [f"Apy/Apy_{i}.png" for i in range(n)]
    if K > 1:
        same += [f"mean/mean_{i}.png" for i in range(n)] + [f"std/std_{i}.png" for i in range(n)]
    for f in same:
        assert truth["files"][f] == given["files"][f], f
    assert sorted(given["files"]) == sorted(same), sorted(given["files"])              # no orig_{i}.png, no y/ folder
    assert sorted(f for f in truth["files"] if not f.startswith("y/")) == sorted(same + [f"Apy/orig_{i}.png" for i in range(n)])
    assert len({truth["files"][f"{i}_0.png"] for i in range(n)}) == n                  # the images differ
    assert "PSNR:" in truth["out"] and "Cons:" not in truth["out"]
    for head in ("PSNR", "SSIM", "Total Average PSNR"):
        assert head + ":" not in given["out"], given["out"][-2000:]
    assert f"Number of samples: {n}" in given["out"] and "Total Average Cons:" in given["out"] and "Max Cons:" in given["out"]
    assert given["metrics"]["psnr"] is None and given["metrics"]["n"] == n
    assert given["metrics"]["cons"] is not None and len(given["metrics"]["cons_per_image"]) == n
    assert truth["metrics"]["cons"] is None and truth["metrics"]["cons_max"] is None and truth["metrics"]["psnr"] > 0
    return truth, given


SR = ["--deg", "sr_averagepooling", "--deg_scale", "4", "--sigma_y", "0."]


@pytest.mark.parametrize("fuse", [None, 2])
def test_round_trip_sr(hip, workdir, fuse):
    """sr_averagepooling x4, batch 1, 3 images -- alone and under DDNM_FUSE_BATCHES=2; the saved rows are the 3 x 16 x 16
    values the sampler was given, measurements.json holds the settings."""
    env = {} if fuse is None else {"DDNM_FUSE_BATCHES": fuse}
    truth, given = _round_trip(workdir, f"sr_{fuse}", SR, SR, 3, **env)
    with open(os.path.join(truth["folder"], "y", "measurements.json")) as f:
        assert json.load(f) == {"deg": "sr_averagepooling", "deg_scale": 4.0, "image_size": 64, "channels": 3, "sigma_y": 0.0,
                                "add_noise": False, "seed": 1234}
    for i in range(3):
        row = np.load(os.path.join(truth["folder"], "y", f"y_{i}.npy"))
        assert row.dtype == np.float32 and row.shape == (3 * 16 * 16,) and np.isfinite(row).all()
    # the given run compared A x^ with exactly these rows
    assert len(given["cons"]) == 3
    for i, call in enumerate(given["cons"]):
        assert np.array_equal(call["y"].cpu().numpy()[0], np.load(os.path.join(truth["folder"], "y", f"y_{i}.npy")))


def test_round_trip_noisy_colorization_with_two_samples(hip, workdir):
    """colorization, --sigma_y 0.05 --add_noise, then --sigma_y 0.05 alone (DDNM+ on the given noisy y), DDNM_SAMPLES=2:
    both samples of every image, mean/ and std/ byte for byte."""
    noisy = ["--deg", "colorization", "--sigma_y", "0.05"]
    truth, given = _round_trip(workdir, "color", noisy + ["--add_noise"], noisy, 3, K=2, DDNM_SAMPLES=2)
    assert "Sample Cons:" in given["out"] and "Samples per image: 2" in given["out"]
    assert len(given["cons"]) == 6                                           # both samples of three batches
    assert np.load(os.path.join(truth["folder"], "y", "y_0.npy")).shape == (64 * 64,)


def test_round_trip_ragged_mask_bank(hip, workdir):
    """inpainting with a 3-mask bank keeping 2730 / 5 / 3871 pixels (rows of 8190 / 15 / 11613 values, none a multiple of
    4) over 4 images, two loader batches per sampler call: the saved rows drop the padding, the loaded ones get it back."""
    os.makedirs(os.path.join(workdir, "exp", "inp_masks"), exist_ok=True)
    np.save(os.path.join(workdir, "exp", "inp_masks", "mask.npy"), bank_masks(64))
    argv = ["--deg", "inpainting", "--sigma_y", "0."]
    truth, given = _round_trip(workdir, "bank", argv, argv, 4, DDNM_FUSE_BATCHES=2)
    sizes = [8190, 15, 11613, 8190]
    for i, n in enumerate(sizes):
        assert np.load(os.path.join(truth["folder"], "y", f"y_{i}.npy")).shape == (n,)
    assert [c["counts"] for c in given["cons"]] == [[n] for n in sizes]
    assert all(c["y"].shape == (1, 11616) for c in given["cons"])


def test_run_from_grey_pngs(hip, workdir):
    """colorization of two grey 8-bit pictures the test writes: the run completes, names its images 0 and 1 in the order
    of the files' numbers, prints no PSNR line, and Apy_{i}.png is the picture itself."""
    from PIL import Image
    src = os.path.join(workdir, "exp", "datasets", "grey")
    os.makedirs(src, exist_ok=True)
    rng = np.random.default_rng(5)
    pics = {"scan_10.png": rng.integers(0, 256, (64, 64), dtype=np.uint8), "scan_9.png": rng.integers(0, 256, (64, 64), dtype=np.uint8)}
    for name, arr in pics.items():
        Image.fromarray(arr).save(os.path.join(src, name))
    run = _run(workdir, "grey", ["--path_y", "measurements:grey", "--deg", "colorization", "--sigma_y", "0."])
    assert "PSNR:" not in run["out"] and "Number of samples: 2" in run["out"] and "Dataset has size 2" in run["out"]
    assert sorted(run["files"]) == ["0_0.png", "1_0.png", "Apy/Apy_0.png", "Apy/Apy_1.png"]
    for i, name in enumerate(("scan_9.png", "scan_10.png")):
        shown = np.asarray(Image.open(os.path.join(run["folder"], f"Apy/Apy_{i}.png")))
        assert np.array_equal(shown, np.repeat(pics[name][:, :, None], 3, 2)), name
    # the restoration is consistent with the picture it was given
    assert run["metrics"]["cons_max"] < 1e-3 and [c["y"].shape for c in run["cons"]] == [(1, 4096)] * 2


def test_a_folder_that_does_not_fit_is_refused_before_the_first_sampler_call(hip, workdir):
    """Rows of the wrong length: main logs the ValueError and writes no restoration."""
    import main
    from ddnm_amd.guided_diffusion.models import Model
    src = os.path.join(workdir, "exp", "datasets", "short")
    os.makedirs(src, exist_ok=True)
    np.save(os.path.join(src, "y_0.npy"), np.zeros(768, np.float32))
    np.save(os.path.join(src, "y_1.npy"), np.zeros(767, np.float32))
    cwd = os.getcwd()
    with pytest.MonkeyPatch.context() as m:
        m.setenv("DDNM_RANDOM_WEIGHTS", "1")
        for name in SWITCHES:
            m.delenv(name, raising=False)
        m.setattr(Model, "__call__", lambda self, x, t: pytest.fail("the network ran"))
        os.chdir(workdir)
        try:
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                main.main(["--ni", "--config", "mini.yml", "-i", "short", "--eta", "0.85", "--path_y", "measurements:short"] + SR)
        finally:
            os.chdir(cwd)
    assert "Number of samples:" not in buf.getvalue()
    assert not [f for f in _files(os.path.join(workdir, "exp", "image_samples", "short")) if f.endswith(".png")]


def test_cons_lines_come_from_ops_consistency(hip, workdir):
    """DDNM_METRICS=cons in a noise-free ground-truth run: one ops.consistency call per loader batch on (A x^, y); the
    printed `Cons:` values are the running means of l1 / (2 n); the hooked operands agree with float64 torch within
    m * 2^-52 (tests/test_gpu_consistency.py); ConsMax of every image is below 1e-3 -- a gross-error guard, 25 x the upper
    end of what the last step (alpha_bar' = 1) is recorded to leave, not a precision claim.  DDNM_SAVE_Y is unset: no y/."""
    from ddnm_amd.functions.svd_operators import SuperResolution
    run = _run(workdir, "cons", ["--path_y", "synthetic:3"] + SR, DDNM_METRICS="cons")
    assert not os.path.exists(os.path.join(run["folder"], "y")) and not any(f.startswith("y/") for f in run["files"])
    assert len(run["cons"]) == 3
    m = 3 * 16 * 16
    total, want_lines, per_image = 0.0, [], []
    op = SuperResolution(3, 64, 4, "cuda")
    for i, call in enumerate(run["cons"]):
        assert call["ax"].shape == call["y"].shape == (1, m) and call["counts"] is None
        d = call["ax"].double() - call["y"].double()
        for got, want in ((call["l1"], d.abs().sum(1)), (call["sse"], (d * d).sum(1))):
            assert bool(((got - want).abs() <= m * 2.0 ** -52 * want).all()), i
        assert torch.equal(call["maxabs"], d.abs().max(1).values.float())
        cons = call["l1"].double().cpu() / (2.0 * torch.tensor([float(m)], dtype=torch.float64))
        total += float(cons.sum())
        per_image += cons.tolist()
        want_lines.append("Cons: %.3e" % (total / (i + 1)))
        cons_max = float(call["maxabs"][0]) / 2
        print(f"image {i}: Cons {per_image[-1]:.3e}, ConsMax {cons_max:.3e}")
        assert cons_max < 1e-3, i
        # y is the measurement of the batch: A of its ground truth, which the runner wrote as Apy/orig_{i}.png (8 bit)
        from PIL import Image
        png = np.asarray(Image.open(os.path.join(run["folder"], f"Apy/orig_{i}.png")), dtype=np.float32) / 255
        shown = op.A(torch.from_numpy(png).permute(2, 0, 1)[None].cuda().contiguous() * 2 - 1)
        assert float((shown - call["y"]).abs().max()) < 1.5 / 255          # half a grey level per pixel, on [-1, 1]
    lines = [ln for ln in run["out"].splitlines() if ln.startswith("Cons: ")]
    assert lines == want_lines
    out = run["out"].splitlines()
    for i, ln in enumerate(out):
        if ln.startswith("Cons: "):
            assert out[i - 1].startswith("PSNR: ")                            # after the PSNR line of the batch
    assert "Total Average Cons: %.3e" % (total / 3) in out
    assert "Max Cons: %.3e" % max(float(c["maxabs"][0]) / 2 for c in run["cons"]) in out
    assert out.index("Total Average Cons: %.3e" % (total / 3)) > out.index([ln for ln in out if ln.startswith("Total Average PSNR")][0])
    met = run["metrics"]
    assert met["cons"] == total / 3 and met["cons_per_image"] == per_image and met["index"] == [0, 1, 2]
    assert met["cons_max"] == max(float(c["maxabs"][0]) / 2 for c in run["cons"])


def test_cons_in_the_simplified_runner(hip, workdir):
    """--simplified with DDNM_METRICS=cons: one ops.consistency call per image on (A x^, y) of the simplified operator, a
    `Cons:` line after each `PSNR:` line with the running mean of l1 / (2 n), the totals at the end."""
    run = _run(workdir, "cons_simplified", ["--path_y", "synthetic:2", "--deg", "colorization", "--sigma_y", "0.", "--simplified"],
               DDNM_METRICS="cons")
    assert len(run["cons"]) == 2 and all(c["ax"].shape == c["y"].shape == (1, 64 * 64) for c in run["cons"])
    total, want = 0.0, []
    for i, call in enumerate(run["cons"]):
        total += float((call["l1"].double().cpu() / (2.0 * 4096.0)).sum())
        want.append("Cons: %.3e" % (total / (i + 1)))
        print(f"simplified image {i}: ConsMax {float(call['maxabs'][0]) / 2:.3e}")
    out = run["out"].splitlines()
    assert [ln for ln in out if ln.startswith("Cons: ")] == want
    assert "Total Average Cons: %.3e" % (total / 2) in out and run["metrics"]["cons"] == total / 2
    assert run["metrics"]["cons_max"] == max(float(c["maxabs"][0]) / 2 for c in run["cons"])


def test_measurement_size_is_the_row_length_of_A_on_the_device(hip):
    """Every operator class at 32 x 32: measurement_size() is the row length of A(x) (a bank's rows: y_dim, of which
    measurement_size are valid and the rest exactly 0), measurement_image_shape() a CHW shape of as many values."""
    from ddnm_amd.functions import svd_operators as E
    d = 32
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(2, 3, d, d, generator=g) * 2 - 1).cuda()
    mask = (torch.rand(d * d, generator=g) < 0.4).float()
    r = torch.nonzero(mask == 0).long().reshape(-1) * 3
    k2, k1 = E.gaussian_taps(20, 4), E.gaussian_taps(1, 4)
    ops_ = [E.Denoising(3, d, "cuda"), E.SuperResolution(3, d, 4, "cuda"), E.Colorization(d, "cuda"),
            E.Inpainting(3, d, torch.cat([r, r + 1, r + 2], 0), "cuda"),
            E.WalshHadamardCS(3, d, 4, torch.randperm(d * d, generator=g), "cuda"),
            E.CS(3, d, 0.25, "cuda", gauss=torch.randn(1024, 1024, generator=g)),
            E.PixelMask(3, d, mask, "cuda"), E.mask_color_sr(3, d, mask, 4, "cuda"),
            E.GeneralA(torch.randn(7, 3 * d * d, generator=g)), E.SRConv(E.bicubic_kernel(4), 3, d, "cuda", stride=4),
            E.Deblurring2D(k1 / k1.sum(), k2 / k2.sum(), 3, d, "cuda"), E.Deblurring(torch.Tensor([1 / 9] * 9), 3, d, "cuda")]
    for op in ops_:
        y = op.A(x).reshape(2, -1)
        assert op.measurement_size() == y.shape[1], type(op).__name__
        shape = op.measurement_image_shape()
        if shape is not None and not isinstance(op, E.Inpainting):
            assert int(np.prod(shape)) == y.shape[1], type(op).__name__
    bank = E.InpaintingBank(3, d, bank_masks(d), "cuda")
    per_image = bank.for_images([1, 2])
    y = per_image.A(x)
    assert y.shape == (2, bank.y_dim) and per_image.measurement_size() == [bank.measurement_size(1), bank.measurement_size(2)]
    for b, n in enumerate(per_image.measurement_size()):
        assert bool((y[b, n:] == 0).all()) and bool((y[b, :n] != 0).any())
