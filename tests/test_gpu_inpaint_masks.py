"""Per-image inpainting masks on the GPU: a batch whose images each have their own hole (InpaintingBank /
PerImageInpainting, the `*_pi_*` entry points) computes, image by image, what the existing single-mask Inpainting
computes for that image alone -- operators, the fused step and Lambda / Lambda_noise bit for bit, the samplers and the
runner within the bar of batched-versus-separate restoration (tests/test_gpu_fuse.py::BAR: the forward need not be
batch-invariant, nothing else may differ)."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import rel
from tests.test_gpu_fuse import BAR, CTRS, KEYS, _mini_yaml, _run_main, _small_net, _sources
from tests.test_inpaint_masks_host import bank_masks, check_pi_validation, single_mask_operator

pytestmark = pytest.mark.gpu

D, ORDER = 32, [2, 0, 1]


@pytest.fixture(scope="module")
def case(hip):
    """The bank of three masks at 32 px, its operator for the images [2, 0, 1], the single-mask operator of each of
    those images, and seeded inputs -- built once, never written to."""
    from ddnm_amd.functions import svd_operators as E
    masks = bank_masks(D)
    bank = E.InpaintingBank(3, D, masks, "cuda")
    g = torch.Generator().manual_seed(17)
    c = dict(masks=masks, bank=bank, op=bank.for_images(ORDER), singles=[single_mask_operator(masks[r], D, "cuda") for r in ORDER])
    c["x"] = (torch.rand(3, 3, D, D, generator=g) * 2 - 1).cuda()
    c["xt"] = torch.randn(3, 3, D, D, generator=g).cuda()
    c["et6"] = torch.randn(3, 6, D, D, generator=g).cuda()
    c["et3"] = c["et6"][:, :3].contiguous()
    c["noise"] = torch.randn(3, 3, D, D, generator=g).cuda()
    return c


def test_A_and_A_pinv_match_the_single_mask_operator_per_image(case):
    op, x = case["op"], case["x"]
    assert len(op) == 3 and op.y_dim == 2400 and op.n_kept == [799, 682, 5]
    y = op.A(x)
    xp = op.A_pinv(y)
    # A^+ must not read the padding: poison it
    yp = y.clone()
    for b, n in enumerate(op.n_kept):
        yp[b, 3 * n:] = float("nan")
    xp_poison = op.A_pinv(yp)
    torch.cuda.synchronize()
    assert y.shape == (3, 2400) and xp.shape == (3, 3 * D * D)
    for b, one in enumerate(case["singles"]):
        n = 3 * op.n_kept[b]
        y1 = one.A(x[b:b + 1])
        assert torch.equal(y[b, :n], y1[0]), b
        assert bool((y[b, n:] == 0).all()) and n < 2400, b
        assert torch.equal(xp[b:b + 1], one.A_pinv(y1)), b
        assert torch.equal(xp_poison[b], xp[b]), b


def _noise_for(kind, noise):
    """(noise argument and scalar stamp of the batched step, the same for image i alone)."""
    from ddnm_amd import ops
    if kind == "tensor":
        return noise, (lambda s: s), (lambda i: noise[i:i + 1].contiguous()), (lambda i, s: s)
    if kind == "philox":
        src = ops.PhiloxNoise(KEYS[1], image_base=4)
        return None, (lambda s: src.stamp(s, 9)), (lambda i: None), \
            (lambda i, s: ops.PhiloxNoise(KEYS[1], image_base=4 + i).stamp(s, 9))
    kn = ops.KeyedPhiloxNoise(KEYS, CTRS)
    return kn, (lambda s: kn.stamp(s, 9)), (lambda i: None), (lambda i, s: _sources()[i].stamp(s, 9))


def _scalars():
    from ddnm_amd import ops
    return ops.step_scalars(torch.tensor(0.5), torch.tensor(0.6), 0.85)


@pytest.mark.parametrize("noise_kind", ["tensor", "philox", "keyed"])
@pytest.mark.parametrize("learn_sigma", [False, True])
def test_step_matches_the_single_mask_step_per_image(case, noise_kind, learn_sigma):
    """B = 3 in image order [2, 0, 1]: x0 and x_t' of image b == Inpainting(mask of image b).ddnm_step on that image alone
    with that image's noise source (the construction of test_gpu_fuse::test_keyed_step_equals_unkeyed_per_image)."""
    op, xt = case["op"], case["xt"]
    et = case["et6"][:, :3] if learn_sigma else case["et3"]
    y = op.A(case["x"])
    nz, stamp, nz_i, stamp_i = _noise_for(noise_kind, case["noise"])
    x0_b, xn_b = torch.empty_like(xt), torch.empty_like(xt)
    op.ddnm_step(xt, et, nz, y, stamp(_scalars()), x0_b, xn_b)
    for i, one in enumerate(case["singles"]):
        x0_i, xn_i = torch.empty_like(xt[:1]), torch.empty_like(xt[:1])
        one.ddnm_step(xt[i:i + 1].contiguous(), et[i:i + 1], nz_i(i), one.A(case["x"][i:i + 1]), stamp_i(i, _scalars()),
                      x0_i, xn_i)
        torch.cuda.synchronize()
        assert torch.equal(x0_b[i:i + 1], x0_i), i
        assert torch.equal(xn_b[i:i + 1], xn_i), i
    assert torch.isfinite(xn_b).all()


@pytest.mark.parametrize("noise_kind", ["tensor", "keyed"])
def test_identical_masks_equal_the_shared_mask_operator(case, noise_kind):
    from ddnm_amd.functions import svd_operators as E
    m0 = case["masks"][0]
    op = E.InpaintingBank(3, D, np.stack([m0, m0, m0]), "cuda").for_images([0, 1, 2])
    shared = single_mask_operator(m0, D, "cuda")
    x, xt, et = case["x"], case["xt"], case["et6"][:, :3]
    n = 3 * shared.n_kept
    y, ys = op.A(x), shared.A(x)
    assert torch.equal(y[:, :n], ys) and bool((y[:, n:] == 0).all())
    assert torch.equal(op.A_pinv(y), shared.A_pinv(ys))
    nz, stamp, _, _ = _noise_for(noise_kind, case["noise"])
    out = [torch.empty_like(xt) for _ in range(4)]
    op.ddnm_step(xt, et, nz, y, stamp(_scalars()), out[0], out[1])
    shared.ddnm_step(xt, et, nz, ys, stamp(_scalars()), out[2], out[3])
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[2]) and torch.equal(out[1], out[3])


@pytest.mark.parametrize("sigma_t", [0.1, 0.5])
def test_lambda_and_lambda_noise_match_per_image(case, sigma_t):
    """sigma_y = 0.2, a = 0.9: sigma_t = 0.1 is below a * sigma_y = 0.18 (lambda < 1), 0.5 above it."""
    op, v, eps = case["op"], case["xt"], case["et3"]
    a, sigma_y, eta = 0.9, 0.2, 0.85
    lam = op.Lambda(v, a, sigma_y, sigma_t, eta)
    lnz = op.Lambda_noise(case["noise"], a, sigma_y, sigma_t, eta, eps)
    torch.cuda.synchronize()
    assert lam.shape == lnz.shape == (3, 3 * D * D)
    for i, one in enumerate(case["singles"]):
        assert torch.equal(lam[i:i + 1], one.Lambda(v[i:i + 1].contiguous(), a, sigma_y, sigma_t, eta)), i
        assert torch.equal(lnz[i:i + 1], one.Lambda_noise(case["noise"][i:i + 1].contiguous(), a, sigma_y, sigma_t, eta,
                                                          eps[i:i + 1].contiguous())), i


@pytest.mark.parametrize("plus", [False, True])
def test_samplers_match_three_single_mask_calls(case, plus):
    """Three images with per-image masks and keyed noise in one sampler call == three calls of one image with
    Inpainting(mask of that image).  Measured rel-L2 on the MI355X (printed): 0 for DDNM and for DDNM+."""
    from ddnm_amd import ops
    from ddnm_amd.functions.svd_ddnm import ddnm_diffusion, ddnm_plus_diffusion
    from oracle import cases
    cfg, model = _small_net()
    cfg.time_travel.T_sampling, cfg.time_travel.travel_length, cfg.time_travel.travel_repeat = 5, 1, 2
    assert cfg.data.image_size == D
    op = case["op"]
    y = op.A(case["x"])
    betas = cases.betas().cuda()
    kn = ops.KeyedPhiloxNoise(KEYS, CTRS)
    x = kn.tensor(ops.PhiloxNoise.XT_ITER, torch.empty(3, 3, D, D, device="cuda"))

    def run(xx, A, yy, noise):
        if plus:
            return ddnm_plus_diffusion(xx, model, betas, 0.85, A, yy, 0.2, config=cfg, noise=noise, return_cpu=False)[0][0]
        return ddnm_diffusion(xx, model, betas, 0.85, A, yy, config=cfg, noise=noise, return_cpu=False)[0][0]

    batched = run(x, op, y, kn)
    parts = []
    for i, (one, src) in enumerate(zip(case["singles"], _sources())):
        xi = src.tensor(ops.PhiloxNoise.XT_ITER, torch.empty(1, 3, D, D, device="cuda"))
        parts.append(run(xi, one, y[i:i + 1, :3 * one.n_kept].contiguous(), src))
    sep = torch.cat(parts, 0)
    torch.cuda.synchronize()
    err = rel(batched, sep)
    print(f"per-image masks B=3 vs single-mask calls ({'DDNM+' if plus else 'DDNM'}): rel-L2 {err:.3e}")
    assert torch.isfinite(batched).all() and err < BAR


def _save_mask(tmp_path, mask):
    os.makedirs(tmp_path / "exp" / "inp_masks", exist_ok=True)
    np.save(tmp_path / "exp" / "inp_masks" / "mask.npy", mask)


RUNNER_ARGV = ["--path_y", "synthetic:5", "--eta", "0.85", "--deg", "inpainting"]


def test_runner_with_a_bank_matches_the_single_mask_runs(hip, tmp_path, monkeypatch, capsys):
    """synthetic:5 at batch 1, T = 4: the run with mask.npy [3, 64, 64] and DDNM_FUSE_BATCHES=4 restores image i like the
    unfused run with the 2-D mask i % 3.  Measured rel-L2 per image on the MI355X (printed): 0 ... 2.8e-7."""
    _mini_yaml(tmp_path)
    monkeypatch.chdir(tmp_path)
    masks = bank_masks(64)
    argv = RUNNER_ARGV + ["--sigma_y", "0."]
    _save_mask(tmp_path, masks)
    calls, psnr_b, img_b, names_b, apy_b = _run_main(tmp_path, monkeypatch, "bank", argv, 4)
    out_b = capsys.readouterr().out
    assert calls == [4, 1] and "Number of samples: 5" in out_b, out_b[-2000:]
    assert names_b == [f"{i}_0.png" for i in range(5)] and len(apy_b) == 10
    singles = []
    for r in range(3):
        _save_mask(tmp_path, masks[r])
        _, psnr, img, names, apy = _run_main(tmp_path, monkeypatch, f"mask{r}", argv, None)
        assert names == names_b and apy == apy_b
        singles.append((psnr, img))
    capsys.readouterr()
    assert psnr_b.shape == (5,) and img_b.shape == (5, 3, 64, 64)
    for i in range(5):
        psnr, img = singles[i % 3]
        err = rel(img_b[i], img[i])
        print(f"runner image {i} (mask {i % 3}): bank fused K=4 vs single-mask unfused rel-L2 {err:.3e}, "
              f"PSNR {float(psnr_b[i]):.4f} vs {float(psnr[i]):.4f}")
        assert err < BAR, i
        assert abs(float(psnr_b[i]) - float(psnr[i])) < 1e-3, i
    # the masks differ: image 1 restored with mask 1 (5 kept pixels) is not image 1 restored with mask 0
    assert rel(img_b[1], singles[0][1][1]) > 1e-2


def test_runner_with_a_bank_and_noisy_measurements(hip, tmp_path, monkeypatch, capsys):
    _mini_yaml(tmp_path)
    monkeypatch.chdir(tmp_path)
    _save_mask(tmp_path, bank_masks(64))
    _, psnr, img, names, apy = _run_main(tmp_path, monkeypatch, "noisy", RUNNER_ARGV + ["--sigma_y", "0.05", "--add_noise"], 4)
    out = capsys.readouterr().out
    assert "Number of samples: 5" in out, out[-2000:]
    assert names == [f"{i}_0.png" for i in range(5)] and len(apy) == 10
    assert torch.isfinite(img).all() and torch.isfinite(psnr).all()


def test_pi_entry_points_validate_on_device_pointers(hip):
    """The refusals of tests/test_inpaint_masks_host.py with a real device address: nothing is launched, the stream stays
    clean."""
    buf = torch.zeros(64, device="cuda")
    check_pi_validation(hip, buf.data_ptr())
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
