"""Demosaicing on the GPU (svd_operators.Mosaic, the `*_mosaic_*` entry points): A / A^+ and the spectral surface
against the reference's Inpainting on CFA indices (tests/golden/mosaic.npz) and the oracle restatement, the fused
noise-free step against the fp32 formula, its three noise sources against each other, the one-launch DDNM+ step against
the engine's generic Lambda composition and a float64 model, both samplers against the oracle's loops, and the runner.

Shapes: d = 16 with `xtrans` (16 % 6 = 4: the period wraps in the middle of a row and a 4-pixel vector straddles it),
d = 32 with `rggb` and `gbrg` (more than one workgroup), B = 3 (batch strides), et as a [B, 3, d, d] tensor and as the
[:, :3] view of [B, 6, d, d].  The bars are those the project holds for the same quantities elsewhere (named at each)."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from tests.helpers import engine_operator, rel
from tests.test_gpu_fuse import BAR, CTRS, KEYS, _mini_yaml, _run_main, _sources
from tests.test_gpu_measurements import SWITCHES, _files, _round_trip, _run
from tests.test_mosaic_host import (ETA, ETA_REG, GOLDEN_B, GOLDEN_D, GOLDEN_PATTERNS, PLUS_CASES, SIGMA_Y,
                                    check_mosaic_validation, golden_inputs, numpy_cfa, numpy_tables)

pytestmark = pytest.mark.gpu

B = 3
CASES = [("xtrans", 16), ("rggb", 32), ("gbrg", 32)]


def _ops(name, d):
    """(engine Mosaic, oracle Inpainting on the CFA's missing entries, sampled mask [3][d*d] bool)."""
    from ddnm_amd.functions import svd_operators as E
    from oracle import operators as O
    _, sampled, missing = numpy_tables(numpy_cfa(name), d)
    return E.Mosaic(3, d, name, "cuda"), O.Inpainting(3, d, torch.from_numpy(missing)), torch.from_numpy(sampled)


def _inputs(d, seed=23):
    """Seeded inputs shared by the step tests of one shape (never written to)."""
    g = torch.Generator().manual_seed(seed + d)
    x = torch.rand(B, 3, d, d, generator=g) * 2 - 1
    xt = torch.randn(B, 3, d, d, generator=g)
    et6 = torch.randn(B, 6, d, d, generator=g)
    nz = torch.randn(B, 3, d, d, generator=g)
    return x, xt, et6, nz


def _et(et6, six):
    """et on the device, as its own tensor or as the strided [:, :3] view of a learn-sigma output."""
    return et6.cuda()[:, :3] if six else et6[:, :3].contiguous().cuda()


# ---------------------------------------------------------------------------------------------- 4. operator
@pytest.mark.parametrize("name,d", CASES)
def test_A_and_A_pinv_equal_the_oracle(hip, name, d):
    op, orc, sampled = _ops(name, d)
    x = _inputs(d)[0]
    y = op.A(x.cuda())
    xp = op.A_pinv(y)
    torch.cuda.synchronize()
    assert y.shape == (B, d * d) and xp.shape == (B, 3 * d * d)
    assert torch.equal(y.cpu(), orc.A(x)) and torch.equal(xp.cpu(), orc.A_pinv(orc.A(x)))
    assert bool((xp.cpu().reshape(B, 3, d * d)[:, ~sampled] == 0).all())


@pytest.mark.parametrize("name", GOLDEN_PATTERNS)
def test_operator_and_spectral_surface_against_the_reference_golden(hip, name, golden_dir):
    """The bars of tests/test_gpu_kernels.py::test_operator_svd_surface / test_superresolution_ratio16_surface:
    permutations rel == 0, At / A_pinv_eta 2e-5, Lambda / Lambda_noise 1e-5; A and A_pinv by torch.equal."""
    from ddnm_amd.functions import svd_operators as E
    g = {k[len(name) + 1:]: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "mosaic.npz")).items()
         if k.startswith(name + "_")}
    d = GOLDEN_D
    op = E.Mosaic(3, d, name, "cuda")
    inp = {k: v.cuda() for k, v in golden_inputs(d, GOLDEN_B).items()}
    assert torch.equal(op.missing_indices, g["missing"])
    assert torch.equal(op.A(inp["x"]).cpu(), g["A"]) and torch.equal(op.A_pinv(inp["y"]).cpu(), g["A_pinv"])
    assert torch.equal(op.singulars().cpu(), g["singulars"])
    assert rel(op.Vt(inp["x"]), g["Vt"]) == 0.0 and rel(op.V(inp["v"]), g["V"]) == 0.0
    assert rel(op.U(inp["y"]), g["U"]) == 0.0 and rel(op.Ut(inp["y"]), g["Ut"]) == 0.0
    assert rel(op.add_zeros(inp["y"]), g["add_zeros"]) == 0.0
    assert rel(op.At(inp["y"]), g["At"]) < 2e-5 and rel(op.A_pinv_eta(inp["y"], ETA_REG), g["A_pinv_eta"]) < 2e-5
    for k, (a, sigma_t) in enumerate(PLUS_CASES):
        assert rel(op.Lambda(inp["v"], a, SIGMA_Y, sigma_t, ETA), g[f"Lambda_{k}"]) < 1e-5, k
        assert rel(op.Lambda_noise(inp["v"], a, SIGMA_Y, sigma_t, ETA, inp["eps"]), g[f"Lambda_noise_{k}"]) < 1e-5, k


# ---------------------------------------------------------------------------------------------- 5. fused step, tensor noise
def _scalars(lam=1.0):
    from ddnm_amd import ops
    from oracle import cases, schedule
    betas = cases.betas()
    at, at_next = schedule.alpha_bar(betas, 500), schedule.alpha_bar(betas, 490)
    return at, at_next, ops.step_scalars(at, at_next, ETA, lam=lam)


@pytest.mark.parametrize("name,d", CASES)
@pytest.mark.parametrize("six", [False, True])
@pytest.mark.parametrize("lam", [1.0, 0.3])
def test_fused_step_against_the_fp32_formula(hip, name, d, six, lam):
    """tests/test_gpu_kernels.py::test_ddnm_step with the oracle's A / A_pinv: x0 within 1e-6, x_{t-1} within 3e-6; the
    result does not depend on whether x0 is asked for.  Measured on the MI355X (printed): 0 and 0 in all twelve cases."""
    op, orc, _ = _ops(name, d)
    x, xt, et6, nz = _inputs(d)
    et = et6[:, :3]
    y = orc.A(x)
    at, at_next, s = _scalars(lam)
    x0 = (xt - et * (1 - at).sqrt()) / at.sqrt()
    x0h = x0 - orc.A_pinv(orc.A(x0.reshape(B, -1)) - y).reshape(x0.shape) * lam
    ref = at_next.sqrt() * x0h + (1 - at_next).sqrt() * ETA * nz + (1 - at_next).sqrt() * ((1 - ETA ** 2) ** 0.5) * et
    x0_e, out, out2 = (torch.empty(B, 3, d, d, device="cuda") for _ in range(3))
    op.ddnm_step(xt.cuda(), _et(et6, six), nz.cuda(), y.cuda(), s, x0_e, out)
    op.ddnm_step(xt.cuda(), _et(et6, six), nz.cuda(), y.cuda(), s, None, out2)
    torch.cuda.synchronize()
    e0, e1 = rel(x0_e, x0), rel(out, ref)
    print(f"mosaic step {name} d={d} six={six} lambda={lam}: x0 rel-L2 {e0:.3e}, x_t-1 rel-L2 {e1:.3e}")
    assert e0 < 1e-6 and e1 < 3e-6
    assert torch.equal(out, out2)


# ---------------------------------------------------------------------------------------------- 6. fused step, noise sources
def _sources_of(kind, like):
    """(noise argument of the batched call, stamp of its scalars, the same draw as a tensor, per-image (argument, stamp))."""
    from ddnm_amd import ops
    if kind == "philox":
        src = ops.PhiloxNoise(KEYS[1], image_base=4)
        return (None, lambda s: src.stamp(s, 9), src.tensor(9, like),
                lambda i: (None, lambda s: ops.PhiloxNoise(KEYS[1], image_base=4 + i).stamp(s, 9)))
    kn = ops.KeyedPhiloxNoise(KEYS, CTRS)
    return kn, (lambda s: kn.stamp(s, 9)), kn.tensor(9, like), lambda i: (None, lambda s: _sources()[i].stamp(s, 9))


@pytest.mark.parametrize("name,d", CASES)
@pytest.mark.parametrize("kind", ["philox", "keyed"])
def test_fused_step_noise_sources_are_the_same_draw(hip, name, d, kind):
    """In-kernel Philox and the keyed table == the tensor source filled by the same keys, and image b of the batch == that
    image stepped alone, all by torch.equal (the step is elementwise)."""
    op, orc, _ = _ops(name, d)
    x, xt, et6, _ = _inputs(d)
    xt, et, y = xt.cuda(), et6.cuda()[:, :3], orc.A(x).cuda()
    arg, stamp, tensor, alone = _sources_of(kind, xt)
    out = [torch.empty_like(xt) for _ in range(4)]
    op.ddnm_step(xt, et, arg, y, stamp(_scalars()[2]), out[0], out[1])
    op.ddnm_step(xt, et, tensor, y, _scalars()[2], out[2], out[3])
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[2]) and torch.equal(out[1], out[3])
    for i in range(B):
        arg_i, stamp_i = alone(i)
        x0_i, xn_i = torch.empty_like(xt[:1]), torch.empty_like(xt[:1])
        op.ddnm_step(xt[i:i + 1].contiguous(), et[i:i + 1], arg_i, y[i:i + 1].contiguous(), stamp_i(_scalars()[2]), x0_i, xn_i)
        torch.cuda.synchronize()
        assert torch.equal(out[0][i:i + 1], x0_i) and torch.equal(out[1][i:i + 1], xn_i), i


# ---------------------------------------------------------------------------------------------- 7. fused noisy step
def _generic_plus_step(op, xt, et, nz, y, s, sigma_y, sigma_t, eta):
    """The body of ddnm_plus_diffusion's step for an operator WITHOUT the hook (functions/svd_ddnm.py): x0 kernel, A,
    residual, A^+, Lambda, Lambda_noise, combine."""
    from ddnm_amd import ops
    from ddnm_amd.functions.svd_operators import _axpby
    a = s.sqrt_at_next
    et = et.contiguous()
    x0, out = torch.empty_like(xt), torch.empty_like(xt)
    ops.step_x0(xt, et, s, out=x0)
    resid = _axpby(op.A(x0), y, 1.0, -1.0)
    corr = op.Lambda(op.A_pinv(resid), a, sigma_y, sigma_t, eta).reshape(x0.shape)
    mixed = op.Lambda_noise(nz, a, sigma_y, sigma_t, eta, et).reshape(x0.shape)
    s.c1, s.c2, s.lam = 1.0, 0.0, 1.0
    ops.step_combine(x0, corr, None, mixed, et, s, out=out)
    return x0, out


@pytest.mark.parametrize("name,d", CASES)
@pytest.mark.parametrize("six", [False, True])
@pytest.mark.parametrize("at_next", [0.99, 0.5])
@pytest.mark.parametrize("kind", ["tensor", "philox", "keyed"])
def test_fused_noisy_step(hip, name, d, six, at_next, kind):
    """One launch against the eight of the generic composition and against a float64 model of
        sampled:  x_{t-1} = a x0 - a lambda (x0 - y) + d1r n + d2r eps      others:  x_{t-1} = a x0 + d1n n + d2n eps
    within 3e-6 (BAR).  sigma_y = 0.4: at_next = 0.99 gives sigma_t = 0.1 below a sigma_y = 0.398 (lambda < 1), at_next = 0.5
    gives 0.707 above 0.283 (lambda = 1, d1r = sqrt(sigma_t^2 - a^2 sigma_y^2)).  Measured on the MI355X (printed): vs the
    generic composition 4.5e-8 ... 6.3e-8, vs float64 6.1e-8 ... 7.5e-8."""
    from ddnm_amd import ops
    from ddnm_amd.functions.svd_operators import cs_plus_coefficients
    op, orc, sampled = _ops(name, d)
    x, xt, et6, nz = _inputs(d)
    xt, et, y = xt.cuda(), _et(et6, six), orc.A(x).cuda()
    s = ops.step_scalars(torch.tensor(0.45), torch.tensor(at_next), ETA)
    a, sigma_t = s.sqrt_at_next, float((1 - torch.tensor(at_next)).sqrt())
    assert (sigma_t < a * SIGMA_Y) == (at_next == 0.99)
    if kind == "tensor":
        arg, tensor = nz.cuda(), nz.cuda()
    else:
        arg, stamp, tensor, _ = _sources_of(kind, xt)
        stamp(s)
    x0_f, out_f = torch.empty_like(xt), torch.empty_like(xt)
    op.begin_plus_run(y)
    op.ddnm_plus_step(xt, et, arg, s, SIGMA_Y, sigma_t, ETA, x0_f, out_f)
    x0_g, out_g = _generic_plus_step(op, xt, et, tensor, y, ops.step_scalars(torch.tensor(0.45), torch.tensor(at_next), ETA),
                                     SIGMA_Y, sigma_t, ETA)
    torch.cuda.synchronize()
    al, d1n, d2n, dd1, dd2 = cs_plus_coefficients(a, SIGMA_Y, sigma_t, ETA)
    m = sampled.reshape(1, 3, d, d)
    xd, ed, nd = xt.double().cpu(), et6[:, :3].double(), tensor.double().cpu()
    yd = y.double().cpu().reshape(B, 1, d, d)
    x0 = (xd - ed * s.sqrt_1m_at) / s.sqrt_at
    want = torch.where(m, a * x0 - al * (x0 - yd) + (d1n + dd1) * nd + (d2n + dd2) * ed, a * x0 + d1n * nd + d2n * ed)
    e_g, e_64 = rel(out_f, out_g), rel(out_f, want)
    print(f"mosaic DDNM+ step {name} d={d} six={six} at_next={at_next} noise={kind}: vs generic {e_g:.3e}, vs float64 {e_64:.3e}")
    assert torch.equal(x0_f, x0_g) and rel(x0_f, x0) < 1e-6
    assert e_g < BAR and e_64 < BAR


# ---------------------------------------------------------------------------------------------- 8. loops
@pytest.fixture(scope="module")
def small_net(hip):
    from ddnm_amd.guided_diffusion.models import Model
    from oracle import cases, unet_celeba
    cfg, sd = cases.celeba_net("small")
    cfg.time_travel.T_sampling, cfg.time_travel.travel_length, cfg.time_travel.travel_repeat = 4, 2, 2
    model = Model(cfg)
    model.load_state_dict(sd)
    return cfg, unet_celeba.Net(sd, cfg), model


@pytest.mark.parametrize("plus", [False, True])
@pytest.mark.parametrize("name", ["rggb", "xtrans"])
def test_samplers_against_the_oracle_loops(small_net, plus, name):
    """ddnm_diffusion / ddnm_plus_diffusion (sigma_y = 0.2) with Mosaic, T = 4 and one time-travel jump of two steps,
    against the oracle's loops with oracle.operators.Inpainting on the same noise tape: within 2e-4, the bar of
    tests/test_gpu_sampler.py / tests/test_ddnm_plus.py.  The whole-pixel Inpainting loop on the same net and tape is
    printed next to it.  Measured on the MI355X: DDNM 4.33e-7 (rggb) / 4.36e-7 (xtrans), DDNM+ 4.41e-7 / 4.41e-7; whole-pixel
    Inpainting 4.39e-7 / 4.40e-7."""
    from ddnm_amd.functions.svd_ddnm import ddnm_diffusion, ddnm_plus_diffusion
    from oracle import cases, sampler, schedule
    cfg, net, model = small_net
    d = cfg.data.image_size
    n_it = len(schedule.jump_times(4, 2, 2)) - 1
    assert n_it == 4 + 2 * 2                      # four reverse steps, one jump two steps back and down again
    x_orig, x_T, tape = cases.sampler_case(cfg, B, n_it)
    pairs = {"mosaic": _ops(name, d)[:2],
             "inpainting": (engine_operator("inpainting", d), cases.make_operator("inpainting", d))}
    errs = {}
    for tag, (op, orc) in pairs.items():
        y = orc.A(x_orig)
        kw = dict(T_sampling=4, travel_length=2, travel_repeat=2)
        if plus:
            ref, ref0 = sampler.ddnm_plus_diffusion(x_T.clone(), net, cases.betas(), ETA, orc, y, 0.2, tape, **kw)
            xs, x0s = ddnm_plus_diffusion(x_T.cuda(), model, cases.betas().cuda(), ETA, op, y.cuda(), 0.2, cls_fn=None,
                                          classes=None, config=cfg, noise=[n.cuda() for n in tape])
        else:
            ref, ref0 = sampler.ddnm_diffusion(x_T.clone(), net, cases.betas(), ETA, orc, y, tape, **kw)
            xs, x0s = ddnm_diffusion(x_T.cuda(), model, cases.betas().cuda(), ETA, op, y.cuda(), cls_fn=None, classes=None,
                                     config=cfg, noise=[n.cuda() for n in tape])
        errs[tag] = (rel(xs[0], ref), rel(x0s[0], ref0))
        print(f"{'DDNM+' if plus else 'DDNM'} loop, {tag} ({name if tag == 'mosaic' else 'random mask'}): "
              f"x rel-L2 {errs[tag][0]:.3e}, x0 rel-L2 {errs[tag][1]:.3e}")
    assert max(errs["mosaic"]) < 2e-4


def test_simplified_loop_against_the_oracle(small_net):
    """tests/test_gpu_cli.py::test_simplified_loop_vs_oracle with A = A^+ = z * (sampled entries), sigma_y = 0 and 0.3:
    its bar of 2e-4."""
    from ddnm_amd.guided_diffusion.diffusion import simplified_loop
    from oracle import cases, sampler, schedule
    cfg, net, model = small_net
    d = cfg.data.image_size
    op, _, sampled = _ops("rggb", d)
    mask = sampled.reshape(1, 3, d, d).float()
    n_it = len(schedule.jump_times(4, 2, 2)) - 1
    x_orig, x_T, tape = cases.sampler_case(cfg, 1, n_it)
    for sigma_y in (0.0, 0.3):
        ref, _ = sampler.simplified_ddnm(x_T.clone(), net, cases.betas(), ETA, lambda z: z * mask, lambda z: z * mask,
                                         x_orig * mask, sigma_y, tape, T_sampling=4, travel_length=2, travel_repeat=2)
        got = simplified_loop(x_T.cuda(), model, cases.betas().cuda(), ETA, op, op.A(x_orig.cuda()), sigma_y, cfg,
                              noise=[n.cuda() for n in tape])
        torch.cuda.synchronize()
        err = rel(got, ref)
        print(f"simplified loop, mosaic rggb, sigma_y={sigma_y}: rel-L2 {err:.3e}")
        assert err < 2e-4


# ---------------------------------------------------------------------------------------------- 9. CLI
ARGV = ["--path_y", "synthetic:3", "--eta", "0.85", "--deg", "demosaic_rggb", "--sigma_y", "0."]


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path), dtype=np.int16)


def test_runner_plain_fused_and_two_samples(hip, tmp_path, monkeypatch, capsys):
    """main.py --deg demosaic_rggb on the mini configuration (64 px, T = 4, synthetic images): DDNM_FUSE_BATCHES=2 and
    sample 0 of DDNM_SAMPLES=2 restore what the plain run restores (BAR), and Apy_{i}.png is the coloured mosaic: black at
    the entries the array does not sample, the ground truth's grey level (Apy/orig_{i}.png) at the others."""
    _mini_yaml(tmp_path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("DDNM_SAMPLES", raising=False)
    calls1, psnr1, img1, names1, apy1 = _run_main(tmp_path, monkeypatch, "plain", ARGV, None)
    calls2, psnr2, img2, names2, apy2 = _run_main(tmp_path, monkeypatch, "fused", ARGV, 2)
    monkeypatch.setenv("DDNM_SAMPLES", "2")
    calls3, _, img3, names3, _ = _run_main(tmp_path, monkeypatch, "samples", ARGV, None)
    monkeypatch.delenv("DDNM_SAMPLES")
    out = capsys.readouterr().out
    assert out.count("Number of samples: 3") == 3, out[-3000:]
    assert calls1 == [1] and calls2 == [2, 1] and calls3 == [2]
    assert names1 == names2 == [f"{i}_0.png" for i in range(3)] and apy1 == apy2 and len(apy1) == 6
    assert names3 == sorted(f"{i}_{k}.png" for i in range(3) for k in range(2))
    e_f, e_s = rel(img2, img1), rel(img3[0::2], img1)
    print(f"demosaic_rggb runner: fused K=2 vs plain rel-L2 {e_f:.3e}, sample 0 of 2 vs plain rel-L2 {e_s:.3e}")
    assert torch.isfinite(img1).all() and e_f < BAR and e_s < BAR
    assert (psnr1 - psnr2).abs().max() < 1e-3 and rel(img3[1::2], img1) > 1e-3          # sample 1 is another draw
    sampled = numpy_tables(numpy_cfa("rggb"), 64)[1].reshape(3, 64, 64).transpose(1, 2, 0)     # [H][W][C]
    for i in range(3):
        shown = _png(tmp_path / "exp" / "image_samples" / "plain" / "Apy" / f"Apy_{i}.png")
        orig = _png(tmp_path / "exp" / "image_samples" / "plain" / "Apy" / f"orig_{i}.png")
        assert shown.shape == (64, 64, 3) and bool((shown[~sampled] == 0).all()), i
        assert int(np.abs(shown[sampled] - orig[sampled]).max()) <= 1, i          # (y + 1) - 1 may move a .5 tie
        assert float((shown[sampled] > 0).mean()) > 0.98, i                            # uniform images: the samples are lit


def test_runner_simplified_and_noisy(hip, tmp_path, monkeypatch, capsys):
    """--simplified takes Mosaic's A / A_pinv; --sigma_y 0.05 --add_noise runs DDNM+ through the one-launch hook (the
    generic Lambda chain would show as ddnm_mask_mix_f32 calls)."""
    from ddnm_amd import ops
    _mini_yaml(tmp_path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("DDNM_SAMPLES", raising=False)
    _, psnr, img, names, apy = _run_main(tmp_path, monkeypatch, "simplified", ARGV + ["--simplified"], None)
    assert names == sorted(f"{i - 1}_0.png" for i in range(3)) and len(apy) == 6 and torch.isfinite(img).all()
    seen = []
    orig_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (seen.append(name), orig_call(name, *a))[1])
    noisy = ARGV[:-2] + ["--sigma_y", "0.05", "--add_noise"]
    _, psnr_n, img_n, names_n, _ = _run_main(tmp_path, monkeypatch, "noisy", noisy, 2)
    out = capsys.readouterr().out
    assert out.count("Number of samples: 3") == 2, out[-3000:]
    assert names_n == [f"{i}_0.png" for i in range(3)] and torch.isfinite(img_n).all() and torch.isfinite(psnr_n).all()
    assert "ddnm_mask_mix_f32" not in seen and "ddnm_op_mosaic_A_f32" in seen


# ---------------------------------------------------------------------------------------------- 10. measurements
@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    root = tmp_path_factory.mktemp("mosaic_measurements")
    _mini_yaml(root)
    return str(root)


def test_round_trip_of_saved_measurements(hip, workdir):
    """DDNM_SAVE_Y=1 with noisy measurements, then the run over measurements:<its y/>: the same PNG bytes
    (tests/test_gpu_measurements.py::_round_trip); the saved rows are the S^2 values of the raw frame."""
    noisy = ["--deg", "demosaic_xtrans", "--sigma_y", "0.05"]
    truth, given = _round_trip(workdir, "xtrans", noisy + ["--add_noise"], noisy, 2)
    for i in range(2):
        row = np.load(os.path.join(truth["folder"], "y", f"y_{i}.npy"))
        assert row.dtype == np.float32 and row.shape == (64 * 64,) and np.isfinite(row).all()
    assert [c["y"].shape for c in given["cons"]] == [(1, 4096)] * 2


def test_run_from_raw_frames_as_pictures(hip, workdir):
    """A folder of one-channel 64 x 64 PNGs is restored (the command line of the issue, --sigma_y 0.02): its rows are
    data_transform of the pixel values exactly, and Apy_{i}.png shows each frame's samples in their colours."""
    from PIL import Image
    src = os.path.join(workdir, "exp", "datasets", "raw")
    os.makedirs(src, exist_ok=True)
    rng = np.random.default_rng(11)
    pics = [rng.integers(1, 256, (64, 64), dtype=np.uint8) for _ in range(2)]
    for i, arr in enumerate(pics):
        Image.fromarray(arr).save(os.path.join(src, f"frame_{i}.png"))
    run = _run(workdir, "raw", ["--path_y", "measurements:raw", "--deg", "demosaic_rggb", "--sigma_y", "0.02"])
    assert "PSNR:" not in run["out"] and "Number of samples: 2" in run["out"] and "Cons: " in run["out"]
    assert sorted(run["files"]) == ["0_0.png", "1_0.png", "Apy/Apy_0.png", "Apy/Apy_1.png"]
    sampled = numpy_tables(numpy_cfa("rggb"), 64)[1].reshape(3, 64, 64).transpose(1, 2, 0)
    for i, arr in enumerate(pics):
        want = torch.from_numpy(arr.astype(np.float32)).div(255.0).mul(2).sub(1.0).reshape(1, -1)
        assert torch.equal(run["cons"][i]["y"].cpu(), want), i
        shown = _png(os.path.join(run["folder"], f"Apy/Apy_{i}.png"))
        assert bool((shown[~sampled] == 0).all()) and int(np.abs(shown[sampled] - arr.reshape(-1)).max()) <= 1, i


@pytest.mark.parametrize("kind", ["rgb", "wide"])
def test_a_picture_that_is_no_raw_frame_is_refused(hip, workdir, kind):
    """A 3-channel or wrong-size picture: main logs the ValueError of MeasurementFolder.bind and restores nothing."""
    import main
    from PIL import Image
    from ddnm_amd.guided_diffusion.models import Model
    src = os.path.join(workdir, "exp", "datasets", kind)
    os.makedirs(src, exist_ok=True)
    shape = (64, 64, 3) if kind == "rgb" else (64, 60)
    Image.fromarray(np.zeros(shape, np.uint8)).save(os.path.join(src, "frame_0.png"))
    cwd = os.getcwd()
    buf = io.StringIO()
    with pytest.MonkeyPatch.context() as m:
        m.setenv("DDNM_RANDOM_WEIGHTS", "1")
        for name in SWITCHES:
            m.delenv(name, raising=False)
        m.setattr(Model, "__call__", lambda self, x, t: pytest.fail("the network ran"))
        os.chdir(workdir)
        try:
            with contextlib.redirect_stdout(buf):
                main.main(["--ni", "--config", "mini.yml", "-i", kind, "--eta", "0.85", "--path_y", f"measurements:{kind}",
                           "--deg", "demosaic_rggb", "--sigma_y", "0."])
        finally:
            os.chdir(cwd)
    assert "Number of samples:" not in buf.getvalue()
    assert not [f for f in _files(os.path.join(workdir, "exp", "image_samples", kind)) if f.endswith(".png")]


def test_cons_metric_in_a_ground_truth_run(hip, workdir):
    """DDNM_METRICS=cons: a `Cons:` line after the PSNR line; the noise-free restoration reproduces its mosaic."""
    run = _run(workdir, "cons", ["--path_y", "synthetic:2", "--deg", "demosaic_gbrg", "--sigma_y", "0."], DDNM_METRICS="cons")
    lines = run["out"].splitlines()
    assert len([ln for ln in lines if ln.startswith("Cons: ")]) == 2 and "Total Average Cons:" in run["out"]
    assert len(run["cons"]) == 2 and all(c["ax"].shape == c["y"].shape == (1, 4096) for c in run["cons"])
    print(f"demosaic_gbrg: Max Cons {run['metrics']['cons_max']:.3e}")
    assert run["metrics"]["cons_max"] < 1e-3          # the gross-error guard of tests/test_gpu_measurements.py


def test_entry_points_validate_on_device_pointers(hip):
    """The refusals of tests/test_mosaic_host.py with a real device address: nothing is launched."""
    buf = torch.zeros(64, device="cuda")
    check_mosaic_validation(hip, buf.data_ptr())
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
