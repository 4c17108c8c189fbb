"""JPEG-artifact restoration on the GPU (svd_operators.JPEG, the `*_jpeg_*` entry points of csrc/jpeg.hip): T, T^+ and the
encoder against the dense float64 model of tests/test_jpeg_host.py, the fused cell-projection step against that model and
against the composition of T / T^+ with the generic step kernels, its three noise sources against each other, the sampler
against the oracle's loop over the wrapped model, and the runner.

Shapes, B = 3: d = 16 (1,1) (2 x 2 blocks), d = 32 (2,2) and (2,1) (2 x 2 and 2 x 4 MCUs), d = 48 (2,2) (27 MCUs: the last
workgroup holds 3 of its 8), d = 64 (1,1) (192 MCUs: 12 workgroups), one direct ABI case with H = 16, W = 64 and (2,1),
BT.709 once; eps as a [B, 3, d, d] tensor and as the [:, :3] view of [B, 6, d, d].  The bars are those the project holds
for the same quantities elsewhere (named at each).  Every test prints what it measured, and next to
the operator's figures the same closed form evaluated in numpy float32 on the CPU."""
import ctypes
import functools
import logging
import os

import numpy as np
import pytest
import torch

from tests.helpers import rel
from tests.test_chroma_host import BT601, BT709, kernel_matrix
from tests.test_gpu_fuse import BAR, _mini_yaml, _run_main
from tests.test_gpu_measurements import _round_trip, _run
from tests.test_gpu_mosaic import _et, _sources_of
from tests.test_jpeg_host import (ETA, CellOperator, JpegModel, check_jpeg_validation, closed_T, closed_T_pinv, steps_of)

pytestmark = pytest.mark.gpu

B = 3
SHAPES = [(16, 1, 1), (32, 2, 2), (32, 2, 1), (48, 2, 2), (64, 1, 1)]            # (d, rw, rh)
CASES = [("bt601", d, rw, rh) for d, rw, rh in SHAPES] + [("bt709", 32, 2, 2)]
MATS = {"bt601": BT601, "bt709": BT709}
ABAR_T = 0.45


@functools.lru_cache(maxsize=None)
def _pair(name, d, rw, rh, quality=50, box=0.98):
    """(engine JPEG, per-MCU float64 model with the matrix and the steps the kernels get); built once per case."""
    from ddnm_amd.functions import svd_operators as E
    q, delta = steps_of(quality)
    return (E.JPEG(3, d, quality, rw, rh, "cuda", matrix=MATS[name], box=box),
            JpegModel(rw, rh, kernel_matrix(MATS[name]), d, d, q, delta))


@functools.lru_cache(maxsize=None)
def _inputs(d):
    """Seeded (x_orig, x_t, eps with 6 channels, n) of one size (the convention of tests/test_gpu_chroma.py), shared by
    its tests and never written to."""
    g = torch.Generator().manual_seed(77 + 100 * d)
    return (torch.rand(B, 3, d, d, generator=g) * 2 - 1, torch.randn(B, 3, d, d, generator=g),
            torch.randn(B, 6, d, d, generator=g), torch.randn(B, 3, d, d, generator=g))


def _np(t):
    return t.detach().double().cpu().reshape(t.shape[0], -1).numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bar(base, f32):
    """The project's bar, or 3 x the numpy-float32 figure of the same closed form where that exceeds a third of it."""
    return base if f32 <= base / 3 else 3 * f32


def test_the_shapes_are_what_the_header_says(hip):
    from ddnm_amd.functions import svd_operators as E
    assert all((d * d + 2 * d * d // (rw * rh)) % 4 == 0 for d, rw, rh in SHAPES)
    big, odd = E.JPEG(3, 64, 50, 1, 1, "cuda"), E.JPEG(3, 48, 50, 2, 2, "cuda")
    assert big.workgroups(B) == 12 >= 3 and big.mcus_per_workgroup() == 16          # d = 64 (1,1): at least three workgroups
    assert B * (48 // 16) ** 2 == 27 and 27 % odd.mcus_per_workgroup() == 3 and odd.workgroups(B) == 4


# ---------------------------------------------------------------------------------------------- 1. operator
@pytest.mark.parametrize("name,d,rw,rh", CASES)
def test_T_and_T_pinv_against_the_model(hip, name, d, rw, rh):
    """A_linear = T, A_pinv = T^+ and T T^+ y = y within 1e-6 (rel-L2) of the float64 model -- or
    3 x the numpy float32 figure of the same closed form where that exceeds a third of the bar; singulars() is the chroma
    spectrum.  Measured on the MI355X (printed, with the numpy float32 figure): T at most 9.7e-8 (1.11e-7), T^+ 1.06e-7
    (1.71e-7), T T^+ y 1.57e-7 (2.15e-7): no float32 figure reaches a third of the bar, which stands at 1e-6."""
    op, M = _pair(name, d, rw, rh)
    Mk = kernel_matrix(MATS[name])
    x = _inputs(d)[0]
    g = torch.Generator().manual_seed(5)
    yr = torch.randn(B, op.measurement_size(), generator=g)
    c, xp = op.A_linear(x.cuda()), op.A_pinv(yr.cuda())
    back = op.A_linear(xp)
    torch.cuda.synchronize()
    assert c.shape == (B, d * d + 2 * d * d // (rw * rh)) and xp.shape == (B, 3 * d * d)
    want_c, want_p = _t(M.apply_T(_np(x))), _t(M.apply_pinv(_np(yr)))
    e_T, e_P, e_back = rel(c, want_c), rel(xp, want_p), rel(back.cpu(), yr)
    xp32 = closed_T_pinv(rw, rh, Mk, d, yr.numpy(), np.float32)
    f_T = rel(_t(closed_T(rw, rh, Mk, d, x.reshape(B, -1).numpy(), np.float32)), want_c)
    f_P, f_back = rel(_t(xp32), want_p), rel(_t(closed_T(rw, rh, Mk, d, xp32, np.float32)), yr)
    print(f"jpeg operator {name} d={d} site={rw}x{rh}: T rel-L2 {e_T:.3e}, T^+ {e_P:.3e}, T T^+ y = y {e_back:.3e}"
          f"   (numpy float32: {f_T:.3e}, {f_P:.3e}, {f_back:.3e})")
    assert e_T <= _bar(1e-6, f_T) and e_P <= _bar(1e-6, f_P) and e_back <= _bar(1e-6, f_back)
    assert op.singulars().numel() == 3 * d * d - 2 * (d * d - d * d // (rw * rh))


@pytest.mark.parametrize("name,d,rw,rh", CASES)
def test_encoder_levels_against_the_model(hip, name, d, rw, rh):
    """A (the encoder) at Q = 10, 50, 90: every level equals the model's, except where the float64 model lies within 1e-3
    level units of a rounding tie, where it may differ by exactly one level; the exempt share is at most 0.5 % (asserted on
    the model).  A_pinv(A x) is finite: the decoded picture."""
    x = _inputs(d)[0]
    for quality in (10, 50, 90):
        op, M = _pair(name, d, rw, rh, quality)
        y = op.A(x.cuda())
        got = op.levels(y).cpu().numpy()
        shown = op.A_pinv(y)
        torch.cuda.synchronize()
        s = M.scaled(_np(x))
        want = np.rint(s)
        exempt = np.abs(np.abs(s - np.floor(s)) - 0.5) < 1e-3
        share, diff = float(exempt.mean()), np.abs(got - want)
        print(f"jpeg encoder {name} d={d} site={rw}x{rh} Q={quality}: exempt share {share:.4%}, levels differing "
              f"{int((diff != 0).sum())} of {diff.size} (all of them exempt: {bool((diff[~exempt] == 0).all())}), "
              f"|level| max {int(np.abs(want).max())}")
        assert share <= 0.005
        assert (diff[~exempt] == 0).all() and (diff[exempt] <= 1).all()
        # y is the dequantised centre of those levels, and the decoder's picture is finite
        assert rel(y, _t(M.q_row * got + M.delta_row)) <= 1e-6 and bool(torch.isfinite(shown).all())


def test_direct_abi_on_a_wide_image(hip):
    """H = 16, W = 64, site (2,1) through the C ABI: T, T^+, the encoder's levels and the fused step (lambda = 0.3, box
    0.98) against the image's dense matrix built entry by entry.  A swap of rw and rh or of rows and columns moves whole
    MCUs.  Bars: 1e-6 for T and T^+, 3e-6 for the step."""
    from ddnm_amd import ops
    H, W, rw, rh = 16, 64, 2, 1
    Mk = kernel_matrix(BT601)
    q, delta = steps_of(50)
    D = JpegModel(rw, rh, Mk, H, W, q, delta, whole=True)
    m9 = (ctypes.c_float * 9)(*[float(v) for v in Mk.reshape(-1)])
    q128 = (ctypes.c_float * 128)(*[float(v) for v in q])
    g = torch.Generator().manual_seed(9)
    x = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    et, nz, n0 = (torch.randn(B, 3, H, W, generator=g) for _ in range(3))
    L = H * W + 2 * H * W // 2
    yr = torch.randn(B, L, generator=g)
    xt = ((x.double() + 0.1 * n0.double()) * ABAR_T ** 0.5 + et.double() * (1 - ABAR_T) ** 0.5).float()
    x_d, xt_d, et_d, nz_d, yr_d = (v.cuda() for v in (x, xt, et, nz, yr))
    c_d, y_d, xp_d = torch.empty(B, L, device="cuda"), torch.empty(B, L, device="cuda"), torch.empty(B, 3 * H * W, device="cuda")
    ops.call("ddnm_op_jpeg_T_f32", x_d.data_ptr(), c_d.data_ptr(), B, H, W, rw, rh, m9)
    ops.call("ddnm_op_jpeg_A_f32", x_d.data_ptr(), y_d.data_ptr(), B, H, W, rw, rh, m9, q128, delta)
    ops.call("ddnm_op_jpeg_pinv_f32", yr_d.data_ptr(), xp_d.data_ptr(), B, H, W, rw, rh, m9)
    torch.cuda.synchronize()
    e_T, e_P = rel(c_d, _t(D.apply_T(_np(x)))), rel(xp_d, _t(D.apply_pinv(_np(yr))))
    s = D.scaled(_np(x))
    exempt = np.abs(np.abs(s - np.floor(s)) - 0.5) < 1e-3
    got = np.rint((_np(y_d) - D.delta_row) / D.q_row)
    assert exempt.mean() <= 0.005 and (got[~exempt] == np.rint(s)[~exempt]).all() and (np.abs(got - np.rint(s)) <= 1).all()
    y64 = _np(y_d)
    sc = ops.step_scalars(torch.tensor(ABAR_T), torch.tensor(0.6), ETA, lam=0.3)
    x0_m, want, share = D.step(_np(xt), _np(et), _np(nz), y64, ABAR_T, 0.6, ETA, 0.3, 0.98)
    x0_d, out_d = torch.empty_like(xt_d), torch.empty_like(xt_d)
    ops.step_call("ddnm_step_jpeg_f32", xt_d, et_d, nz_d, y_d, x0_d.data_ptr(), out_d.data_ptr(), B, H, W, rw, rh, m9, q128,
                  0.98, sc)
    torch.cuda.synchronize()
    e_S = rel(out_d.reshape(B, -1), _t(want))
    print(f"jpeg ABI 16 x 64 site 2x1: T {e_T:.3e}, T^+ {e_P:.3e}, step {e_S:.3e} (clamped share {share:.1%}), "
          f"exempt levels {exempt.mean():.4%}")
    assert e_T <= 1e-6 and e_P <= 1e-6 and e_S <= 3e-6 and 0.05 <= share <= 0.95
    assert torch.equal(x0_d, ops.step_x0(xt_d, et_d, sc))


# ---------------------------------------------------------------------------------------------- 2. the fused step
def _step_inputs(d):
    """(x_t, eps with 6 channels, n) with x0 = x_orig + 0.1 n': a restoration in progress, near its measurement (with a
    random x_t nearly every coefficient is clamped)."""
    x, n0, et6, nz = _inputs(d)
    xt = ((x.double() + 0.1 * n0.double()) * ABAR_T ** 0.5 + et6[:, :3].double() * (1 - ABAR_T) ** 0.5).float()
    return xt, et6, nz


class _Centre:
    """T / T^+ as the A / A_pinv of the generic two-part step (A_functions.ddnm_step): x0 - lambda T^+(T x0 - y)."""

    def __init__(self, op):
        self.A, self.A_pinv = op.A_linear, op.A_pinv


@pytest.mark.parametrize("name,d,rw,rh", CASES)
@pytest.mark.parametrize("six", [False, True])
def test_fused_step_against_the_model(hip, name, d, rw, rh, six):
    """Q = 50, lambda = 1 and 0.3, box = 0.98, 0.5 and 0: x0 bit-identical to ddnm_step_x0_f32, x_{t-1} within 3e-6 (the
    project's step bar) of the float64 model; the clamped share of the model lies in [5 %, 95 %] for box 0.98 and 0.5 (both
    branches of the clamp carry weight); box = 0 agrees within 3e-6 with x0 - lambda T^+(T x0 - y) composed from the T / T^+
    entry points and the generic step kernels; the result does not depend on whether x0 is asked for.  Measured on the
    MI355X (printed): at most 9.2e-8 against float64, clamped shares 13.8 ... 16.4 % and 48.8 ... 53.2 %, and the box = 0
    result bit-identical to the composition."""
    from ddnm_amd import ops
    from ddnm_amd.functions.svd_operators import A_functions
    x = _inputs(d)[0]
    xt, et6, nz = _step_inputs(d)
    xt_d, et_d, nz_d = xt.cuda(), _et(et6, six), nz.cuda()
    for box in (0.98, 0.5, 0.0):
        op, M = _pair(name, d, rw, rh, 50, box)
        y_d = op.A(x.cuda())
        y64 = _np(y_d)
        for lam in (1.0, 0.3):
            s = ops.step_scalars(torch.tensor(ABAR_T), torch.tensor(0.6), ETA, lam=lam)
            x0_m, want, share = M.step(_np(xt), _np(et6[:, :3]), _np(nz), y64, ABAR_T, 0.6, ETA, lam, box)
            x0_e, out, out2 = (torch.empty(B, 3, d, d, device="cuda") for _ in range(3))
            op.ddnm_step(xt_d, et_d, nz_d, y_d, s, x0_e, out)
            op.ddnm_step(xt_d, et_d, nz_d, y_d, s, None, out2)
            x0_k = ops.step_x0(xt_d, et_d, s)
            torch.cuda.synchronize()
            e64 = rel(out.reshape(B, -1), _t(want))
            line = f"jpeg step {name} d={d} site={rw}x{rh} six={six} box={box} lambda={lam}: vs float64 {e64:.3e}, clamped share {share:.1%}"
            assert torch.equal(x0_e, x0_k) and rel(x0_e.reshape(B, -1), _t(x0_m)) < 1e-6
            assert torch.equal(out, out2)
            if box > 0:
                assert 0.05 <= share <= 0.95, line
            else:
                x0_g, out_g = torch.empty_like(out), torch.empty_like(out)
                A_functions.ddnm_step(_Centre(op), xt_d, et_d, nz_d, y_d, s, x0_g, out_g)
                torch.cuda.synchronize()
                eg = rel(out, out_g)
                line += f", vs the composition of T / T^+ {eg:.3e}"
                assert eg <= 3e-6, line
            print(line)
            assert e64 <= 3e-6, line


@pytest.mark.parametrize("d,rw,rh", SHAPES)
@pytest.mark.parametrize("kind", ["philox", "keyed"])
def test_fused_step_noise_sources_are_the_same_draw(hip, d, rw, rh, kind):
    """In-kernel Philox and the keyed table == the tensor source filled by the same keys, and image b of the batch == that
    image stepped alone, all by torch.equal."""
    from ddnm_amd import ops
    op, _ = _pair("bt601", d, rw, rh)
    x = _inputs(d)[0]
    xt, et6, _ = _step_inputs(d)
    xt_d, et_d = xt.cuda(), et6.cuda()[:, :3]
    y_d = op.A(x.cuda())
    sc = lambda: ops.step_scalars(torch.tensor(ABAR_T), torch.tensor(0.6), ETA, lam=0.3)      # noqa: E731
    arg, stamp, tensor, alone = _sources_of(kind, xt_d)
    out = [torch.empty_like(xt_d) for _ in range(4)]
    op.ddnm_step(xt_d, et_d, arg, y_d, stamp(sc()), out[0], out[1])
    op.ddnm_step(xt_d, et_d, tensor, y_d, sc(), out[2], out[3])
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[2]) and torch.equal(out[1], out[3])
    for i in range(B):
        arg_i, stamp_i = alone(i)
        x0_i, xn_i = torch.empty_like(xt_d[:1]), torch.empty_like(xt_d[:1])
        op.ddnm_step(xt_d[i:i + 1].contiguous(), et_d[i:i + 1], arg_i, y_d[i:i + 1].contiguous(), stamp_i(sc()), x0_i, xn_i)
        torch.cuda.synchronize()
        assert torch.equal(out[0][i:i + 1], x0_i) and torch.equal(out[1][i:i + 1], xn_i), i


# ---------------------------------------------------------------------------------------------- 3. the loop
@pytest.fixture(scope="module")
def small_net(hip):
    from ddnm_amd.guided_diffusion.models import Model
    from oracle import cases, unet_celeba
    cfg, sd = cases.celeba_net("small")
    cfg.time_travel.T_sampling, cfg.time_travel.travel_length, cfg.time_travel.travel_repeat = 4, 2, 2
    model = Model(cfg)
    model.load_state_dict(sd)
    return cfg, unet_celeba.Net(sd, cfg), model


@pytest.mark.parametrize("rw,rh", [(1, 1), (2, 2)])
def test_sampler_against_the_oracle_loop(small_net, rw, rh):
    """ddnm_diffusion with JPEG (Q = 50, box 0.98) at 32 px, B = 3, T = 4 and one time-travel jump of two steps, against the
    oracle's unchanged loop over the wrapped model on the same noise tape: within 2e-4, the project's loop bar.  The
    restoration re-encodes to the measured levels everywhere.  Measured on the MI355X (printed): 1.21e-6 at (1,1), 4.5e-7 at
    (2,2), x and x0 alike; no level re-encodes differently."""
    from ddnm_amd.functions.svd_ddnm import ddnm_diffusion
    from oracle import cases, sampler, schedule
    cfg, net, model = small_net
    d = cfg.data.image_size
    assert d == 32
    op, M = _pair("bt601", d, rw, rh)
    n_it = len(schedule.jump_times(4, 2, 2)) - 1
    assert n_it == 4 + 2 * 2
    x_orig, x_T, tape = cases.sampler_case(cfg, B, n_it)
    y_d = op.A(x_orig.cuda())
    measured = op.levels(y_d)
    y = y_d.cpu()
    kw = dict(T_sampling=4, travel_length=2, travel_repeat=2)
    ref, ref0 = sampler.ddnm_diffusion(x_T.clone(), net, cases.betas(), ETA, CellOperator(M, _np(y), 0.98), y, tape, **kw)
    xs, x0s = ddnm_diffusion(x_T.cuda(), model, cases.betas().cuda(), ETA, op, y_d, cls_fn=None, classes=None, config=cfg,
                             noise=[n.cuda() for n in tape])
    e, e0 = rel(xs[0], ref), rel(x0s[0], ref0)
    again = op.levels(op.A(xs[0].cuda()))
    wrong = int((again != measured).sum())
    print(f"DDNM loop, jpeg site={rw}x{rh} Q=50: x rel-L2 {e:.3e}, x0 rel-L2 {e0:.3e}; levels that re-encode differently: "
          f"{wrong} of {measured.numel()}")
    assert max(e, e0) < 2e-4
    assert wrong == 0


# ---------------------------------------------------------------------------------------------- 4. runner
J420 = ["--path_y", "synthetic:3", "--eta", "0.85", "--deg", "jpeg_420", "--deg_scale", "30"]


def test_runner_plain_fused_and_two_samples(hip, tmp_path, monkeypatch, capsys):
    """main.py on the mini configuration (64 px, T = 4, synthetic images) with `--deg jpeg_420 --deg_scale 30`: the plain
    run completes with its PNGs and a PSNR line; DDNM_FUSE_BATCHES=2 and sample 0 of DDNM_SAMPLES=2 restore what it
    restores, within 3e-6 (BAR of tests/test_gpu_fuse.py); the only step entry point is ddnm_step_jpeg_f32 (ops.step_call
    picks its keyed form); Apy_0.png, the decoded JPEG, is a full picture."""
    from PIL import Image
    from ddnm_amd import ops
    _mini_yaml(tmp_path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("DDNM_SAMPLES", raising=False)
    seen = []
    orig = ops.step_call
    monkeypatch.setattr(ops, "step_call", lambda name, *a: (seen.append(name), orig(name, *a))[1])
    argv = J420 + ["--sigma_y", "0."]
    calls1, psnr1, img1, names1, apy1 = _run_main(tmp_path, monkeypatch, "plain", argv, None)
    calls2, psnr2, img2, names2, apy2 = _run_main(tmp_path, monkeypatch, "fused", argv, 2)
    monkeypatch.setenv("DDNM_SAMPLES", "2")
    calls3, _, img3, names3, _ = _run_main(tmp_path, monkeypatch, "samples", argv, None)
    monkeypatch.delenv("DDNM_SAMPLES")
    out = capsys.readouterr().out
    assert out.count("Number of samples: 3") == 3 and out.count("Total Average PSNR") == 3, out[-3000:]
    assert set(seen) == {"ddnm_step_jpeg_f32"}
    assert calls1 == [1] and calls2 == [2, 1] and calls3 == [2]
    assert names1 == names2 == [f"{i}_0.png" for i in range(3)] and apy1 == apy2 and len(apy1) == 6
    assert names3 == sorted(f"{i}_{k}.png" for i in range(3) for k in range(2))
    e_f, e_s = rel(img2, img1), rel(img3[0::2], img1)
    print(f"jpeg_420 Q=30 runner: fused K=2 vs plain rel-L2 {e_f:.3e}, sample 0 of 2 vs plain rel-L2 {e_s:.3e}, "
          f"PSNR {[round(float(p), 2) for p in psnr1]}")
    assert torch.isfinite(img1).all() and torch.isfinite(psnr1).all() and len(psnr1) == 3
    assert e_f < BAR and e_s < BAR
    assert (psnr1 - psnr2).abs().max() < 1e-3 and rel(img3[1::2], img1) > 1e-3          # sample 1 is another draw
    shown = np.asarray(Image.open(tmp_path / "exp" / "image_samples" / "plain" / "Apy" / "Apy_0.png"))
    assert shown.shape == (64, 64, 3) and len(np.unique(shown)) > 16


@pytest.mark.parametrize("extra,message", [(["--sigma_y", "0.1"], "bounded, not Gaussian"),
                                           (["--sigma_y", "0.", "--simplified"], "--simplified with --deg jpeg_420"),
                                           (["--sigma_y", "0.", "--deg_scale", "0.5"], "1..100")])
def test_runner_refusals(hip, tmp_path, monkeypatch, caplog, extra, message):
    """--sigma_y 0.1, --simplified and a --deg_scale that is no quality end the run with the documented message (main.py
    logs the exception) before anything is restored."""
    import main
    _mini_yaml(tmp_path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("DDNM_RANDOM_WEIGHTS", "1")
    with caplog.at_level(logging.ERROR):
        assert main.main(["--ni", "--config", "mini.yml", "-i", "refused"] + J420 + extra) == 0
    assert message in caplog.text, caplog.text[-2000:]
    assert not list((tmp_path / "exp" / "image_samples" / "refused").glob("*.png"))


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    root = tmp_path_factory.mktemp("jpeg_measurements")
    _mini_yaml(root)
    return str(root)


def test_round_trip_of_saved_measurements(hip, workdir):
    """DDNM_SAVE_Y=1, then the run over measurements:<its y/>: the same PNG bytes
    (tests/test_gpu_measurements.py::_round_trip); the saved rows hold the 64 x 64 luma and the two 32 x 32 chroma planes
    of dequantised coefficients."""
    deg = ["--deg", "jpeg_420", "--deg_scale", "30", "--sigma_y", "0."]
    truth, given = _round_trip(workdir, "jpeg", deg, deg, 2)
    for i in range(2):
        row = np.load(os.path.join(truth["folder"], "y", f"y_{i}.npy"))
        assert row.dtype == np.float32 and row.shape == (6144,) and np.isfinite(row).all()
    assert [c["y"].shape for c in given["cons"]] == [(1, 6144)] * 2


def test_cons_metric_in_a_ground_truth_run(hip, workdir):
    """DDNM_METRICS=cons: `Cons:` lines and `Max Cons`; the value is printed for the record and is no bar
    (0 exactly when every restoration re-encodes to its measured levels)."""
    run = _run(workdir, "cons", ["--path_y", "synthetic:2", "--sigma_y", "0.", "--deg", "jpeg_420", "--deg_scale", "30"],
               DDNM_METRICS="cons")
    lines = run["out"].splitlines()
    assert len([ln for ln in lines if ln.startswith("Cons: ")]) == 2 and "Max Cons:" in run["out"]
    assert len(run["cons"]) == 2 and all(c["ax"].shape == c["y"].shape for c in run["cons"])
    print(f"--deg jpeg_420 --deg_scale 30: Max Cons {run['metrics']['cons_max']:.3e}")
    assert np.isfinite(run["metrics"]["cons_max"])


def test_entry_points_validate_on_device_pointers(hip):
    """The refusals of tests/test_jpeg_host.py with real device addresses: nothing is launched."""
    buf = torch.zeros(256, device="cuda")
    check_jpeg_validation(hip, buf.data_ptr())
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
