"""Chroma-subsampled restoration on the GPU (svd_operators.ChromaSubsample, the `*_chroma_*` entry points): A / A^+ against
the dense float64 model of tests/test_chroma_host.py, the fused noise-free step and the one-launch DDNM+ step against that
model, their three noise sources against each other, both samplers against the oracle's loops over the model, and the
runner.

Shapes: d = 16 with the five sites (at (8,8) two lanes share a site, at rw = 2 a lane holds two), d = 64 with (2,2) (three
workgroups), d = 12 with (4,4) (nine sites: a measurement row of 162 entries, so the rows of images 1 and 2 are not
16-byte aligned and Y moves one float at a time), one direct ABI case with H = 8, W = 32 and (4,1); B = 3, eps as a
[B, 3, d, d] tensor and as the [:, :3] view of [B, 6, d, d].  The bars are those the project holds for the same
quantities elsewhere (named at each).  Every test prints what it measured, and next to the operator's
figures the same closed form evaluated in numpy float32 on the CPU, the figure a bar would be derived from."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests.helpers import rel
from tests.test_chroma_host import (BT601, BT709, ETA, PLUS_SETTINGS, _Dense, check_chroma_validation, closed_A, closed_pinv,
                                    dense_matrix, kernel_matrix, model_operator)
from tests.test_gpu_fuse import BAR, _mini_yaml, _run_main
from tests.test_gpu_measurements import _round_trip, _run
from tests.test_gpu_mosaic import _et, _sources_of

pytestmark = pytest.mark.gpu

B = 3
SHAPES = [(16, 2, 1), (16, 4, 1), (16, 2, 2), (16, 4, 4), (16, 8, 8), (64, 2, 2), (12, 4, 4)]      # (d, rw, rh)
CASES = [("bt601", d, rw, rh) for d, rw, rh in SHAPES] + [("bt709", 16, 2, 2), ("bt709", 16, 8, 8)]
MATS = {"bt601": BT601, "bt709": BT709}
ABAR_T = 0.45


@functools.lru_cache(maxsize=None)
def _pair(name, d, rw, rh):
    """(engine ChromaSubsample, dense float64 model with the matrix the kernels get); built once per case."""
    from ddnm_amd.functions import svd_operators as E
    return E.ChromaSubsample(3, d, rw, rh, "cuda", matrix=MATS[name]), model_operator(rw, rh, kernel_matrix(MATS[name]), d)


@functools.lru_cache(maxsize=None)
def _inputs(d):
    """Seeded (x_orig, x_t, eps with 6 channels, n) of one size, shared by its tests and never written to."""
    g = torch.Generator().manual_seed(77 + 100 * d)
    return (torch.rand(B, 3, d, d, generator=g) * 2 - 1, torch.randn(B, 3, d, d, generator=g),
            torch.randn(B, 6, d, d, generator=g), torch.randn(B, 3, d, d, generator=g))


def _np(t):
    return t.detach().double().cpu().reshape(t.shape[0], -1).numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_the_shapes_are_what_the_header_says():
    assert (12 * 12 + 2 * 9) % 4 == 2 and all((d * d + 2 * d * d // (rw * rh)) % 4 == 0 for d, rw, rh in SHAPES[:-1])
    assert (64 // 2) * (64 // 4) * B > 2 * 256                      # strips of d = 64, (2,2): more than two workgroups


# ---------------------------------------------------------------------------------------------- 1. operator
@pytest.mark.parametrize("name,d,rw,rh", CASES)
def test_A_and_A_pinv_against_the_model(hip, name, d, rw, rh):
    """A, A^+ and A A^+ y = y within 1e-6 (rel-L2) of the float64 model; singulars() is the closed-form spectrum.
    Measured on the MI355X (printed, with the numpy float32 figure of the same closed form): A at most 4.7e-8, A^+ 5.4e-8,
    A A^+ y 7.8e-8 (8 x 8, where A^+ divides by 0.068; numpy float32 7.5e-8)."""
    op, M = _pair(name, d, rw, rh)
    Mk = kernel_matrix(MATS[name])
    x = _inputs(d)[0]
    g = torch.Generator().manual_seed(5)
    yr = torch.randn(B, op.measurement_size(), generator=g)
    y, xp = op.A(x.cuda()), op.A_pinv(yr.cuda())
    back = op.A(xp)
    torch.cuda.synchronize()
    assert y.shape == (B, d * d + 2 * d * d // (rw * rh)) and xp.shape == (B, 3 * d * d)
    e_A, e_P, e_back = rel(y, M.A(x.double())), rel(xp, M.A_pinv(yr.double())), rel(back.cpu(), yr)
    xp32 = closed_pinv(rw, rh, Mk, d, yr.numpy(), np.float32)
    f_A = rel(_t(closed_A(rw, rh, Mk, d, x.numpy(), np.float32)), M.A(x.double()))
    f_P, f_back = rel(_t(xp32), M.A_pinv(yr.double())), rel(_t(closed_A(rw, rh, Mk, d, xp32, np.float32)), yr)
    print(f"chroma operator {name} d={d} site={rw}x{rh}: A rel-L2 {e_A:.3e}, A^+ {e_P:.3e}, A A^+ y = y {e_back:.3e}"
          f"   (numpy float32: {f_A:.3e}, {f_P:.3e}, {f_back:.3e})")
    assert e_A <= 1e-6 and e_P <= 1e-6 and e_back <= 1e-6
    assert rel(op.singulars(), _t(M.S)) <= 1e-6 and op.singulars().numel() == y.shape[1]


def test_direct_abi_on_a_wide_image(hip):
    """H = 8, W = 32, site (4,1) through the C ABI: A, A^+, the noise-free step (lambda = 0.3) and the DDNM+ step (mixed)
    against the image's dense matrix built entry by entry.  A swap of rw and rh or of rows and columns moves whole sites.
    Bars: 1e-6 for A and A^+, 3e-6 for the steps."""
    from ddnm_amd import ops
    H, W, rw, rh = 8, 32, 4, 1
    Mk = kernel_matrix(BT601)
    D = _Dense(dense_matrix(rw, rh, Mk, H, W))
    m9 = (ctypes.c_float * 9)(*[float(v) for v in Mk.reshape(-1)])
    g = torch.Generator().manual_seed(9)
    x, xt, et, nz = (torch.randn(B, 3, H, W, generator=g) for _ in range(4))
    L = H * W + 2 * H * W // 4
    yr = torch.randn(B, L, generator=g)
    x_d, xt_d, et_d, nz_d, yr_d = (v.cuda() for v in (x, xt, et, nz, yr))
    y_d, xp_d = torch.empty(B, L, device="cuda"), torch.empty(B, 3 * H * W, device="cuda")
    ops.call("ddnm_op_chroma_A_f32", x_d.data_ptr(), y_d.data_ptr(), B, H, W, rw, rh, m9)
    ops.call("ddnm_op_chroma_pinv_f32", yr_d.data_ptr(), xp_d.data_ptr(), B, H, W, rw, rh, m9)
    torch.cuda.synchronize()
    e_A, e_P = rel(y_d, _t(_np(x) @ D.Amat.T)), rel(xp_d, _t(_np(yr) @ D.pinv.T))
    y64 = _np(x) @ D.Amat.T
    yy_d = _t(y64).float().cuda()
    y64 = _np(yy_d)
    abar_next, sigma_y = PLUS_SETTINGS["mixed"]
    s = ops.step_scalars(torch.tensor(ABAR_T), torch.tensor(abar_next), ETA, lam=0.3)
    a, sigma_t = abar_next ** 0.5, (1 - abar_next) ** 0.5
    x0 = (_np(xt) - _np(et) * (1 - ABAR_T) ** 0.5) / ABAR_T ** 0.5
    want = a * (x0 - 0.3 * ((x0 @ D.Amat.T - y64) @ D.pinv.T)) + sigma_t * ETA * _np(nz) + sigma_t * (1 - ETA ** 2) ** 0.5 * _np(et)
    want_p = D.plus(x0, _np(et), _np(nz), y64, a, sigma_y, sigma_t, ETA)
    x0_d, out_d, x0p_d, outp_d = (torch.empty_like(xt_d) for _ in range(4))
    ops.step_call("ddnm_step_chroma_f32", xt_d, et_d, nz_d, yy_d, x0_d.data_ptr(), out_d.data_ptr(), B, H, W, rw, rh, m9, s)
    ops.step_call("ddnm_step_plus_chroma_f32", xt_d, et_d, nz_d, yy_d, x0p_d.data_ptr(), outp_d.data_ptr(), B, H, W, rw, rh, m9,
                  float(sigma_y), float(sigma_t), ETA, s)
    torch.cuda.synchronize()
    e_S, e_Sp = rel(out_d.reshape(B, -1), _t(want)), rel(outp_d.reshape(B, -1), _t(want_p))
    print(f"chroma ABI 8 x 32 site 4x1: A {e_A:.3e}, A^+ {e_P:.3e}, step {e_S:.3e}, DDNM+ step {e_Sp:.3e}")
    assert e_A <= 1e-6 and e_P <= 1e-6 and e_S <= 3e-6 and e_Sp <= 3e-6
    assert torch.equal(x0_d, ops.step_x0(xt_d, et_d, s)) and torch.equal(x0p_d, x0_d)


# ---------------------------------------------------------------------------------------------- 2. noise-free step
@pytest.mark.parametrize("name,d,rw,rh", CASES)
@pytest.mark.parametrize("six", [False, True])
def test_fused_step_against_the_model(hip, name, d, rw, rh, six):
    """lambda = 1 and 0.3: x0 bit-identical to ddnm_step_x0_f32, x_{t-1} within 3e-6 of the float64 model and of the generic
    A_functions.ddnm_step composition over the same object; the result does not depend on whether x0 is asked for.
    Measured on the MI355X (printed): at most 1.18e-7 against float64, 3.3e-8 against the generic composition."""
    from ddnm_amd import ops
    from ddnm_amd.functions.svd_operators import A_functions
    op, M = _pair(name, d, rw, rh)
    x, xt, et6, nz = _inputs(d)
    y = M.A(x.double())
    xt_d, et_d, nz_d, y_d = xt.cuda(), _et(et6, six), nz.cuda(), y.float().cuda()
    for lam in (1.0, 0.3):
        s = ops.step_scalars(torch.tensor(ABAR_T), torch.tensor(0.6), ETA, lam=lam)
        x0_m, want = M.step(_np(xt), _np(et6[:, :3]), _np(nz), _np(y.float()), ABAR_T, 0.6, 0.0, ETA, lam=lam)
        x0_e, out, out2, x0_g, out_g = (torch.empty(B, 3, d, d, device="cuda") for _ in range(5))
        op.ddnm_step(xt_d, et_d, nz_d, y_d, s, x0_e, out)
        op.ddnm_step(xt_d, et_d, nz_d, y_d, s, None, out2)
        A_functions.ddnm_step(op, xt_d, et_d, nz_d, y_d, s, x0_g, out_g)
        x0_k = ops.step_x0(xt_d, et_d, s)
        torch.cuda.synchronize()
        e64, eg = rel(out.reshape(B, -1), _t(want)), rel(out, out_g)
        print(f"chroma step {name} d={d} site={rw}x{rh} six={six} lambda={lam}: vs float64 {e64:.3e}, vs generic {eg:.3e}")
        assert torch.equal(x0_e, x0_k) and rel(x0_e.reshape(B, -1), _t(x0_m)) < 1e-6
        assert e64 <= 3e-6 and eg <= 3e-6
        assert torch.equal(out, out2)


@pytest.mark.parametrize("d,rw,rh", SHAPES)
@pytest.mark.parametrize("kind", ["philox", "keyed"])
def test_fused_step_noise_sources_are_the_same_draw(hip, d, rw, rh, kind):
    """In-kernel Philox and the keyed table == the tensor source filled by the same keys, and image b of the batch == that
    image stepped alone, all by torch.equal."""
    from ddnm_amd import ops
    op, M = _pair("bt601", d, rw, rh)
    x, xt, et6, _ = _inputs(d)
    xt_d, et_d, y_d = xt.cuda(), et6.cuda()[:, :3], M.A(x.double()).float().cuda()
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


# ---------------------------------------------------------------------------------------------- 3. DDNM+ step
def _plus_scalars(abar_next):
    from ddnm_amd import ops
    s = ops.step_scalars(torch.tensor(ABAR_T), torch.tensor(abar_next), ETA)
    return s, float((1 - torch.tensor(abar_next)).sqrt())


@pytest.mark.parametrize("name,d,rw,rh", CASES)
@pytest.mark.parametrize("setting", sorted(PLUS_SETTINGS))
def test_fused_noisy_step(hip, name, d, rw, rh, setting):
    """One launch against the float64 model within 3e-6, with luma full and chroma damped (mixed), everything damped and
    everything full (tests/test_chroma_host.py::test_regimes_are_what_their_names_say), for a tensor (eps as a tensor and
    as the 6-channel view), the in-kernel Philox and the keyed noise source.  Philox and keyed equal the tensor source
    filled by the same keys bit for bit, and so does an image of the batch stepped alone; x0 is that of ddnm_step_x0_f32.
    Measured on the MI355X (printed): at most 8.2e-8 / 1.23e-7 / 1.19e-7 in the damped / full / mixed setting."""
    from ddnm_amd import ops
    op, M = _pair(name, d, rw, rh)
    abar_next, sigma_y = PLUS_SETTINGS[setting]
    x, xt, et6, nz = _inputs(d)
    y = M.A(x.double()).float()
    xt_d, y_d = xt.cuda(), y.cuda()
    for kind, six in (("tensor", False), ("tensor", True), ("philox", True), ("keyed", False)):
        et_d = _et(et6, six)
        s, sigma_t = _plus_scalars(abar_next)
        if kind == "tensor":
            arg, tensor, alone = nz.cuda(), nz.cuda(), None
        else:
            arg, stamp, tensor, alone = _sources_of(kind, xt_d)
            stamp(s)
        x0_f, out_f = torch.empty_like(xt_d), torch.empty_like(xt_d)
        op.begin_plus_run(y_d)
        op.ddnm_plus_step(xt_d, et_d, arg, s, sigma_y, sigma_t, ETA, x0_f, out_f)
        x0_k = ops.step_x0(xt_d, et_d, s)
        torch.cuda.synchronize()
        x0_m, want = M.step(_np(xt), _np(et6[:, :3]), _np(tensor), _np(y), ABAR_T, abar_next, sigma_y, ETA)
        e64 = rel(out_f.reshape(B, -1), _t(want))
        print(f"chroma DDNM+ step {name} d={d} site={rw}x{rh} {setting} noise={kind} six={six}: vs float64 {e64:.3e}")
        assert torch.equal(x0_f, x0_k) and rel(x0_f.reshape(B, -1), _t(x0_m)) < 1e-6
        assert e64 <= 3e-6
        if kind != "tensor":                                # the same draw through the tensor source: the same bits
            s2, _ = _plus_scalars(abar_next)
            x0_t, out_t = torch.empty_like(xt_d), torch.empty_like(xt_d)
            op.ddnm_plus_step(xt_d, et_d, tensor, s2, sigma_y, sigma_t, ETA, x0_t, out_t)
            torch.cuda.synchronize()
            assert torch.equal(x0_f, x0_t) and torch.equal(out_f, out_t)
        for i in range(B):                                  # an image of the batch == that image alone
            s_i, _ = _plus_scalars(abar_next)
            if kind == "tensor":
                arg_i = tensor[i:i + 1].contiguous()
            else:
                arg_i, stamp_i = alone(i)
                stamp_i(s_i)
            x0_i, out_i = torch.empty_like(xt_d[:1]), torch.empty_like(xt_d[:1])
            op.begin_plus_run(y_d[i:i + 1].contiguous())
            op.ddnm_plus_step(xt_d[i:i + 1].contiguous(), et_d[i:i + 1], arg_i, s_i, sigma_y, sigma_t, ETA, x0_i, out_i)
            torch.cuda.synchronize()
            assert torch.equal(x0_f[i:i + 1], x0_i) and torch.equal(out_f[i:i + 1], out_i), (kind, i)


# ---------------------------------------------------------------------------------------------- 4. loops
@pytest.fixture(scope="module")
def small_net(hip):
    from ddnm_amd.guided_diffusion.models import Model
    from oracle import cases, unet_celeba
    cfg, sd = cases.celeba_net("small")
    cfg.time_travel.T_sampling, cfg.time_travel.travel_length, cfg.time_travel.travel_repeat = 4, 2, 2
    model = Model(cfg)
    model.load_state_dict(sd)
    return cfg, unet_celeba.Net(sd, cfg), model


@pytest.mark.parametrize("rw,rh", [(2, 2), (8, 8)])
@pytest.mark.parametrize("plus", [False, True])
def test_samplers_against_the_oracle_loops(small_net, plus, rw, rh):
    """ddnm_diffusion / ddnm_plus_diffusion (sigma_y = 0.2) with ChromaSubsample at 32 px, B = 3, T = 4 and one time-travel
    jump of two steps, against the oracle's loops over the dense model on the same noise tape: within 2e-4, the bar of the
    mosaic and old-photo loops.  Measured on the MI355X (printed): DDNM 4.39e-7 (2 x 2) and 4.51e-7 (8 x 8), DDNM+ 4.46e-7
    and 4.59e-7, x and x0 alike."""
    from ddnm_amd.functions import svd_operators as E
    from ddnm_amd.functions.svd_ddnm import ddnm_diffusion, ddnm_plus_diffusion
    from oracle import cases, sampler, schedule
    cfg, net, model = small_net
    d = cfg.data.image_size
    assert d == 32
    op, M = E.ChromaSubsample(3, d, rw, rh, "cuda"), model_operator(rw, rh, kernel_matrix(BT601), d)
    n_it = len(schedule.jump_times(4, 2, 2)) - 1
    assert n_it == 4 + 2 * 2
    x_orig, x_T, tape = cases.sampler_case(cfg, B, n_it)
    y = M.A(x_orig)
    kw = dict(T_sampling=4, travel_length=2, travel_repeat=2)
    if plus:
        ref, ref0 = sampler.ddnm_plus_diffusion(x_T.clone(), net, cases.betas(), ETA, M, y, 0.2, tape, **kw)
        xs, x0s = ddnm_plus_diffusion(x_T.cuda(), model, cases.betas().cuda(), ETA, op, y.cuda(), 0.2, cls_fn=None,
                                      classes=None, config=cfg, noise=[n.cuda() for n in tape])
    else:
        ref, ref0 = sampler.ddnm_diffusion(x_T.clone(), net, cases.betas(), ETA, M, y, tape, **kw)
        xs, x0s = ddnm_diffusion(x_T.cuda(), model, cases.betas().cuda(), ETA, op, y.cuda(), cls_fn=None, classes=None,
                                 config=cfg, noise=[n.cuda() for n in tape])
    e, e0 = rel(xs[0], ref), rel(x0s[0], ref0)
    print(f"{'DDNM+' if plus else 'DDNM'} loop, chroma site={rw}x{rh}: x rel-L2 {e:.3e}, x0 rel-L2 {e0:.3e}")
    assert max(e, e0) < 2e-4


# ---------------------------------------------------------------------------------------------- 5. runner
C420 = ["--path_y", "synthetic:3", "--eta", "0.85", "--deg", "chroma_420"]


def test_runner_noisy_fused(hip, tmp_path, monkeypatch, capsys):
    """main.py on the mini configuration (64 px, T = 4, synthetic images): `--deg chroma_420 --sigma_y 0.1 --add_noise`
    fused by two (DDNM+ through the one-launch hook with per-image keys) completes with its PNGs and a PSNR line;
    Apy_{i}.png shows A^+ y, a full picture."""
    from PIL import Image
    from ddnm_amd import ops
    _mini_yaml(tmp_path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("DDNM_SAMPLES", raising=False)
    seen = []
    orig = ops.step_call
    monkeypatch.setattr(ops, "step_call", lambda name, *a: (seen.append(name), orig(name, *a))[1])
    _, psnr, img, names, apy = _run_main(tmp_path, monkeypatch, "noisy", C420 + ["--sigma_y", "0.1", "--add_noise"], 2)
    assert names == [f"{i}_0.png" for i in range(3)] and len(apy) == 6
    assert torch.isfinite(img).all() and torch.isfinite(psnr).all() and len(psnr) == 3
    assert set(seen) == {"ddnm_step_plus_chroma_f32"}
    shown = np.asarray(Image.open(tmp_path / "exp" / "image_samples" / "noisy" / "Apy" / "Apy_0.png"))
    assert shown.shape == (64, 64, 3) and len(np.unique(shown)) > 16
    out = capsys.readouterr().out
    assert out.count("Number of samples: 3") == 1 and out.count("Total Average PSNR") == 1, out[-3000:]


def test_runner_plain_fused_and_two_samples(hip, tmp_path, monkeypatch, capsys):
    """DDNM_FUSE_BATCHES=2 and sample 0 of DDNM_SAMPLES=2 restore what the plain run restores, within 3e-6 (BAR of
    tests/test_gpu_fuse.py); --deg_scale is not read."""
    from ddnm_amd import ops
    _mini_yaml(tmp_path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("DDNM_SAMPLES", raising=False)
    seen = []
    orig = ops.step_call
    monkeypatch.setattr(ops, "step_call", lambda name, *a: (seen.append(name), orig(name, *a))[1])
    argv = C420 + ["--sigma_y", "0."]
    calls1, psnr1, img1, names1, apy1 = _run_main(tmp_path, monkeypatch, "plain", argv, None)
    calls2, psnr2, img2, names2, apy2 = _run_main(tmp_path, monkeypatch, "fused", argv + ["--deg_scale", "7"], 2)
    monkeypatch.setenv("DDNM_SAMPLES", "2")
    calls3, _, img3, names3, _ = _run_main(tmp_path, monkeypatch, "samples", argv, None)
    monkeypatch.delenv("DDNM_SAMPLES")
    out = capsys.readouterr().out
    assert out.count("Number of samples: 3") == 3, out[-3000:]
    assert set(seen) == {"ddnm_step_chroma_f32"}
    assert calls1 == [1] and calls2 == [2, 1] and calls3 == [2]
    assert names1 == names2 == [f"{i}_0.png" for i in range(3)] and apy1 == apy2 and len(apy1) == 6
    assert names3 == sorted(f"{i}_{k}.png" for i in range(3) for k in range(2))
    e_f, e_s = rel(img2, img1), rel(img3[0::2], img1)
    print(f"chroma_420 runner: fused K=2 vs plain rel-L2 {e_f:.3e}, sample 0 of 2 vs plain rel-L2 {e_s:.3e}")
    assert torch.isfinite(img1).all() and e_f < BAR and e_s < BAR
    assert (psnr1 - psnr2).abs().max() < 1e-3 and rel(img3[1::2], img1) > 1e-3          # sample 1 is another draw


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    root = tmp_path_factory.mktemp("chroma_measurements")
    _mini_yaml(root)
    return str(root)


def test_round_trip_of_saved_measurements(hip, workdir):
    """DDNM_SAVE_Y=1 with noisy measurements, then the run over measurements:<its y/>: the same PNG bytes
    (tests/test_gpu_measurements.py::_round_trip); the saved rows hold the luma plane and the two 32 x 32 chroma planes."""
    noisy = ["--deg", "chroma_420", "--sigma_y", "0.1"]
    truth, given = _round_trip(workdir, "chroma", noisy + ["--add_noise"], noisy, 2)
    for i in range(2):
        row = np.load(os.path.join(truth["folder"], "y", f"y_{i}.npy"))
        assert row.dtype == np.float32 and row.shape == (64 * 64 + 2 * 32 * 32,) and np.isfinite(row).all()
    assert [c["y"].shape for c in given["cons"]] == [(1, 6144)] * 2


def test_cons_metric_in_a_ground_truth_run(hip, workdir):
    """DDNM_METRICS=cons: `Cons:` lines and `Max Cons`; the value is printed for the record and is no
    bar."""
    for deg in (["--deg", "chroma_420"], ["--deg", "chroma_sub", "--deg_scale", "8"]):
        run = _run(workdir, "cons_" + deg[-1], ["--path_y", "synthetic:2", "--sigma_y", "0."] + deg, DDNM_METRICS="cons")
        lines = run["out"].splitlines()
        assert len([ln for ln in lines if ln.startswith("Cons: ")]) == 2 and "Max Cons:" in run["out"]
        assert len(run["cons"]) == 2 and all(c["ax"].shape == c["y"].shape for c in run["cons"])
        print(f"{' '.join(deg)}: Max Cons {run['metrics']['cons_max']:.3e}")
        assert np.isfinite(run["metrics"]["cons_max"])


def test_entry_points_validate_on_device_pointers(hip):
    """The refusals of tests/test_chroma_host.py with real device addresses: nothing is launched."""
    buf = torch.zeros(256, device="cuda")
    check_chroma_validation(hip, buf.data_ptr())
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
