"""Old-photo restoration on the GPU (svd_operators.MaskColorSR, the `*_mcsr_*` entry points): A / A^+ against the dense
float64 model of tests/test_mcsr_host.py and against the Composition of the simplified path, the fused noise-free step
and the one-launch DDNM+ step against that model, their three noise sources against each other, both samplers against
the oracle's loops over the model, and the runner.

Shapes: d = 16 with r = 1, 2, 4, 8 (r = 8: two lanes share a site; r = 1, 2: a lane holds several) and d = 64 with r = 4
(three workgroups), B = 3, eps as a [B, 3, d, d] tensor and as the [:, :3] view of [B, 6, d, d].  Masks: none (the NULL
path), all ones, random at 60 %, random with an empty site, random with a site whose one kept pixel is its last, and
site-aligned.  The bars are those the project holds for the same quantities elsewhere (named at each)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.helpers import rel
from tests.test_gpu_fuse import BAR, _mini_yaml, _run_main
from tests.test_gpu_measurements import _round_trip, _run
from tests.test_gpu_mosaic import _et, _sources_of
from tests.test_mcsr_host import (ETA, PLUS_SETTINGS, W_LUMA, W_THIRDS, check_mcsr_validation, kernel_weights, model_operator,
                                  site_counts)

pytestmark = pytest.mark.gpu

B = 3
SHAPES = [(16, 1), (16, 2), (16, 4), (16, 8), (64, 4)]
MASKS = ["null", "ones", "random", "empty_site", "k1_last", "aligned"]
ABAR_T = 0.45


def make_mask(name, d, r):
    """The mask `name` of a d x d image pooled by r (None: the NULL path)."""
    if name == "null":
        return None
    if name == "ones":
        return np.ones((d, d), np.float32)
    rng = np.random.default_rng(1000 + 10 * d + r)
    n = d // r
    if name == "aligned":                                   # whole sites kept or missing
        return np.kron((rng.random((n, n)) < 0.6), np.ones((r, r))).astype(np.float32)
    m = (rng.random((d, d)) < 0.6).astype(np.float32)
    sy, sx = n // 2, n - 1                                   # a site off the first row, in the last column
    if name == "empty_site":
        m[sy * r:(sy + 1) * r, sx * r:(sx + 1) * r] = 0
    elif name == "k1_last":
        m[sy * r:(sy + 1) * r, sx * r:(sx + 1) * r] = 0
        m[(sy + 1) * r - 1, (sx + 1) * r - 1] = 1
    return m


@functools.lru_cache(maxsize=None)
def _pair(name, d, r, w=W_THIRDS):
    """(engine MaskColorSR, dense float64 model with the weights the kernels get, mask); built once per case."""
    from ddnm_amd.functions import svd_operators as E
    mask = make_mask(name, d, r)
    return E.MaskColorSR(3, d, mask, r, "cuda", weights=w), model_operator(mask, r, kernel_weights(w), d), mask


@functools.lru_cache(maxsize=None)
def _inputs(d, r):
    """Seeded (x_orig, x_t, eps with 6 channels, n) of one shape, shared by its tests and never written to."""
    g = torch.Generator().manual_seed(77 + 100 * d + r)
    return (torch.rand(B, 3, d, d, generator=g) * 2 - 1, torch.randn(B, 3, d, d, generator=g),
            torch.randn(B, 6, d, d, generator=g), torch.randn(B, 3, d, d, generator=g))


def _np(t):
    return t.detach().double().cpu().reshape(t.shape[0], -1).numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


CASES = [(m, d, r) for d, r in SHAPES for m in MASKS]


def test_the_masks_are_what_their_names_say():
    for d, r in SHAPES:
        assert site_counts(make_mask("ones", d, r), r, d).min() == r * r
        assert site_counts(make_mask("empty_site", d, r), r, d).min() == 0
        m = make_mask("k1_last", d, r)
        n = d // r
        assert site_counts(m, r, d).reshape(n, n)[n // 2, n - 1] == 1 and m[(n // 2 + 1) * r - 1, d - 1] == 1
        assert set(site_counts(make_mask("aligned", d, r), r, d).tolist()) == {0, r * r}
        k = site_counts(make_mask("random", d, r), r, d)
        assert r == 1 or (0 < k.min() < k.max())            # sites the mask cuts, at several counts


# ---------------------------------------------------------------------------------------------- 1. operator
@pytest.mark.parametrize("name,d,r", CASES + [("luma", 16, 4)])
def test_A_and_A_pinv_against_the_model(hip, name, d, r):
    """A and A^+ within 1e-6 (rel-L2) of the float64 model, A A^+ y = y on the sites that keep a pixel, singulars() the
    s_j, and A equal to the Composition of the simplified path within 1e-6.  Measured on the MI355X (printed): A at most
    9.5e-8, A^+ 9.8e-8, A A^+ y 2.3e-7 (r = 8), against the Composition 1.9e-7."""
    from ddnm_amd.functions import svd_operators as E
    luma = name == "luma"
    op, M, mask = _pair("random", d, r, W_LUMA) if luma else _pair(name, d, r)
    x = _inputs(d, r)[0]
    g = torch.Generator().manual_seed(5)
    yr = torch.randn(B, (d // r) ** 2, generator=g)
    y, xp = op.A(x.cuda()), op.A_pinv(yr.cuda())
    back = op.A(xp)
    torch.cuda.synchronize()
    assert y.shape == (B, (d // r) ** 2) and xp.shape == (B, 3 * d * d)
    e_A, e_P = rel(y, M.A(x.double())), rel(xp, M.A_pinv(yr.double()))
    kept = _t(site_counts(mask, r, d) > 0)
    e_back = rel(back.cpu()[:, kept], yr[:, kept])
    print(f"mcsr operator {name} d={d} r={r}: A rel-L2 {e_A:.3e}, A^+ {e_P:.3e}, A A^+ y = y {e_back:.3e}")
    assert e_A <= 1e-6 and e_P <= 1e-6 and e_back <= 1e-6
    missing = torch.zeros(d * d, dtype=torch.bool) if mask is None else _t(mask.reshape(-1)) == 0
    assert bool((back.cpu()[:, ~kept] == 0).all()) and bool((xp.cpu().reshape(B, 3, -1)[:, :, missing] == 0).all())
    s = np.sqrt(site_counts(mask, r, d)) * np.sqrt((np.asarray(kernel_weights(op.weights)) ** 2).sum()) / r ** 2
    assert rel(op.singulars(), _t(s)) <= 1e-6 and op.measurement_size() == y.shape[1]
    if not luma:
        ones = torch.ones(d, d) if mask is None else _t(mask)
        comp = E.mask_color_sr(3, d, ones, r, "cuda")
        e_C = rel(y, comp.A(x.cuda()))
        print(f"    against the Composition: {e_C:.3e}")
        assert e_C <= 1e-6


# ---------------------------------------------------------------------------------------------- 2. noise-free step
@pytest.mark.parametrize("name,d,r", CASES + [("luma", 16, 4)])
@pytest.mark.parametrize("six", [False, True])
def test_fused_step_against_the_model(hip, name, d, r, six):
    """lambda = 1 and 0.3: x0 bit-identical to ddnm_step_x0_f32, x_{t-1} within 3e-6 of the float64 model (the bar of
    tests/test_gpu_mosaic.py) and of the generic A_functions.ddnm_step composition over the same object; the result does
    not depend on whether x0 is asked for.  Measured on the MI355X (printed): at most 9.5e-8 against float64, 2.1e-8
    against the generic composition."""
    from ddnm_amd import ops
    from ddnm_amd.functions.svd_operators import A_functions
    op, M, _ = _pair("random", d, r, W_LUMA) if name == "luma" else _pair(name, d, r)
    x, xt, et6, nz = _inputs(d, r)
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
        print(f"mcsr step {name} d={d} r={r} six={six} lambda={lam}: vs float64 {e64:.3e}, vs generic {eg:.3e}")
        assert torch.equal(x0_e, x0_k) and rel(x0_e.reshape(B, -1), _t(x0_m)) < 1e-6
        assert e64 <= 3e-6 and eg <= 3e-6
        assert torch.equal(out, out2)


# ---------------------------------------------------------------------------------------------- 3. DDNM+ step
def _plus_scalars(abar_next):
    from ddnm_amd import ops
    s = ops.step_scalars(torch.tensor(ABAR_T), torch.tensor(abar_next), ETA)
    return s, float((1 - torch.tensor(abar_next)).sqrt())


@pytest.mark.parametrize("name,d,r", CASES + [("luma", 16, 4)])
@pytest.mark.parametrize("setting", sorted(PLUS_SETTINGS))
def test_fused_noisy_step(hip, name, d, r, setting):
    """One launch against the float64 model within 3e-6, in the mixed-regime setting (abar' = 0.5, sigma_y = 0.1), with
    every site damped (0.99, 0.4) and with every site full (0.5, 0.001), for a tensor (eps as a tensor and as the 6-channel
    view), the in-kernel Philox and the keyed noise source.  Philox and keyed equal the tensor source filled by the same
    keys bit for bit, and so does an image of the batch stepped alone.  Measured on the MI355X (printed): at most 1.09e-7
    (r = 1, every site full); k = 1 at r = 8: 7.7e-8 / 8.6e-8 / 8.5e-8 in the damped / full / mixed setting."""
    op, M, mask = _pair("random", d, r, W_LUMA) if name == "luma" else _pair(name, d, r)
    abar_next, sigma_y = PLUS_SETTINGS[setting]
    x, xt, et6, nz = _inputs(d, r)
    y = M.A(x.double()).float()
    xt_d, y_d = xt.cuda(), y.cuda()
    op.begin_plus_run(y_d)
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
        torch.cuda.synchronize()
        x0_m, want = M.step(_np(xt), _np(et6[:, :3]), _np(tensor), _np(y), ABAR_T, abar_next, sigma_y, ETA)
        e64 = rel(out_f.reshape(B, -1), _t(want))
        print(f"mcsr DDNM+ step {name} d={d} r={r} {setting} noise={kind} six={six}: vs float64 {e64:.3e}")
        assert rel(x0_f.reshape(B, -1), _t(x0_m)) < 1e-6
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
    if setting == "mixed" and name in ("random", "k1_last") and r == 4:      # mixed at r = 4: both regimes in one launch
        a = abar_next ** 0.5
        thr = a * sigma_y / M.S[M.S > 0]
        assert (sigma_t < thr).any() and (sigma_t > thr).any()


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


@pytest.mark.parametrize("plus", [False, True])
def test_samplers_against_the_oracle_loops(small_net, plus):
    """ddnm_diffusion / ddnm_plus_diffusion (sigma_y = 0.2) with MaskColorSR at 32 px, r = 4, B = 3, T = 4 and one
    time-travel jump of two steps, against the oracle's loops over the dense model on the same noise tape: within 2e-4,
    the bar of the mosaic loops.  The mask is random at 60 % with an empty site and a site that keeps its last pixel.
    Measured on the MI355X (printed): DDNM 4.38e-7, DDNM+ 4.46e-7, x and x0 alike."""
    from ddnm_amd.functions import svd_operators as E
    from ddnm_amd.functions.svd_ddnm import ddnm_diffusion, ddnm_plus_diffusion
    from oracle import cases, sampler, schedule
    cfg, net, model = small_net
    d = cfg.data.image_size
    assert d == 32
    mask = make_mask("k1_last", d, 4)
    mask[0:4, 0:4] = 0
    assert sorted(site_counts(mask, 4, d).tolist())[:2] == [0, 1]
    op, M = E.MaskColorSR(3, d, mask, 4, "cuda"), model_operator(mask, 4, kernel_weights(W_THIRDS), d)
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
    print(f"{'DDNM+' if plus else 'DDNM'} loop, mask_color_sr r=4: x rel-L2 {e:.3e}, x0 rel-L2 {e0:.3e}")
    assert max(e, e0) < 2e-4


# ---------------------------------------------------------------------------------------------- 5. runner
def _runner_mask(root):
    os.makedirs(os.path.join(root, "exp", "inp_masks"), exist_ok=True)
    mask = make_mask("k1_last", 64, 4)
    mask[0:4, 0:4] = 0
    np.save(os.path.join(root, "exp", "inp_masks", "mask.npy"), mask)
    return mask


OLD = ["--path_y", "synthetic:3", "--eta", "0.85", "--deg", "mask_color_sr", "--deg_scale", "4"]


def test_runner_noisy_and_sr_color(hip, tmp_path, monkeypatch, capsys):
    """main.py on the mini configuration (64 px, T = 4, synthetic images): `--deg mask_color_sr --deg_scale 4 --sigma_y 0.1
    --add_noise` (fused by two: DDNM+ through the one-launch hook with per-image keys) and `--deg sr_color` complete with
    their PNGs and a PSNR line; Apy_{i}.png shows A^+ y, which is 0 (mid-grey) where the mask is."""
    from PIL import Image
    from ddnm_amd import ops
    _mini_yaml(tmp_path)
    mask = _runner_mask(tmp_path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("DDNM_SAMPLES", raising=False)
    seen = []
    orig = ops.step_call
    monkeypatch.setattr(ops, "step_call", lambda name, *a: (seen.append(name), orig(name, *a))[1])
    _, psnr, img, names, apy = _run_main(tmp_path, monkeypatch, "noisy", OLD + ["--sigma_y", "0.1", "--add_noise"], 2)
    assert names == [f"{i}_0.png" for i in range(3)] and len(apy) == 6
    assert torch.isfinite(img).all() and torch.isfinite(psnr).all() and len(psnr) == 3
    assert set(seen) == {"ddnm_step_plus_mcsr_f32"}
    shown = np.asarray(Image.open(tmp_path / "exp" / "image_samples" / "noisy" / "Apy" / "Apy_0.png"))
    assert shown.shape == (64, 64, 3) and set(np.unique(shown[mask == 0]).tolist()) <= {127, 128}       # A^+ y = 0 there
    assert len(np.unique(shown[mask == 1])) > 16
    del seen[:]
    argv = OLD[:4] + ["--deg", "sr_color", "--deg_scale", "4", "--sigma_y", "0."]
    _, psnr2, img2, names2, apy2 = _run_main(tmp_path, monkeypatch, "sr_color", argv, None)
    assert names2 == [f"{i}_0.png" for i in range(3)] and len(apy2) == 6 and torch.isfinite(img2).all() and len(psnr2) == 3
    assert set(seen) == {"ddnm_step_mcsr_f32"}
    out = capsys.readouterr().out
    assert out.count("Number of samples: 3") == 2 and out.count("Total Average PSNR") == 2, out[-3000:]


def test_runner_plain_fused_and_two_samples(hip, tmp_path, monkeypatch, capsys):
    """DDNM_FUSE_BATCHES=2 and sample 0 of DDNM_SAMPLES=2 restore what the plain run restores, within 3e-6 (BAR of
    tests/test_gpu_fuse.py).  Measured on the MI355X (printed): 2.1e-7 and 2.6e-7."""
    _mini_yaml(tmp_path)
    _runner_mask(tmp_path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("DDNM_SAMPLES", raising=False)
    argv = OLD + ["--sigma_y", "0."]
    calls1, psnr1, img1, names1, apy1 = _run_main(tmp_path, monkeypatch, "plain", argv, None)
    calls2, psnr2, img2, names2, apy2 = _run_main(tmp_path, monkeypatch, "fused", argv, 2)
    monkeypatch.setenv("DDNM_SAMPLES", "2")
    calls3, _, img3, names3, _ = _run_main(tmp_path, monkeypatch, "samples", argv, None)
    monkeypatch.delenv("DDNM_SAMPLES")
    out = capsys.readouterr().out
    assert out.count("Number of samples: 3") == 3, out[-3000:]
    assert calls1 == [1] and calls2 == [2, 1] and calls3 == [2]
    assert names1 == names2 == [f"{i}_0.png" for i in range(3)] and apy1 == apy2 and len(apy1) == 6
    assert names3 == sorted(f"{i}_{k}.png" for i in range(3) for k in range(2))
    e_f, e_s = rel(img2, img1), rel(img3[0::2], img1)
    print(f"mask_color_sr runner: fused K=2 vs plain rel-L2 {e_f:.3e}, sample 0 of 2 vs plain rel-L2 {e_s:.3e}")
    assert torch.isfinite(img1).all() and e_f < BAR and e_s < BAR
    assert (psnr1 - psnr2).abs().max() < 1e-3 and rel(img3[1::2], img1) > 1e-3          # sample 1 is another draw


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    root = tmp_path_factory.mktemp("mcsr_measurements")
    _mini_yaml(root)
    _runner_mask(str(root))
    return str(root)


def test_round_trip_of_saved_measurements(hip, workdir):
    """DDNM_SAVE_Y=1 with noisy measurements, then the run over measurements:<its y/>: the same PNG bytes
    (tests/test_gpu_measurements.py::_round_trip); the saved rows are the (S / r)^2 values of the small grey picture."""
    noisy = ["--deg", "mask_color_sr", "--deg_scale", "4", "--sigma_y", "0.1"]
    truth, given = _round_trip(workdir, "oldphoto", noisy + ["--add_noise"], noisy, 2)
    for i in range(2):
        row = np.load(os.path.join(truth["folder"], "y", f"y_{i}.npy"))
        assert row.dtype == np.float32 and row.shape == (16 * 16,) and np.isfinite(row).all()
    assert [c["y"].shape for c in given["cons"]] == [(1, 256)] * 2


def test_run_from_a_folder_of_small_grey_scans(hip, workdir):
    """A folder of one-channel 16 x 16 PNGs is restored to 64 x 64 colour pictures (the command line of the README): its
    rows are data_transform of the pixel values exactly."""
    from PIL import Image
    src = os.path.join(workdir, "exp", "datasets", "scans")
    os.makedirs(src, exist_ok=True)
    rng = np.random.default_rng(11)
    pics = [rng.integers(1, 256, (16, 16), dtype=np.uint8) for _ in range(2)]
    for i, arr in enumerate(pics):
        Image.fromarray(arr).save(os.path.join(src, f"scan_{i}.png"))
    run = _run(workdir, "scans", ["--path_y", "measurements:scans", "--deg", "mask_color_sr", "--deg_scale", "4", "--sigma_y",
                                  "0.05"])
    assert "PSNR:" not in run["out"] and "Number of samples: 2" in run["out"] and "Cons: " in run["out"]
    assert sorted(run["files"]) == ["0_0.png", "1_0.png", "Apy/Apy_0.png", "Apy/Apy_1.png"]
    for i, arr in enumerate(pics):
        want = torch.from_numpy(arr.astype(np.float32)).div(255.0).mul(2).sub(1.0).reshape(1, -1)
        assert torch.equal(run["cons"][i]["y"].cpu(), want), i
        assert np.asarray(Image.open(os.path.join(run["folder"], f"{i}_0.png"))).shape == (64, 64, 3)


def test_cons_metric_in_a_ground_truth_run(hip, workdir):
    """DDNM_METRICS=cons: `Cons:` lines and `Max Cons`; the value is printed for the record (3.241e-07 on the
    MI355X) and is no bar."""
    run = _run(workdir, "cons", ["--path_y", "synthetic:2", "--deg", "mask_color_sr", "--deg_scale", "4", "--sigma_y", "0."],
               DDNM_METRICS="cons")
    lines = run["out"].splitlines()
    assert len([ln for ln in lines if ln.startswith("Cons: ")]) == 2 and "Max Cons:" in run["out"]
    assert len(run["cons"]) == 2 and all(c["ax"].shape == c["y"].shape == (1, 256) for c in run["cons"])
    print(f"mask_color_sr: Max Cons {run['metrics']['cons_max']:.3e}")
    assert np.isfinite(run["metrics"]["cons_max"])


def test_entry_points_validate_on_device_pointers(hip):
    """The refusals of tests/test_mcsr_host.py with real device addresses: nothing is launched."""
    buf = torch.zeros(256, device="cuda")
    check_mcsr_validation(hip, buf.data_ptr())
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
