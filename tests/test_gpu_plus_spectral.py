"""DDNM+ (sigma_y > 0) for sr_bicubic and deblur_aniso on the GPU: the `ddnm_plus_step` hook (x0 kernel, two two-sided
GEMMs, ddnm_step_plus_spectral_f32) against the float64 model of tests/test_plus_spectral_host.py, its three noise
sources against each other, the noise-free limit against SRConv.ddnm_step, the whole loop against the oracle sampler,
and the command line.  Shapes: d = 32 (every GEMM on the naive path, odd B) and d = 64 (the V side on the 64-tile MFMA
GEMM, the U side of sr_bicubic -- m = 16 -- on the naive one)."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import engine_operator, rel
from tests.test_plus_spectral_host import ETA, REGIMES, model_operator, regime_counts, step_inputs

pytestmark = pytest.mark.gpu

OPS = ["sr_bicubic", "deblur_aniso"]
SHAPES = [(32, 3), (64, 2)]
ABAR_T = 0.37
KEYS = [0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x0123456789ABCDEF]
CTRS = [0, 5, 1]
# measured rel-L2 on the MI355X (printed by the tests); each bar is 10x the largest, and none may exceed its cap
BAR_STEP = 3e-6          # one step vs the float64 model: measured 3.0e-7; cap 1e-5 (the bar of Deblurring's Lambda: same four-GEMM structure)
BAR_LINK = 6e-6          # noise-free limit vs SRConv.ddnm_step: measured 6.1e-7; cap 1e-5
BAR_LOOP = 2.6e-4        # whole loop vs the oracle sampler on this host: measured 2.6e-5; cap 3e-4 (the same-host bar of the blur operators)
BAR_BATCH = 3e-6         # images stepped together vs alone: BAR of tests/test_gpu_fuse.py (GEMM tiling may differ with batch;
                         # measured 0 at these shapes)


def f32(v):
    """The value the C ABI receives for a `float` argument."""
    return float(np.float32(v))


_CASES = {}


def _case(name, d, B, six=False):
    """Engine operator, float64 model and device inputs of one (operator, d, B); built once per module."""
    key = (name, d, B, six)
    if key not in _CASES:
        eng, mdl = engine_operator(name, d), model_operator(name, d)
        x_orig, xt, et, n = step_inputs(name, d, B, channels_et=6 if six else 3)
        y = eng.A(x_orig.cuda())
        y = (y + 0.4 * torch.randn(y.shape, generator=torch.Generator().manual_seed(2)).cuda()).contiguous()
        torch.cuda.synchronize()
        _CASES[key] = dict(eng=eng, mdl=mdl, xt=xt.cuda(), et=et.cuda()[:, :3], n=n.cuda(), y=y)
    return _CASES[key]


def _scalars(a, eta=ETA):
    """ddnm_step_scalars of a step with abar_t = ABAR_T whose sqrt(abar_t') is exactly fp32(a) (the regimes of the issue
    pick a and sigma_t independently)."""
    from ddnm_amd import ops
    s = ops.step_scalars(torch.tensor(ABAR_T), torch.tensor(a) ** 2, eta)
    s.sqrt_at_next = a
    return s


def _step(c, noise, a, sigma_y, sigma_t, eta=ETA, stamp=None, rows=None):
    """One `ddnm_plus_step` of case `c` (on the images `rows` only, as a batch of their own) -> (x0, x_{t-1})."""
    sl = slice(None) if rows is None else slice(rows, rows + 1)
    xt, et, y = c["xt"][sl].contiguous(), c["et"][sl], c["y"][sl].contiguous()
    s = _scalars(a, eta)
    if stamp is not None:
        stamp[0].stamp(s, stamp[1])
    x0, xn = torch.empty_like(xt), torch.empty_like(xt)
    c["eng"].begin_plus_run(y)
    c["eng"].ddnm_plus_step(xt, et, noise, s, sigma_y, sigma_t, eta, x0, xn)
    torch.cuda.synchronize()
    return x0, xn


# ------------------------------------------------------------------------------------------------ 1. one step
@pytest.mark.parametrize("name,d,B,six", [(n, d, B, False) for n in OPS for d, B in SHAPES] + [("sr_bicubic", 32, 3, True),
                                                                                            ("deblur_aniso", 64, 2, True)])
@pytest.mark.parametrize("regime", REGIMES)
def test_one_step_against_float64_model(hip, name, d, B, six, regime):
    """x0|t and x_{t-1} of one step with a noise tensor vs the float64 model's fused form (the CPU tests tie that to the
    unfused Lambda / Lambda_noise composition).  Measured on the MI355X, largest over all cases: x0 5.4e-8,
    x_{t-1} 3.0e-7 (deblur_aniso, d = 64, regime 3)."""
    a, sigma_y, sigma_t = (f32(v) for v in regime)
    c = _case(name, d, B, six)
    if regime == REGIMES[0]:         # all three regimes inside this one launch, from the host table
        below, above, null = regime_counts(c["eng"]._plus_factors()["gains"], a, sigma_y, sigma_t)
        assert below > 0 and above > 0 and null > 0, (below, above, null)
    x0, xn = _step(c, c["n"], a, sigma_y, sigma_t)
    m0, mn = c["mdl"].fused_step(c["xt"].cpu(), c["et"].cpu(), c["n"].cpu(), c["y"].cpu(), ABAR_T, a, sigma_y, sigma_t,
                                 f32(ETA))
    e0, en = rel(x0, m0), rel(xn, mn)
    print(f"one step {name} d={d} B={B} six={six} {regime}: rel-L2 x0 {e0:.3e}  xt_next {en:.3e}")
    assert torch.isfinite(xn).all()
    assert e0 < BAR_STEP and en < BAR_STEP


# ------------------------------------------------------------------------------------------------ 2. noise sources
@pytest.mark.parametrize("name", OPS)
@pytest.mark.parametrize("d,B", SHAPES)
def test_noise_sources_agree(hip, name, d, B):
    """In-kernel Philox == the same step fed PhiloxNoise.tensor(k, .); the keyed entry point with rows
    {seed, image_base + b} == the unkeyed one (both bit for bit); images with different keys in one batch == each image
    stepped alone, within BAR_BATCH."""
    from ddnm_amd import ops
    a, sigma_y, sigma_t = (f32(v) for v in REGIMES[0])
    c = _case(name, d, B)
    ph = ops.PhiloxNoise(KEYS[0], image_base=5)
    x0_t, xn_t = _step(c, ph.tensor(9, c["xt"]), a, sigma_y, sigma_t)
    x0_p, xn_p = _step(c, None, a, sigma_y, sigma_t, stamp=(ph, 9))
    assert torch.equal(xn_p, xn_t) and torch.equal(x0_p, x0_t)
    kn = ops.KeyedPhiloxNoise([KEYS[0]] * B, [5 + b for b in range(B)])
    x0_k, xn_k = _step(c, kn, a, sigma_y, sigma_t, stamp=(kn, 9))
    assert torch.equal(xn_k, xn_p) and torch.equal(x0_k, x0_p)
    mixed = ops.KeyedPhiloxNoise(KEYS[:B], CTRS[:B])
    _, xn_m = _step(c, mixed, a, sigma_y, sigma_t, stamp=(mixed, 9))
    for i in range(B):
        src = ops.PhiloxNoise(KEYS[i], image_base=CTRS[i])
        _, xn_i = _step(c, None, a, sigma_y, sigma_t, stamp=(src, 9), rows=i)
        err = rel(xn_m[i:i + 1], xn_i)
        print(f"noise {name} d={d}: image {i} in the batch vs alone rel-L2 {err:.3e}")
        assert err < BAR_BATCH


def test_in_kernel_draw_is_the_philox_tensor_draw(hip):
    """The kernel's n itself: on zero planes with a = 0 (no regime change), eta = 1 and sigma_t = 1 the kernel's output
    is n, which must be ddnm_randn_philox_f32 on [B][C * plane] bit for bit."""
    from ddnm_amd import ops
    d, B = 32, 3
    c = _case("sr_bicubic", d, B)
    ph = ops.PhiloxNoise(KEYS[1], image_base=2)
    s = ph.stamp(_scalars(0.0, eta=1.0), 4)
    hat = torch.zeros(B, 3, d, d, device="cuda")
    g = c["eng"]._plus_factors()["gains"]
    out = ops.step_plus_spectral(hat, hat.clone(), hat.clone(), g, 0, None, s, 0.4, 1.0, 1.0)
    want = ph.tensor(4, hat)
    torch.cuda.synchronize()
    assert torch.equal(out, want)            # x^_0 = 0, mu * 0 = 0, 0 * a = 0, n * 1, e^ * 0: exact


# ------------------------------------------------------------------------------------------------ 3. link to tested code
@pytest.mark.parametrize("d,B", SHAPES)
def test_noise_free_limit_reproduces_srconv_ddnm_step(hip, d, B):
    """sigma_y = 0, eta = 0: mu = 1 on the measured entries, (d1, d2) = (0, sigma_t) everywhere -- the DDNM step of
    SRConv.ddnm_step (A / A^+ as Ae / Pe products).  Measured on the MI355X: x_{t-1} 4.7e-7 (d = 32), 6.1e-7 (d = 64); x0 is the same
    kernel on the same inputs, bit for bit."""
    from ddnm_amd import ops
    c = _case("sr_bicubic", d, B)
    at_next = torch.tensor(0.52)
    s = ops.step_scalars(torch.tensor(ABAR_T), at_next, 0.0)
    x0_r, xn_r = torch.empty_like(c["xt"]), torch.empty_like(c["xt"])
    c["eng"].ddnm_step(c["xt"], c["et"], c["n"], c["y"], s, x0_r, xn_r)
    s2 = ops.step_scalars(torch.tensor(ABAR_T), at_next, 0.0)
    x0, xn = torch.empty_like(c["xt"]), torch.empty_like(c["xt"])
    c["eng"].begin_plus_run(c["y"])
    c["eng"].ddnm_plus_step(c["xt"], c["et"], c["n"], s2, 0.0, float((1 - at_next).sqrt()), 0.0, x0, xn)
    torch.cuda.synchronize()
    err = rel(xn, xn_r)
    print(f"noise-free limit sr_bicubic d={d}: rel-L2 xt_next {err:.3e}")
    assert torch.equal(x0, x0_r)
    assert err < BAR_LINK


# ------------------------------------------------------------------------------------------------ 4. spectral_mix unchanged
@pytest.mark.parametrize("regime", REGIMES)
def test_spectral_mix_keeps_its_values(hip, regime):
    """ddnm_spectral_mix_f32 now calls the shared coefficient function: per entry it still applies the float64 rule
    (`spectral_coefficients` of the un-thresholded table) to 1e-5, entries whose lambda is 1 pass through bit for bit, and
    Deblurring.Lambda / Lambda_noise still match the oracle within the existing 1e-5."""
    from ddnm_amd.functions.svd_operators import spectral_coefficients
    from oracle import cases
    a, sigma_y, sigma_t = (f32(v) for v in regime)
    d, B = 32, 2
    eng, orc = engine_operator("deblur_gauss", d), cases.make_operator("deblur_gauss", d)
    g = torch.Generator().manual_seed(3)
    v, e = torch.randn(B, 3 * d * d, generator=g), torch.randn(B, 3 * d * d, generator=g)
    tab = torch.tensor([spectral_coefficients(float(s), a, sigma_y, sigma_t, f32(ETA)) for s in eng.S_orig.cpu()],
                       dtype=torch.float64)                                       # [d*d][lambda, d1, d2]
    lam, d1, d2 = (tab[:, k].repeat(B * 3).reshape(B, -1) for k in range(3))
    m0 = eng._spectral_mix(v.cuda(), None, a, sigma_y, sigma_t, ETA, 0).cpu()
    m1 = eng._spectral_mix(v.cuda(), e.cuda(), a, sigma_y, sigma_t, ETA, 1).cpu()
    assert rel(m0, v.double() * lam) < 1e-5 and rel(m1, v.double() * d1 + e.double() * d2) < 1e-5
    assert torch.equal(m0[lam == 1.0], v[lam == 1.0])
    assert rel(eng.Lambda(v.cuda(), a, sigma_y, sigma_t, ETA).reshape(B, -1), orc.Lambda(v.clone(), a, sigma_y, sigma_t, ETA)) < 1e-5
    assert rel(eng.Lambda_noise(v.cuda(), a, sigma_y, sigma_t, ETA, e.cuda()).reshape(B, -1),
               orc.Lambda_noise(v.clone(), a, sigma_y, sigma_t, ETA, e.clone())) < 1e-5


# ------------------------------------------------------------------------------------------------ 5. whole loop
@pytest.mark.parametrize("name", OPS)
def test_whole_loop_against_oracle_sampler(hip, name):
    """Engine ddnm_plus_diffusion vs oracle.sampler.ddnm_plus_diffusion with the float64-model operator on this host:
    the small CelebA net, T = 20, travel 2 / 2, sigma_y = 0.2, tape noise.  Measured on the MI355X: x 8.7e-6 / x0 8.4e-6
    (sr_bicubic), x 2.6e-5 / x0 2.5e-5 (deblur_aniso)."""
    from ddnm_amd.functions.svd_ddnm import ddnm_plus_diffusion
    from ddnm_amd.guided_diffusion.models import Model
    from oracle import cases, sampler, schedule, unet_celeba
    cfg, sd = cases.celeba_net("small")
    cfg.time_travel.T_sampling, cfg.time_travel.travel_length, cfg.time_travel.travel_repeat = 20, 2, 2
    n_it = len(schedule.jump_times(20, 2, 2)) - 1
    x_orig, x_T, tape = cases.sampler_case(cfg, 2, n_it)
    d = cfg.data.image_size
    mdl = model_operator(name, d)
    y = mdl.A(x_orig.reshape(2, -1))
    y = y + 0.2 * torch.randn(y.shape, generator=torch.Generator().manual_seed(4))
    model = Model(cfg)
    model.load_state_dict(sd)
    xs, x0s = ddnm_plus_diffusion(x_T.cuda(), model, cases.betas().cuda(), ETA, engine_operator(name, d), y.cuda(), 0.2,
                                  cls_fn=None, classes=None, config=cfg, noise=[n.cuda() for n in tape])
    torch.cuda.synchronize()
    x, x0 = sampler.ddnm_plus_diffusion(x_T.clone(), unet_celeba.Net(sd, cfg), cases.betas(), ETA, mdl, y, 0.2, tape,
                                        T_sampling=20, travel_length=2, travel_repeat=2)
    ex, e0 = rel(xs[0], x), rel(x0s[0], x0)
    print(f"whole loop {name}: rel-L2 x {ex:.3e}  x0 {e0:.3e}")
    assert torch.isfinite(xs[0]).all()
    assert ex < BAR_LOOP and e0 < BAR_LOOP


# ------------------------------------------------------------------------------------------------ 6. command line
def _mini_yaml(tmp_path, batch, T=4):
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "configs", "celeba_hq.yml")))
    cfg["time_travel"]["T_sampling"] = T
    cfg["sampling"]["batch_size"] = batch
    cfg["data"]["image_size"] = 64
    cfg["model"]["ch_mult"] = [1, 1, 2]
    os.makedirs(tmp_path / "configs", exist_ok=True)
    with open(tmp_path / "configs" / "mini.yml", "w") as f:
        yaml.safe_dump(cfg, f)


def _main(tmp_path, monkeypatch, capsys, folder, deg, scale, fuse=None):
    import main
    with monkeypatch.context() as m:
        m.setenv("DDNM_RANDOM_WEIGHTS", "1")
        m.delenv("DDNM_NOISE", raising=False)
        if fuse:
            m.setenv("DDNM_FUSE_BATCHES", str(fuse))
        else:
            m.delenv("DDNM_FUSE_BATCHES", raising=False)
        rc = main.main(["--ni", "--config", "mini.yml", "--path_y", "synthetic:4", "--eta", "0.85", "--deg", deg,
                        "--deg_scale", scale, "--sigma_y", "0.1", "--add_noise", "-i", folder])
    out = capsys.readouterr().out
    assert rc == 0
    assert "Total Average PSNR" in out and "Number of samples: 4" in out, out[-2000:]
    assert "NotImplementedError" not in out
    out_dir = tmp_path / "exp" / "image_samples" / folder
    assert sorted(p.name for p in out_dir.glob("*.png")) == [f"{i}_0.png" for i in range(4)]
    return out_dir


def test_cli_sr_bicubic_with_measurement_noise_unfused_and_fused(hip, tmp_path, monkeypatch, capsys):
    """`--deg sr_bicubic --deg_scale 4 --sigma_y 0.1 --add_noise` completes, and DDNM_FUSE_BATCHES=2 at batch_size 1
    writes the images of the unfused run (PNG criterion of tests/test_gpu_fuse.py)."""
    from PIL import Image
    _mini_yaml(tmp_path, batch=1)
    monkeypatch.chdir(tmp_path)
    d1 = _main(tmp_path, monkeypatch, capsys, "one", "sr_bicubic", "4")
    d2 = _main(tmp_path, monkeypatch, capsys, "two", "sr_bicubic", "4", fuse=2)
    for i in range(4):
        a = np.asarray(Image.open(d1 / f"{i}_0.png"), dtype=np.int16)
        b = np.asarray(Image.open(d2 / f"{i}_0.png"), dtype=np.int16)
        assert np.abs(a - b).max() <= 1 and (a != b).mean() < 1e-3, i


def test_cli_deblur_aniso_with_measurement_noise(hip, tmp_path, monkeypatch, capsys):
    _mini_yaml(tmp_path, batch=2)
    monkeypatch.chdir(tmp_path)
    _main(tmp_path, monkeypatch, capsys, "aniso", "deblur_aniso", "0")
