"""DDNM+ (sigma_y > 0) for cs_blockbased on the GPU: the `CS.ddnm_plus_step` hook (ddnm_step_plus_cs_pre_f32, the two
GEMMs of A / A^+, ddnm_step_plus_cs_post_f32) against the float64 model of tests/test_plus_cs_host.py, its three noise
sources against each other, the noise-free limit against the generic `CS.ddnm_step`, the whole loop against the oracle
sampler, and the command line.  Shapes: d = 32, B = 3 (one patch per plane, an odd batch, 9 patch rows: no multiple of
any GEMM tile) and d = 64, B = 2 (a 2 x 2 patch grid: the py / px terms of the patch index matter); ratio 0.25
(cs = 256), one case at ratio 0.5 (cs = 512)."""
import numpy as np
import pytest
import torch

from tests.helpers import engine_operator, rel
from tests.test_gpu_plus_spectral import ABAR_T, CTRS, KEYS, _main, _mini_yaml, _scalars, f32
from tests.test_plus_cs_host import CS_REGIMES, model_operator
from tests.test_plus_spectral_host import ETA, REGIMES, step_inputs

pytestmark = pytest.mark.gpu

SHAPES = [(32, 3), (64, 2)]
# measured rel-L2 on the MI355X (printed by the tests); each bar is 10x the largest, and none may exceed its cap
BAR_STEP = 1e-5          # one step vs the float64 model: measured 1.3e-6, so 10x would be 1.3e-5; the cap 1e-5 holds (the step
                         # chains the GEMMs of A and A^+, 5e-6 each in tests/test_cs.py)
BAR_LINK = 6.3e-6        # noise-free limit vs the generic CS.ddnm_step: measured 6.3e-7; cap 1e-5
BAR_LOOP = 5.8e-6        # whole loop vs the oracle sampler on this host: measured 5.8e-7; cap 3e-4 (the same-host bar of the blur operators)
BAR_BATCH = 3e-6         # images stepped together vs alone: BAR of tests/test_gpu_fuse.py (GEMM tiling may differ with batch;
                         # measured 0 at these shapes)

_CASES = {}


def _case(d, B, six=False, ratio=0.25):
    """Engine operator, float64 model and device inputs of one (d, B, ratio); built once per module."""
    key = (d, B, six, ratio)
    if key not in _CASES:
        if ratio == 0.25:
            eng = engine_operator("cs_blockbased", d)
        else:
            from ddnm_amd.functions import svd_operators as E
            from oracle import cases
            from oracle import operators as O
            eng = E.CS(3, d, ratio, "cuda", gauss=O.gauss_matrix(cases.SEED + 21))
        x_orig, xt, et, n = step_inputs("cs_blockbased", d, B, channels_et=6 if six else 3)
        y = eng.A(x_orig.cuda())
        y = (y + 0.4 * torch.randn(y.shape, generator=torch.Generator().manual_seed(2)).cuda()).contiguous()
        torch.cuda.synchronize()
        _CASES[key] = dict(eng=eng, mdl=model_operator(d, ratio), xt=xt.cuda(), et=et.cuda()[:, :3], n=n.cuda(), y=y)
    return _CASES[key]


def _step(c, noise, a, sigma_y, sigma_t, eta=ETA, stamp=None, rows=None):
    """One `ddnm_plus_step` of case `c` (on the image `rows` only, as a batch of its own) -> (x0, x_{t-1})."""
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
@pytest.mark.parametrize("d,B,six,ratio", [(d, B, False, 0.25) for d, B in SHAPES] + [(64, 2, True, 0.25),
                                                                                      (32, 3, False, 0.5)])
@pytest.mark.parametrize("regime", CS_REGIMES)
def test_one_step_against_float64_model(hip, d, B, six, ratio, regime):
    """x0|t and x_{t-1} of one step with a noise tensor vs the float64 model's fused form (the CPU tests tie that to the
    unfused Lambda / Lambda_noise composition); x0|t is the x0 kernel's value bit for bit.  Measured on the MI355X,
    largest over all cases: x0 5.4e-8; x_{t-1} 7.6e-7 at ratio 0.25 (d = 32, sigma_y = 0) and 1.3e-6 at ratio 0.5 (the
    projected share of x_{t-1} doubles), 5.3e-8 at the last step, where lambda = 0 leaves x_{t-1} = x0.  (The model's
    re-orthonormalised V differs from the engine's fp32 factor by 1.3e-6, tests/test_plus_cs_host.py.)"""
    from ddnm_amd import ops
    a, sigma_y, sigma_t = (f32(v) for v in regime)
    c = _case(d, B, six, ratio)
    assert c["eng"].cs_size == int(1024 * ratio)
    x0, xn = _step(c, c["n"], a, sigma_y, sigma_t)
    x0_k = ops.step_x0(c["xt"], c["et"], _scalars(a))
    torch.cuda.synchronize()
    assert torch.equal(x0, x0_k)
    m0, mn = c["mdl"].fused_step(c["xt"].cpu(), c["et"].cpu(), c["n"].cpu(), c["y"].cpu(), ABAR_T, a, sigma_y, sigma_t,
                                 f32(ETA))
    e0, en = rel(x0, m0), rel(xn, mn)
    print(f"one step cs_blockbased d={d} B={B} six={six} ratio={ratio} {regime}: rel-L2 x0 {e0:.3e}  xt_next {en:.3e}")
    assert torch.isfinite(xn).all()
    assert e0 < BAR_STEP and en < BAR_STEP


# ------------------------------------------------------------------------------------------------ 2. noise sources
@pytest.mark.parametrize("d,B", SHAPES)
def test_noise_sources_agree(hip, d, B):
    """In-kernel Philox == the same step fed PhiloxNoise.tensor(k, .); the keyed entry point with rows
    {seed, image_base + b} == the unkeyed one (both bit for bit on x0 and x_{t-1}); images with different keys in one
    batch == each image stepped alone, within BAR_BATCH."""
    from ddnm_amd import ops
    a, sigma_y, sigma_t = (f32(v) for v in REGIMES[0])
    c = _case(d, B)
    ph = ops.PhiloxNoise(KEYS[0], image_base=5)
    x0_t, xn_t = _step(c, ph.tensor(9, c["xt"]), a, sigma_y, sigma_t)
    x0_p, xn_p = _step(c, None, a, sigma_y, sigma_t, stamp=(ph, 9))
    assert torch.equal(xn_p, xn_t) and torch.equal(x0_p, x0_t)
    kn = ops.KeyedPhiloxNoise([KEYS[0]] * B, [5 + b for b in range(B)])
    x0_k, xn_k = _step(c, kn, a, sigma_y, sigma_t, stamp=(kn, 9))
    assert torch.equal(xn_k, xn_p) and torch.equal(x0_k, x0_p)
    mixed = ops.KeyedPhiloxNoise(KEYS[:B], CTRS[:B])
    _, xn_m = _step(c, mixed, a, sigma_y, sigma_t, stamp=(mixed, 9))
    assert not torch.equal(xn_m[1], xn_k[1])                   # another key: another draw
    for i in range(B):
        src = ops.PhiloxNoise(KEYS[i], image_base=CTRS[i])
        _, xn_i = _step(c, None, a, sigma_y, sigma_t, stamp=(src, 9), rows=i)
        err = rel(xn_m[i:i + 1], xn_i)
        print(f"noise cs_blockbased d={d}: image {i} in the batch vs alone rel-L2 {err:.3e}")
        assert err < BAR_BATCH


# ------------------------------------------------------------------------------------------------ 3. link to tested code
@pytest.mark.parametrize("d,B", SHAPES)
def test_noise_free_limit_reproduces_the_generic_ddnm_step(hip, d, B):
    """sigma_y = 0, eta = 0: lambda = 1 and (d1, d2) = (0, sigma_t) on both subspaces, so w = -a x0 and the step is the
    DDNM step of the generic `CS.ddnm_step` (x0 kernel, A, A^+, combine) with the same noise tensor; x0 is the same
    arithmetic on the same inputs, bit for bit.  Measured on the MI355X: x_{t-1} 6.3e-7 (d = 32), 6.1e-7 (d = 64)."""
    from ddnm_amd import ops
    c = _case(d, B)
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
    print(f"noise-free limit cs_blockbased d={d}: rel-L2 xt_next {err:.3e}")
    assert torch.equal(x0, x0_r)
    assert err < BAR_LINK


def test_hook_refuses_another_batch_and_a_wrong_measurement(hip):
    c = _case(32, 3)
    x = torch.empty(2, 3, 32, 32, device="cuda")
    c["eng"].begin_plus_run(c["y"])
    with pytest.raises(RuntimeError, match="begin_plus_run"):
        c["eng"].ddnm_plus_step(x, x, None, _scalars(0.5), 0.4, 0.9, ETA, x.clone(), x.clone())
    with pytest.raises(ValueError, match="measurement rows"):
        c["eng"].begin_plus_run(c["y"][:, :-4])


# ------------------------------------------------------------------------------------------------ 4. whole loop
def test_whole_loop_against_oracle_sampler(hip):
    """Engine ddnm_plus_diffusion vs oracle.sampler.ddnm_plus_diffusion with the float64-model operator on this host:
    the small CelebA net, B = 2, T = 20, travel 2 / 2, sigma_y = 0.2, tape noise.  Measured on the MI355X: x 5.8e-7, x0 5.8e-7
    (equal: at the last step sigma_t = 0 < a sigma_y gives lambda = 0, so x_{t-1} = x0|t)."""
    from ddnm_amd.functions.svd_ddnm import ddnm_plus_diffusion
    from ddnm_amd.guided_diffusion.models import Model
    from oracle import cases, sampler, schedule, unet_celeba
    cfg, sd = cases.celeba_net("small")
    cfg.time_travel.T_sampling, cfg.time_travel.travel_length, cfg.time_travel.travel_repeat = 20, 2, 2
    n_it = len(schedule.jump_times(20, 2, 2)) - 1
    x_orig, x_T, tape = cases.sampler_case(cfg, 2, n_it)
    d = cfg.data.image_size
    mdl = model_operator(d)
    y = mdl.A(x_orig.reshape(2, -1))
    y = y + 0.2 * torch.randn(y.shape, generator=torch.Generator().manual_seed(4))
    model = Model(cfg)
    model.load_state_dict(sd)
    xs, x0s = ddnm_plus_diffusion(x_T.cuda(), model, cases.betas().cuda(), ETA, engine_operator("cs_blockbased", d),
                                  y.cuda(), 0.2, cls_fn=None, classes=None, config=cfg, noise=[n.cuda() for n in tape])
    torch.cuda.synchronize()
    x, x0 = sampler.ddnm_plus_diffusion(x_T.clone(), unet_celeba.Net(sd, cfg), cases.betas(), ETA, mdl, y, 0.2, tape,
                                        T_sampling=20, travel_length=2, travel_repeat=2)
    ex, e0 = rel(xs[0], x), rel(x0s[0], x0)
    print(f"whole loop cs_blockbased: rel-L2 x {ex:.3e}  x0 {e0:.3e}")
    assert torch.isfinite(xs[0]).all()
    assert ex < BAR_LOOP and e0 < BAR_LOOP


# ------------------------------------------------------------------------------------------------ 5. command line
def test_cli_cs_blockbased_with_measurement_noise_unfused_and_fused(hip, tmp_path, monkeypatch, capsys):
    """`--deg cs_blockbased --deg_scale 0.25 --sigma_y 0.1 --add_noise` completes (it ended in NotImplementedError), and
    DDNM_FUSE_BATCHES=2 at batch_size 1 writes the images of the unfused run (PNG criterion of tests/test_gpu_fuse.py);
    both runs seed the global generator identically, so they draw the same Gaussian matrix."""
    from PIL import Image
    _mini_yaml(tmp_path, batch=1)
    monkeypatch.chdir(tmp_path)
    d1 = _main(tmp_path, monkeypatch, capsys, "one", "cs_blockbased", "0.25")
    d2 = _main(tmp_path, monkeypatch, capsys, "two", "cs_blockbased", "0.25", fuse=2)
    for i in range(4):
        a = np.asarray(Image.open(d1 / f"{i}_0.png"), dtype=np.int16)
        b = np.asarray(Image.open(d2 / f"{i}_0.png"), dtype=np.int16)
        assert np.abs(a - b).max() <= 1 and (a != b).mean() < 1e-3, i
