"""CPU tests: the oracle restatement against the golden vectors produced by the REAL reference
(tests/golden/make_golden.py), plus direct pins against what the reference computes on the same seeded inputs
(recorded in tests/golden/reference_pins.npz by tests/golden/make_golden_ref_pins.py).  No GPU, no HIP calls."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import cases, sampler, schedule, unet_celeba, weights
from tests.helpers import real_mask, rel

OPS = ["sr_averagepooling", "sr_bicubic", "colorization", "inpainting", "cs_walshhadamard", "denoising"]


def test_schedule_golden(golden_dir):
    g = np.load(f"{golden_dir}/schedule.npz")
    for (T, l, r) in [(100, 1, 1), (100, 10, 3), (100, 2, 2), (20, 2, 2)]:
        assert schedule.jump_times(T, l, r) == g[f"jump_{T}_{l}_{r}"].tolist()
    assert len(schedule.jump_times(100, 1, 1)) == 101
    t = schedule.jump_times(100, 10, 3)
    assert len(t) == 461 and sum(1 for a, b in zip(t[:-1], t[1:]) if b < a) == 280
    betas = cases.betas()
    ab = torch.stack([schedule.alpha_bar(betas, i) for i in range(-1, 1000)])
    assert torch.equal(ab, torch.from_numpy(g["alpha_bar_m1_to_999"]))
    assert schedule.alpha_bar(betas, -1).item() == 1.0


def test_state_dict_keys_golden(golden_dir):
    keys = json.load(open(f"{golden_dir}/celeba_state_dict_keys.json"))
    mine = weights.celeba_shapes(weights.celeba_config())
    assert [[k, list(v)] for k, v in mine.items()] == keys
    assert sum(int(np.prod(v)) for v in mine.values()) == 113_673_219      # 113.67 M params


@pytest.mark.parametrize("name", OPS)
@pytest.mark.parametrize("d", [64, 256])
def test_operator_golden(name, d, golden_dir):
    g = np.load(f"{golden_dir}/operators.npz")
    mask = real_mask(golden_dir) if (name == "inpainting" and d == 256) else None
    op = cases.make_operator(name, d, mask)
    x = cases.operator_input(d, 2)
    y = op.A(x)
    gy = torch.from_numpy(g[f"{name}_{d}_y"])
    ysum = g[f"{name}_{d}_ysum"]
    assert abs(y.double().abs().sum().item() - ysum[1]) <= 1e-5 * ysum[1]
    if d == 64:
        assert rel(y, gy) < 2e-6
        p = op.A_pinv(gy)
        assert rel(p.reshape(2, 3, d, d), torch.from_numpy(g[f"{name}_{d}_pinv"])) < 2e-6
    else:
        assert rel(y[:, ::31], gy) < 2e-6
        p = op.A_pinv(y)
        assert rel(p.reshape(2, 3, d, d)[..., ::8, ::8], torch.from_numpy(g[f"{name}_{d}_pinv"])) < 2e-6
    # invariants the reference satisfies: A A^+ y = y, A^+ A idempotent
    assert rel(op.A(op.A_pinv(y)), y) < 1e-5
    z = op.A_pinv(op.A(x))
    assert rel(op.A_pinv(op.A(z)), z) < 1e-5


def test_inpainting_mask_fixture(golden_dir):
    m = real_mask(golden_dir)
    assert m.shape == (256, 256) and int(m.sum()) == 48438            # 73.9 % kept
    op = cases.make_operator("inpainting", 256, m)
    assert op.kept.numel() == 3 * 48438


@pytest.mark.parametrize("kind,batch", [("small", 2), ("mid", 2)])
def test_unet_forward_golden(kind, batch, golden_dir):
    g = np.load(f"{golden_dir}/celeba_forward.npz")
    cfg, sd = cases.celeba_net(kind)
    x, t = cases.forward_inputs(cfg, batch)
    e = unet_celeba.Net(sd, cfg)(x, t)
    assert torch.equal(e, torch.from_numpy(g[f"{kind}_eps"])), "restatement must be bit-identical on CPU"


@pytest.mark.slow
def test_unet_forward_golden_full(golden_dir):
    g = np.load(f"{golden_dir}/celeba_forward.npz")
    cfg, sd = cases.celeba_net("full")
    x, t = cases.forward_inputs(cfg, 1)
    e = unet_celeba.Net(sd, cfg)(x, t)
    assert torch.equal(e[..., ::4, ::4], torch.from_numpy(g["full_eps"]))


@pytest.mark.parametrize("name", OPS)
def test_sampler_golden_small(name, golden_dir):
    g = np.load(f"{golden_dir}/ddnm_small.npz")
    cfg, sd = cases.celeba_net("small")
    n_it = len(schedule.jump_times(20, 2, 2)) - 1
    x_orig, x_T, tape = cases.sampler_case(cfg, 2, n_it)
    op = cases.make_operator(name, cfg.data.image_size)
    y = op.A(x_orig)
    x, x0 = sampler.ddnm_diffusion(x_T.clone(), unet_celeba.Net(sd, cfg), cases.betas(), 0.85, op, y, tape,
                                   T_sampling=20, travel_length=2, travel_repeat=2)
    assert rel(x, torch.from_numpy(g[f"{name}_x"])) < 1e-5
    assert rel(x0, torch.from_numpy(g[f"{name}_x0"])) < 1e-5
    assert (op.A(x) - y).abs().max().item() <= 1e-4 * max(1.0, x.abs().max().item())


def test_full_c2_golden_metadata(golden_dir):
    g = np.load(f"{golden_dir}/ddnm_full_c2.npz")
    assert g["x_sub"].shape == (1, 3, 64, 64) and np.isfinite(g["x_sub"]).all()
    assert 4.0 < float(g["psnr"][0]) < 6.0          # random weights: garbage image (SURVEY 8c caveat)
    assert float(g["ref_cpu_seconds"][0]) > 10


# ---- direct pins against what the reference computes (tests/golden/make_golden_ref_pins.py) -----------------
@pytest.fixture(scope="module")
def ref_pins(golden_dir):
    return np.load(os.path.join(golden_dir, "reference_pins.npz"))


def _digest(obj):
    """The 8-byte digest make_golden_ref_pins.py stores for each reference schedule result (numbers by value)."""
    key = obj if isinstance(obj, str) else [float(v) for v in obj]
    return int.from_bytes(hashlib.blake2b(repr(key).encode(), digest_size=8).digest(), "little")


def test_reference_unet_bit_identical(ref_pins):
    cfg, sd = cases.celeba_net("small")
    x, t = cases.forward_inputs(cfg, 2, seed=7)
    a = torch.from_numpy(ref_pins["unet_small_eps_seed7"])                 # the reference's Model(cfg) on (x, t)
    assert torch.equal(a, unet_celeba.Net(sd, cfg)(x, t))


def test_reference_sampler_direct(ref_pins):
    cfg, sd = cases.celeba_net("small")
    cfg.time_travel.T_sampling, cfg.time_travel.travel_length, cfg.time_travel.travel_repeat = 10, 1, 1
    x_orig, x_T, tape = cases.sampler_case(cfg, 1, 10, seed=11)
    op = cases.make_operator("sr_averagepooling", 32)
    y = torch.from_numpy(ref_pins["sampler_direct_y"])                   # the reference's SuperResolution(3, 32, 4).A
    assert torch.equal(op.A(x_orig), y)
    # the reference's ddnm_diffusion with its own Model and operator, the same noise tape
    xs0, x0s0 = torch.from_numpy(ref_pins["sampler_direct_x"]), torch.from_numpy(ref_pins["sampler_direct_x0"])
    x, x0 = sampler.ddnm_diffusion(x_T.clone(), unet_celeba.Net(sd, cfg), cases.betas(), 0.85, op, y, tape,
                                   T_sampling=10)
    assert rel(x, xs0) < 1e-5 and rel(x0, x0s0) < 1e-5


def test_reference_simplified_loop_restatement(ref_pins):
    """The simplified loop is inlined in a method full of file I/O (diffusion.py:333-397); its
    restatement is pinned through its building blocks: same schedule, MeanUpsample, and the
    sigma_t = sqrt(1 - abar'^2) quirk documented at diffusion.py:356."""
    x = torch.randn(1, 3, 8, 8, generator=torch.Generator().manual_seed(8))
    assert torch.equal(torch.from_numpy(ref_pins["simplified_mean_upsample"]), sampler.mean_upsample(x, 4))
    from oracle import operators as O
    assert torch.equal(torch.from_numpy(ref_pins["simplified_color2gray"]), O.color2gray(x))
    assert torch.equal(torch.from_numpy(ref_pins["simplified_gray2color"]), O.gray2color(x))
    assert ref_pins["simplified_jump_100_10_3"].tolist() == schedule.jump_times(100, 10, 3)


@pytest.mark.parametrize("case", cases.SIMPLIFIED_CASES, ids=[c["name"] for c in cases.SIMPLIFIED_CASES])
def test_oracle_simplified_loop_golden(case, golden_dir):
    """`sampler.simplified_ddnm` + the A / Ap lambdas of the simplified path against goldens produced by driving the
    REAL `Diffusion.simplified_ddnm_plus` (tests/golden/make_golden.py::make_simplified): colorization, noisy
    denoising, average-pool SR, noisy inpainting with the repository mask, and the composed mask_color_sr."""
    from oracle import operators as O
    g = np.load(f"{golden_dir}/simplified.npz")
    cfg, sd = cases.simplified_net(case["res"])
    T, (tl, tr) = case["T"], case["travel"]
    n_it = len(schedule.jump_times(T, tl, tr)) - 1
    x_orig, x_T, tape = cases.sampler_case(cfg, 1, n_it)
    d, deg = case["res"], case["deg"]
    mask = None
    if deg in ("inpainting", "mask_color_sr"):
        mask = real_mask(golden_dir)                                         # exp/inp_masks/mask.npy, committed packed
    if deg == "colorization":
        A, Ap = O.color2gray, O.gray2color
    elif deg == "denoising":
        A = Ap = lambda z: z                                                 # noqa: E731
    elif deg == "sr_averagepooling":
        A = torch.nn.AdaptiveAvgPool2d((256 // 4, 256 // 4))
        Ap = lambda z: sampler.mean_upsample(z, 4)                           # noqa: E731
    elif deg == "inpainting":
        A = Ap = lambda z: z * mask                                          # noqa: E731
    else:
        A, Ap = O.mask_color_sr(mask, 4, d)
    x, _ = sampler.simplified_ddnm(x_T.clone(), unet_celeba.Net(sd, cfg), cases.betas(), 0.85, A, Ap, A(x_orig),
                                   case["sigma_y"], tape, T_sampling=T, travel_length=tl, travel_repeat=tr)
    got = x if d == 32 else x[..., ::4, ::4]
    assert rel(got, torch.from_numpy(g[f"{case['name']}_x"])) < 2e-5
    st = g[f"{case['name']}_stats"]
    assert abs(x.double().abs().sum().item() - st[2]) < 2e-5 * st[2]


def test_schedules_match_reference_on_random_parameters(ref_pins):
    """The DDNM time-travel schedule (functions/svd_ddnm.py:167-206) on 3000 random (T, length, repeat) triples:
    reference == oracle == engine, including the parameter sets the reference rejects."""
    from ddnm_amd.functions.svd_ddnm import get_schedule_jump
    params, digests = ref_pins["jump_params"], ref_pins["jump_digests"]
    assert len(params) == len(digests) == 3000
    for (T, tl, tr), want in zip(params.tolist(), digests.tolist()):
        outs = []
        for fn in (schedule.jump_times, get_schedule_jump):
            try:
                outs.append(fn(T, tl, tr))
            except AssertionError:
                outs.append("assert")
        assert _digest(outs[0]) == want and outs[0] == outs[1], (T, tl, tr)


def test_hq_host_logic_matches_reference_on_random_parameters(ref_pins):
    """hq_demo's scheduler and respacing (hq_demo/guided_diffusion/{scheduler,respace}.py) on random parameters:
    reference == oracle == engine."""
    from oracle import hq_demo as H
    from ddnm_amd.hq_demo import get_schedule_jump, space_timesteps
    keys = ("t_T", "n_sample", "jump_length", "jump_n_sample", "jump2_length", "jump2_n_sample", "jump3_length",
            "jump3_n_sample", "start_resampling")
    assert len(ref_pins["hq_jump_params"]) == len(ref_pins["hq_jump_digests"]) == 2000
    for p, want in zip(ref_pins["hq_jump_params"].tolist(), ref_pins["hq_jump_digests"].tolist()):
        kw = dict(zip(keys, p))
        outs = []
        for fn in (H.schedule_jump, get_schedule_jump):
            try:
                outs.append(fn(**kw))
            except AssertionError:
                outs.append("assert")
        assert _digest(outs[0]) == want and outs[0] == outs[1], kw
    assert len(ref_pins["hq_space_steps"]) == len(ref_pins["hq_space_specs"]) == len(ref_pins["hq_space_digests"]) == 5000
    for steps, spec, want in zip(ref_pins["hq_space_steps"].tolist(), ref_pins["hq_space_specs"].tolist(),
                                 ref_pins["hq_space_digests"].tolist()):
        outs = []
        for fn in (H.space_timesteps, space_timesteps):
            try:
                outs.append(sorted(fn(steps, spec)))
            except ValueError:
                outs.append("ValueError")
        assert _digest(outs[0]) == want and outs[0] == outs[1], (steps, spec)


@pytest.mark.parametrize("factor", [2, 4, 8, 16])
def test_bicubic_and_gaussian_kernels_match_reference_source(factor, ref_pins):
    """The operator factory of the reference is inlined in `svd_based_ddnm_plus` (diffusion.py:451-523) and cannot be
    imported; the kernel its kernel-building statements produce (executed verbatim from the source file by
    tests/golden/make_golden_ref_pins.py) is compared with the oracle's and the engine's builders (bit-exact)."""
    from oracle import operators as O
    from ddnm_amd.functions import svd_operators as E
    ref = torch.from_numpy(ref_pins[f"bicubic_kernel_{factor}"])           # the argument SRConv receives (:498)
    assert torch.equal(O.bicubic_kernel(factor), ref)
    assert torch.equal(E.bicubic_kernel(factor), ref)
    if factor == 2:
        for sigma, radius, marker in ((10, 2, "sigma = 10"), (20, 4, "sigma = 20"), (1, 4, "sigma = 1\n")):
            pdf = lambda x: torch.exp(torch.Tensor([-0.5 * (x / sigma) ** 2]))        # noqa: E731  (:507,513,517)
            want = torch.Tensor([pdf(x) for x in range(-radius, radius + 1)])
            assert torch.equal(O.gaussian_taps(sigma, radius), want)
            assert torch.equal(E.gaussian_taps(sigma, radius), want)


def test_beta_schedules_and_alpha_table_match_reference(ref_pins):
    """`get_beta_schedule` for every schedule name (diffusion.py:46-76) and `compute_alpha` for every t in
    [-1, 999] (svd_ddnm.py:10-13): reference == engine, bit for bit."""
    from ddnm_amd.functions.svd_ddnm import _AlphaTable, compute_alpha
    from ddnm_amd.guided_diffusion.diffusion import get_beta_schedule
    for name in ("quad", "linear", "const", "jsd", "sigmoid"):
        for n in (10, 1000):
            kw = dict(beta_start=1e-4, beta_end=0.02, num_diffusion_timesteps=n)
            assert np.array_equal(ref_pins[f"beta_schedule_{name}_{n}"], get_beta_schedule(name, **kw)), name
    betas = torch.from_numpy(get_beta_schedule("linear", beta_start=1e-4, beta_end=0.02,
                                               num_diffusion_timesteps=1000)).float()
    table = _AlphaTable(betas)
    alphas = torch.from_numpy(ref_pins["compute_alpha_m1_to_999"])           # the reference's compute_alpha, t = -1 .. 999
    assert alphas.shape[0] == 1001
    for t in range(-1, 1000):
        tt = torch.full((2,), t, dtype=torch.long)
        want = alphas[t + 1]
        assert torch.equal(compute_alpha(betas, tt), want)
        assert float(table(t)) == float(want[0, 0, 0, 0])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_inpainting_real_constructor_small(seed, ref_pins):
    """The REAL `Inpainting.__init__` (its O(n*m) kept-index loop, svd_operators.py:324-333) at 16x16 -- the golden
    generator bypasses it at full size -- against the oracle operator: A, A_pinv and the index order."""
    from oracle import operators as O
    g = torch.Generator().manual_seed(seed)
    d = 16
    mask = (torch.rand(d, d, generator=g) > 0.3).long()
    orc = O.Inpainting(3, d, O.Inpainting.missing_from_mask(mask))
    x = torch.randn(2, 3, d, d, generator=g)
    y = torch.from_numpy(ref_pins[f"inpainting_ctor_{seed}_y"])              # the reference's Inpainting(...).A(x)
    assert torch.equal(orc.A(x), y)
    assert torch.equal(orc.A_pinv(y).reshape(2, -1), torch.from_numpy(ref_pins[f"inpainting_ctor_{seed}_pinv"]))


def test_oracle_superresolution_ratio16_golden(golden_dir):
    """The oracle's SuperResolution at ratio 16 (evaluation.sh:18) against the reference class
    (functions/svd_operators.py:479-623; tests/golden/spectral_sr16.npz from make_golden.py --spectral-sr16-only)."""
    import numpy as np
    g = {k: torch.from_numpy(v) for k, v in np.load(f"{golden_dir}/spectral_sr16.npz").items()}
    op = cases.make_operator("sr_averagepooling", 64, ratio=16)
    x = cases.operator_input(64, 2)

    def r(a, b):
        return ((a.double().reshape(2, -1) - b.double()).norm() / b.double().norm()).item()
    assert r(op.A(x), g["A"]) < 1e-6 and r(op.A_pinv(g["w"]), g["A_pinv"]) < 1e-6
    for tag, (a, st) in {"early": (0.2, 0.97), "late": (0.98, 0.15)}.items():
        assert r(op.Lambda(g["z"].clone(), torch.tensor(a), 0.4, torch.tensor(st), 0.85), g[f"Lambda_{tag}"]) < 1e-6
        assert r(op.Lambda_noise(g["z"].clone(), torch.tensor(a), 0.4, torch.tensor(st), 0.85, g["e"].clone()),
                 g[f"Lambda_noise_{tag}"]) < 1e-6
