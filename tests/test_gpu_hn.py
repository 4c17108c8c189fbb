"""Per-entry measurement noise (shot + read noise, noise maps) on the GPU: the two one-launch DDNM+ steps
(`ddnm_step_plus_mosaic_hn_f32`, `ddnm_step_plus_denoise_hn_f32`, hooks `Mosaic` / `Denoising.ddnm_plus_step_hn`) bit for
bit against the CPU model of tests/hn_model.py for all three noise sources, against the steps that exist for a constant
sigma, `ddnm_plus_diffusion` under a `NoiseModel` against the oracle's loop with a per-entry float64 operator, the runner
(plain / fused / two samples, saved measurements and back, refusals) and the entry points' checks on device pointers."""
import logging
import os

import numpy as np
import pytest
import torch

from oracle import operators as O
from tests import hn_model as H
from tests.helpers import rel
from tests.test_gpu_fuse import BAR, _mini_yaml, _run_main
from tests.test_gpu_measurements import _files, _round_trip, _run
from tests.test_hn_host import check_hn_validation
from tests.test_mosaic_host import numpy_cfa, numpy_tables

pytestmark = pytest.mark.gpu

F = np.float32
ETA = 0.85


def _E():
    from ddnm_amd.functions import svd_operators as E
    return E


def _operator(kernel, pattern, d):
    E = _E()
    return E.Mosaic(3, d, pattern, "cuda") if kernel == "mosaic" else E.Denoising(3, d, "cuda")


def _step_scalars(sc):
    """The StepScalars of the model's scalars (c1, c2 and lambda are not read by the `*_hn_*` kernels)."""
    from ddnm_amd._lib import StepScalars
    s = StepScalars()
    s.sqrt_1m_at, s.sqrt_at, s.sqrt_at_next = float(sc.s1), float(sc.s2), float(sc.a)
    return s


# ---------------------------------------------------------------------------------------------- 1. bit for bit
@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c.name)
def test_kernels_equal_the_model_bit_for_bit_for_every_noise_source(hip, case):
    """x0 and x_{t-1} of both kernels == hn_model.model by torch.equal, with the noise as a tensor, drawn in-kernel and
    drawn through the keyed table: one draw, one model.  Every entry is held bit for bit: the device's sqrtf and / are
    correctly rounded (were they not, the entries through them would fail here first)."""
    from ddnm_amd import ops
    E = _E()
    p = case.p
    B, d = p["B"], p["d"]
    lo, hi, it, base = H.noise_key(case)
    src = ops.PhiloxNoise((hi << 32) | lo, image_base=base)
    like = torch.empty(B, 3, d, d, device="cuda")
    nz = src.tensor(it, like)
    t = H.make_inputs(case, nz=nz.cpu().numpy())
    want = H.model(case, t)
    op = _operator(case.kernel, p.get("pattern"), d)
    nm = E.NoiseModel.map(t["row"]) if p["sigma"] == "map" else E.NoiseModel.shot(*t["shot"])
    xt, y = torch.from_numpy(t["xt"]).cuda(), torch.from_numpy(t["y"]).cuda()
    et6 = torch.from_numpy(t["et6"]).cuda()
    et = et6[:, :3] if p["six"] else et6[:, :3].contiguous()
    assert et.is_contiguous() != p["six"]
    op.begin_plus_run(y, nm)
    keyed = ops.KeyedPhiloxNoise.from_sources([(src, i) for i in range(B)])
    for kind in H.NOISE_SOURCES:
        s = _step_scalars(t["s"])
        arg = nz if kind == "tensor" else src.kernel_arg(s, it) if kind == "in_kernel" else keyed.kernel_arg(s, it)
        x0, xn = torch.full_like(xt, float("nan")), torch.full_like(xt, float("nan"))
        op.ddnm_plus_step_hn(xt, et, arg, s, float(t["s"].st), p["eta"], x0, xn)
        torch.cuda.synchronize()
        for name, got in (("x0", x0), ("xn", xn)):
            g = got.cpu().numpy()
            bad = g.view(np.uint32) != want[name].view(np.uint32)
            assert not bad.any(), (case.name, kind, name, int(bad.sum()),
                                   {int(b): int((bad & (want["branch"] == b)).sum()) for b in (-1, 0, 1, 2)})
            assert torch.equal(got.cpu(), torch.from_numpy(want[name]))


# ---------------------------------------------------------------------------------------------- 2. against what exists
def _generic_plus_step(op, xt, et, nz, y, s, sigma_y, sigma_t, eta):
    """The body of ddnm_plus_diffusion's step for an operator WITHOUT a hook (tests/test_gpu_mosaic.py, restated): x0
    kernel, A, residual, A^+, Lambda, Lambda_noise, combine -- eight launches."""
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


SIGMA_Y = 0.4          # engine scale, as tests/test_mosaic_host.py: at_next = 0.99 lies below a sigma_y, at_next = 0.5 above


@pytest.mark.parametrize("kernel,pattern,d", [("mosaic", "xtrans", 16), ("mosaic", "rggb", 32), ("denoise", None, 16)])
@pytest.mark.parametrize("form", ["map", "shot_g0"])
@pytest.mark.parametrize("at_next", [0.99, 0.5])
def test_constant_sigma_equals_the_existing_steps(hip, kernel, pattern, d, form, at_next):
    """A constant map and g = 0 against today's launches at sigma_y = sigma: the mosaic against ddnm_step_plus_mosaic_f32,
    denoising against the generic eight-launch chain; 3e-6 relative L2, the project's bar for these comparisons (BAR of
    tests/test_gpu_fuse.py).  Not bitwise: today's coefficients are rounded from double on the host.  Measured on the
    MI355X (printed), map and shot form alike: mosaic 0 at at_next = 0.99 and 3.60e-8 (xtrans) / 3.63e-8 (rggb) at 0.5;
    denoising against the chain 5.70e-8 and 7.25e-8; x0 bit-identical."""
    from ddnm_amd import ops
    E = _E()
    B = 3
    n = d * d if kernel == "mosaic" else 3 * d * d
    g = torch.Generator().manual_seed(31 + d)
    xt, et6, nz = (torch.randn(B, c, d, d, generator=g).cuda() for c in (3, 6, 3))
    y = (torch.rand(B, n, generator=g) * 2 - 1).cuda()
    et = et6[:, :3]
    op = _operator(kernel, pattern, d)
    nm = E.NoiseModel.map(np.full(n, SIGMA_Y / 2, F)) if form == "map" else E.NoiseModel("shot", sigma=SIGMA_Y / 2, gain=0.0)

    def scalars():
        return ops.step_scalars(torch.tensor(0.45), torch.tensor(at_next), ETA)

    sigma_t = float((1 - torch.tensor(at_next)).sqrt())
    assert (sigma_t < scalars().sqrt_at_next * SIGMA_Y) == (at_next == 0.99)
    x0_n, out_n = torch.empty_like(xt), torch.empty_like(xt)
    op.begin_plus_run(y, nm)
    op.ddnm_plus_step_hn(xt, et, nz, scalars(), sigma_t, ETA, x0_n, out_n)
    if kernel == "mosaic":
        x0_o, out_o = torch.empty_like(xt), torch.empty_like(xt)
        op.begin_plus_run(y)
        op.ddnm_plus_step(xt, et, nz, scalars(), SIGMA_Y, sigma_t, ETA, x0_o, out_o)
    else:
        x0_o, out_o = _generic_plus_step(op, xt, et, nz, y, scalars(), SIGMA_Y, sigma_t, ETA)
    torch.cuda.synchronize()
    err = rel(out_n, out_o)
    print(f"hn step vs existing, {kernel} {pattern or ''} d={d} {form} at_next={at_next}: x_t-1 rel-L2 {err:.3e}")
    assert torch.equal(x0_n, x0_o)
    assert torch.isfinite(out_n).all() and err < BAR


# ---------------------------------------------------------------------------------------------- 3. loops
@pytest.fixture(scope="module")
def small_net(hip):
    from ddnm_amd.guided_diffusion.models import Model
    from oracle import cases, unet_celeba
    cfg, sd = cases.celeba_net("small")
    cfg.time_travel.T_sampling, cfg.time_travel.travel_length, cfg.time_travel.travel_repeat = 4, 2, 2
    model = Model(cfg)
    model.load_state_dict(sd)
    return cfg, unet_celeba.Net(sd, cfg), model


class _PerEntryTable:
    """Mixin over an oracle operator: Lambda / Lambda_noise apply the per-entry table in float64; each entry's branch comes
    from the kernel's own fp32 comparison of thr = a sigma_j with sigma_t (hn_model.branches32), so a rounding-level tie
    cannot flip a branch between the two.  The `sigma_y` the sampler passes on is ignored."""

    def bind(self, y, kernel, pattern, sigma_kind, row, shot):
        self._geometry = (kernel, pattern, self.img_dim)
        self._sig = H.sigma32(sigma_kind, y.numpy().astype(F), row, shot)                  # [B][n] fp32, engine scale
        return self

    def _coef(self, a, sigma_t, eta):
        a32, st32 = F(float(a)), F(float(sigma_t))
        br, _ = H.branches32(a32, self._sig, st32)
        al, d1, d2 = H.coef64(float(a32), self._sig.astype(np.float64), float(st32), eta, br)
        c1, c2 = float(st32) * eta, float(st32) * (1 - eta ** 2) ** 0.5
        B = self._sig.shape[0]
        return [torch.from_numpy(np.ascontiguousarray(H.expand(*self._geometry, v, fill).reshape(B, -1)))
                for v, fill in ((al / float(a32), 1.0), (d1, c1), (d2, c2))]

    def Lambda(self, vec, a, sigma_y, sigma_t, eta):
        lam, _, _ = self._coef(a, sigma_t, eta)
        return (vec.reshape(vec.shape[0], -1).double() * lam).float()

    def Lambda_noise(self, vec, a, sigma_y, sigma_t, eta, epsilon):
        _, d1, d2 = self._coef(a, sigma_t, eta)
        n = vec.shape[0]
        return (vec.reshape(n, -1).double() * d1 + epsilon.reshape(n, -1).double() * d2).float()


class PerEntryInpainting(_PerEntryTable, O.Inpainting):
    pass


class PerEntryDenoising(_PerEntryTable, O.Denoising):
    pass


@pytest.mark.parametrize("kernel", ["mosaic", "denoise"])
@pytest.mark.parametrize("sigma_kind", ["map", "shot"])
def test_loops_against_the_oracle_with_a_per_entry_operator(small_net, kernel, sigma_kind):
    """ddnm_plus_diffusion under a map and under a shot model, Mosaic `rggb` and Denoising, T = 4 with one time-travel jump
    (travel_length = 2, travel_repeat = 2), against oracle.sampler.ddnm_plus_diffusion on the same noise tape: 2e-4
    relative L2 on x and x0, the bar of tests/test_gpu_sampler.py / tests/test_ddnm_plus.py.  Measured on the MI355X
    (printed), x and x0 alike: map 4.36e-7 (Mosaic) / 4.84e-7 (Denoising), shot 4.39e-7 / 4.88e-7."""
    from ddnm_amd.functions.svd_ddnm import ddnm_plus_diffusion
    from oracle import cases, sampler, schedule
    E = _E()
    cfg, net, model = small_net
    d, B = cfg.data.image_size, 3
    n_it = len(schedule.jump_times(4, 2, 2)) - 1
    x_orig, x_T, tape = cases.sampler_case(cfg, B, n_it)
    if kernel == "mosaic":
        missing = numpy_tables(numpy_cfa("rggb"), d)[2]
        op, orc, n = E.Mosaic(3, d, "rggb", "cuda"), PerEntryInpainting(3, d, torch.from_numpy(missing)), d * d
    else:
        op, orc, n = E.Denoising(3, d, "cuda"), PerEntryDenoising(3, d), 3 * d * d
    g = torch.Generator().manual_seed(77)
    row, shot = None, None
    if sigma_kind == "map":
        row = (torch.rand(n, generator=g) * 0.3).numpy().astype(F)
        row[::7] = 0                                                   # entries measured exactly
        nm = E.NoiseModel.map(row)
    else:
        shot = (0.05, 0.08)
        nm = E.NoiseModel.shot(*shot)
    y_clean = orc.A(x_orig)
    y = (y_clean + nm.std(y_clean) * torch.randn(B, n, generator=g)).float().contiguous()
    orc.bind(y, kernel, "rggb", sigma_kind, row, shot)
    kw = dict(T_sampling=4, travel_length=2, travel_repeat=2)
    ref, ref0 = sampler.ddnm_plus_diffusion(x_T.clone(), net, cases.betas(), ETA, orc, y, None, tape, **kw)
    xs, x0s = ddnm_plus_diffusion(x_T.cuda(), model, cases.betas().cuda(), ETA, op, y.cuda(), nm, cls_fn=None, classes=None,
                                  config=cfg, noise=[t.cuda() for t in tape])
    e, e0 = rel(xs[0], ref), rel(x0s[0], ref0)
    print(f"DDNM+ loop under a {sigma_kind} model, {kernel}: x rel-L2 {e:.3e}, x0 rel-L2 {e0:.3e}")
    assert torch.isfinite(xs[0]).all() and e < 2e-4 and e0 < 2e-4


def test_scalar_model_runs_the_scalar_launches_and_other_operators_refuse(small_net, monkeypatch):
    """NoiseModel.scalar(s) is the float 2 s: the same launches and the same bits; an operator without the hook refuses a
    per-entry model and names the two that have it."""
    from ddnm_amd import ops
    from ddnm_amd.functions.svd_ddnm import ddnm_plus_diffusion
    from oracle import cases, schedule
    E = _E()
    cfg, _, model = small_net
    d, B = cfg.data.image_size, 2
    n_it = len(schedule.jump_times(4, 2, 2)) - 1
    x_orig, x_T, tape = cases.sampler_case(cfg, B, n_it)
    tape = [t.cuda() for t in tape]
    seen = []
    orig = ops.step_call
    monkeypatch.setattr(ops, "step_call", lambda name, *a: (seen.append(name), orig(name, *a))[1])
    op = E.Mosaic(3, d, "rggb", "cuda")
    y = op.A(x_orig.cuda())
    run = lambda sy: ddnm_plus_diffusion(x_T.cuda(), model, cases.betas().cuda(), ETA, op, y, sy, config=cfg,    # noqa: E731
                                         noise=tape, return_cpu=False)[0][0]
    x_float = run(0.2)
    names_float, seen[:] = list(seen), []
    x_model = run(E.NoiseModel.scalar(0.1))
    assert seen == names_float and set(seen) == {"ddnm_step_plus_mosaic_f32"} and torch.equal(x_float, x_model)
    seen[:] = []
    run(E.NoiseModel.shot(0.1, 0.05))
    assert len(seen) == len(names_float) and set(seen) == {"ddnm_step_plus_mosaic_hn_f32"}
    with pytest.raises(ValueError, match="Mosaic.*Denoising"):
        ddnm_plus_diffusion(x_T.cuda(), model, cases.betas().cuda(), ETA, E.Colorization(d, "cuda"), y, E.NoiseModel.shot(0.1, 0.05),
                            config=cfg, noise=tape)


# ---------------------------------------------------------------------------------------------- 4. runner
SHOT = ["--path_y", "synthetic:3", "--eta", "0.85", "--deg", "demosaic_rggb", "--sigma_y", "0.02", "--sigma_y_shot", "0.01",
        "--add_noise"]


def _pngs(tmp_path, folder):
    out = tmp_path / "exp" / "image_samples" / folder
    return {p.name: p.read_bytes() for p in out.glob("*.png")}


def test_runner_plain_fused_and_two_samples_write_the_same_pngs(hip, tmp_path, monkeypatch, capsys):
    """main.py --deg demosaic_rggb --sigma_y 0.02 --sigma_y_shot 0.01 --add_noise on synthetic:3 (64 px, T = 4): the plain
    run, DDNM_FUSE_BATCHES=2 and sample 0 of DDNM_SAMPLES=2 write byte-identical PNGs for the images they share; every
    step went through the one-launch per-entry step.  Measured on the MI355X (printed): the restored tensors differ by
    2.1e-7 (fused) and 2.5e-7 (sample 0 of 2) rel-L2, below a grey level."""
    from ddnm_amd import ops
    _mini_yaml(tmp_path)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("DDNM_SAMPLES", raising=False)
    seen = []
    orig = ops.step_call
    monkeypatch.setattr(ops, "step_call", lambda name, *a: (seen.append(name), orig(name, *a))[1])
    calls1, psnr1, img1, names1, _ = _run_main(tmp_path, monkeypatch, "plain", SHOT, None)
    assert set(seen) == {"ddnm_step_plus_mosaic_hn_f32"} and len(seen) >= 3 * 4
    calls2, psnr2, img2, names2, _ = _run_main(tmp_path, monkeypatch, "fused", SHOT, 2)
    monkeypatch.setenv("DDNM_SAMPLES", "2")
    calls3, _, img3, names3, _ = _run_main(tmp_path, monkeypatch, "samples", SHOT, None)
    monkeypatch.delenv("DDNM_SAMPLES")
    out = capsys.readouterr().out
    assert out.count("Number of samples: 3") == 3, out[-3000:]
    assert calls1 == [1] and calls2 == [2, 1] and calls3 == [2]
    assert names1 == names2 == [f"{i}_0.png" for i in range(3)]
    assert names3 == sorted(f"{i}_{k}.png" for i in range(3) for k in range(2))
    print(f"shot-noise runner: fused K=2 vs plain rel-L2 {rel(img2, img1):.3e}, sample 0 of 2 vs plain rel-L2 "
          f"{rel(img3[0::2], img1):.3e}")
    plain, fused, samples = (_pngs(tmp_path, f) for f in ("plain", "fused", "samples"))
    assert torch.isfinite(img1).all() and len({plain[n] for n in names1}) == 3
    for name in names1:
        assert plain[name] == fused[name], name
        assert plain[name] == samples[name], name
    assert rel(img3[1::2], img1) > 1e-3                                   # sample 1 is another draw


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    root = tmp_path_factory.mktemp("hn_measurements")
    _mini_yaml(root)
    rng = np.random.default_rng(5)
    row = rng.uniform(0.0, 0.08, 64 * 64).astype(F)
    row[::5] = 0
    np.save(os.path.join(str(root), "map.npy"), row.reshape(1, 64, 64))
    np.save(os.path.join(str(root), "map_other.npy"), (row * F(1.5)).reshape(1, 64, 64))
    np.save(os.path.join(str(root), "map_short.npy"), row[:-4])
    return str(root)


@pytest.mark.parametrize("form", ["shot", "map"])
def test_round_trip_of_saved_measurements(hip, workdir, form):
    """DDNM_SAVE_Y=1 with the model simulated by --add_noise, then the run over measurements:<its y/> with the model
    stated alone: the same PNG bytes (tests/test_gpu_measurements.py::_round_trip); measurements.json carries the model,
    and DDNM_METRICS=cons of the second run compares A x^ with the saved rows."""
    import json
    model = (["--sigma_y", "0.02", "--sigma_y_shot", "0.01"] if form == "shot"
             else ["--sigma_y_map", os.path.join(workdir, "map.npy")])
    argv = ["--deg", "demosaic_rggb"] + model
    truth, given = _round_trip(workdir, f"hn_{form}", argv + ["--add_noise"], argv, 2)
    with open(os.path.join(truth["folder"], "y", "measurements.json")) as f:
        saved = json.load(f)
    if form == "shot":
        assert saved["sigma_y"] == 0.02 and saved["sigma_y_shot"] == 0.01 and saved["sigma_y_map_sha256"] is None
    else:
        assert saved["sigma_y"] == 0.0 and saved["sigma_y_map_len"] == 4096 and len(saved["sigma_y_map_sha256"]) == 64
    rows = [np.load(os.path.join(truth["folder"], "y", f"y_{i}.npy")) for i in range(2)]
    assert all(r.dtype == np.float32 and r.shape == (4096,) and np.isfinite(r).all() for r in rows)
    assert [c["y"].shape for c in given["cons"]] == [(1, 4096)] * 2
    if form == "map":                                                      # entries with sigma_j = 0 were not disturbed
        clean = _run(workdir, "hn_clean", ["--path_y", "synthetic:2", "--deg", "demosaic_rggb", "--sigma_y", "0."], DDNM_SAVE_Y=1)
        ref = np.load(os.path.join(clean["folder"], "y", "y_0.npy"))
        assert np.array_equal(rows[0][::5], ref[::5]) and not np.array_equal(rows[0], ref)


def _refused(workdir, folder, argv, caplog, *words):
    """main.main logs the ValueError and restores nothing: no `Number of samples` line, no PNG, the network never ran."""
    import contextlib
    import io
    import main
    from ddnm_amd.guided_diffusion.models import Model
    from tests.test_gpu_measurements import SWITCHES
    cwd, buf = os.getcwd(), io.StringIO()
    caplog.clear()
    with pytest.MonkeyPatch.context() as m, caplog.at_level(logging.ERROR):
        m.setenv("DDNM_RANDOM_WEIGHTS", "1")
        for name in SWITCHES:
            m.delenv(name, raising=False)
        m.setattr(Model, "__call__", lambda self, x, t: pytest.fail("the network ran"))
        os.chdir(workdir)
        try:
            with contextlib.redirect_stdout(buf):
                assert main.main(["--ni", "--config", "mini.yml", "-i", folder, "--eta", "0.85"] + argv) == 0
        finally:
            os.chdir(cwd)
    assert "Number of samples:" not in buf.getvalue()
    assert not [f for f in _files(os.path.join(workdir, "exp", "image_samples", folder)) if f.endswith(".png")]
    assert "ValueError" in caplog.text
    for w in words:
        assert w in caplog.text, (w, caplog.text[-1500:])


def test_runner_refusals(hip, workdir, caplog):
    """--simplified, a map of the wrong length, a map together with a non-zero --sigma_y, an operator without the hook and
    a folder of measurements formed under another model: each is a ValueError that says what is wrong, before anything
    is restored."""
    shot = ["--sigma_y", "0.02", "--sigma_y_shot", "0.01"]
    syn = ["--path_y", "synthetic:1"]
    _refused(workdir, "r_simplified", syn + ["--deg", "demosaic_rggb", "--simplified"] + shot, caplog, "--simplified")
    _refused(workdir, "r_short", syn + ["--deg", "demosaic_rggb", "--sigma_y_map", os.path.join(workdir, "map_short.npy")],
             caplog, "map_short.npy", "4096", "4092")
    _refused(workdir, "r_both", syn + ["--deg", "demosaic_rggb", "--sigma_y", "0.02", "--sigma_y_map",
                                      os.path.join(workdir, "map.npy")], caplog, "map.npy", "--sigma_y")
    _refused(workdir, "r_op", syn + ["--deg", "colorization"] + shot, caplog, "Mosaic", "Denoising", "colorization")
    # changed settings: a folder saved under one model, restored under another
    saved = _run(workdir, "r_saved", syn + ["--deg", "demosaic_rggb", "--add_noise"] + shot, DDNM_SAVE_Y=1)
    ydir = os.path.join(saved["folder"], "y")
    other = ["--path_y", f"measurements:{ydir}", "--deg", "demosaic_rggb"]
    _refused(workdir, "r_gain", other + ["--sigma_y", "0.02", "--sigma_y_shot", "0.02"], caplog, "sigma_y_shot", "0.01", "0.02")


def test_denoising_runner_takes_the_one_launch_step(hip, workdir):
    """--deg denoising with a shot model: DDNM+ in one launch per step (today's scalar run takes the Lambda chain), under
    DDNM_FUSE_BATCHES=2 and DDNM_METRICS=cons."""
    from ddnm_amd import ops
    seen = []
    orig = ops.step_call
    with pytest.MonkeyPatch.context() as m:
        m.setattr(ops, "step_call", lambda name, *a: (seen.append(name), orig(name, *a))[1])
        run = _run(workdir, "den", ["--path_y", "synthetic:3", "--deg", "denoising", "--sigma_y", "0.03", "--sigma_y_shot", "0.02",
                                    "--add_noise"], DDNM_FUSE_BATCHES=2, DDNM_METRICS="cons")
    assert set(seen) == {"ddnm_step_plus_denoise_hn_f32"}          # (ops.step_call picks the keyed twin of a fused call itself)
    assert "Total Average Cons:" in run["out"] and len(run["cons"]) == 3 and run["metrics"]["psnr"] > 0


# ---------------------------------------------------------------------------------------------- 5. entry points
def test_entry_points_validate_on_device_pointers(hip):
    """The refusals of tests/test_hn_host.py with a real device address: the launch refuses and nothing is written."""
    buf = torch.zeros(64, device="cuda")
    check_hn_validation(hip, buf.data_ptr())
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
