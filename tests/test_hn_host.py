"""Per-entry measurement noise (shot + read noise, noise maps) on the host: the CPU model of the two `*_hn_*` step kernels
(tests/hn_model.py) against its float64 twin and its planted faults, the identity that makes the step correct, the
degeneration to today's scalar coefficients, `NoiseModel` with every refusal, the settings of measurements.json, the
hook's marshalling (dry run), the loop's dispatch and the entry points' argument checks.  No GPU call."""
import argparse
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import hn_model as H
from tests.test_measurements_host import _args, _config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _E():
    from ddnm_amd.functions import svd_operators as E
    return E


# ---------------------------------------------------------------------------------------------- 1. the model
@pytest.fixture(scope="module")
def modelled():
    """{case name: (inputs, model, twin)}, computed once."""
    out = {}
    for c in H.CASES:
        t = H.make_inputs(c)
        out[c.name] = (t, H.model(c, t), H.twin(c, t))
    return out


@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c.name)
def test_model_lies_within_the_bar_of_its_float64_twin(modelled, case):
    t, m, tw = modelled[case.name]
    for k in ("x0", "xn"):
        err, bar = np.abs(m[k].astype(np.float64) - tw[k].v), tw[k].bar()
        assert np.isfinite(m[k]).all() and np.isfinite(bar).all(), k
        assert (err <= bar).all(), (k, float((err / np.maximum(bar, 1e-300)).max()))


def test_cases_cover_the_matrix_of_the_issue():
    """Shapes, et layouts, sigma sources, eta and alpha-bar values as a union; the map cases at a = 0.5 hold sigma_j = 0,
    both thresholded branches and an exact tie in one launch; the shot cases take the clamp on both sides."""
    ps = [c.p for c in H.CASES]
    assert {(c.kernel, c.p.get("pattern"), c.p["d"]) for c in H.CASES} >= {("mosaic", "xtrans", 16), ("mosaic", "rggb", 32),
                                                                             ("denoise", None, 16)}
    assert all(p["B"] == 3 for p in ps) and {p["six"] for p in ps} == {False, True}
    assert {p["eta"] for p in ps} == {0.85, 1.0, 0.0} and {p["at_next"] for p in ps} == {0.99, 0.25}
    for kernel in ("mosaic", "denoise"):
        assert {c.p["sigma"] for c in H.CASES if c.kernel == kernel} == {"map", "shot"}
    for c in H.CASES:
        t = H.make_inputs(c)
        sig = H.sigma_of(c, t)
        br, thr = H.branches32(t["s"].a, sig, t["s"].st)
        assert (br == H.BR_BELOW).any() and (br == H.BR_ABOVE).any(), c.name
        if c.p["sigma"] == "map" and c.p["at_next"] == 0.25:
            assert t["s"].a == F(0.5)
            assert (sig == 0).any() and ((thr == t["s"].st) & (sig > 0)).sum() > 16, c.name      # exact ties
        if c.p["sigma"] == "shot":
            assert (t["y"] < -1).any() and (t["y"] > 1).any(), c.name


@pytest.mark.parametrize("fault", H.FAULTS)
def test_every_planted_fault_is_noticed(modelled, fault):
    noticed = []
    for c in H.CASES:
        t, m, _ = modelled[c.name]
        bad = H.model(c, t, fault)
        differs = not (np.array_equal(bad["x0"], m["x0"]) and np.array_equal(bad["xn"], m["xn"], equal_nan=True))
        if fault in H.faults_of(c):
            assert differs, (fault, c.name)
        noticed.append(differs)
    assert any(noticed), fault


def test_the_variance_identity_of_the_thresholded_branches():
    """(a lambda sigma_j)^2 + d1^2 + d2^2 = sigma_t^2 in float64 to 1e-12 relative, for every measured entry with
    sigma_j > 0 in the two thresholded branches, over a grid of a, sigma_t, eta and sigma_j: the noise the corrected entry
    carries into x_{t-1} (a lambda sigma_j from y, d1 fresh, d2 through eps) has the variance of the schedule."""
    sig = np.concatenate([np.geomspace(1e-4, 50.0, 97), [0.25, 0.5, 1.0, 2.0]])
    checked = 0
    for at_next in (0.9999, 0.99, 0.9, 0.5, 0.25, 0.01, 1e-4):
        a, st = np.sqrt(at_next), np.sqrt(1 - at_next)
        for eta in (0.0, 0.3, 0.85, 1.0):
            br, _ = H.branches32(F(a), sig.astype(F), F(st))
            al, d1, d2 = H.coef64(a, sig, st, eta, br)
            m = br != H.BR_PASS
            total = (al * sig) ** 2 + d1 ** 2 + d2 ** 2
            # (an entry whose fp32 branch differs from the float64 comparison sits at the threshold, where both hold)
            exact = np.where(br == H.BR_BELOW, st < a * sig, st > a * sig)
            m &= exact
            assert np.abs(total[m] / st ** 2 - 1).max() <= 1e-12, (at_next, eta)
            checked += int(m.sum())
            assert (br == H.BR_BELOW).any() or at_next < 0.01, at_next
    assert checked > 2000


@pytest.mark.parametrize("eta", [0.0, 0.85, 1.0])
@pytest.mark.parametrize("a,sigma_t", [(0.995, 0.0999), (0.5, 0.866), (0.9, 0.05), (1e-4, 0.5)])
def test_both_forms_degenerate_to_the_scalar_coefficients(a, sigma_t, eta):
    """A constant map and g = 0 give the (a lambda, d1r, d2r) of svd_operators.cs_plus_coefficients at sigma_y = sigma."""
    E = _E()
    for s01 in (0.0, 0.01, 0.2, 0.6):
        sig = np.full(8, 2 * s01)                                           # engine scale
        br, _ = H.branches32(F(a), sig.astype(F), F(sigma_t))
        al, d1, d2 = H.coef64(a, sig, sigma_t, eta, br)
        wal, d1n, d2n, dd1, dd2 = E.cs_plus_coefficients(a, 2 * s01, sigma_t, eta)
        for got, want in ((al, wal), (d1, d1n + dd1), (d2, d2n + dd2)):
            assert np.allclose(got, want, rtol=1e-12, atol=1e-15), (s01, got[0], want)
        # g = 0 is the scalar form itself
        nm = E.NoiseModel.shot(s01, 0.0)
        assert nm.is_scalar and nm.sigma_engine() == 2 * s01
    y = torch.linspace(-1.5, 1.5, 16).reshape(2, 8)
    assert torch.equal(E.NoiseModel.shot(0.1, 0.0).std(y).expand(2, 8), torch.full((2, 8), 0.2))
    assert torch.equal(E.NoiseModel.map(np.full(8, 0.1, F)).std(y).expand(2, 8), torch.full((2, 8), 0.2))


# ---------------------------------------------------------------------------------------------- 2. NoiseModel
def test_noise_model_forms_and_scales():
    E = _E()
    nm = E.NoiseModel.shot(0.02, 0.01)
    assert nm.kind == "shot" and not nm.is_scalar and nm.kernel_args("cpu", 16) == (None, 1, 0.02 ** 2, 0.01)
    y = torch.tensor([[-3.0, -1.0, 0.0, 1.0, 3.0]])
    want = 2 * torch.tensor([0.0004, 0.0004, 0.0004 + 0.005, 0.0104, 0.0104]).sqrt()
    assert torch.allclose(nm.std(y), want[None], rtol=1e-6, atol=0)
    with pytest.raises(ValueError, match="no single sigma_y"):
        nm.sigma_engine()
    row = np.arange(16, dtype=np.float64) / 64
    for shaped in (row, row[None], row.reshape(1, 4, 4)):
        m = E.NoiseModel.map(shaped, 16, (1, 4, 4), "m.npy")
        assert m.kind == "map" and m.row.dtype == np.float32 and m.row.shape == (16,)
        assert torch.equal(m.device_row("cpu"), torch.from_numpy((row * 2).astype(F)))
    ptr, mode, s2, g = m.kernel_args("cpu", 16)
    assert ptr == m.device_row("cpu").data_ptr() and (mode, s2, g) == (0, 0.0, 0.0)
    with pytest.raises(ValueError, match="16 entries.*64"):
        m.kernel_args("cpu", 64)
    assert E.NoiseModel.map(np.zeros(16, F)).row.max() == 0                  # zeros are allowed
    s = m.settings()
    assert s["sigma_y_shot"] == 0.0 and s["sigma_y_map_len"] == 16 and len(s["sigma_y_map_sha256"]) == 64
    assert nm.settings() == {"sigma_y_shot": 0.01, "sigma_y_map_sha256": None, "sigma_y_map_len": None}


def test_noise_map_refusals_name_the_file_the_size_and_what_was_found(tmp_path):
    E = _E()
    op = E.Mosaic(3, 8, "rggb", "cpu")
    den = E.Denoising(3, 8, "cpu")
    good = tmp_path / "good.npy"
    np.save(good, np.full((1, 8, 8), 0.05, F))
    assert E.NoiseModel.from_options(0.0, 0.0, str(good), op).row.shape == (64,)
    np.save(good, np.full((3, 8, 8), 0.05))                                   # float64, the denoiser's picture shape
    assert E.NoiseModel.from_options(0.0, None, str(good), den).row.shape == (192,)

    def refused(arr, *words, sigma_y=0.0, shot=0.0, operator=op, save=True):
        path = tmp_path / "bad.npy"
        if save:
            np.save(path, arr)
        with pytest.raises(ValueError) as e:
            E.NoiseModel.from_options(sigma_y, shot, str(path), operator)
        for w in ("bad.npy",) + words:
            assert w in str(e.value), (w, str(e.value))

    refused(np.zeros(60, F), "64", "[60]", "60 entries")                      # wrong length
    refused(np.zeros((2, 64), F), "64", "[2, 64]")                            # per-image maps are out of scope
    refused(np.zeros((8, 8), F), "64", "[8, 8]")                              # not one of the three accepted shapes
    refused(np.zeros((1, 8, 8), F), "192", "[1, 8, 8]", operator=den)
    bad = np.full(64, 0.1, F)
    bad[5] = np.nan
    refused(bad, "64", "finite", "entry 5")
    bad[5] = -0.25
    refused(bad, "64", "negative", "-0.25")
    refused(np.array(["a"] * 64), "64", "dtype")
    refused(np.full(64, 0.1, F), "--sigma_y", "0.02", sigma_y=0.02)           # a map together with a non-zero --sigma_y
    refused(np.full(64, 0.1, F), "--sigma_y_shot", shot=0.01)
    (tmp_path / "bad.npy").write_bytes(b"not an array")
    refused(None, "readable", save=False)
    with pytest.raises(ValueError, match="Mosaic.*Denoising"):                # an operator without the hook
        E.NoiseModel.from_options(0.0, 0.0, str(good), E.Colorization(8, "cpu"))
    for bad_g in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma_y_shot"):
            E.NoiseModel.shot(0.02, bad_g)
    with pytest.raises(ValueError, match="sigma_y"):
        E.NoiseModel.scalar(-1.0)


# ---------------------------------------------------------------------------------------------- 3. runner settings
def test_settings_round_trip_through_measurements_json(tmp_path):
    """run_settings carries sigma_y_shot and a map's SHA-256 and length; check_noise_settings refuses another shot gain,
    a changed map and a run without the model; a scalar run writes exactly what it wrote before."""
    from ddnm_amd.guided_diffusion import diffusion as D
    E = _E()
    op = E.Mosaic(3, 8, "rggb", "cpu")
    cfg = _config(size=8)
    np.save(tmp_path / "y_0.npy", np.zeros(64, F))
    np.save(tmp_path / "map.npy", np.linspace(0, 0.1, 64).astype(F))
    np.save(tmp_path / "map2.npy", np.linspace(0, 0.1001, 64).astype(F))

    def args(**kw):
        return _args(deg="demosaic_rggb", deg_scale=0.0, **kw)

    scalar = D.run_settings(args(sigma_y=0.05), cfg, 0.05, D.noise_model_of(args(sigma_y=0.05), op))
    assert scalar == D.run_settings(args(sigma_y=0.05), cfg, 0.05) and "sigma_y_shot" not in scalar
    a_shot = args(sigma_y=0.02, sigma_y_shot=0.01, sigma_y_map=None)
    shot = D.run_settings(a_shot, cfg, 0.02, D.noise_model_of(a_shot, op))
    assert shot["sigma_y_shot"] == 0.01 and shot["sigma_y_map_sha256"] is None and shot["sigma_y"] == 0.02
    a_map = args(sigma_y=0.0, sigma_y_map=str(tmp_path / "map.npy"))
    mapped = D.run_settings(a_map, cfg, 0.0, D.noise_model_of(a_map, op))
    assert mapped["sigma_y_map_len"] == 64 and len(mapped["sigma_y_map_sha256"]) == 64 and mapped["sigma_y_shot"] == 0.0
    a_map2 = args(sigma_y=0.0, sigma_y_map=str(tmp_path / "map2.npy"))
    mapped2 = D.run_settings(a_map2, cfg, 0.0, D.noise_model_of(a_map2, op))
    ds = D.MeasurementFolder(str(tmp_path))
    for saved, same, others in ((shot, shot, (scalar, mapped, {**shot, "sigma_y_shot": 0.02})),
                                (mapped, mapped, (scalar, shot, mapped2))):
        (tmp_path / "measurements.json").write_text(json.dumps(json.loads(json.dumps(saved))))
        ds.check_settings(same)
        ds.check_noise_settings(same)
        for other in others:
            with pytest.raises(ValueError, match="sigma_y_(shot|map)"):
                ds.check_noise_settings(other)
    (tmp_path / "measurements.json").write_text(json.dumps(scalar))       # a folder that records no model: the run states it
    for run in (scalar, shot, mapped):
        ds.check_noise_settings(run)


def test_runner_refuses_what_it_cannot_do():
    from ddnm_amd.guided_diffusion import diffusion as D
    E = _E()
    with pytest.raises(ValueError, match="simplified"):
        D.check_noise_flags(_args(sigma_y_shot=0.01), True)
    with pytest.raises(ValueError, match="simplified"):
        D.check_noise_flags(_args(sigma_y_map="m.npy"), True)
    D.check_noise_flags(_args(sigma_y_shot=0.01), False)
    D.check_noise_flags(_args(), True)                                   # a namespace without the flags: the scalar model
    assert D.noise_model_of(_args(sigma_y=0.05), E.Colorization(8, "cpu")).is_scalar
    with pytest.raises(ValueError, match="Mosaic.*Denoising"):
        D.noise_model_of(_args(sigma_y=0.02, sigma_y_shot=0.01, deg="colorization"), E.Colorization(8, "cpu"))


def test_command_lines_know_the_flags(tmp_path, monkeypatch, capsys):
    import importlib.util
    import main
    names = {n for group in (main.FLAGS, main.ENGINE_FLAGS) for ns, _ in group for n in ns}
    assert {"--sigma_y_shot", "--sigma_y_map"} <= names
    monkeypatch.chdir(tmp_path)
    args, _ = main.parse_args_and_config(["--ni", "--config", "celeba_hq.yml", "--path_y", "synthetic:1", "--deg",
                                          "demosaic_rggb", "--sigma_y", "0.02", "--sigma_y_shot", "0.01", "-i", "t"])
    assert args.sigma_y_shot == 0.01 and args.sigma_y_map is None
    spec = importlib.util.spec_from_file_location("hq_main_for_hn", os.path.join(ROOT, "hq_demo", "main.py"))
    hq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hq)
    assert "sigma_y_shot" not in hq.parse([]) and "sigma_y_map" not in hq.parse([])
    for argv in (["--sigma_y_shot", "0.01"], ["--sigma_y_map", "m.npy"]):
        with pytest.raises(SystemExit):
            hq.parse(argv)
        assert "per-entry measurement noise" in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------- 4. hook, loop, entry points
def test_hook_marshals_its_arguments_and_the_loop_dispatches():
    """Host-only dry run (tools/dry_run.py): the hook of both operators reaches its entry point with arguments of the
    declared types for a tensor and an in-kernel noise source (the keyed table lives on the GPU: tests/test_gpu_hn.py);
    the loop refuses an operator without the hook by name."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import dry_run
    finally:
        sys.path.pop(0)
    from ddnm_amd import _lib, ops
    from ddnm_amd.functions import svd_ddnm
    E = _E()
    saved = (_lib._lib, ops._stream, ops._f32c, ops._f16c)
    try:
        dry = dry_run.install()
        d, B = 16, 2
        x = torch.zeros(B, 3, d, d)
        et6 = torch.zeros(B, 6, d, d)
        s = ops.step_scalars(torch.tensor(0.5), torch.tensor(0.6), 0.85)
        out = torch.zeros_like(x), torch.zeros_like(x)
        for op, n in ((E.Mosaic(3, d, "xtrans", "cpu"), d * d), (E.Denoising(3, d, "cpu"), 3 * d * d)):
            y = torch.zeros(B, n)
            with pytest.raises(RuntimeError, match="begin_plus_run"):
                op.ddnm_plus_step_hn(x, et6[:, :3], None, s, 0.5, 0.85, *out)
            op.begin_plus_run(y)
            with pytest.raises(RuntimeError, match="noise_model"):
                op.ddnm_plus_step_hn(x, et6[:, :3], None, s, 0.5, 0.85, *out)
            with pytest.raises(ValueError, match=f"{n + 4}"):
                op.begin_plus_run(y, E.NoiseModel.map(np.zeros(n + 4, F)))
            with pytest.raises(ValueError):
                op.begin_plus_run(y[:, :-4], E.NoiseModel.shot(0.02, 0.01))
            for nm in (E.NoiseModel.map(np.full(n, 0.1, F)), E.NoiseModel.shot(0.02, 0.01)):
                op.begin_plus_run(y, nm)
                op.ddnm_plus_step_hn(x, et6[:, :3], torch.zeros_like(x), s, 0.5, 0.85, *out)
                op.ddnm_plus_step_hn(x, et6[:, :3], None, ops.PhiloxNoise(5).stamp(s, 1), 0.5, 0.85, *out)
        assert dry.calls == {"ddnm_step_plus_mosaic_hn_f32": 4, "ddnm_step_plus_denoise_hn_f32": 4}
    finally:
        _lib._lib, ops._stream, ops._f32c, ops._f16c = saved
    # the loop refuses before anything runs (the tensors only have to claim a GPU: nothing is launched)
    fake = argparse.Namespace(is_cuda=True)
    with pytest.raises(ValueError, match="Mosaic.*Denoising"):
        svd_ddnm.ddnm_plus_diffusion(fake, None, None, 0.85, E.Colorization(8, "cpu"), None, E.NoiseModel.shot(0.02, 0.01))


def check_hn_validation(lib, ptr):
    """Every refusal of the four `*_hn_*` entry points with `ptr` standing for each tensor (never dereferenced: all of it
    happens before a launch).  DDNM_E_BADARG = -1 comes before DDNM_E_SHAPE = -2."""
    from ddnm_amd._lib import StepScalars
    s = StepScalars()
    s.rng_on = 1
    sp = ctypes.byref(s)
    pat = (ctypes.c_uint8 * 4)(0, 1, 1, 2)
    bad_pat = (ctypes.c_uint8 * 4)(0, 1, 3, 2)
    nan, inf = float("nan"), float("inf")

    def mosaic(fn, xt=ptr, et=ptr, es=768, nz=None, y=ptr, x0=ptr, xn=ptr, B=2, H=16, W=16, p=pat, ph=2, pw=2, smap=ptr, mode=0,
               s2=0.0, g=0.0, st=0.5, st2=0.25, c1=0.4, c2=0.3, sc=sp):
        return fn(xt, et, es, nz, y, x0, xn, B, H, W, p, ph, pw, smap, mode, s2, g, st, st2, c1, c2, sc, None)

    def denoise(fn, xt=ptr, et=ptr, es=768, nz=None, y=ptr, x0=ptr, xn=ptr, B=2, chw=768, smap=ptr, mode=0, s2=0.0, g=0.0,
                st=0.5, st2=0.25, c1=0.4, c2=0.3, sc=sp):
        return fn(xt, et, es, nz, y, x0, xn, B, chw, smap, mode, s2, g, st, st2, c1, c2, sc, None)

    table = ((mosaic, lib.ddnm_step_plus_mosaic_hn_f32, False), (mosaic, lib.ddnm_step_plus_mosaic_hn_keyed_f32, True),
             (denoise, lib.ddnm_step_plus_denoise_hn_f32, False), (denoise, lib.ddnm_step_plus_denoise_hn_keyed_f32, True))
    off = StepScalars()                                                    # rng_on = 0 and no noise tensor: no source
    for call, fn, keyed in table:
        nz = ptr if keyed else None
        name = fn.__name__
        # null pointers, batch, noise source, the row in map mode: DDNM_E_BADARG
        for k in ("xt", "et", "y", "x0", "xn", "sc"):
            assert call(fn, nz=nz, **{k: None}) == -1, (name, k)
        assert call(fn, nz=nz, B=0) == -1 and call(fn, nz=nz, smap=None) == -1 and call(fn, nz=nz, smap=ptr + 4) == -1, name
        if keyed:
            assert call(fn, nz=None) == -1 and call(fn, nz=ptr + 4) == -1, name
        else:
            assert call(fn, sc=ctypes.byref(off)) == -1, name
        # ... and it wins over a bad shape or a bad model
        assert call(fn, nz=nz, y=None, es=6) == -1 and call(fn, nz=nz, smap=None, mode=0, es=6) == -1, name
        assert call(fn, nz=nz, B=0, mode=7) == -1, name
        # sizes: DDNM_E_SHAPE
        assert call(fn, nz=nz, es=6) == -2 and call(fn, nz=nz, es=770) == -2, name
        if call is mosaic:
            assert call(fn, nz=nz, p=None) == -1 and call(fn, nz=nz, H=0) == -1, name
            assert call(fn, nz=nz, W=6) == -2 and call(fn, nz=nz, H=18) == -2 and call(fn, nz=nz, pw=9) == -2, name
            assert call(fn, nz=nz, ph=0) == -2 and call(fn, nz=nz, p=bad_pat) == -2, name
        else:
            assert call(fn, nz=nz, chw=0) == -1 and call(fn, nz=nz, chw=770) == -2, name
        # the model: DDNM_E_SHAPE
        assert call(fn, nz=nz, mode=2) == -2 and call(fn, nz=nz, mode=-1) == -2, name
        for bad in (-1e-6, nan, inf):
            assert call(fn, nz=nz, smap=None, mode=1, s2=bad, g=0.01) == -2, (name, bad)
            assert call(fn, nz=nz, smap=None, mode=1, s2=1e-4, g=bad) == -2, (name, bad)
            assert call(fn, nz=nz, st=bad) == -2 and call(fn, nz=nz, st2=bad) == -2, (name, bad)
        assert call(fn, nz=nz, c1=nan) == -2 and call(fn, nz=nz, c2=inf) == -2, name


def test_entry_points_validate_their_arguments():
    from ddnm_amd import _lib, build
    build.build()
    check_hn_validation(_lib.lib(), 4096)
