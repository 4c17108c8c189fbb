"""CPU checks of tests/step_model.py, the model tests/test_gpu_step_edges.py holds the kernels of csrc/ddnm_step.hip to:
the case table reaches every branch of the written list below and every case lands on the branch its name claims; the
fp32 restatement lies within the derived bar of its float64 twin, and the twin agrees with the oracle's CPU operators where
there is one (square shapes); every planted fault a case is meant to catch changes at least one bit of the model's output;
the second-trip launches are just past one trip of the capped grid."""
import numpy as np
import pytest
import torch

from tests import step_model as SM

CASE_IDS = [c.name for c in SM.CASES]


def _inputs(name):
    return SM.make_inputs(SM.BY_NAME[name])


def _of(kernel):
    return [c for c in SM.CASES if c.kernel == kernel]


# ----------------------------------------------------------------------------- coverage
def _has(kernel, **want):
    return any(all(c.p.get(k) == v for k, v in want.items()) for c in _of(kernel))


STEP_KERNELS = ("step_x0", "step_combine", "step_sr4", "step_color", "step_inpaint", "step_inpaint_pi", "step_denoise")

# (branch, how the table is asked for it).  Noise source, et stride and the x0 option are not properties of a case: the GPU
# test launches EVERY fused-step case once per entry of SM.variants(kernel), which is what the list asks about them.
COVERAGE = []
for _k in STEP_KERNELS:
    for _B in SM.BATCHES:
        COVERAGE.append((f"{_k}: B = {_B}", lambda k=_k, B=_B: _has(k, B=B)))
    if _k != "step_x0":               # step_x0 takes neither lambda nor c1 / c2
        for _lam in SM.LAMBDAS:
            COVERAGE.append((f"{_k}: lambda = {_lam}", lambda k=_k, v=_lam: _has(k, lam=v)))
        for _eta in SM.ETAS:
            COVERAGE.append((f"{_k}: eta = {_eta}" + (" (c2 == 0)" if _eta == 1.0 else " (c1 == 0)" if _eta == 0.0 else ""),
                             lambda k=_k, v=_eta: _has(k, eta=v)))
for _k in STEP_KERNELS:              # launched for every case of the kernel
    for _n in ((None,) if _k == "step_x0" else SM.NOISE_SOURCES):
        for _e in SM.ET_STRIDES:
            for _x in (SM.X0_OPTIONS if _k not in ("step_x0", "step_combine") else (None,)):
                COVERAGE.append((f"{_k}: noise {_n}, et {_e}, {_x or 'x0 not optional'}",
                                 lambda k=_k, v=(_n, _e, _x): v in SM.variants(k)))
for _hw in ((4, 4), (4, 12), (12, 4), (8, 20)):
    COVERAGE.append((f"step_sr4: (H, W) = {_hw}", lambda hw=_hw: _has("step_sr4", H=hw[0], W=hw[1])))
for _HW in (4, 12, 160):
    COVERAGE.append((f"step_color: HW = {_HW}", lambda v=_HW: _has("step_color", HW=v)))
for _w in (None, SM.W_CUSTOM):
    COVERAGE.append((f"step_color: w3_host = {_w}", lambda v=_w: _has("step_color", w3=v)))
    for _k in ("color_A", "color_pinv"):
        for _HW in (1, 7, 160):
            COVERAGE.append((f"{_k}: HW = {_HW}, w3_host = {_w}", lambda k=_k, h=_HW, v=_w: _has(k, HW=h, w3=v)))
for _HW, _m in ((4, "one"), (60, "all"), (60, "part")):
    for _k in ("step_inpaint", "inpaint_A", "inpaint_pinv"):
        COVERAGE.append((f"{_k}: shared mask, HW = {_HW}, kept {_m}", lambda k=_k, h=_HW, m=_m: _has(k, HW=h, mask=m)))
for _k in ("step_inpaint_pi", "inpaint_A_pi", "inpaint_pinv_pi"):
    COVERAGE.append((f"{_k}: B = 3 masks with one / all / part kept, padded rows",
                     lambda k=_k: any(c.p["B"] == 3 and set(c.p["masks"]) == {"one", "all", "part"}
                                      and c.p["y_stride"] > 180 for c in _of(k))))
for _chw in (4, 12, 480):
    for _k in ("step_x0", "step_denoise", "step_combine"):
        COVERAGE.append((f"{_k}: chw = {_chw}", lambda k=_k, v=_chw: _has(k, chw=v)))
for _apy in (False, True):
    COVERAGE.append((f"step_combine: apy {'given' if _apy else 'NULL'}", lambda v=_apy: _has("step_combine", apy=v)))
for _s in ((6, 9, 3), (4, 12, 4), (5, 7, 1), (16, 32, 16), (8, 4, 2)):
    for _k in ("avgpool", "upsample"):
        COVERAGE.append((f"{_k}: (H, W, r) = {_s}, BC = 5", lambda k=_k, s=_s: _has(k, H=s[0], W=s[1], r=s[2], BC=5)))
for _s in ((4, 4), (12, 4), (24, 8), (64, 32)):
    COVERAGE.append((f"patchify: (D, ps) = {_s}, 5 planes", lambda s=_s: _has("patchify", D=s[0], ps=s[1], planes=5)))
for _scale in (False, True):
    for _rel, _cmp in (("above", lambda o, i: o > i), ("below", lambda o, i: o < i), ("equal", lambda o, i: o == i)):
        COVERAGE.append((f"gather_scale: idx NULL, n_out {_rel} n_in, scale {_scale}",
                         lambda s=_scale, f=_cmp: any(not c.p["idx"] and c.p["scale"] == s and c.p["B"] == 3
                                                      and f(c.p["n_out"], c.p["n_in"]) for c in _of("gather_scale"))))
    COVERAGE.append((f"gather_scale: idx a permutation with -1 entries, scale {_scale}",
                     lambda s=_scale: _has("gather_scale", idx=True, scale=s, B=3)))
for _n in (1, 3, 4, 16):
    for _t in (0, 1):
        COVERAGE.append((f"site_matmul: site-major, n = {_n}, trans = {_t}",
                         lambda n=_n, t=_t: _has("site_matmul", n=n, trans=t, layout="site", B=2)))
for _t in (0, 1):
    COVERAGE.append((f"site_matmul: plane layout, n = 3, trans = {_t}", lambda t=_t: _has("site_matmul", n=3, trans=t, layout="plane")))
for _op, _y in ((0, False), (1, False), (1, True)):
    for _s in ((4, 6, 2), (8, 4, 4), (6, 9, 3)):
        COVERAGE.append((f"site_spectral: mode 0, (H, W, r) = {_s}, op {_op}, y {_y}",
                         lambda s=_s, o=_op, y=_y: _has("site_spectral", mode=0, H=s[0], W=s[1], r=s[2], op=o, y=y)))
    for _HW in (1, 35):
        COVERAGE.append((f"site_spectral: mode 1, H W = {_HW}, op {_op}, y {_y}",
                         lambda h=_HW, o=_op, y=_y: any(c.p["mode"] == 1 and c.p["H"] * c.p["W"] == h and c.p["op"] == o
                                                        and c.p["y"] == y for c in _of("site_spectral"))))
for _pm in (0, 1, 3):
    for _y in (False, True):
        COVERAGE.append((f"mask_mix: planes_mask = {_pm} (0: NULL) over 6 planes, y {_y}",
                         lambda m=_pm, y=_y: _has("mask_mix", planes_mask=m, y=y, planes=6)))
for _pt in (1, 3):
    COVERAGE.append((f"mul_planes: planes_table = {_pt}, 6 planes of 35",
                     lambda v=_pt: _has("mul_planes", planes_table=v, planes=6, plane_elems=35)))
for _n in (1, 257):
    for _y in (False, True):
        COVERAGE.append((f"axpby: n = {_n}, y {_y}", lambda n=_n, y=_y: _has("axpby", n=n, y=y)))
    COVERAGE.append((f"fill: n = {_n}", lambda n=_n: _has("fill", n=n)))
COVERAGE.append(("axpby_strided: x_bstride = 2 chw, chw = 35, B = 3", lambda: _has("axpby_strided", chw=35, B=3)))
for _mode in (0, 1):
    COVERAGE.append((f"spectral_mix: mode {_mode}, tie / zeros / both sides", lambda m=_mode: any(
        c.p["mode"] == m and c.p["a"] != 0 and c.p["sigma_y"] != 0 and c.p["planes"] == 3 and c.p["plane_elems"] == 35
        for c in _of("spectral_mix"))))
    COVERAGE.append((f"spectral_mix: mode {_mode}, a == 0", lambda m=_mode: _has("spectral_mix", mode=m, a=0.0)))
    COVERAGE.append((f"spectral_mix: mode {_mode}, sigma_y == 0", lambda m=_mode: _has("spectral_mix", mode=m, sigma_y=0.0)))
for _n in (4, 1028):
    COVERAGE.append((f"renoise: n = {_n}", lambda n=_n: _has("renoise", n=n)))
for _chw in (1, 3 * 32 * 32, 16384 + 5):
    for _img, _xo in ((True, True), (False, True), (True, False)):
        COVERAGE.append((f"finalize_psnr: chw = {_chw}, img {_img}, x_orig {_xo}, B = 3",
                         lambda c=_chw, i=_img, x=_xo: _has("finalize_psnr", chw=c, img=i, x_orig=x, B=3)))
for _chw in (4, 12):
    for _base in (0, 5):
        COVERAGE.append((f"randn_philox: chw = {_chw}, image_base = {_base}, B = 3",
                         lambda c=_chw, b=_base: _has("randn_philox", chw=c, image_base=b, B=3)))
# Not reachable from any entry point, so not in the list: finalize_psnr with img NULL AND x_orig NULL does nothing (the
# wrapper never asks for it); site_matmul with in == out is refused (pinned by the replay in conv_host_plans.json).


def test_the_table_reaches_every_branch_of_the_list():
    missing = [name for name, reached in COVERAGE if not reached()]
    assert not missing, missing
    assert len({name for name, _ in COVERAGE}) == len(COVERAGE)
    kernels = {c.kernel for c in SM.CASES}
    assert kernels == set(STEP_KERNELS) | {"avgpool", "upsample", "color_A", "color_pinv", "inpaint_A", "inpaint_pinv",
                                           "inpaint_A_pi", "inpaint_pinv_pi", "axpby", "axpby_strided", "mask_mix", "mul_planes",
                                           "gather_scale", "site_matmul", "site_spectral", "spectral_mix", "patchify", "renoise",
                                           "fill", "finalize_psnr", "randn_philox"}
    assert SM.NOISE_SOURCES == ("tensor", "in_kernel", "keyed") and SM.ET_STRIDES == ("contiguous", "six_channel")
    assert SM.X0_OPTIONS == ("x0_out", "x0_null")
    assert all(c.why for c in SM.CASES)


@pytest.mark.parametrize("name", CASE_IDS)
def test_case_lands_on_the_branch_its_name_claims(name):
    case, t = SM.BY_NAME[name], _inputs(name)
    p, k = case.p, case.kernel
    if k.startswith("step_"):
        s = t["s"]
        assert float(s.lam) == float(np.float32(p["lam"]))
        assert (float(s.c2) == 0.0) == (p["eta"] == 1.0) and (float(s.c1) == 0.0) == (p["eta"] == 0.0)
        C, H, W = SM.step_shape(case)
        assert t["xt"].shape == (p["B"], C, H, W) and t["et6"].shape == (p["B"], 2 * C, H, W)
        assert (C * H * W) % 4 == 0
        if "chw" in p:
            assert C * H * W == p["chw"]
        if "HW" in p:
            assert H * W == p["HW"] and p["HW"] % 4 == 0
        if k == "step_combine":
            assert (t["apy"] is not None) == p["apy"]
    if "mask" in t and k != "mask_mix":
        m = np.atleast_2d(t["mask"])
        kinds = p["masks"] if "masks" in p else (p["mask"],)
        for row, kind in zip(m, kinds):
            n = int(row.sum())
            assert {"one": n == 1, "all": n == p["HW"], "part": 0.2 * p["HW"] < n < 0.6 * p["HW"]}[kind], (kind, n)
        rk = np.atleast_2d(t["rank"])
        for row, mrow in zip(rk, m):
            assert sorted(row[row >= 0].tolist()) == list(range(int(mrow.sum()))) and bool(((row >= 0) == mrow).all())
        if "masks" in p:
            assert p["y_stride"] % 4 == 0 and p["y_stride"] > 3 * int(m.sum(axis=1).max())
            if "y" in t:
                for b, mrow in enumerate(m):
                    nk = 3 * int(mrow.sum())
                    assert not np.isnan(t["y"][b, :nk]).any() and np.isnan(t["y"][b, nk:]).all()
    if k == "gather_scale":
        assert (t["idx"] is not None) == p["idx"] and (t["scale"] is not None) == p["scale"]
        if p["idx"]:
            idx = t["idx"]
            pos = idx[idx >= 0]
            assert 0.25 < float((idx < 0).mean()) < 0.75 and len(set(pos.tolist())) == len(pos) and int(pos.max()) == p["n_in"] - 1
    if k == "site_matmul":
        base, (sb, ss, sj) = SM.site_offsets(p)
        assert (ss, sj) == ((p["n"], 1) if p["layout"] == "site" else (1, p["sites"]))
        assert (p["B"] * p["sites"]) % 256 != 0 and p["B"] * p["sites"] > 256
        cover = np.sort((base[:, None] + np.arange(p["n"])[None, :] * sj).reshape(-1))
        assert np.array_equal(cover, np.arange(t["in"].size))
    if k == "site_spectral":
        V = t["V"].astype(np.float64)
        assert np.abs(V @ V.T - np.eye(p["n"])).max() < 1e-6 and (t["y"] is not None) == p["y"]
    if k == "mask_mix":
        assert (t["mask"] is None) == (p["planes_mask"] == 0) and (t["y"] is not None) == p["y"]
        if t["mask"] is not None:
            m = t["mask"]
            assert m[0, 0] == 0 and not np.signbit(m[0, 0]) and m[0, 1] == 0 and np.signbit(m[0, 1])
            assert 0.2 < float((m == 0).mean()) < 0.8
    if k == "spectral_mix":
        lam, d1, d2, regime = SM.spectral_coef(t["stab"], t["a"], t["sy"], t["st"], t["eta"], t["eta_c"])
        if p["a"] != 0 and p["sigma_y"] != 0:
            thr = (t["a"] * t["sy"]) * (np.float32(1) / t["stab"][0])
            assert thr == t["st"] and regime[0] == 0 and t["stab"][0] != 0             # the exact tie, in fp32
            assert (lam[0], d1[0], d2[0]) == (1.0, t["st"] * t["eta"], t["st"] * t["eta_c"])
            assert t["stab"][1] == 0 and regime[3] == 1 and regime[4] == -1
            assert (regime == 1).sum() > 3 and (regime == -1).sum() > 3 and (regime[5:] != 0).all()
        else:
            assert (regime == 0).all() and (lam == 1).all()
    if k == "finalize_psnr":
        h = (t["x"] + np.float32(1)) / np.float32(2)
        assert (h > 1).any() and (h < 0).any() and ((h > 0) & (h < 1)).any()
        assert (t["xo"] is not None) == p["x_orig"]


# ----------------------------------------------------------------------------- the model is the operation
def _finite_normal(a, what):
    a = np.asarray(a)
    v = a[~np.isnan(a)]
    assert np.isfinite(v).all(), what
    assert not ((v != 0) & (np.abs(v) < SM.TINY)).any(), f"{what}: an fp32 subnormal"


@pytest.mark.parametrize("name", CASE_IDS)
def test_model_within_the_bar_of_its_float64_twin(name):
    case, t = SM.BY_NAME[name], _inputs(name)
    for key, v in t.items():
        if isinstance(v, np.ndarray) and v.dtype == np.float32:
            _finite_normal(v, f"{name} input {key}")
    got, ref = SM.model(case, t), SM.twin(case, t)
    assert set(got) == set(ref)
    for key in got:
        g, r = got[key], ref[key]
        assert g.shape == r.v.shape, (key, g.shape, r.v.shape)
        _finite_normal(g, f"{name} output {key}")
        assert np.array_equal(np.isnan(g), np.isnan(r.v)), f"{name} {key}: NaN pattern"
        ok = ~np.isnan(g)
        err, bar = np.abs(g.astype(np.float64) - r.v)[ok], r.bar()[ok]
        over = err > bar
        assert not over.any(), f"{name} {key}: {int(over.sum())} elements over the bar (k = {r.k}), worst ratio " \
                               f"{float((err[over] / bar[over]).max())}"
        if r.k == 0:
            assert (err == 0).all()


def _square_oracle_cases():
    """Ad-hoc square cases of the kernels the oracle has a CPU operator for (the table's own shapes are mostly not square)."""
    C = SM.Case
    return [
        C("o_sr4", "step_sr4", "oracle", dict(B=2, lam=0.3, eta=0.85, H=8, W=8)),
        C("o_color", "step_color", "oracle", dict(B=2, lam=0.3, eta=0.85, hw=(4, 4), HW=16, w3=None)),
        C("o_inpaint", "step_inpaint", "oracle", dict(B=2, lam=0.3, eta=0.85, hw=(4, 4), HW=16, mask="part")),
        C("o_denoise", "step_denoise", "oracle", dict(B=2, lam=0.3, eta=0.85, shape=(3, 4, 4), chw=48)),
    ]


def _oracle_operator(case, t):
    from oracle import operators as O
    d = SM.step_shape(case)[1]
    if case.kernel == "step_sr4":
        return O.SuperResolution(3, d, 4)
    if case.kernel == "step_color":
        return O.Colorization(d)
    if case.kernel == "step_denoise":
        return O.Denoising(3, d)
    mask = torch.from_numpy(t["mask"].reshape(d, d).astype(np.int64))
    return O.Inpainting(3, d, O.Inpainting.missing_from_mask(mask))


@pytest.mark.parametrize("case", _square_oracle_cases(), ids=lambda c: c.name)
def test_twin_agrees_with_the_oracle_step(case):
    """x0 and x_t' of the twin against the DDNM step of test_ddnm_step written with the oracle's A / A_pinv, in float64."""
    t = SM.make_inputs(case)
    s, B = t["s"], case.p["B"]
    op = _oracle_operator(case, t)
    xt, et, nz = (torch.from_numpy(np.ascontiguousarray(a)).double() for a in (t["xt"], SM.et_of(t), t["nz"]))
    y = torch.from_numpy(t["y"]).double().reshape(B, -1)
    x0 = (xt - et * float(s.s1)) / float(s.s2)
    x0h = x0 - float(s.lam) * op.A_pinv(op.A(x0.reshape(B, -1)) - y).reshape(x0.shape)
    xn = float(s.a) * x0h + float(s.c1) * nz + float(s.c2) * et
    ref = SM.twin(case, t)
    for key, want in (("x0", x0), ("xn", xn)):
        err = np.abs(ref[key].v - want.numpy())
        assert (err <= ref[key].bar()).all(), (case.name, key, float((err / ref[key].bar()).max()))


@pytest.mark.parametrize("kernel,d,extra", [("avgpool", 8, dict(r=2)), ("upsample", 8, dict(r=4)), ("color_A", 4, dict(w3=None)),
                                            ("color_pinv", 4, dict(w3=None)), ("inpaint_A", 4, dict(mask="part")),
                                            ("inpaint_pinv", 4, dict(mask="part"))])
def test_twin_agrees_with_the_oracle_operator(kernel, d, extra):
    from oracle import operators as O
    B = 2
    p = dict(B=B, HW=d * d, **extra)
    if kernel in ("avgpool", "upsample"):
        p = dict(BC=3 * B, H=d, W=d, **extra)
    case = SM.Case("o_" + kernel, kernel, "oracle", p)
    t = SM.make_inputs(case)
    ref = SM.twin(case, t)
    if kernel in ("avgpool", "upsample"):
        op = O.SuperResolution(3, d, extra["r"])
    elif kernel.startswith("color"):
        op = O.Colorization(d)
    else:
        op = O.Inpainting(3, d, O.Inpainting.missing_from_mask(torch.from_numpy(t["mask"].reshape(d, d).astype(np.int64))))
    if kernel in ("avgpool", "color_A", "inpaint_A"):
        key, want = "y", op.A(torch.from_numpy(t["x"]).double().reshape(B, -1))
    else:
        key, want = "x", op.A_pinv(torch.from_numpy(t["x" if kernel == "upsample" else "y"]).double().reshape(B, -1))
    err = np.abs(ref[key].v.reshape(B, -1) - want.numpy())
    assert (err <= ref[key].bar().reshape(B, -1) + 0.0).all(), float(err.max())


# ----------------------------------------------------------------------------- the comparison has teeth
@pytest.mark.parametrize("name", CASE_IDS)
def test_planted_faults_change_the_model(name):
    case, t = SM.BY_NAME[name], _inputs(name)
    good = SM.model(case, t)
    for fault in SM.faults_of(case):
        assert fault in SM.FAULTS
        bad = SM.model(case, t, fault)
        changed = any(not np.array_equal(good[k], bad[k], equal_nan=True) for k in good)
        assert changed, f"{name}: planted fault {fault!r} leaves every output bit unchanged"


def test_every_fault_is_caught_where_it_applies():
    """Each planted fault is carried by cases of every kernel it can occur in."""
    by_fault = {f: {c.kernel for c in SM.CASES if f in SM.faults_of(c)} for f in SM.FAULTS}
    assert by_fault["fma"] >= set(STEP_KERNELS) | {"color_A", "axpby", "axpby_strided", "renoise", "mask_mix", "site_spectral",
                                                   "spectral_mix"}
    assert by_fault["colmajor"] == {"step_sr4", "avgpool"}
    assert by_fault["swap_hw"] >= {"step_sr4", "avgpool", "upsample", "site_spectral", "patchify"}
    assert by_fault["shift"] >= {"step_sr4", "step_color", "step_inpaint", "step_inpaint_pi", "upsample", "patchify",
                                 "gather_scale", "site_matmul", "site_spectral", "mask_mix", "mul_planes"}
    assert by_fault["et_stride"] == set(STEP_KERNELS) | {"axpby_strided"}
    assert by_fault["key_row"] == set(SM.NOISY)
    assert by_fault["lambda_operand"] == set(STEP_KERNELS) - {"step_x0"}
    assert by_fault["swap_kept"] == {"step_inpaint", "step_inpaint_pi", "inpaint_A", "inpaint_pinv", "inpaint_A_pi",
                                     "inpaint_pinv_pi"}
    assert by_fault["tie_lt"] == by_fault["tie_gt"] == {"spectral_mix"}
    # every case that is not a plain copy / fill / draw catches something
    for c in SM.CASES:
        if c.kernel not in ("fill", "finalize_psnr", "randn_philox") and not (c.kernel == "patchify" and c.p["D"] == c.p["ps"]) \
                and not (c.kernel == "site_matmul" and c.p["n"] == 1) and not (c.kernel == "avgpool" and c.p["r"] == 1):
            assert SM.faults_of(c) or c.kernel in ("axpby", "mask_mix", "mul_planes", "spectral_mix", "site_spectral"), c.name


# ----------------------------------------------------------------------------- second-trip sizes
PER_IMAGE = ("step_x0", "step_combine", "step_denoise", "step_color", "step_inpaint", "randn_philox", "upsample", "gather_scale")


@pytest.mark.parametrize("kernel", sorted(SM.SECOND_TRIP))
def test_second_trip_sizes(kernel):
    """Work items in (8192 * 256, 1.01 * 8192 * 256]: every workgroup the cap allows is launched and the first threads take
    a second trip `i += gridDim.x * 256`; per-image kernels start that trip in another image than the first."""
    p = SM.SECOND_TRIP[kernel]
    items, per_image = SM.work_items(kernel, p)
    full = SM.GRID_CAP * SM.BLOCK
    assert full + 1 <= items <= int(1.01 * full), (items, full)
    assert SM.grid_of(items) == SM.GRID_CAP and SM.second_trip_start(items) == full
    if kernel in PER_IMAGE:
        assert per_image is not None and full // per_image != 0 and full // per_image < p.get("B", p.get("BC"))
    if kernel == "step_sr4":
        assert p["H"] % 4 == 0 and p["W"] % 4 == 0 and 5 * 4 * 3 * p["H"] * p["W"] < 0.75 * 2 ** 30
    for c in SM.CASES:                   # and no case of the table reaches a second trip by accident
        if c.kernel == kernel:
            assert SM.work_items(kernel, c.p)[0] <= full


def test_second_trip_covers_every_shape_class():
    assert set(SM.SECOND_TRIP) >= {"step_x0", "step_combine", "step_denoise", "step_color", "step_inpaint", "renoise",
                                   "randn_philox", "patchify", "step_sr4", "gather_scale"}
    assert {"upsample", "site_spectral"} & set(SM.SECOND_TRIP)
