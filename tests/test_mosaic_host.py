"""Demosaicing on the host: the colour filter array tables of svd_operators.Mosaic against an independent numpy
construction, the `--deg demosaic*` names of build_operator, the reference's Inpainting on CFA indices
(tests/golden/mosaic.npz, written by tests/golden/make_golden_mosaic.py) against the oracle restatement, and the
argument validation of the `*_mosaic_*` entry points through the built library.  No GPU.

The helpers below are shared with tests/golden/make_golden_mosaic.py and tests/test_gpu_mosaic.py."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

# the five named arrays, written out here a second time on purpose: rows of R / G / B letters
CFA_LETTERS = {
    "rggb": ["RG", "GB"],
    "bggr": ["BG", "GR"],
    "grbg": ["GR", "BG"],
    "gbrg": ["GB", "RG"],
    "xtrans": ["GBGGRG", "RGRBGB", "GBGGRG", "GRGGBG", "BGBRGR", "GRGGBG"],
}
GOLDEN_D, GOLDEN_B, GOLDEN_PATTERNS = 16, 2, ("rggb", "xtrans")
SIGMA_Y, ETA, ETA_REG = 0.4, 0.85, 0.3
# (a, sigma_t), one pair on each side of the threshold sigma_t = a * sigma_y.
#   (0.9, 0.05): 0.05 < 0.36, lambda < 1, (d1, d2) = (sigma_t eta, 0) on the sampled entries.
#   (1e-4, 0.5): 0.5 > 4e-5, lambda = 1, d1 = sqrt(sigma_t^2 - a^2 sigma_y^2).  The reference takes that root in fp32 tensor
#     arithmetic, the oracle in float64 and rounds once, so the two agree to the last bit only where the root is the same
#     number both ways (at the first pair tried, (0.5, 0.8), they are 0.77459663 and 0.7745967: one fp32 ulp on every sampled
#     entry, rel-L2 4.7e-8).  Here it is by the formats alone: a^2 sigma_y^2 = 1.6e-9 is below half the fp32 spacing under
#     0.25 (2^-26 = 1.5e-8), so the reference's difference rounds to 0.25 and its root is 0.5; in float64 the root is
#     0.5 - 1.6e-9, within half the fp32 spacing under 0.5 (2^-25 = 3.0e-8), and rounds to 0.5 as well.  The null space keeps
#     (sigma_t eta, sigma_t sqrt(1 - eta^2)) = (0.425, 0.263): the two sets of entries are still told apart.
PLUS_CASES = ((0.9, 0.05), (1e-4, 0.5))


def numpy_cfa(name):
    """[ph, pw] channel codes (0 = R, 1 = G, 2 = B) of a named array, from the letters above."""
    return np.array([["RGB".index(ch) for ch in row] for row in CFA_LETTERS[name]], dtype=np.int64)


def numpy_tables(pattern, d):
    """(code [d*d], sampled [3][d*d] bool, missing HWC-interleaved indices ascending) by plain loops."""
    ph, pw = pattern.shape
    code = np.zeros(d * d, dtype=np.int64)
    for r in range(d):
        for c in range(d):
            code[r * d + c] = pattern[r % ph][c % pw]
    sampled = np.zeros((3, d * d), dtype=bool)
    missing = []
    for p in range(d * d):
        for ch in range(3):
            if ch == code[p]:
                sampled[ch, p] = True
            else:
                missing.append(3 * p + ch)
    return code, sampled, np.array(missing, dtype=np.int64)


def golden_inputs(d=GOLDEN_D, B=GOLDEN_B):
    """Seeded inputs of the golden file and of the GPU tests: an image-sized x, v, eps and a measurement-sized y.  The
    values are fp16 numbers (held in fp32), so the permutations stored in the golden file compress."""
    g = torch.Generator().manual_seed(4321 + d)
    draw = lambda n: torch.randn(B, n, generator=g).half().float()      # noqa: E731
    return dict(x=draw(3 * d * d).reshape(B, 3, d, d), v=draw(3 * d * d), eps=draw(3 * d * d), y=draw(d * d))


def _config(d):
    return argparse.Namespace(data=argparse.Namespace(channels=3, image_size=d))


# ---------------------------------------------------------------------------------------------- 1. tables and names
@pytest.mark.parametrize("name", sorted(CFA_LETTERS))
@pytest.mark.parametrize("d", [8, 16])
def test_tables_match_an_independent_construction(name, d):
    from ddnm_amd.functions import svd_operators as E
    op = E.Mosaic(3, d, name, "cpu")
    pattern = numpy_cfa(name)
    code, sampled, missing = numpy_tables(pattern, d)
    assert np.array_equal(op.pattern, pattern) and op.pattern.dtype == np.uint8
    assert np.array_equal(op.missing_indices.numpy(), missing) and len(missing) == 2 * d * d
    assert np.array_equal(op.sampled_mask.numpy(), sampled.astype(np.float32))
    assert op.measurement_size() == d * d and op.measurement_image_shape() == (1, d, d)
    assert op.singulars().shape == (d * d,) and bool((op.singulars() == 1).all())
    assert [int(v) for v in op._cfa[0]] == [int(v) for v in pattern.reshape(-1)] and op._cfa[1:] == pattern.shape


def test_xtrans_samples_20_green_8_red_8_blue_per_period():
    from ddnm_amd.functions import svd_operators as E
    p = np.asarray(E.CFA_PATTERNS["xtrans"])
    assert p.shape == (6, 6) and [int((p == c).sum()) for c in range(3)] == [8, 20, 8]
    for name in ("rggb", "bggr", "grbg", "gbrg"):
        q = np.asarray(E.CFA_PATTERNS[name])
        assert q.shape == (2, 2) and [int((q == c).sum()) for c in range(3)] == [1, 2, 1]
    assert sorted(E.CFA_PATTERNS) == sorted(CFA_LETTERS)


def test_constructor_refusals():
    from ddnm_amd.functions import svd_operators as E
    with pytest.raises(ValueError, match="channels"):
        E.Mosaic(1, 16, "rggb", "cpu")
    with pytest.raises(ValueError, match="multiple of 4"):
        E.Mosaic(3, 18, "rggb", "cpu")
    with pytest.raises(ValueError, match="codes"):
        E.Mosaic(3, 16, [[0, 3], [1, 2]], "cpu")
    with pytest.raises(ValueError, match="codes"):
        E.Mosaic(3, 16, [[0, -1]], "cpu")
    with pytest.raises(ValueError, match="period"):
        E.Mosaic(3, 16, np.zeros((9, 2), np.int64), "cpu")
    with pytest.raises(ValueError, match="2-D"):
        E.Mosaic(3, 16, [0, 1, 2], "cpu")
    with pytest.raises(ValueError, match="rggb"):
        E.Mosaic(3, 16, "rgbg", "cpu")
    # a pattern that never samples a channel is allowed: blue then lies in the null space
    op = E.Mosaic(3, 16, [[0, 1]], "cpu")
    assert float(op.sampled_mask[2].sum()) == 0 and op.missing_indices.numel() == 2 * 256
    # whole-pixel Inpainting keeps refusing per-channel indices: that is Mosaic's ground
    with pytest.raises(NotImplementedError):
        E.Inpainting(3, 16, op.missing_indices, "cpu")


def test_build_operator_maps_every_name(tmp_path, monkeypatch):
    from ddnm_amd.functions import svd_operators as E
    for name in CFA_LETTERS:
        op = E.build_operator("demosaic_" + name, 0.0, _config(16), "cpu")
        assert isinstance(op, E.Mosaic) and np.array_equal(op.pattern, numpy_cfa(name))
    assert E.demosaic_choices() == ["demosaic", "demosaic_rggb", "demosaic_bggr", "demosaic_grbg", "demosaic_gbrg",
                                    "demosaic_xtrans"]
    for bad in ("demosaic_rgbg", "demosaic_", "demosaicx"):
        with pytest.raises(ValueError) as e:
            E.build_operator(bad, 0.0, _config(16), "cpu")
        assert all(choice in str(e.value) for choice in E.demosaic_choices()), str(e.value)
    # --deg demosaic reads exp/cfa/pattern.npy below the working directory
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="demosaic_xtrans"):                # no file
        E.build_operator("demosaic", 0.0, _config(16), "cpu")
    os.makedirs(tmp_path / "exp" / "cfa")
    own = np.array([[0, 1, 1], [1, 2, 1]])
    np.save(tmp_path / "exp" / "cfa" / "pattern.npy", own)
    op = E.build_operator("demosaic", 0.0, _config(16), "cpu")
    assert np.array_equal(op.pattern, own) and np.array_equal(op.missing_indices.numpy(), numpy_tables(own, 16)[2])
    for bad in (np.array([0, 1, 2]), np.array([[0.0, 1.0]]), np.array([[0, 4]]), np.zeros((2, 9), np.int64)):
        np.save(tmp_path / "exp" / "cfa" / "pattern.npy", bad)
        with pytest.raises(ValueError, match="demosaic_rggb"):
            E.build_operator("demosaic", 0.0, _config(16), "cpu")


def test_a_colour_picture_is_no_one_channel_measurement(tmp_path):
    """A raw frame is a grey S x S picture: that loads to data_transform of its pixels exactly; an RGB picture or one of
    another size is refused when the folder is bound."""
    from PIL import Image
    from ddnm_amd.functions import svd_operators as E
    from ddnm_amd.guided_diffusion import diffusion as D
    cfg = argparse.Namespace(data=argparse.Namespace(channels=3, image_size=16, rescaled=True))
    op = E.Mosaic(3, 16, "rggb", "cpu")
    rng = np.random.default_rng(8)
    grey = rng.integers(0, 256, (16, 16), dtype=np.uint8)
    good = tmp_path / "good"
    good.mkdir()
    Image.fromarray(grey).save(good / "raw_0.png")
    np.save(good / "raw_1.npy", np.zeros(256, np.float32))
    ds = D.MeasurementFolder(str(good)).bind(op, cfg)
    x, picture = ds[0]
    assert picture and x.shape == (1, 16, 16)
    assert torch.equal(x, D.data_transform(cfg, torch.from_numpy(grey.copy()).float().div(255.0))[None])
    assert ds[1][0].shape == (256,) and not ds[1][1]
    for name, arr, words in (("rgb", rng.integers(0, 256, (16, 16, 3), dtype=np.uint8), ("3 channels", "has 1")),
                             ("wide", rng.integers(0, 256, (16, 20), dtype=np.uint8), ("20 x 16", "16 x 16"))):
        folder = tmp_path / name
        folder.mkdir()
        Image.fromarray(arr).save(folder / "raw_0.png")
        with pytest.raises(ValueError) as e:
            D.MeasurementFolder(str(folder)).bind(op, cfg)
        assert "raw_0.png" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    short = tmp_path / "short"
    short.mkdir()
    np.save(short / "raw_0.npy", np.zeros(255, np.float32))
    with pytest.raises(ValueError, match="255"):
        D.MeasurementFolder(str(short)).bind(op, cfg)


# ---------------------------------------------------------------------------------------------- 2. golden
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "mosaic.npz"))


def test_golden_file_is_small(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "mosaic.npz")) < 100 * 1024


@pytest.mark.parametrize("name", GOLDEN_PATTERNS)
def test_oracle_inpainting_reproduces_the_reference_on_cfa_indices(golden, name):
    """The reference's Inpainting built with the CFA's missing entries (the golden file) == oracle.operators.Inpainting
    built with the same indices: A, A_pinv, Lambda and Lambda_noise exactly, and A is `x[b, cfa(p), p]` in pixel order."""
    from oracle import operators as O
    d, B = GOLDEN_D, GOLDEN_B
    code, sampled, missing = numpy_tables(numpy_cfa(name), d)
    assert np.array_equal(golden[f"{name}_missing"], missing)
    orc = O.Inpainting(3, d, torch.from_numpy(missing))
    inp = golden_inputs()
    y = orc.A(inp["x"])
    assert torch.equal(y, torch.from_numpy(golden[f"{name}_A"]))
    flat = inp["x"].reshape(B, 3, d * d)
    assert torch.equal(y, flat[:, torch.from_numpy(code), torch.arange(d * d)])
    xp = orc.A_pinv(inp["y"])
    assert torch.equal(xp, torch.from_numpy(golden[f"{name}_A_pinv"]))
    want = torch.where(torch.from_numpy(sampled)[None], inp["y"][:, None, :].expand(B, 3, d * d), torch.zeros(()))
    assert torch.equal(xp.reshape(B, 3, d * d), want)
    assert np.array_equal(golden[f"{name}_singulars"], np.ones(d * d, np.float32))
    for k, (a, sigma_t) in enumerate(PLUS_CASES):
        assert (sigma_t < a * SIGMA_Y) == (k == 0)
        assert torch.equal(orc.Lambda(inp["v"], a, SIGMA_Y, sigma_t, ETA), torch.from_numpy(golden[f"{name}_Lambda_{k}"]))
        assert torch.equal(orc.Lambda_noise(inp["v"], a, SIGMA_Y, sigma_t, ETA, inp["eps"]),
                           torch.from_numpy(golden[f"{name}_Lambda_noise_{k}"]))


# ---------------------------------------------------------------------------------------------- 3. argument validation
def check_mosaic_validation(lib, ptr):
    """Every refusal of the `*_mosaic_*` entry points with `ptr` standing for each tensor (never dereferenced: all of it
    happens before a launch).  DDNM_E_BADARG = -1 comes before DDNM_E_SHAPE = -2."""
    from ddnm_amd._lib import StepScalars
    s = StepScalars()
    s.rng_on = 1
    sp = ctypes.byref(s)
    pat = (ctypes.c_uint8 * 4)(0, 1, 1, 2)
    bad = (ctypes.c_uint8 * 4)(0, 1, 3, 2)
    long_ = (ctypes.c_uint8 * 18)(*([1] * 18))
    plus = (0.1, 0.2, 0.3, 0.4, 0.5)

    def op_A(x=ptr, y=ptr, B=2, H=16, W=16, p=pat, ph=2, pw=2):
        return lib.ddnm_op_mosaic_A_f32(x, y, B, H, W, p, ph, pw, None)

    def op_pinv(y=ptr, x=ptr, B=2, H=16, W=16, p=pat, ph=2, pw=2):
        return lib.ddnm_op_mosaic_pinv_f32(y, x, B, H, W, p, ph, pw, None)

    def step(fn=lib.ddnm_step_mosaic_f32, xt=ptr, et=ptr, es=768, nz=None, y=ptr, x0=ptr, xn=ptr, B=2, H=16, W=16, p=pat,
             ph=2, pw=2, sc=sp):
        extra = plus if "plus" in fn.__name__ else ()
        return fn(xt, et, es, nz, y, x0, xn, B, H, W, p, ph, pw, *extra, sc, None)

    steps = (lib.ddnm_step_mosaic_f32, lib.ddnm_step_plus_mosaic_f32)
    keyed = (lib.ddnm_step_mosaic_keyed_f32, lib.ddnm_step_plus_mosaic_keyed_f32)
    # null pointers, batch, noise source: DDNM_E_BADARG
    assert op_A(y=None) == -1 and op_A(x=None) == -1 and op_A(p=None) == -1 and op_A(B=0) == -1 and op_A(H=0) == -1
    assert op_pinv(y=None) == -1 and op_pinv(x=None) == -1 and op_pinv(p=None) == -1 and op_pinv(B=-1) == -1
    for fn in steps + keyed:
        nz = ptr if fn in keyed else None           # (ptr is 16-byte aligned: a valid key table address)
        assert step(fn, nz=nz, y=None) == -1, fn.__name__
        assert step(fn, nz=nz, xt=None) == -1 and step(fn, nz=nz, et=None) == -1 and step(fn, nz=nz, xn=None) == -1
        assert step(fn, nz=nz, sc=None) == -1 and step(fn, nz=nz, p=None) == -1 and step(fn, nz=nz, B=0) == -1
        # ... and it wins over a bad shape
        assert step(fn, nz=nz, y=None, W=6) == -1 and step(fn, nz=nz, B=0, pw=9) == -1
    for fn in keyed:
        assert step(fn, nz=None) == -1, fn.__name__                       # a null key table
        assert step(fn, nz=ptr + 4) == -1, fn.__name__                    # ... or a misaligned one
    off = StepScalars()                                                    # rng_on = 0 and no noise tensor: no source
    for fn in steps:
        assert step(fn, sc=ctypes.byref(off)) == -1, fn.__name__
    assert step(lib.ddnm_step_plus_mosaic_f32, x0=None) == -1             # the noisy step always writes x0
    # sizes and pattern: DDNM_E_SHAPE
    for call in (op_A, op_pinv):
        assert call(W=6) == -2 and call(H=6) == -2 and call(pw=9) == -2 and call(ph=0) == -2 and call(p=bad) == -2
        assert call(p=long_, ph=2, pw=9) == -2 and call(p=long_, ph=9, pw=2) == -2
    for fn in steps + keyed:
        nz = ptr if fn in keyed else None
        assert step(fn, nz=nz, W=6) == -2 and step(fn, nz=nz, H=18) == -2, fn.__name__
        assert step(fn, nz=nz, es=6) == -2 and step(fn, nz=nz, es=770) == -2, fn.__name__
        assert step(fn, nz=nz, pw=9) == -2 and step(fn, nz=nz, ph=9) == -2 and step(fn, nz=nz, pw=0) == -2, fn.__name__
        assert step(fn, nz=nz, p=bad) == -2, fn.__name__                  # a code of 3


def test_argument_validation_without_gpu():
    """The pattern of tests/test_cabi.py::test_argument_validation_without_gpu: the entry points refuse bad arguments
    before touching the device, so the built library answers on a host without one."""
    from ddnm_amd import _lib, build
    build.build()
    lib = _lib.lib()
    assert lib.ddnm_version() == 7
    check_mosaic_validation(lib, 4096)


def test_plus_step_hook_marshals_its_arguments():
    """Host-only dry run (tools/dry_run.py): Mosaic's A, A_pinv, ddnm_step and the DDNM+ hook reach their entry points
    with arguments of the declared types, for a tensor, an in-kernel and a keyed noise source."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import dry_run
    finally:
        sys.path.pop(0)
    from ddnm_amd import _lib, ops
    from ddnm_amd.functions import svd_operators as E
    saved = (_lib._lib, ops._stream, ops._f32c, ops._f16c)
    try:
        dry = dry_run.install()
        d, B = 16, 2
        op = E.Mosaic(3, d, "xtrans", "cpu")
        x = torch.zeros(B, 3, d, d)
        y = op.A(x)
        assert y.shape == (B, d * d) and op.A_pinv(y).shape == (B, 3 * d * d)
        et6 = torch.zeros(B, 6, d, d)
        s = ops.step_scalars(torch.tensor(0.5), torch.tensor(0.6), 0.85)
        out = torch.zeros_like(x), torch.zeros_like(x)
        op.ddnm_step(x, et6[:, :3], torch.zeros_like(x), y, s, *out)
        op.ddnm_step(x, et6[:, :3], None, y, ops.PhiloxNoise(5).stamp(s, 1), *out)
        with pytest.raises(RuntimeError, match="begin_plus_run"):
            op.ddnm_plus_step(x, et6[:, :3], None, s, 0.2, 0.5, 0.85, *out)
        op.begin_plus_run(y)
        op.ddnm_plus_step(x, et6[:, :3], torch.zeros_like(x), s, 0.2, 0.5, 0.85, *out)
        with pytest.raises(ValueError):
            op.ddnm_step(x, et6[:, :3], None, y[:, :-4], s, *out)
        assert dry.calls == {"ddnm_op_mosaic_A_f32": 1, "ddnm_op_mosaic_pinv_f32": 1, "ddnm_step_mosaic_f32": 2,
                             "ddnm_step_plus_mosaic_f32": 1}
    finally:
        _lib._lib, ops._stream, ops._f32c, ops._f16c = saved
