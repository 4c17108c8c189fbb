"""SSIM without a GPU: the float64 numpy model the GPU tests compare the kernel with (direct separable sums, float64
weights), its self-checks, the C ABI of ddnm_ssim_f32 / ddnm_ssim_workspace_elems (exports, prototypes, argument
validation before any launch), the runner's DDNM_METRICS switch and the pairing of the folder evaluator."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1, C2 = 0.01 ** 2, 0.03 ** 2
E_BADARG, E_SHAPE = -1, -2            # DDNM_E_BADARG, DDNM_E_SHAPE (include/ddnm_hip.h)


# ------------------------------------------------------------------------------------------------ float64 model
def window():
    g = np.exp(-(np.arange(11, dtype=np.float64) - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    return g / g.sum()


def _filter_valid(a):
    """w * a over the valid positions of the last two axes, w = g (x) g: eleven shifted slices per axis, added in order."""
    g = window()
    H, W = a.shape[-2:]
    h = sum(g[k] * a[..., :, k:k + W - 10] for k in range(11))
    return sum(g[k] * h[..., k:k + H - 10, :] for k in range(11))


def ssim_map(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mx, my = _filter_valid(x), _filter_valid(y)
    vx, vy, vxy = _filter_valid(x * x) - mx * mx, _filter_valid(y * y) - my * my, _filter_valid(x * y) - mx * my
    return ((2 * (mx * my) + C1) * (2 * vxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def ssim_f64(x, y):
    """Per-image SSIM of [B, C, H, W] images on the [0, 1] scale: float64 [B]."""
    m = ssim_map(x, y)
    return m.reshape(m.shape[0], -1).mean(axis=1)


def test_window_is_normalised_and_symmetric():
    g = window()
    assert abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(g[4] / g[5] - np.exp(-1 / 4.5)) < 1e-15


def test_model_identity_and_symmetry():
    rng = np.random.default_rng(0)
    x, y = rng.random((2, 3, 20, 27)), rng.random((2, 3, 20, 27))
    assert np.array_equal(ssim_f64(x, x), np.ones(2))
    assert np.array_equal(ssim_f64(x, y), ssim_f64(y, x))
    assert np.all(ssim_f64(x, y) < 0.2)                      # independent noise


def test_model_constants_follow_the_closed_form():
    a, b = np.full((1, 3, 16, 19), 0.3), np.full((1, 3, 16, 19), 0.7)
    want = (2 * 0.3 * 0.7 + C1) / (0.3 ** 2 + 0.7 ** 2 + C1)
    # the variances are rounding residue (~1e-16) against C2 = 9e-4; 0.72418551 is the figure of the fp32 images 0.3f, 0.7f
    assert abs(ssim_f64(a, b)[0] - want) < 1e-11 and abs(want - 0.72418551) < 1e-7
    a32, b32 = np.full((1, 3, 16, 19), np.float32(0.3)), np.full((1, 3, 16, 19), np.float32(0.7))
    assert abs(ssim_f64(a32, b32)[0] - 0.72418551) < 1e-8
    black, white = np.zeros((1, 1, 12, 12)), np.ones((1, 1, 12, 12))
    assert abs(ssim_f64(black, white)[0] - C1 / (1 + C1)) < 1e-11


def test_model_11x11_has_one_valid_position():
    rng = np.random.default_rng(1)
    x, y = rng.random((1, 1, 11, 11)), rng.random((1, 1, 11, 11))
    assert ssim_map(x, y).shape == (1, 1, 1, 1)
    w = np.outer(window(), window())
    mx, my = (w * x[0, 0]).sum(), (w * y[0, 0]).sum()
    vx, vy = (w * x[0, 0] ** 2).sum() - mx ** 2, (w * y[0, 0] ** 2).sum() - my ** 2
    vxy = (w * x[0, 0] * y[0, 0]).sum() - mx * my
    want = (2 * mx * my + C1) * (2 * vxy + C2) / ((mx ** 2 + my ** 2 + C1) * (vx + vy + C2))
    assert abs(ssim_f64(x, y)[0] - want) < 1e-13


# ------------------------------------------------------------------------------------------------ C ABI
SYMBOLS = {"ddnm_ssim_f32": ("int", ctypes.c_int32), "ddnm_ssim_workspace_elems": ("int64_t", ctypes.c_int64)}


@pytest.fixture(scope="module")
def lib():
    from ddnm_amd import _lib, build
    build.build()
    return _lib.lib()


def _header_args(name, ret):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddnm_hip.h")).read(), flags=re.S)
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{ret} {name}(...) is not declared in include/ddnm_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype_of(decl):
    if "*" in decl:
        return ctypes.c_void_p
    return {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}[decl.split()[0]]


def test_library_exports_the_ssim_entry_points(lib):
    from ddnm_amd import _lib
    for name, (ret, restype) in SYMBOLS.items():
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES
        got_res, argtypes = _lib.PROTOTYPES[name]
        assert got_res is restype
        assert list(argtypes) == [_ctype_of(a) for a in _header_args(name, ret)], name
    assert [a.split()[-1].lstrip("*") for a in _header_args("ddnm_ssim_f32", "int")] == [
        "x", "y", "ssim", "work", "work_elems", "B", "C", "H", "W", "transform", "stream"]
    assert lib.ddnm_version() == _lib.ABI_VERSION == 7
    assert "metrics.hip" in __import__("ddnm_amd.build", fromlist=["SOURCES"]).SOURCES


def test_ssim_workspace_query(lib):
    q = lib.ddnm_ssim_workspace_elems
    assert q(1, 1, 11, 11) == 1 and q(1, 3, 26, 42) == 3             # one tile: 32 x 16 valid positions
    assert q(1, 1, 27, 42) == 2 and q(1, 1, 26, 43) == 2             # a one-pixel second tile in either axis
    assert q(8, 3, 256, 256) == 8 * 3 * 8 * 16
    assert q(2, 1, 40, 75) == 2 * 3 * 2
    assert q(0, 1, 11, 11) == E_BADARG and q(1, -1, 11, 11) == E_BADARG
    assert q(1, 1, 10, 64) == E_SHAPE and q(1, 1, 64, 10) == E_SHAPE and q(1, 1, 0, 0) == E_SHAPE
    assert q(1 << 20, 1 << 10, 64, 64) == E_SHAPE                    # more tiles than one grid holds


def test_ssim_argument_validation_without_gpu(lib):
    """Every refusal happens before any launch: the dummy pointers are never dereferenced."""
    p = [4096 * (i + 1) for i in range(4)]
    ok = dict(x=p[0], y=p[1], ssim=p[2], work=p[3], n=2 * 3 * 2 * 4, B=2, C=3, H=64, W=64)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ddnm_ssim_f32(a["x"], a["y"], a["ssim"], a["work"], a["n"], a["B"], a["C"], a["H"], a["W"], 1, None)

    for key in ("x", "y", "ssim", "work"):
        assert call(**{key: None}) == E_BADARG, key
    for key in ("B", "C"):
        assert call(**{key: 0}) == E_BADARG and call(**{key: -3}) == E_BADARG, key
    assert call(H=10) == E_SHAPE and call(W=10) == E_SHAPE and call(H=-1) == E_SHAPE
    assert call(n=ok["n"] - 1) == E_SHAPE and call(n=0) == E_SHAPE
    assert call(H=10, x=None) == E_BADARG                            # the null pointer is reported first


# ------------------------------------------------------------------------------------------------ runner switch
def test_metrics_switch_parsing(monkeypatch):
    from ddnm_amd.guided_diffusion import diffusion as D
    monkeypatch.delenv("DDNM_METRICS", raising=False)
    assert D.extra_metrics() == () and D.extra_metrics(8) == ()
    monkeypatch.setenv("DDNM_METRICS", "")
    assert D.extra_metrics() == ()
    monkeypatch.setenv("DDNM_METRICS", "ssim")
    assert D.extra_metrics() == ("ssim",) and D.extra_metrics(11) == ("ssim",) and D.extra_metrics(256) == ("ssim",)
    with pytest.raises(ValueError, match="11"):
        D.extra_metrics(10)
    for bad in ("lpips", "ssim,fid", "SSIM"):
        monkeypatch.setenv("DDNM_METRICS", bad)
        with pytest.raises(ValueError, match="accepted values: ssim"):
            D.extra_metrics()


def test_metric_log_without_the_switch_prints_the_psnr_lines_only(monkeypatch, capsys):
    """No GPU call and no SSIM line when the switch is unset; the totals are the running sums."""
    import torch
    from ddnm_amd.guided_diffusion import diffusion as D
    monkeypatch.delenv("DDNM_METRICS", raising=False)
    log = D.MetricLog(8)
    x = torch.zeros(2, 3, 8, 8)
    log.add(x, x, torch.tensor([20.0, 30.0], dtype=torch.float64), 5)
    log.add(x[:1], x[:1], torch.tensor([10.0], dtype=torch.float64), 7)
    res = log.total(0, "cpu", reduce=False)
    assert capsys.readouterr().out == "PSNR: 25.00\nPSNR: 20.00\nTotal Average PSNR: 20.00\nNumber of samples: 3\n"
    assert res["psnr"] == 20.0 and res["ssim"] is None and res["ssim_per_image"] is None
    assert res["index"] is None and res["psnr_per_image"] is None and res["n"] == 3      # per-image lists: with the switch


def test_main_has_no_metrics_flag():
    import main
    assert not any("metric" in n for names, _ in main.FLAGS for n in names)


# ------------------------------------------------------------------------------------------------ evaluator pairing
def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").close()


def test_evaluator_pairs_by_index_and_lists_missing(tmp_path):
    from ddnm_amd.evaluate import pair_files
    root = str(tmp_path / "run")
    for i in (0, 1, 2, 10):
        _touch(os.path.join(root, "Apy", f"orig_{i}.png"))
    for i in (0, 2, 10):
        _touch(os.path.join(root, "Apy", f"Apy_{i}.png"))
    for i in (0, 1, 10, 11):
        _touch(os.path.join(root, f"{i}_0.png"))
    _touch(os.path.join(root, "-1_0.png"))                   # the simplified runner's first name: no index
    _touch(os.path.join(root, "notes.txt"))
    pairs, missing = pair_files(root)
    assert [(i, os.path.relpath(a, root), os.path.relpath(b, root)) for i, a, b in pairs] == [
        (0, "Apy/orig_0.png", "0_0.png"), (1, "Apy/orig_1.png", "1_0.png"), (10, "Apy/orig_10.png", "10_0.png")]
    assert missing == {"orig": [11], "restored": [2]}
    pairs, missing = pair_files(root, "Apy")
    assert [(i, os.path.basename(b)) for i, _, b in pairs] == [(0, "Apy_0.png"), (2, "Apy_2.png"), (10, "Apy_10.png")]
    assert missing == {"orig": [], "Apy": [1]}
    with pytest.raises(ValueError, match="accepted values"):
        pair_files(root, "nothing")


def test_evaluator_refuses_an_empty_pairing(tmp_path):
    from ddnm_amd.evaluate import pair_files
    with pytest.raises(FileNotFoundError):
        pair_files(str(tmp_path))
    _touch(str(tmp_path / "Apy" / "orig_3.png"))
    _touch(str(tmp_path / "4_0.png"))
    with pytest.raises(FileNotFoundError):
        pair_files(str(tmp_path))


def test_evaluator_loads_eight_bit_images_as_u_over_255(tmp_path):
    from PIL import Image
    from ddnm_amd.evaluate import load_image
    u = np.random.default_rng(2).integers(0, 256, (13, 17, 3), dtype=np.uint8)
    Image.fromarray(u).save(tmp_path / "a.png")
    v = load_image(str(tmp_path / "a.png"))
    assert v.dtype == np.float32 and v.shape == (3, 13, 17) and v.flags["C_CONTIGUOUS"]
    assert np.array_equal(v, (u.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
