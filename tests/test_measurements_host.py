"""Measurements in and out, on the host: the MeasurementFolder dataset of `--path_y measurements:DIR` (ordering, duplicate
stems, the checks of every file against the operator, measurements.json, pictures, bank padding), what a measurement of
every operator class looks like (measurement_size / measurement_image_shape), the DDNM_METRICS=cons and DDNM_SAVE_Y
switches, the refusals of a run over given measurements, the new C symbols and the argument checks of ops.consistency.
No GPU call."""
import argparse
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 32      # image size of the host cases (a multiple of the CS patch)


def _config(size=S, channels=3):
    return argparse.Namespace(data=argparse.Namespace(image_size=size, channels=channels, rescaled=True),
                              sampling=argparse.Namespace(batch_size=1))


def _args(**kw):
    base = dict(path_y="measurements:m", exp="exp", add_noise=False, deg="sr_averagepooling", deg_scale=4.0, sigma_y=0.0,
                seed=1234, subset_start=-1, subset_end=-1, simplified=False, image_folder="out")
    base.update(kw)
    return argparse.Namespace(**base)


def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def _engine():
    from ddnm_amd.functions import svd_operators as E
    return E


# ------------------------------------------------------------------------------------------------ the dataset
def test_entries_are_ordered_by_the_last_integer_of_the_stem(tmp_path):
    from ddnm_amd.guided_diffusion import diffusion as D
    E = _engine()
    op = E.Colorization(S, "cpu")
    rng = np.random.default_rng(0)
    for name in ("y_10.npy", "y_2.npy", "y_0.npy", "run3_y_1.npy"):
        np.save(tmp_path / name, rng.standard_normal(S * S).astype(np.float32))
    _png(tmp_path / "y_5.png", rng.integers(0, 256, (S, S), dtype=np.uint8))
    (tmp_path / "measurements.json").write_text("{}")
    (tmp_path / "notes.txt").write_text("not an entry")
    np.save(tmp_path / "zz.npy", np.zeros(S * S, np.float32))           # no digit: after the numbered ones
    ds = D.MeasurementFolder(str(tmp_path)).bind(op, _config())
    assert ds.names == ["y_0.npy", "run3_y_1.npy", "y_2.npy", "y_5.png", "y_10.npy", "zz.npy"]
    assert len(ds) == 6
    kinds = [ds[p][1] for p in range(6)]
    assert kinds == [False, False, False, True, False, False]
    assert ds[0][0].shape == (S * S,) and ds[3][0].shape == (1, S, S) and ds[0][0].dtype == torch.float32
    assert torch.equal(ds[4][0], torch.from_numpy(np.load(tmp_path / "y_10.npy")))
    # the same number: by name
    np.save(tmp_path / "a_2.npy", np.zeros(S * S, np.float32))
    assert D.MeasurementFolder(str(tmp_path)).names[2:4] == ["a_2.npy", "y_2.npy"]
    # --subset_end - --subset_start entries at most
    assert D.MeasurementFolder(str(tmp_path), limit=2).names == ["y_0.npy", "run3_y_1.npy"]


def test_an_npy_of_any_shape_and_dtype_is_taken_as_the_row(tmp_path):
    from ddnm_amd.guided_diffusion import diffusion as D
    op = _engine().SuperResolution(3, S, 4, "cpu")
    v = np.arange(3 * 8 * 8, dtype=np.float64).reshape(3, 8, 8) / 7
    np.save(tmp_path / "y_0.npy", v)
    row, picture = D.MeasurementFolder(str(tmp_path)).bind(op, _config())[0]
    assert not picture and row.dtype == torch.float32
    assert torch.equal(row, torch.from_numpy(v.astype(np.float32).reshape(-1)))


def test_a_duplicate_stem_is_refused(tmp_path):
    from ddnm_amd.guided_diffusion import diffusion as D
    np.save(tmp_path / "y_1.npy", np.zeros(4, np.float32))
    _png(tmp_path / "y_1.png", np.zeros((S, S), np.uint8))
    with pytest.raises(ValueError) as e:
        D.MeasurementFolder(str(tmp_path))
    assert "y_1.npy" in str(e.value) and "y_1.png" in str(e.value)


def test_an_empty_or_missing_folder_is_refused(tmp_path):
    from ddnm_amd.guided_diffusion import diffusion as D
    with pytest.raises(FileNotFoundError):
        D.MeasurementFolder(str(tmp_path))
    with pytest.raises(FileNotFoundError):
        D.MeasurementFolder(str(tmp_path / "nowhere"))


def test_a_wrong_element_count_or_pixel_size_names_the_file(tmp_path):
    from ddnm_amd.guided_diffusion import diffusion as D
    E = _engine()
    sr = E.SuperResolution(3, S, 4, "cpu")
    good = tmp_path / "good"
    good.mkdir()
    np.save(good / "y_0.npy", np.zeros((3, 8, 8), np.float32))
    _png(good / "y_1.png", np.zeros((8, 8, 3), np.uint8))
    D.MeasurementFolder(str(good)).bind(sr, _config())
    short = tmp_path / "short"
    short.mkdir()
    np.save(short / "y_0.npy", np.zeros((3, 8, 8), np.float32))
    np.save(short / "y_1.npy", np.zeros(191, np.float32))
    with pytest.raises(ValueError) as e:
        D.MeasurementFolder(str(short)).bind(sr, _config())
    assert "y_1.npy" in str(e.value) and "191" in str(e.value) and "192" in str(e.value)
    big = tmp_path / "big"
    big.mkdir()
    _png(big / "y_0.png", np.zeros((8, 9, 3), np.uint8))             # 9 wide, 8 tall
    with pytest.raises(ValueError) as e:
        D.MeasurementFolder(str(big)).bind(sr, _config())
    assert "y_0.png" in str(e.value) and "9 x 8" in str(e.value) and "8 x 8" in str(e.value)
    # an operator whose measurement is no picture takes .npy only
    wh = E.WalshHadamardCS(3, S, 4, torch.randperm(S * S, generator=torch.Generator().manual_seed(1)), "cpu")
    with pytest.raises(ValueError) as e:
        D.MeasurementFolder(str(big)).bind(wh, _config())
    assert "y_0.png" in str(e.value) and ".npy" in str(e.value)


def test_measurements_json_must_agree_with_the_run(tmp_path):
    from ddnm_amd.guided_diffusion import diffusion as D
    np.save(tmp_path / "y_0.npy", np.zeros(192, np.float32))
    ds = D.MeasurementFolder(str(tmp_path))
    run = D.run_settings(_args(), _config(), 0.0)
    assert sorted(run) == ["add_noise", "channels", "deg", "deg_scale", "image_size", "seed", "sigma_y"]
    assert ds.settings() is None
    ds.check_settings(run)                                          # no file: nothing to compare
    (tmp_path / "measurements.json").write_text(json.dumps(run))
    ds.check_settings(run)
    # seed, sigma_y and add_noise describe the first run; the second one may differ in them
    ds.check_settings(D.run_settings(_args(seed=5, add_noise=True), _config(), 0.1))
    for key, other in (("deg", dict(deg="sr_bicubic")), ("deg_scale", dict(deg_scale=2.0))):
        with pytest.raises(ValueError, match=key):
            ds.check_settings(D.run_settings(_args(**other), _config(), 0.0))
    with pytest.raises(ValueError, match="image_size"):
        ds.check_settings(D.run_settings(_args(), _config(size=64), 0.0))
    with pytest.raises(ValueError, match="channels"):
        ds.check_settings(D.run_settings(_args(), _config(channels=1), 0.0))


def test_a_grey_png_loads_to_the_data_transform_of_its_pixels(tmp_path):
    from ddnm_amd.guided_diffusion import diffusion as D
    pixels = np.random.default_rng(3).integers(0, 256, (S, S), dtype=np.uint8)
    pixels[0, :3] = (0, 255, 128)
    _png(tmp_path / "y_0.png", pixels)
    cfg = _config()
    x, picture = D.MeasurementFolder(str(tmp_path)).bind(_engine().Colorization(S, "cpu"), cfg)[0]
    want = D.data_transform(cfg, torch.from_numpy(pixels.copy()).float().div(255.0))[None]
    assert picture and x.dtype == torch.float32 and x.shape == (1, S, S) and torch.equal(x, want)
    assert float(x[0, 0, 0]) == -1.0 and float(x[0, 0, 1]) == 1.0
    # an RGB picture for a three-channel measurement keeps CHW order; a grey one is spread over the channels
    rgb = np.random.default_rng(4).integers(0, 256, (S, S, 3), dtype=np.uint8)
    _png(tmp_path / "y_1.png", rgb)
    ds = D.MeasurementFolder(str(tmp_path)).bind(_engine().Denoising(3, S, "cpu"), cfg)
    assert torch.equal(ds[1][0], D.data_transform(cfg, torch.from_numpy(rgb.copy()).permute(2, 0, 1).float().div(255.0)))
    assert torch.equal(ds[0][0], want.expand(3, S, S))


def test_bank_rows_are_zero_padded_to_y_dim(tmp_path):
    """Masks keeping 5, 9 and 2 pixels: rows of 15, 27 and 6 values in a bank whose y_dim is 28; image i uses mask i % 3,
    with --subset_start counted in."""
    from ddnm_amd.guided_diffusion import diffusion as D
    masks = np.zeros((3, S * S), np.float32)
    for r, n in enumerate((5, 9, 2)):
        masks[r, 7 * r:7 * r + n] = 1
    bank = _engine().InpaintingBank(3, S, masks.reshape(3, S, S), "cpu")
    assert bank.y_dim == 28 and [bank.measurement_size(i) for i in range(5)] == [15, 27, 6, 15, 27]
    assert bank.measurement_image_shape() == (3, S, S)
    per_image = bank.for_images([4, 5, 6])
    assert per_image.measurement_size() == [27, 6, 15] and per_image.measurement_image_shape() == (3, S, S)
    rows = [np.arange(1, n + 1, dtype=np.float32) for n in (27, 6, 15)]       # images 4, 5, 6
    for p, row in enumerate(rows):
        np.save(tmp_path / f"y_{4 + p}.npy", row)
    ds = D.MeasurementFolder(str(tmp_path)).bind(bank, _config(), start=4)
    for p, row in enumerate(rows):
        got, picture = ds[p]
        assert not picture and got.shape == (28,)
        assert torch.equal(got[:row.size], torch.from_numpy(row)) and bool((got[row.size:] == 0).all())
    with pytest.raises(ValueError, match="y_4.npy"):                  # read as images 0, 1, 2 the counts do not fit
        D.MeasurementFolder(str(tmp_path)).bind(bank, _config(), start=0)


# ------------------------------------------------------------------------------------------------ the operators
def _oracle_rows(name, d):
    from oracle import cases
    orc = cases.make_operator(name, d)
    return orc, orc.A(torch.zeros(1, 3, d, d)).reshape(1, -1).shape[1]


def test_measurement_size_and_shape_of_every_operator_class():
    """measurement_size against the row length of the CPU oracle's A at the same sizes; measurement_image_shape is a CHW
    shape of that many values where the row is a picture -- for inpainting the full-size picture A reads it from."""
    from oracle import cases, operators as O
    E = _engine()
    d = S
    perm = cases.wh_perm(d)
    mask = cases.random_mask(d)
    miss = O.Inpainting.missing_from_mask(mask)
    k9 = torch.Tensor([1 / 9] * 9)
    g2, g1 = E.gaussian_taps(20, 4), E.gaussian_taps(1, 4)
    built = {
        "denoising": (E.Denoising(3, d, "cpu"), (3, d, d)),
        "sr_averagepooling": (E.SuperResolution(3, d, 4, "cpu"), (3, d // 4, d // 4)),
        "sr_bicubic": (E.SRConv(E.bicubic_kernel(4), 3, d, "cpu", stride=4), (3, d // 4, d // 4)),
        "colorization": (E.Colorization(d, "cpu"), (1, d, d)),
        "deblur_uni": (E.Deblurring(k9, 3, d, "cpu"), (3, d, d)),
        "deblur_aniso": (E.Deblurring2D(g1 / g1.sum(), g2 / g2.sum(), 3, d, "cpu"), (3, d, d)),
        "cs_walshhadamard": (E.WalshHadamardCS(3, d, 4, perm, "cpu"), None),
        "cs_blockbased": (E.CS(3, d, 0.25, "cpu", gauss=O.gauss_matrix(5)), None),
    }
    for name, (op, shape) in built.items():
        _, rows = _oracle_rows(name, d)
        assert op.measurement_size() == rows, name
        assert op.measurement_image_shape() == shape, name
        if shape is not None:
            assert int(np.prod(shape)) == rows, name
    inp = E.Inpainting(3, d, miss, "cpu")
    orc = O.Inpainting(3, d, miss)
    assert inp.measurement_size() == orc.A(torch.zeros(1, 3, d, d)).reshape(1, -1).shape[1] == 3 * inp.n_kept
    assert inp.measurement_image_shape() == (3, d, d)
    # the simplified path's operators, and the dense one, take .npy only
    pm = E.PixelMask(3, d, torch.from_numpy(np.asarray(mask)).float(), "cpu")
    assert pm.measurement_size() == 3 * d * d and pm.measurement_image_shape() is None
    comp = E.mask_color_sr(3, d, torch.from_numpy(np.asarray(mask)).float(), 4, "cpu")
    assert comp.measurement_size() == (d // 4) ** 2 and comp.measurement_image_shape() is None
    dense = E.GeneralA.__new__(E.GeneralA)
    dense._m, dense._d = 7, 48
    assert dense.measurement_size() == 7 and dense.measurement_image_shape() is None
    with pytest.raises(NotImplementedError):
        E.A_functions().measurement_size()
    assert E.A_functions().measurement_image_shape() is None
    # every operator class answers both questions
    for cls in (E.Denoising, E.SuperResolution, E.Colorization, E.Inpainting, E.PerImageInpainting, E.WalshHadamardCS,
                E.CS, E.PixelMask, E.Composition, E.GeneralA, E.SRConv, E.Deblurring2D, E.Deblurring):
        assert cls.measurement_size is not E.A_functions.measurement_size, cls.__name__


# ------------------------------------------------------------------------------------------------ the switches
def test_metrics_switch_accepts_cons(monkeypatch):
    from ddnm_amd.guided_diffusion import diffusion as D
    assert D.METRICS == ("ssim", "cons")
    monkeypatch.setenv("DDNM_METRICS", "cons")
    assert D.extra_metrics() == ("cons",) and D.extra_metrics(8) == ("cons",)        # no window: any image size
    monkeypatch.setenv("DDNM_METRICS", "ssim,cons")
    assert D.extra_metrics(64) == ("ssim", "cons")
    monkeypatch.setenv("DDNM_METRICS", "cons, ssim")
    assert D.extra_metrics(64) == ("cons", "ssim")
    monkeypatch.setenv("DDNM_METRICS", "cons,psnr")
    with pytest.raises(ValueError, match="accepted values: ssim, cons"):
        D.extra_metrics()


def test_save_y_switch(monkeypatch):
    from ddnm_amd.guided_diffusion import diffusion as D
    monkeypatch.delenv("DDNM_SAVE_Y", raising=False)
    assert D.save_y() is False
    monkeypatch.setenv("DDNM_SAVE_Y", "0")
    assert D.save_y() is False
    monkeypatch.setenv("DDNM_SAVE_Y", "1")
    assert D.save_y() is True
    monkeypatch.setenv("DDNM_SAVE_Y", "yes")
    with pytest.raises(ValueError, match="DDNM_SAVE_Y"):
        D.save_y()


def test_measurement_dir_is_absolute_or_below_the_datasets(tmp_path):
    from ddnm_amd.guided_diffusion import diffusion as D
    assert D.measurement_dir("celeba_hq", "exp") is None and D.measurement_dir("synthetic:3", "exp") is None
    assert D.measurement_dir("measurements:run1/y", "exp") == os.path.join("exp", "datasets", "run1/y")
    assert D.measurement_dir(f"measurements:{tmp_path}", "exp") == str(tmp_path)
    with pytest.raises(ValueError):
        D.measurement_dir("measurements:", "exp")


def test_metric_log_cons_lines(monkeypatch, capsys):
    """Cons = l1 / (2 n) per image, ConsMax = maxabs / 2; running mean of sample 0, total, max; a run without ground
    truth prints no PSNR line and reports Cons unasked."""
    from ddnm_amd.guided_diffusion import diffusion as D
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64)                       # noqa: E731
    monkeypatch.setenv("DDNM_METRICS", "cons")
    log = D.MetricLog(8)
    x = torch.zeros(2, 3, 8, 8)
    log.add(x, x, f64(20.0, 30.0), 5)
    log.add_cons(f64(4e-3, 8e-3), torch.tensor([2e-4, 6e-4]), [10, 20], 0)
    log.add(x[:1], x[:1], f64(10.0), 7)
    log.add_cons(f64(6e-3), torch.tensor([1e-4]), [10], 0)
    res = log.total(0, "cpu", reduce=False)
    assert capsys.readouterr().out == ("PSNR: 25.00\nCons: 2.000e-04\nPSNR: 20.00\nCons: 2.333e-04\n"
                                       "Total Average PSNR: 20.00\nTotal Average Cons: 2.333e-04\nMax Cons: 3.000e-04\n"
                                       "Number of samples: 3\n")
    assert res["index"] == [5, 6, 7] and res["psnr"] == 20.0
    assert res["cons_per_image"] == pytest.approx([2e-4, 2e-4, 3e-4], rel=1e-12)
    assert res["cons"] == pytest.approx(7e-4 / 3, rel=1e-12)
    assert res["cons_max"] == pytest.approx(3e-4, rel=1e-6)
    monkeypatch.delenv("DDNM_METRICS")
    log = D.MetricLog(8, samples=2, ground_truth=False)
    assert log.with_cons
    log.count(1, 0)
    log.add_cons(f64(2e-3), torch.tensor([2e-4]), [10], 0)
    log.add_cons(f64(4e-3), torch.tensor([8e-4]), [10], 1)
    log.add_samples(None, None, f64(0.25), None, None)
    res = log.total(0, "cpu", reduce=False)
    assert capsys.readouterr().out == ("Cons: 1.000e-04\nSample Cons: 1.500e-04\nStd: 0.2500\n"
                                       "Total Average Cons: 1.000e-04\nMax Cons: 4.000e-04\nTotal Average Std: 0.2500\n"
                                       "Total Average Sample Cons: 1.500e-04\nNumber of samples: 1\nSamples per image: 2\n")
    assert res["psnr"] is None and res["cons"] == pytest.approx(1e-4) and res["n"] == 1


# ------------------------------------------------------------------------------------------------ the refusals
def _runner(D, args):
    class Runner(D.Diffusion):
        def __init__(self):
            self.args, self.config = args, _config()

        def _build_model(self):
            raise AssertionError("the model was built before the refusal")

        def _loader(self):
            raise AssertionError("a loader was built before the refusal")

    return Runner()


def test_what_a_run_over_measurements_refuses(monkeypatch):
    from ddnm_amd.guided_diffusion import diffusion as D
    monkeypatch.delenv("DDNM_METRICS", raising=False)
    monkeypatch.delenv("DDNM_SAMPLES", raising=False)
    monkeypatch.delenv("DDNM_SAVE_Y", raising=False)
    D.check_measurements(_args(), False)
    D.check_measurements(_args(sigma_y=0.05), False)                              # --sigma_y alone: DDNM+ at that level
    D.check_measurements(_args(path_y="synthetic:3", add_noise=True), True)       # not a run over measurements
    with pytest.raises(ValueError, match="add_noise"):
        _runner(D, _args(add_noise=True, sigma_y=0.05)).sample(False)
    with pytest.raises(ValueError, match="simplified"):
        _runner(D, _args()).sample(True)
    monkeypatch.setenv("DDNM_METRICS", "ssim,cons")
    with pytest.raises(ValueError, match="ssim"):
        _runner(D, _args()).sample(False)
    monkeypatch.setenv("DDNM_METRICS", "cons")
    with pytest.raises(AssertionError, match="model"):                            # nothing to refuse: the run starts
        _runner(D, _args()).sample(False)


def test_the_hq_demo_refuses_measurements():
    spec = importlib.util.spec_from_file_location("hq_main_measurements", os.path.join(ROOT, "hq_demo", "main.py"))
    hq_main = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hq_main)
    with pytest.raises(ValueError, match="measurements"):
        hq_main.main({}, {"path_y": "measurements:some/folder"})


# ------------------------------------------------------------------------------------------------ the C boundary
def test_the_new_symbols_are_declared_and_mirrored():
    from ddnm_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddnm_hip.h")).read(), flags=re.S)
    assert re.search(r"int64_t\s+ddnm_consistency_workspace_elems\s*\(\s*int32_t B,\s*int64_t m\s*\)", src)
    decl = re.search(r"int\s+ddnm_consistency_f32\s*\(([^;]*)\)\s*;", src).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert names == ["ax", "y", "row_stride", "counts", "l1", "sse", "maxabs", "work", "work_elems", "B", "m", "stream"]
    res, argt = _lib.PROTOTYPES["ddnm_consistency_f32"]
    assert res is _lib.c_int32 and len(argt) == 12
    assert [argt[i] for i in (2, 8, 9, 10)] == [_lib.c_int64, _lib.c_int64, _lib.c_int32, _lib.c_int64]
    assert _lib.PROTOTYPES["ddnm_consistency_workspace_elems"] == (_lib.c_int64, [_lib.c_int32, _lib.c_int64])
    assert _lib.ABI_VERSION == 7


def test_consistency_checks_its_arguments_before_the_library(monkeypatch):
    from ddnm_amd import _lib, ops

    def no_library():
        raise AssertionError("the library was touched before the refusal")

    monkeypatch.setattr(_lib, "lib", no_library)
    a = torch.zeros(2, 6)
    for ax, y in ((a, torch.zeros(2, 5)), (a[0], a[0]), (a.reshape(2, 3, 2), a.reshape(2, 3, 2)), (a, [0.0] * 12),
                  (torch.zeros(0, 6), torch.zeros(0, 6))):
        with pytest.raises(ValueError, match="consistency"):
            ops.consistency(ax, y)
    for counts in ([1], [1, 2, 3], [1, 7], [-1, 2], [1.5, 2], torch.tensor([1, 2]), torch.tensor([1, 7], dtype=torch.int32),
                   torch.tensor([[1, 2]], dtype=torch.int32)):
        with pytest.raises(ValueError, match="counts"):
            ops.consistency(a, a, counts)
    with pytest.raises(ValueError, match="device"):                      # host tensors are not copied over behind the caller
        ops.consistency(a, a, [6, 0])
