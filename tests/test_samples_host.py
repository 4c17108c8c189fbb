"""DDNM_SAMPLES on the host: the key rule of the K samples, the switch parser, the row order of a sampler call over
samples, the refusal of --simplified, the K-sample lines of MetricLog and the evaluator's --sample / --against mean.
No GPU call."""
import os

import pytest


def _key(src):
    return (src.seed_hi << 32) | src.seed_lo


def test_sample_k_draws_as_the_run_under_seed_plus_k():
    from ddnm_amd import ops
    from ddnm_amd.guided_diffusion import diffusion as D
    for seed, bi, lo in ((1234, 0, 0), (1234, 7, 3), (2 ** 40 + 5, 2, 1)):
        srcs = D.sample_sources(seed, bi, 4, lo)
        assert len(srcs) == 4 and all(isinstance(s, ops.PhiloxNoise) for s in srcs)
        for k, src in enumerate(srcs):
            assert _key(src) == D._mix64(seed + k, bi) and src.image_base == lo, (seed, bi, lo, k)
        # sample 0 is the source of the plain run
        plain = ops.PhiloxNoise(D._mix64(seed, bi), image_base=lo)
        assert (_key(srcs[0]), srcs[0].image_base) == (_key(plain), plain.image_base)
        assert len({_key(s) for s in srcs}) == 4
    # sample k of this run == sample 0 of the run under seed + k
    assert _key(D.sample_sources(1234, 5, 3, 0)[2]) == _key(D.sample_sources(1236, 5, 1, 0)[0])


def test_switch_parser(monkeypatch):
    from ddnm_amd.guided_diffusion import diffusion as D
    monkeypatch.delenv("DDNM_SAMPLES", raising=False)
    assert D.samples() == 1
    monkeypatch.setenv("DDNM_SAMPLES", "8")
    assert D.samples() == 8
    for bad in ("0", "-2"):
        monkeypatch.setenv("DDNM_SAMPLES", bad)
        with pytest.raises(ValueError, match="DDNM_SAMPLES"):
            D.samples()


def test_rows_run_batch_major_then_sample_then_image():
    from ddnm_amd.guided_diffusion import diffusion as D
    assert D.sample_rows([4, 5], [2], 1) == [4, 5]
    assert D.sample_rows([4, 5], [2], 3) == [4, 5, 4, 5, 4, 5]
    # a fused group of a batch of two and a ragged batch of one
    assert D.sample_rows([4, 5, 6], [2, 1], 2) == [4, 5, 4, 5, 6, 6]
    assert D.sample_rows([0, 1, 2], [1, 1, 1], 2) == [0, 0, 1, 1, 2, 2]
    with pytest.raises(ValueError):
        D.sample_rows([0, 1, 2], [2], 2)


def test_simplified_is_refused_with_more_than_one_sample(monkeypatch):
    from ddnm_amd.guided_diffusion import diffusion as D
    D.check_samples(1, True)
    D.check_samples(2, False)
    with pytest.raises(ValueError, match="simplified"):
        D.check_samples(2, True)

    # ... and `sample` asks before it builds the model or opens the loader
    class Runner(D.Diffusion):
        def __init__(self):
            pass

        def _build_model(self):
            raise AssertionError("the model was built before the refusal")

    monkeypatch.setenv("DDNM_SAMPLES", "2")
    with pytest.raises(ValueError, match="simplified"):
        Runner().sample(True)


def test_metric_log_prints_the_k_sample_lines_after_sample_zero(monkeypatch, capsys):
    import torch
    from ddnm_amd.guided_diffusion import diffusion as D
    monkeypatch.delenv("DDNM_METRICS", raising=False)
    log = D.MetricLog(8, samples=2)
    x = torch.zeros(2, 3, 8, 8)
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64)                                       # noqa: E731
    log.add(x, x, f64(20.0, 30.0), 0)
    log.add_samples(f64(26.0, 28.0), torch.stack([f64(20.0, 30.0), f64(22.0, 24.0)]), f64(0.1, 0.3), x, x)
    res = log.total(0, "cpu", reduce=False)
    assert capsys.readouterr().out == (
        "PSNR: 25.00\nMean-of-K PSNR: 27.00\nSample PSNR: 24.00\nStd: 0.2000\n"
        "Total Average PSNR: 25.00\nTotal Average Mean-of-K PSNR: 27.00\nTotal Average Sample PSNR: 24.00\n"
        "Total Average Std: 0.2000\nNumber of samples: 2\nSamples per image: 2\n")
    assert res["psnr"] == 25.0 and res["n"] == 2 and res["samples"] == 2
    assert res["psnr_mean_image"] == 27.0 and res["psnr_all_samples"] == 24.0 and abs(res["std"] - 0.2) < 1e-15
    # one sample: the result has today's keys only
    plain = D.MetricLog(8)
    plain.add(x, x, f64(20.0, 30.0), 0)
    keys = set(plain.total(0, "cpu", reduce=False))
    assert keys == {"psnr", "ssim", "n", "index", "psnr_per_image", "ssim_per_image"}
    assert set(res) - keys == {"samples", "psnr_mean_image", "psnr_all_samples", "std"}


def _png(path, value):
    import numpy as np
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.full((2, 2, 3), value, dtype=np.uint8)).save(path)


def test_evaluator_pairs_a_chosen_sample_and_the_mean(tmp_path):
    from ddnm_amd.evaluate import load_image, pair_files
    root = str(tmp_path / "run")
    for i in (0, 1, 2):
        _png(os.path.join(root, "Apy", f"orig_{i}.png"), 10 + i)
        _png(os.path.join(root, f"{i}_0.png"), 20 + i)
    for i in (0, 2):
        _png(os.path.join(root, f"{i}_1.png"), 30 + i)
    for i in (1, 2, 3):
        _png(os.path.join(root, "mean", f"mean_{i}.png"), 40 + i)
    _png(os.path.join(root, "std", "std_0.png"), 50)
    rel = lambda pairs: [(i, os.path.relpath(a, root), os.path.relpath(b, root)) for i, a, b in pairs]      # noqa: E731
    # current calls keep their pairing
    pairs, missing = pair_files(root)
    assert rel(pairs) == [(i, f"Apy/orig_{i}.png", f"{i}_0.png") for i in (0, 1, 2)]
    assert missing == {"orig": [], "restored": []}
    assert pair_files(root, "restored", 0)[0] == pairs
    pairs, missing = pair_files(root, sample=1)
    assert rel(pairs) == [(0, "Apy/orig_0.png", "0_1.png"), (2, "Apy/orig_2.png", "2_1.png")]
    assert missing == {"orig": [], "restored": [1]}
    assert int(round(load_image(pairs[1][2])[0, 0, 0] * 255)) == 32
    pairs, missing = pair_files(root, against="mean")
    assert rel(pairs) == [(1, "Apy/orig_1.png", "mean/mean_1.png"), (2, "Apy/orig_2.png", "mean/mean_2.png")]
    assert missing == {"orig": [3], "mean": [0]}
    with pytest.raises(FileNotFoundError):
        pair_files(root, sample=2)
    with pytest.raises(ValueError):
        pair_files(root, against="mean", sample=1)
    with pytest.raises(ValueError):
        pair_files(root, sample=-1)


def test_evaluator_cli_takes_the_new_options(tmp_path, monkeypatch, capsys):
    from ddnm_amd import evaluate
    root = str(tmp_path / "run")
    _png(os.path.join(root, "Apy", "orig_0.png"), 10)
    _png(os.path.join(root, "0_1.png"), 30)
    _png(os.path.join(root, "mean", "mean_0.png"), 40)
    seen = []
    monkeypatch.setattr(evaluate, "evaluate", lambda pairs: seen.append(pairs) or [(i, 1.0, 0.5) for i, _, _ in pairs])
    assert evaluate.main([root, "--sample", "1"]) == 0
    assert evaluate.main([root, "--against", "mean"]) == 0
    assert [os.path.basename(p[0][2]) for p in seen] == ["0_1.png", "mean_0.png"]
    assert capsys.readouterr().out.count("Number of images: 1") == 2
