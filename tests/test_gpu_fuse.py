"""Batch fusing on the GPU: per-image Philox keys (ddnm_*_keyed_f32, ops.KeyedPhiloxNoise) reproduce the per-batch
draws bit for bit, the samplers restore K independently seeded images in one call as K separate calls do, and the
runner with DDNM_FUSE_BATCHES=K writes what the unfused runner writes."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import rel

pytestmark = pytest.mark.gpu

KEYS = [0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x0123456789ABCDEF]
CTRS = [0, 5, 1]
# the forward need not be batch-invariant (split-K / persistent choice by B): measured rel-L2 (printed) 2.6e-7 for the
# runner at T = 4 on the MI355X, 0 for the samplers at B = 3 vs 1; the bar is about 10x the largest
BAR = 3e-6


def _sources():
    from ddnm_amd import ops
    return [ops.PhiloxNoise(k, image_base=c) for k, c in zip(KEYS, CTRS)]


@pytest.mark.parametrize("n", [3 * 64 * 64, 4, 5, 6, 7, 3 * 1001])
def test_keyed_draw_matches_per_batch_draw_and_oracle(hip, n):
    from ddnm_amd import ops
    from tests.test_fuse_host import keyed_oracle
    kn = ops.KeyedPhiloxNoise(KEYS, CTRS)
    like = torch.empty(3, n, device="cuda")
    for it in (0, 7, ops.PhiloxNoise.XT_ITER):
        got = kn.tensor(it, like)
        torch.cuda.synchronize()
        if n % 4 == 0:
            ref = torch.cat([src.tensor(it, like[:1]) for src in _sources()], 0)
            assert torch.equal(got, ref)
        exp = torch.from_numpy(keyed_oracle(KEYS, CTRS, n, it))
        assert torch.allclose(got.cpu(), exp, rtol=0, atol=3e-5), (it, (got.cpu() - exp).abs().max())
    with pytest.raises(ValueError):
        kn.tensor(0, torch.empty(2, n, device="cuda"))


def _operators(d):
    from ddnm_amd.functions import svd_operators as E
    g = torch.Generator().manual_seed(3)
    mask = (torch.rand(d * d, generator=g) < 0.4).float()
    r = torch.nonzero(mask == 0).long().reshape(-1) * 3
    return {"denoise": E.Denoising(3, d, "cuda"), "sr_avgpool": E.SuperResolution(3, d, 4, "cuda"),
            "color": E.Colorization(d, "cuda"), "inpaint": E.Inpainting(3, d, torch.cat([r, r + 1, r + 2], 0), "cuda"),
            "combine": E.SuperResolution(3, d, 2, "cuda")}              # ratio 2: generic x0 / A / A^+ / combine chain


@pytest.mark.parametrize("name", ["denoise", "sr_avgpool", "color", "inpaint", "combine"])
@pytest.mark.parametrize("learn_sigma", [False, True])
def test_keyed_step_equals_unkeyed_per_image(hip, name, learn_sigma):
    """Each keyed step entry point on B = 3 images with mixed keys == the unkeyed one run per image with that image's
    (seed, image_base) -- x0 and x_t' bit for bit."""
    from ddnm_amd import ops
    d, B = 64, 3
    op = _operators(d)[name]
    g = torch.Generator().manual_seed(11)
    xt = torch.randn(B, 3, d, d, generator=g).cuda()
    et_full = torch.randn(B, 6 if learn_sigma else 3, d, d, generator=g).cuda()
    et = et_full[:, :3]
    y = op.A(torch.rand(B, 3, d, d, generator=g).cuda() * 2 - 1).reshape(B, -1).contiguous()
    s = ops.step_scalars(torch.tensor(0.5), torch.tensor(0.6), 0.85)
    kn = ops.KeyedPhiloxNoise(KEYS, CTRS)
    x0_k, xn_k = torch.empty_like(xt), torch.empty_like(xt)
    op.ddnm_step(xt, et, kn, y, kn.stamp(s, 9), x0_k, xn_k)
    for i, src in enumerate(_sources()):
        x0_i, xn_i = torch.empty_like(xt[:1]), torch.empty_like(xt[:1])
        s_i = ops.step_scalars(torch.tensor(0.5), torch.tensor(0.6), 0.85)
        op.ddnm_step(xt[i:i + 1].contiguous(), et[i:i + 1], None, y[i:i + 1].contiguous(), src.stamp(s_i, 9), x0_i, xn_i)
        torch.cuda.synchronize()
        assert torch.equal(x0_k[i:i + 1], x0_i), i
        assert torch.equal(xn_k[i:i + 1], xn_i), i


def _small_net():
    from ddnm_amd.guided_diffusion.models import Model
    from oracle import cases
    cfg, sd = cases.celeba_net("small")
    model = Model(cfg)
    model.load_state_dict(sd)
    return cfg, model


@pytest.mark.parametrize("plus", [False, True])
def test_sampler_with_keyed_noise_equals_separate_calls(hip, plus):
    """ddnm_diffusion / ddnm_plus_diffusion on K = 3 images with per-image keys (time travel on, sigma_y > 0 for DDNM+)
    == three calls of one image with PhiloxNoise(key, image_base)."""
    from ddnm_amd import ops
    from ddnm_amd.functions.svd_ddnm import ddnm_diffusion, ddnm_plus_diffusion
    from ddnm_amd.functions import svd_operators as E
    from oracle import cases
    cfg, model = _small_net()
    cfg.time_travel.T_sampling, cfg.time_travel.travel_length, cfg.time_travel.travel_repeat = 5, 1, 2
    d = cfg.data.image_size
    op = E.SuperResolution(3, d, 4, "cuda")
    g = torch.Generator().manual_seed(5)
    y = op.A(torch.rand(3, 3, d, d, generator=g).cuda() * 2 - 1).reshape(3, -1).contiguous()
    betas = cases.betas().cuda()
    kn = ops.KeyedPhiloxNoise(KEYS, CTRS)
    x = kn.tensor(ops.PhiloxNoise.XT_ITER, torch.empty(3, 3, d, d, device="cuda"))

    def run(xx, yy, noise):
        if plus:
            return ddnm_plus_diffusion(xx, model, betas, 0.85, op, yy, 0.2, config=cfg, noise=noise, return_cpu=False)[0][0]
        return ddnm_diffusion(xx, model, betas, 0.85, op, yy, config=cfg, noise=noise, return_cpu=False)[0][0]

    fused = run(x, y, kn)
    parts = []
    for i, src in enumerate(_sources()):
        xi = src.tensor(ops.PhiloxNoise.XT_ITER, torch.empty(1, 3, d, d, device="cuda"))
        assert torch.equal(xi, x[i:i + 1])
        parts.append(run(xi, y[i:i + 1].contiguous(), src))
    sep = torch.cat(parts, 0)
    torch.cuda.synchronize()
    err = rel(fused, sep)
    print(f"keyed K=3 vs separate calls ({'DDNM+' if plus else 'DDNM'}): rel-L2 {err:.3e}")
    assert torch.isfinite(fused).all() and err < BAR


def _mini_yaml(tmp_path, batch=1, T=4):
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


def _run_main(tmp_path, monkeypatch, folder, argv, fuse, torch_noise=False):
    """main.main([...]) in-process; returns (model batch sizes, per-image PSNR, restored images, PNG names, stdout)."""
    import main
    from ddnm_amd import ops
    from ddnm_amd.guided_diffusion.models import Model
    calls, psnrs, imgs = [], [], []
    orig_call, orig_fin = Model.__call__, ops.finalize_psnr

    def call(self, x, t):
        calls.append(int(x.shape[0]))
        return orig_call(self, x, t)

    def fin(x, x_orig=None, want_img=True):
        img, psnr = orig_fin(x, x_orig, want_img)
        if x_orig is not None:
            psnrs.append(psnr.double().cpu())
            imgs.append(x.detach().clone())
        return img, psnr

    with monkeypatch.context() as m:
        m.setattr(Model, "__call__", call)
        m.setattr(ops, "finalize_psnr", fin)
        m.setenv("DDNM_RANDOM_WEIGHTS", "1")
        if fuse:
            m.setenv("DDNM_FUSE_BATCHES", str(fuse))
        else:
            m.delenv("DDNM_FUSE_BATCHES", raising=False)
        if torch_noise:
            m.setenv("DDNM_NOISE", "torch")
        else:
            m.delenv("DDNM_NOISE", raising=False)
        torch.manual_seed(1234)                      # the simplified path draws from the global generator
        rc = main.main(["--ni", "--config", "mini.yml", "-i", folder] + argv)
    assert rc == 0
    out_dir = tmp_path / "exp" / "image_samples" / folder
    names = sorted(p.name for p in out_dir.glob("*.png"))
    apy = sorted(p.name for p in (out_dir / "Apy").glob("*.png"))
    dedup = [c for i, c in enumerate(calls) if i == 0 or c != calls[i - 1]]
    return dedup, torch.cat(psnrs), torch.cat(imgs, 0), names, apy


@pytest.mark.parametrize("mode", ["svd", "simplified", "torch_noise"])
def test_runner_fuses_batches_of_one(hip, tmp_path, monkeypatch, capsys, mode):
    """synthetic:6 at batch 1: DDNM_FUSE_BATCHES=4 calls the model with batch 4 then 2 and writes the files, PSNR lines
    and images of the unfused run."""
    _mini_yaml(tmp_path)
    monkeypatch.chdir(tmp_path)
    deg = ["--deg", "sr_averagepooling", "--deg_scale", "4"]
    argv = ["--path_y", "synthetic:6", "--eta", "0.85", "--sigma_y", "0."] + deg
    if mode == "simplified":
        argv.append("--simplified")
    tn = mode == "torch_noise"
    calls1, psnr1, img1, names1, apy1 = _run_main(tmp_path, monkeypatch, "one", argv, None, tn)
    out1 = capsys.readouterr().out
    calls4, psnr4, img4, names4, apy4 = _run_main(tmp_path, monkeypatch, "four", argv, 4, tn)
    out4 = capsys.readouterr().out
    assert calls1 == [1] and calls4 == [4, 2], (calls1, calls4)
    expect = [f"{i - 1}_0.png" for i in range(6)] if mode == "simplified" else [f"{i}_0.png" for i in range(6)]
    assert names1 == names4 == sorted(expect)
    assert apy1 == apy4 and len(apy1) == 12
    for out in (out1, out4):
        assert "Number of samples: 6" in out and out.count("\nPSNR: ") == 6, out[-2000:]
    assert psnr1.shape == psnr4.shape == (6,)
    assert (psnr1 - psnr4).abs().max() < 1e-3, (psnr1, psnr4)
    err = rel(img4, img1)
    print(f"runner {mode}: fused K=4 vs unfused rel-L2 {err:.3e}")
    assert err < BAR


def test_inpainting_add_noise_with_odd_measurement_length(hip, tmp_path, monkeypatch, capsys):
    """--deg inpainting --add_noise with a mask whose 3 * n_kept is not a multiple of 4 (Philox measurement noise of any
    length through the keyed draw), unfused and fused."""
    _mini_yaml(tmp_path)
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(0)
    mask = np.zeros(64 * 64, dtype=np.float32)
    mask[rng.choice(64 * 64, 2001, replace=False)] = 1.0           # 2001 kept pixels: 3 * 2001 = 6003 = 3 mod 4
    os.makedirs(tmp_path / "exp" / "inp_masks", exist_ok=True)
    np.save(tmp_path / "exp" / "inp_masks" / "mask.npy", mask.reshape(64, 64))
    argv = ["--path_y", "synthetic:3", "--eta", "0.85", "--deg", "inpainting", "--sigma_y", "0.05", "--add_noise"]
    _, psnr1, img1, names1, _ = _run_main(tmp_path, monkeypatch, "inp1", argv, None)
    out1 = capsys.readouterr().out
    _, psnr2, img2, names2, _ = _run_main(tmp_path, monkeypatch, "inp2", argv, 2)
    out2 = capsys.readouterr().out
    assert "Number of samples: 3" in out1 and "Number of samples: 3" in out2, out1[-2000:] + out2[-2000:]
    assert names1 == names2 == ["0_0.png", "1_0.png", "2_0.png"]
    assert torch.isfinite(img1).all() and (psnr1 - psnr2).abs().max() < 1e-3
    assert rel(img2, img1) < BAR


def _run_cli(tmp_path, nproc, folder, port, fuse):
    """`main.py` under torchrun (gloo, ranks sharing this GPU), as tests/test_gpu_cli.py::_run_cli does."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DDNM_RANDOM_WEIGHTS="1", DDNM_DIST_BACKEND="gloo", PYTHONPATH=root, DDNM_FUSE_BATCHES=str(fuse))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(root, "main.py"), "--ni", "--config", "mini.yml",
           "--path_y", "synthetic:5", "--eta", "0.85", "--deg", "sr_averagepooling", "--deg_scale", "4", "--sigma_y", "0.",
           "-i", folder]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_two_ranks_deal_mode_fused_match_one_rank(hip, tmp_path):
    import socket
    from PIL import Image
    _mini_yaml(tmp_path)

    def port():
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        p = s.getsockname()[1]
        s.close()
        return p
    out1 = _run_cli(tmp_path, 1, "one", port(), 1)
    out2 = _run_cli(tmp_path, 2, "two", port(), 2)
    assert "Number of samples: 5" in out1 and "Number of samples: 5" in out2
    psnr = lambda o: float(o.split("Total Average PSNR:")[1].split()[0])                        # noqa: E731
    assert abs(psnr(out1) - psnr(out2)) <= 0.01
    d1, d2 = tmp_path / "exp" / "image_samples" / "one", tmp_path / "exp" / "image_samples" / "two"
    names = sorted(p.name for p in d1.glob("*.png"))
    assert names == sorted(p.name for p in d2.glob("*.png")) == [f"{i}_0.png" for i in range(5)]
    for n in names:
        a = np.asarray(Image.open(d1 / n), dtype=np.int16)
        b = np.asarray(Image.open(d2 / n), dtype=np.int16)
        assert np.abs(a - b).max() <= 1 and (a != b).mean() < 1e-3, n
