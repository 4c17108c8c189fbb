"""DDNM_SAMPLES on the GPU: the sample-statistics kernel (ddnm_sample_stats_f32, ops.sample_stats) against a float64
numpy model of its definition, and the runner restoring every measurement K times in one sampler call -- sample k as
the plain run under `--seed seed + k` restores it, one shared measurement, every sharding and fusing mode.

The runner derives three things from `--seed`: the noise, and (for `--path_y synthetic:N` with DDNM_RANDOM_WEIGHTS=1)
the images, their loader order and the weights.  Sample k promises the NOISE of seed + k on the SAME measurement, so the
plain runs these tests compare with keep data, order and weights at the base seed (`_pin_data_and_weights`) and move the
noise seed alone."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from tests.helpers import rel
from tests.test_gpu_fuse import BAR, _mini_yaml

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
LAYOUTS = ("samples_major", "images_major")
SEED = 1234


# ------------------------------------------------------------------------------------------------ the kernel
def unit(x):
    """clamp((x + 1) / 2, 0, 1) in fp32, as finalize_psnr_kernel forms it."""
    return np.clip((x.astype(F32) + F32(1.0)) / F32(2.0), F32(0.0), F32(1.0)).astype(F32)


def model(x, B, K, layout, x_orig=None):
    """The definition in float64: x [B * K, chw] fp32 rows in `layout`; returns (mean fp32 [B, chw], std fp32 [B, chw],
    sse_mean [B] or None, std_mean [B])."""
    chw = x.shape[1]
    v = unit(x)
    v = v.reshape(K, B, chw) if layout == "samples_major" else v.reshape(B, K, chw).transpose(1, 0, 2)
    v = v.astype(F64)
    m = v.sum(0) / K
    s = np.sqrt(((v - m) ** 2).sum(0) / (K - 1)) if K > 1 else np.zeros_like(m)
    m32 = m.astype(F32)
    sse = None
    if x_orig is not None:
        d = m32 - unit(x_orig)                      # fp32, the convention of finalize_psnr_kernel
        sse = (d * d).astype(F64).sum(1)
    return m32, s.astype(F32), sse, s.sum(1) / chw


def planted(B, K, chw, layout, seed):
    """0.8 N(0, 1) with three planted regions per image: all samples +3 (saturates at 1), all samples -3 (saturates at
    0), 0.8 + 1e-6 N(0, 1) (small variance on a large mean).  Returns the rows [B * K, chw] and the masks [B, chw] of
    the two saturated regions together and of the small-variance region.  Images of fewer than five values hold one
    region each: image b is of kind b % 4 (0: none)."""
    rng = np.random.default_rng(seed)
    x = (0.8 * rng.standard_normal((K, B, chw))).astype(F32)
    sat, small = np.zeros((B, chw), bool), np.zeros((B, chw), bool)
    for b in range(B):
        if chw >= 5:
            n = max(1, chw // 8)
            regions = [(1, 0, n), (2, chw // 4, n), (3, chw // 2, n)]
        else:
            regions = [(b % 4, 0, chw)] if b % 4 else []
        for kind, lo, n in regions:
            if kind == 1:
                x[:, b, lo:lo + n] = 3.0
            elif kind == 2:
                x[:, b, lo:lo + n] = -3.0
            else:
                x[:, b, lo:lo + n] = (0.8 + 1e-6 * rng.standard_normal((K, n))).astype(F32)
            (small if kind == 3 else sat)[b, lo:lo + n] = True
    rows = x.reshape(K * B, chw) if layout == "samples_major" else x.transpose(1, 0, 2).reshape(B * K, chw)
    return np.ascontiguousarray(rows), sat, small


def raw(x, B, K, layout, x_orig=None, work_elems=None, with_sse=None):
    """ddnm_sample_stats_f32 itself on device tensors; returns (code, mean, std, sse, std_mean) -- outputs prefilled
    with -7 so that a refused call shows it launched nothing."""
    from ddnm_amd import _lib
    lib = _lib.lib()
    chw = x.numel() // (B * max(K, 1))
    n = int(lib.ddnm_sample_stats_workspace_elems(B, chw))
    assert n == 2 * B * ((chw + 2047) // 2048)
    strides = (chw, B * chw) if layout == "samples_major" else (K * chw, chw)
    mean = torch.full((B, chw), -7.0, device="cuda")
    std = torch.full((B, chw), -7.0, device="cuda")
    sse = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    std_mean = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    want_sse = (x_orig is not None) if with_sse is None else with_sse
    work = torch.zeros(n, dtype=torch.float64, device="cuda")
    code = lib.ddnm_sample_stats_f32(x.data_ptr(), strides[0], strides[1], None if x_orig is None else x_orig.data_ptr(),
                                     mean.data_ptr(), std.data_ptr(), sse.data_ptr() if want_sse else None,
                                     std_mean.data_ptr(), work.data_ptr(), n if work_elems is None else work_elems,
                                     B, K, chw, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code, mean, std, sse, std_mean


def within_one_ulp(got, want):
    """|got - want| <= spacing(want), elementwise, for fp32 arrays."""
    return bool((np.abs(got.astype(F64) - want.astype(F64)) <= np.spacing(np.abs(want)).astype(F64)).all())


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("chw", [1, 5, 1027, 3 * 64 * 64])
def test_kernel_matches_the_float64_model(hip, chw, K):
    """mean_img, std_img within ONE fp32 ulp of the float64 model rounded to fp32 (the fp64 moments carry ~1e-16; the one
    rounding to fp32 may land on the other side of a tie), std exactly 0 where every sample saturates and for K = 1,
    sse_mean and std_mean within 1e-12 relative.  A one-pass sum(v^2) - sum(v)^2 / K is 1e4 ... 3e5 ulp off on the
    small-variance region for K >= 3.  Measured on the MI355X: 0 ulp in every case (two passes, like the
    model), 2.8e-16 relative at most."""
    from ddnm_amd import ops
    worst_ulp, worst_rel = 0.0, 0.0
    for B in (1, 3):
        for layout in LAYOUTS:
            x_np, sat, small = planted(B, K, chw, layout, seed=chw * 100 + K * 10 + B)
            xo_np = (np.random.default_rng(chw + B).random((B, chw)) * 2.4 - 1.2).astype(F32)      # clamps on both sides
            x, xo = torch.from_numpy(x_np).cuda(), torch.from_numpy(xo_np).cuda()
            for x_orig in (xo, None):
                code, mean, std, sse, std_mean = raw(x, B, K, layout, x_orig)
                assert code == 0
                m32, s32, sse_w, sm_w = model(x_np, B, K, layout, None if x_orig is None else xo_np)
                mean, std = mean.cpu().numpy(), std.cpu().numpy()
                case = (B, layout, x_orig is not None)
                for got, want in ((mean, m32), (std, s32)):
                    ulp = np.abs(got.astype(F64) - want.astype(F64)) / np.spacing(np.abs(want)).astype(F64)
                    worst_ulp = max(worst_ulp, float(ulp.max()))
                assert within_one_ulp(mean, m32), case
                assert within_one_ulp(std, s32), case
                assert (std[sat] == 0).all() and (std >= 0).all(), case
                if K == 1:
                    assert (std == 0).all() and (std_mean.cpu().numpy() == 0).all(), case
                elif small.any():
                    # v = 0.9 + 5e-7 N(0, 1) on a grid of 6e-8: s is a few 1e-7 (0 where the K values coincide), where
                    # a cancelled sum of squares leaves 1e-4
                    assert (std[small] < 1e-5).all() and (small.sum() < 64 or std[small].max() > 0), case
                sm = std_mean.cpu().numpy()
                assert (np.abs(sm - sm_w) <= 1e-12 * np.abs(sm_w)).all(), (case, sm, sm_w)
                if sm_w.any():
                    worst_rel = max(worst_rel, float((np.abs(sm - sm_w) / np.maximum(sm_w, 1e-300)).max()))
                if x_orig is None:
                    assert (sse.cpu().numpy() == -7.0).all(), case                          # not written
                else:
                    se = sse.cpu().numpy()
                    assert (np.abs(se - sse_w) <= 1e-12 * np.abs(sse_w)).all(), (case, se, sse_w)
                    worst_rel = max(worst_rel, float((np.abs(se - sse_w) / np.maximum(sse_w, 1e-300)).max()))
                    # the Python wrapper: the same images, PSNR by finalize_psnr's formula
                    shape = (B * K, 1, 1, chw)
                    mi, si, psnr, smw = ops.sample_stats(x.view(shape), B, K, layout, xo.view(B, 1, 1, chw))
                    assert mi.shape == si.shape == (B, 1, 1, chw) and psnr.dtype == smw.dtype == torch.float64
                    assert np.array_equal(mi.cpu().numpy().reshape(B, chw), mean)
                    assert np.array_equal(si.cpu().numpy().reshape(B, chw), std)
                    assert torch.equal(psnr, 10.0 * torch.log10(1.0 / (sse / chw))) and torch.equal(smw, std_mean)
    print(f"sample_stats chw={chw} K={K}: worst {worst_ulp:.2f} ulp, worst relative {worst_rel:.2e}")


def test_wrapper_without_an_original(hip):
    from ddnm_amd import ops
    x = torch.randn(6, 3, 8, 8, device="cuda")
    mean, std, psnr, std_mean = ops.sample_stats(x, 2, 3)
    assert psnr is None and mean.shape == std.shape == (2, 3, 8, 8) and std_mean.shape == (2,)
    m32, s32, _, sm = model(x.cpu().numpy().reshape(6, -1), 2, 3, "samples_major")
    assert within_one_ulp(mean.cpu().numpy().reshape(2, -1), m32) and within_one_ulp(std.cpu().numpy().reshape(2, -1), s32)


@pytest.mark.parametrize("chw", [1027, 3 * 64 * 64])
def test_one_sample_is_finalize_psnr(hip, chw):
    """K = 1: mean_img is the img of ops.finalize_psnr bit for bit, sse_mean its sse within 1e-12 relative (the
    summation order differs, nothing else)."""
    from ddnm_amd import _lib
    g = torch.Generator().manual_seed(chw)
    x = (torch.randn(3, chw, generator=g) * 0.8).cuda()
    xo = (torch.rand(3, chw, generator=g) * 2 - 1).cuda()
    code, mean, std, sse, std_mean = raw(x, 3, 1, "samples_major", xo)
    assert code == 0
    img = torch.empty_like(x)
    sse_f = torch.empty(3, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().ddnm_finalize_psnr_f32(x.data_ptr(), xo.data_ptr(), img.data_ptr(), sse_f.data_ptr(), 3, chw,
                                                 torch.cuda.current_stream().cuda_stream), "ddnm_finalize_psnr_f32")
    torch.cuda.synchronize()
    assert torch.equal(mean, img)
    assert ((sse - sse_f).abs() <= 1e-12 * sse_f.abs()).all(), (sse, sse_f)
    assert (std == 0).all() and (std_mean == 0).all()


@pytest.mark.parametrize("chw", [1027, 3 * 64 * 64])
def test_an_image_does_not_depend_on_its_batch(hip, chw):
    """All four outputs of an image, alone and as row 0 / row 2 of a batch of three, in both layouts -- and on the
    element-wise path a misaligned pointer selects: torch.equal."""
    K = 3
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(K, 3, chw, generator=g) * 0.8).cuda()            # [k][b]
    xo = (torch.rand(3, chw, generator=g) * 2 - 1).cuda()
    batch = {"samples_major": x.reshape(K * 3, chw).contiguous(),
             "images_major": x.transpose(0, 1).reshape(3 * K, chw).contiguous()}
    outs = {lay: raw(batch[lay], 3, K, lay, xo) for lay in LAYOUTS}
    for lay in LAYOUTS:
        assert outs[lay][0] == 0
        for a, b in zip(outs[lay][1:], outs["samples_major"][1:]):
            assert torch.equal(a, b), lay
    _, mean, std, sse, std_mean = outs["samples_major"]
    for row in (0, 2):
        alone = x[:, row].contiguous()                                 # [K, chw]: both layouts coincide for one image
        for lay in LAYOUTS:
            code, m1, s1, e1, sm1 = raw(alone, 1, K, lay, xo[row:row + 1].contiguous())
            assert code == 0
            assert torch.equal(m1[0], mean[row]) and torch.equal(s1[0], std[row]), (row, lay)
            assert torch.equal(e1[0], sse[row]) and torch.equal(sm1[0], std_mean[row]), (row, lay)
        # four bytes off a 16-byte boundary: the scalar path, same bits
        buf = torch.empty(K * chw + 1, device="cuda")
        off = buf[1:].view(K, chw)
        off.copy_(alone)
        assert off.data_ptr() % 16 == 4
        code, m1, s1, e1, sm1 = raw(off, 1, K, "samples_major", xo[row:row + 1].contiguous())
        assert code == 0 and torch.equal(m1[0], mean[row]) and torch.equal(s1[0], std[row])
        assert torch.equal(e1[0], sse[row]) and torch.equal(sm1[0], std_mean[row])


def test_bad_arguments_are_refused_before_any_launch(hip):
    from ddnm_amd import _lib, ops
    x = torch.randn(6, 64, device="cuda")
    xo = torch.randn(2, 64, device="cuda")

    def refused(code, *outs):
        with pytest.raises(_lib.DDNMHipError):
            _lib.check(code, "ddnm_sample_stats_f32")
        return all(bool((o == -7.0).all()) for o in outs)

    code, *outs = raw(x, 2, 0, "samples_major", xo)                               # K = 0
    assert code == -1 and refused(code, *outs)
    code, *outs = raw(x, 2, 3, "samples_major", xo, work_elems=3)                 # short workspace (needs 4)
    assert code == -2 and refused(code, *outs)
    code, *outs = raw(x, 2, 3, "samples_major", xo, with_sse=False)               # x_orig without sse_mean
    assert code == -1 and refused(code, *outs)
    assert _lib.lib().ddnm_sample_stats_workspace_elems(0, 64) == -1
    assert _lib.lib().ddnm_sample_stats_workspace_elems(2, 0) == -1
    assert _lib.lib().ddnm_sample_stats_workspace_elems(2 ** 21, 2 ** 22) == -2      # 2^32 workgroups: no such grid
    for bad in (dict(n_images=2, n_samples=0), dict(n_images=0, n_samples=3), dict(n_images=2, n_samples=2),
                dict(n_images=2, n_samples=3, layout="rows"), dict(n_images=2, n_samples=3, x_orig=xo[:1])):
        with pytest.raises(ValueError):
            ops.sample_stats(x, **bad)


# ------------------------------------------------------------------------------------------------ the runner
def _pin_data_and_weights(m):
    """Images, loader order and random weights of every run follow the base seed; `--seed` moves the noise alone."""
    from ddnm_amd.guided_diffusion.diffusion import Diffusion

    def pinned(fn):
        def call(self, *a, **kw):
            keep, self.args.seed = self.args.seed, SEED
            try:
                return fn(self, *a, **kw)
            finally:
                self.args.seed = keep
        return call

    m.setattr(Diffusion, "_loader", pinned(Diffusion._loader))
    m.setattr(Diffusion, "_build_model", pinned(Diffusion._build_model))


def _read(folder):
    from PIL import Image
    return {os.path.relpath(os.path.join(d, f), folder): np.asarray(Image.open(os.path.join(d, f)), dtype=np.int16)
            for d, _, files in os.walk(folder) for f in files if f.endswith(".png")}


def _run(root, folder, argv, seed=SEED, samples=None, fuse=None, torch_noise=False):
    """main.main([...]) in-process, in `root`.  Returns a dict: `calls` (model batch sizes, repeats dropped), `x` /
    `psnr` (the [-1, 1] tensors and PSNRs of every ops.finalize_psnr call that had an original, in call order), `stats`
    (arguments and results of every ops.sample_stats call), `out` (stdout), `png` ({relative path: pixels})."""
    import main
    from ddnm_amd import ops
    from ddnm_amd.guided_diffusion.models import Model
    calls, xs, psnrs, stats = [], [], [], []
    orig_call, orig_fin, orig_stats = Model.__call__, ops.finalize_psnr, ops.sample_stats

    def call(self, x, t):
        calls.append(int(x.shape[0]))
        return orig_call(self, x, t)

    def fin(x, x_orig=None, want_img=True):
        img, psnr = orig_fin(x, x_orig, want_img)
        if x_orig is not None:
            psnrs.append(psnr.double().cpu())
            xs.append(x.detach().clone())
        return img, psnr

    def sample_stats(x, n_images, n_samples, layout="samples_major", x_orig=None):
        res = orig_stats(x, n_images, n_samples, layout, x_orig)
        stats.append(dict(x=x.detach().clone(), B=n_images, K=n_samples, layout=layout, x_orig=x_orig.detach().clone(),
                          mean=res[0].clone(), std=res[1].clone(), psnr=res[2].clone(), std_mean=res[3].clone()))
        return res

    buf = io.StringIO()
    cwd = os.getcwd()
    with pytest.MonkeyPatch.context() as m:
        m.setattr(Model, "__call__", call)
        m.setattr(ops, "finalize_psnr", fin)
        m.setattr(ops, "sample_stats", sample_stats)
        _pin_data_and_weights(m)
        m.setenv("DDNM_RANDOM_WEIGHTS", "1")
        for name, value in (("DDNM_SAMPLES", samples), ("DDNM_FUSE_BATCHES", fuse), ("DDNM_NOISE", "torch" if torch_noise else None)):
            if value is None:
                m.delenv(name, raising=False)
            else:
                m.setenv(name, str(value))
        m.delenv("DDNM_METRICS", raising=False)
        os.chdir(root)
        try:
            with contextlib.redirect_stdout(buf):
                rc = main.main(["--ni", "--config", "mini.yml", "-i", folder, "--seed", str(seed)] + argv)
        finally:
            os.chdir(cwd)
    assert rc == 0
    out = buf.getvalue()
    assert "Number of samples:" in out, out[-3000:]          # main logs an exception of the run and still returns 0
    return dict(calls=[c for i, c in enumerate(calls) if i == 0 or c != calls[i - 1]], x=xs, psnr=psnrs, stats=stats,
                out=out, png=_read(os.path.join(root, "exp", "image_samples", folder)))


def _sample(run, k, K):
    """Sample k of every loader batch of a K-sample run, concatenated in loader order (the runner finishes a batch
    sample by sample)."""
    assert len(run["x"]) % K == 0
    return torch.cat(run["x"][k::K], 0), torch.cat(run["psnr"][k::K])


def _running(values):
    """Running means as MetricLog forms them: one float sum, one division per line."""
    total, means = 0.0, []
    for i, v in enumerate(values):
        total += v
        means.append(total / (i + 1))
    return means


def _lines(out, head):
    return [float(line[len(head):]) for line in out.splitlines() if line.startswith(head)]


SR = ["--path_y", "synthetic:3", "--eta", "0.85", "--sigma_y", "0.", "--deg", "sr_averagepooling", "--deg_scale", "4"]
_plain = {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    root = tmp_path_factory.mktemp("samples")
    _mini_yaml(root)
    return str(root)


def plain_sr(workdir, seed, torch_noise=False):
    """The plain run (one sample) of SR under noise seed `seed`, computed once per module."""
    key = (seed, torch_noise)
    if key not in _plain:
        _plain[key] = _run(workdir, f"plain_{seed}_{int(torch_noise)}", SR, seed=seed, torch_noise=torch_noise)
        assert _plain[key]["calls"] == [1] and len(_plain[key]["x"]) == 3 and not _plain[key]["stats"]
    return _plain[key]


def check_stats_of(run, K, b_of_batch):
    """Every ops.sample_stats call of the run: its rows are the captured samples of that batch, its results are the
    float64 model of them within the bar of test_kernel_matches_the_float64_model, and the PNGs hold them."""
    assert len(run["stats"]) == len(b_of_batch)
    first, pos = 0, 0
    for st, b in zip(run["stats"], b_of_batch):
        assert (st["B"], st["K"], st["layout"]) == (b, K, "samples_major")
        rows = torch.cat(run["x"][pos:pos + K], 0)
        assert torch.equal(st["x"].reshape(rows.shape), rows)
        chw = rows[0].numel()
        m32, s32, sse, sm = model(rows.cpu().numpy().reshape(K * b, chw), b, K, "samples_major",
                                  st["x_orig"].cpu().numpy().reshape(b, chw))
        mean, std = st["mean"].cpu().numpy().reshape(b, chw), st["std"].cpu().numpy().reshape(b, chw)
        assert within_one_ulp(mean, m32) and within_one_ulp(std, s32)
        assert (np.abs(st["std_mean"].cpu().numpy() - sm) <= 1e-12 * sm).all()
        psnr = 10 * np.log10(chw / sse)
        assert np.abs(st["psnr"].cpu().numpy() - psnr).max() < 1e-9
        for j in range(b):
            shown = lambda v: np.floor(np.clip(v.astype(F32) * F32(255) + F32(0.5), 0, 255)).astype(np.int16)      # noqa: E731
            want_mean = shown(mean[j]).reshape(3, 64, 64).transpose(1, 2, 0)
            want_std = shown(np.clip(std[j] * F32(4.0), 0, 1)).reshape(3, 64, 64).transpose(1, 2, 0)
            assert np.array_equal(run["png"][f"mean/mean_{first + j}.png"], want_mean)
            assert np.array_equal(run["png"][f"std/std_{first + j}.png"], want_std)
        assert float(st["std"].max()) > 0
        first, pos = first + b, pos + K
    return [float(st["psnr"].sum()) for st in run["stats"]], [float(st["std_mean"].sum()) for st in run["stats"]]


@pytest.mark.parametrize("mode", ["one_call_per_batch", "fused", "torch_noise"])
def test_runner_restores_three_samples_per_image(hip, workdir, mode):
    """synthetic:3 at batch 1, T = 4, DDNM_SAMPLES=3: the model runs at batch 3 (6 then 3 with DDNM_FUSE_BATCHES=2),
    sample k is the plain run under --seed 1234 + k (rel-L2 < BAR: the forward's launch plans depend on the batch
    size), the PSNR lines are those of sample 0, mean/ and std/ hold the float64 model of the samples."""
    K, tn = 3, mode == "torch_noise"
    run = _run(workdir, f"k3_{mode}", SR, samples=K, fuse=2 if mode == "fused" else None, torch_noise=tn)
    assert run["calls"] == ([6, 3] if mode == "fused" else [3]), run["calls"]
    plain = [plain_sr(workdir, SEED + k, tn) for k in range(K)]
    names = sorted(run["png"])
    assert names == sorted([f"{i}_{k}.png" for i in range(3) for k in range(K)] + [f"mean/mean_{i}.png" for i in range(3)] +
                           [f"std/std_{i}.png" for i in range(3)] + sorted(n for n in plain[0]["png"] if n.startswith("Apy/")))
    assert sorted(plain[0]["png"]) == sorted([f"{i}_0.png" for i in range(3)] + [f"Apy/{p}_{i}.png" for p in ("Apy", "orig")
                                                                                   for i in range(3)])
    for n in plain[0]["png"]:
        if n.startswith("Apy/"):
            assert np.array_equal(run["png"][n], plain[0]["png"][n]), n
    all_psnr = []
    for k in range(K):
        x_k, psnr_k = _sample(run, k, K)
        x_p, psnr_p = torch.cat(plain[k]["x"], 0), torch.cat(plain[k]["psnr"])
        err = rel(x_k, x_p)
        print(f"runner {mode}: sample {k} of K=3 vs plain run under seed {SEED + k}: rel-L2 {err:.3e}")
        assert x_k.shape == (3, 3, 64, 64) and torch.isfinite(x_k).all() and err < BAR, k
        assert (psnr_k - psnr_p).abs().max() < 1e-3, k
        all_psnr.append(psnr_k)
        if k:
            assert rel(x_k, _sample(run, 0, K)[0]) > 1e-3                 # another restoration, not a copy
    # the PSNR lines: running means of sample 0, equal to the plain run's
    running = _running(all_psnr[0].tolist())
    assert _lines(run["out"], "PSNR: ") == [float("%.2f" % r) for r in running]
    plain_running = _running(torch.cat(plain[0]["psnr"]).tolist())
    assert max(abs(a - b) for a, b in zip(running, plain_running)) < 1e-3
    assert _lines(plain[0]["out"], "PSNR: ") == [float("%.2f" % r) for r in plain_running]
    assert "Mean-of-K" not in plain[0]["out"] and "Samples per image" not in plain[0]["out"]
    # the K-sample figures
    mean_psnr, std_mean = check_stats_of(run, K, [1, 1, 1])
    assert _lines(run["out"], "Mean-of-K PSNR: ") == [float("%.2f" % r) for r in _running(mean_psnr)]
    assert _lines(run["out"], "Std: ") == [float("%.4f" % r) for r in _running(std_mean)]
    every = torch.stack(all_psnr)                                          # [K, 3]
    assert _lines(run["out"], "Sample PSNR: ") == [float("%.2f" % (r / K)) for r in _running(every.sum(0).tolist())]
    assert _lines(run["out"], "Total Average Mean-of-K PSNR: ") == [float("%.2f" % (sum(mean_psnr) / 3))]
    assert _lines(run["out"], "Total Average Sample PSNR: ") == [float("%.2f" % (float(every.sum()) / 9))]
    assert _lines(run["out"], "Total Average Std: ") == [float("%.4f" % (sum(std_mean) / 3))]
    assert "Samples per image: 3\n" in run["out"] and "Number of samples: 3\n" in run["out"]
    # the mean of K samples is the better estimate
    assert sum(mean_psnr) / 3 > float(every.mean())


def test_ragged_loader_batch(hip, tmp_path):
    """Batch size 2 over three images, K = 2: the model runs at batch 4, then 2; sample 1 is the run under seed 1235."""
    _mini_yaml(tmp_path, batch=2)
    run = _run(str(tmp_path), "k2", SR, samples=2)
    plain = _run(str(tmp_path), "plain", SR, seed=SEED + 1)
    assert run["calls"] == [4, 2] and plain["calls"] == [2, 1], (run["calls"], plain["calls"])
    assert [tuple(x.shape) for x in run["x"]] == [(2, 3, 64, 64)] * 2 + [(1, 3, 64, 64)] * 2
    x_1, psnr_1 = _sample(run, 1, 2)
    err = rel(x_1, torch.cat(plain["x"], 0))
    print(f"ragged batches, sample 1 vs plain run under seed {SEED + 1}: rel-L2 {err:.3e}")
    assert err < BAR and (psnr_1 - torch.cat(plain["psnr"])).abs().max() < 1e-3
    check_stats_of(run, 2, [2, 1])
    assert sorted(n for n in run["png"] if "/" not in n) == sorted(f"{i}_{k}.png" for i in range(3) for k in range(2))


def test_samples_share_one_measurement(hip, tmp_path):
    """--sigma_y 0.05 --add_noise, K = 2: y and its noise are drawn once, with the run's own seed -- the Apy files are
    the plain run's, sample 0 is the plain run, sample 1 is another restoration of the same y."""
    _mini_yaml(tmp_path)
    argv = ["--path_y", "synthetic:2", "--eta", "0.85", "--sigma_y", "0.05", "--add_noise", "--deg", "sr_averagepooling",
            "--deg_scale", "4"]
    run = _run(str(tmp_path), "k2", argv, samples=2)
    plain = _run(str(tmp_path), "plain", argv)
    assert run["calls"] == [2] and plain["calls"] == [1]
    apy = sorted(n for n in plain["png"] if n.startswith("Apy/"))
    assert len(apy) == 4 and apy == sorted(n for n in run["png"] if n.startswith("Apy/"))
    for n in apy:
        assert np.array_equal(run["png"][n], plain["png"][n]), n
    x_0, psnr_0 = _sample(run, 0, 2)
    err = rel(x_0, torch.cat(plain["x"], 0))
    between = rel(_sample(run, 1, 2)[0], x_0)
    print(f"noisy measurement: sample 0 vs plain run rel-L2 {err:.3e}; sample 1 vs sample 0 {between:.3e}")
    assert err < BAR and (psnr_0 - torch.cat(plain["psnr"])).abs().max() < 1e-3
    assert between > 1e-3


def test_mask_bank(hip, tmp_path):
    """A bank of two masks (3-D mask.npy), --deg inpainting, three images, K = 2: image i keeps mask i % 2 in every
    sample; sample 0 is the plain bank run."""
    _mini_yaml(tmp_path)
    rng = np.random.default_rng(4)
    masks = np.stack([(rng.random((64, 64)) < 0.5), (rng.random((64, 64)) < 0.25)]).astype(np.float32)
    os.makedirs(tmp_path / "exp" / "inp_masks", exist_ok=True)
    np.save(tmp_path / "exp" / "inp_masks" / "mask.npy", masks)
    argv = ["--path_y", "synthetic:3", "--eta", "0.85", "--sigma_y", "0.", "--deg", "inpainting"]
    run = _run(str(tmp_path), "k2", argv, samples=2)
    plain = _run(str(tmp_path), "plain", argv)
    assert run["calls"] == [2] and plain["calls"] == [1]
    x_0, psnr_0 = _sample(run, 0, 2)
    err = rel(x_0, torch.cat(plain["x"], 0))
    print(f"mask bank: sample 0 vs plain bank run rel-L2 {err:.3e}")
    assert err < BAR and (psnr_0 - torch.cat(plain["psnr"])).abs().max() < 1e-3
    # both samples agree with the measurement where image 1's mask (mask 1) keeps the pixel
    kept = torch.from_numpy(masks[1] != 0).cuda()
    x_1 = _sample(run, 1, 2)[0]
    assert rel(x_1[1][:, kept], x_0[1][:, kept]) < 1e-5 and rel(x_1[1][:, ~kept], x_0[1][:, ~kept]) > 1e-3


def _run_cli(tmp_path, nproc, folder, n_images):
    """`main.py` under torch.distributed.run (gloo, the ranks sharing this GPU), a fresh child per run, as
    tests/test_gpu_fuse.py::_run_cli does."""
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, DDNM_RANDOM_WEIGHTS="1", DDNM_DIST_BACKEND="gloo", PYTHONPATH=root, DDNM_SAMPLES="2")
    for name in ("DDNM_FUSE_BATCHES", "DDNM_NOISE", "DDNM_METRICS"):
        env.pop(name, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(root, "main.py"), "--ni", "--config", "mini.yml",
           "--path_y", f"synthetic:{n_images}", "--eta", "0.85", "--deg", "sr_averagepooling", "--deg_scale", "4",
           "--sigma_y", "0.", "-i", folder]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout, _read(os.path.join(tmp_path, "exp", "image_samples", folder))


@pytest.mark.parametrize("mode,batch,n_images", [("split", 2, 4), ("deal", 1, 3)])
def test_two_ranks_match_one_rank(hip, tmp_path, mode, batch, n_images):
    """K = 2 on two ranks -- split mode (each rank restores its images for both samples; one gather of [b][K * chw] per
    batch) and deal mode (whole batches per rank, the sums reduced) -- against the one-rank run: the same files, every
    PNG within one grey level on fewer than 1e-3 of its pixels, the totals within 0.01 dB."""
    _mini_yaml(tmp_path, batch=batch)
    out1, png1 = _run_cli(tmp_path, 1, "one", n_images)
    out2, png2 = _run_cli(tmp_path, 2, "two", n_images)
    want = sorted([f"{i}_{k}.png" for i in range(n_images) for k in range(2)] +
                  [f"{d}/{d}_{i}.png" for d in ("mean", "std") for i in range(n_images)] +
                  [f"Apy/{p}_{i}.png" for p in ("Apy", "orig") for i in range(n_images)])
    assert sorted(png1) == sorted(png2) == want
    for n in want:
        a, b = png1[n], png2[n]
        assert np.abs(a - b).max() <= 1 and (a != b).mean() < 1e-3, n
    for out in (out1, out2):
        assert f"Number of samples: {n_images}" in out and "Samples per image: 2" in out, out[-2000:]
    for head in ("Total Average PSNR:", "Total Average Mean-of-K PSNR:", "Total Average Sample PSNR:"):
        t1, t2 = (float(o.split(head)[1].split()[0]) for o in (out1, out2))
        assert abs(t1 - t2) <= 0.01, (head, t1, t2)
    s1, s2 = (float(o.split("Total Average Std:")[1].split()[0]) for o in (out1, out2))
    assert s1 > 0 and abs(s1 - s2) <= 1.01e-4          # printed with four decimals: one unit of rounding
