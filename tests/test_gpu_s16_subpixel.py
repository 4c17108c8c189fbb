"""Sub-pixel form of the split-fp16 upsample convolution (ddnm_amd/csrc/conv_s16_subpixel.hip, ddnm_conv3x3_s16_f32 with
DDNM_CONV_UPS_SUBPIXEL) on the GPU: against an fp64 evaluation of `nearest x2 -> conv3x3` and against the unchanged `ups` launch
of the 3x3 kernels on the same inputs, GroupNorm partials included, and at the model level against the switch turned off."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"

# B, low-resolution H, W, Cin, Cout
CASES = [
    (2, 8, 32, 64, 128),      # one tile per image and workgroup: every border inside the tile, two chunks
    (5, 64, 64, 96, 128),     # 320 tiles over 256 workgroups: some walk two tiles (deferred epilogue, next-tile prefetch), a MID chunk
    (1, 32, 64, 64, 256),     # several 64-channel blocks per row phase
]


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _stats_err(act, B):
    """Summed partials vs fp64 sums over the launch's own output (the quantity and normalisation of tests/test_gpu_s16.py)."""
    o = act.t.double()
    st = act.stats.view(B, act.tiles, -1, 2).double().sum(1)
    s1, s2 = o.sum((1, 2)), (o * o).sum((1, 2))
    return max(((st[..., 0] - s1).abs().max() / s1.abs().max()).item(), ((st[..., 1] - s2).abs().max() / s2.abs().max()).item())


@pytest.mark.parametrize("case", CASES)
def test_subpixel_launch_vs_fp64_and_the_ups_launch(case):
    from ddnm_amd import ops
    B, H, W, cin, cout = case
    assert ops.conv_runs_ups_subpixel(B, H, W, cin, cout)
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(B, H, W, cin, device=DEV, generator=g) * 1.5
    w = torch.randn(cout, cin, 3, 3, device=DEV, generator=g) / (3.0 * cin ** 0.5)
    bias = torch.randn(cout, device=DEV, generator=g)
    y = F.conv2d(F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), w.double(), bias.double(),
                 padding=1).permute(0, 2, 3, 1)
    sc = ops.s16_weight_scale(w)
    old = ops.conv2d(x, ops.pack_conv_weight(w), cout, 3, bias=bias, ups=True, emit_stats=True,
                     weight_s16=(ops.pack_conv_weight_s16(w, sc), sc, None))
    new = ops.conv2d(x, ops.pack_conv_weight(w), cout, 3, bias=bias, ups=True, emit_stats=True,
                     weight_s16=ops.upsample_weight_s16(w), ups_subpixel=True)
    torch.cuda.synchronize()
    assert new.t.shape == old.t.shape == y.shape
    e_old, e_new = _rel(old.t, y), _rel(new.t, y)
    print(f"case {case}: rel-L2 vs fp64: ups launch {e_old:.3e}, sub-pixel {e_new:.3e}; new vs old {_rel(new.t, old.t):.3e}")
    assert e_old < 8e-7                                             # the yardstick itself is fp32-grade (tests/test_gpu_s16.py)
    # one extra rounding of the pre-summed weights and a different summation order
    assert e_new <= 2.0 * e_old, (e_new, e_old)
    assert new.stats is not None and new.tiles == 4 * H * W // 256  # one partial row per (low-resolution tile, py, px)
    s_new = _stats_err(new, B)
    print(f"case {case}: GroupNorm partials vs fp64 sums of the output: {s_new:.3e}")
    assert s_new < 2e-6


def test_flagged_launch_that_does_not_qualify_is_an_error():
    from ddnm_amd import ops
    x = torch.randn(1, 8, 16, 64, device=DEV)                       # low-resolution W = 16: no 32-wide tile
    w = torch.randn(64, 64, 3, 3, device=DEV) * 0.05
    assert not ops.conv_runs_ups_subpixel(1, 8, 16, 64, 64)
    with pytest.raises(ValueError):
        ops.conv2d(x, ops.pack_conv_weight(w), 64, 3, ups=True, weight_s16=ops.upsample_weight_s16(w), ups_subpixel=True)


def test_full_model_switch_on_vs_off_is_closer_than_split_vs_fp32_engine():
    from oracle import cases
    from ddnm_amd.guided_diffusion.models import Model
    cfg, _ = cases.celeba_net("full")
    a, b = Model(cfg, device=DEV, split16=True), Model(cfg, device=DEV, split16=False)
    sd = a.random_state_dict(seed=7)
    a.load_state_dict(sd)
    b.load_state_dict(sd)
    assert any(k.endswith(".s16_subpixel") for k in a.w) and not any(k.endswith(".s16_subpixel") for k in b.w)
    r = cfg.data.image_size
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(2, 3, r, r, device=DEV, generator=g)
    t = torch.tensor([999.0, 37.0], device=DEV)
    from ddnm_amd import ops
    outs = {}
    for mode in ("all", "1", "0"):
        a.ups_subpixel = mode
        kt = ops.KernelTimer()
        ops.set_kernel_timer(kt)
        try:
            outs[mode] = a(x, t).clone()
        finally:
            ops.set_kernel_timer(None)
        outs[mode + "/n"] = sum(1 for rec in kt.records if rec[0].startswith("conv2x2x4_s16_subpixel"))
    e32 = b(x, t)
    assert outs["all/n"] >= outs["1/n"] >= 1 and outs["0/n"] == 0, {k: v for k, v in outs.items() if k.endswith("/n")}
    d_engine = _rel(outs["0"], e32)
    for mode in ("all", "1"):
        d_switch = _rel(outs[mode], outs["0"])
        print(f"DDNM_UPS_SUBPIXEL={mode} ({outs[mode + '/n']} launches) vs 0: {d_switch:.3e}; split-fp16 vs fp32-MFMA engine: {d_engine:.3e}")
        assert d_switch < d_engine, (mode, d_switch, d_engine)
