"""Dynamic range INSIDE one launch of the split-fp16 convolutions (conv_igemm_f16.hip <SPLIT>, conv_gather_s16.hip,
conv_s16_subpixel.hip) on the GPU: outlier activation channels and weight rows whose norms differ by 1e3 ... 2^20, judged per
OUTPUT CHANNEL -- a whole-tensor L2 norm hides a few channels that lost three digits.

Every case runs the split launch, the exact-fp32 MFMA launch (the same call without `weight_s16`) and an fp64 evaluation on the
device, and holds the split launch to the documented error model (tests/s16_model.py, pinned on the CPU by
tests/test_s16_dynamic_range_host.py): channels the model puts in the RELATIVE regime must be within 2x of the fp32 kernel's own
error, channel by channel; channels in the ABSOLUTE regime get the fp32 kernel's error plus the model's bound and nothing else.
Operands come from the seeded CPU generators of the model module, so the host test judged the very same numbers.

The persistent form (conv_s16_persist.hip) is not repeated here: tests/test_gpu_s16.py::
test_persistent_split_kernel_equals_the_one_tile_kernel pins it bit for bit to the one-tile kernel these cases run.

At the model level the loader's weight-range guard (Model._guard_weight_range) is checked to leave `spec` weights alone and to
send exactly the layers with outlier columns to the fp32 kernel.  Run with -s for the measured ratios and tier counts."""
import pytest
import torch

from tests import s16_model as sm

pytestmark = pytest.mark.gpu

DEV = "cuda"
GATHER_FORMS = ("down", "qkv_1x1_gn", "nin_1x1_concat", "level8_gn")


def _launch(t, split, amax, subpixel=False):
    from ddnm_amd import ops
    w, wsk = t["w"], t["wsk"]
    cout, k = w.shape[0], w.shape[-1]
    s16 = None
    if subpixel:
        s16 = ops.upsample_weight_s16(w)
    elif split:
        scale = ops.s16_weight_scale(*([w] + ([wsk] if wsk is not None else [])))
        s16 = (ops.pack_conv_weight_s16(w, scale), scale, ops.pack_conv_weight_s16(wsk, scale) if wsk is not None else None)
    B, H, W = t["a"].shape[:3]
    Ho, Wo = (2 * H, 2 * W) if t["ups"] else (H // t["stride"], W // t["stride"])
    return ops.conv2d(t["a"], ops.pack_conv_weight(w), cout, k, src1=t["b"], bias=t["bias"], res=t["res"],
                      gn=None if t["sc"] is None else (t["sc"], t["sh"]), gn_silu=t["gn_silu"], badd=t["badd"],
                      badd_stride=(cout if t["badd"] is not None else 0), ups=t["ups"], stride=t["stride"],
                      pad=(0 if t["stride"] == 2 else k // 2), out_hw=(Ho, Wo), emit_stats=True, weight_s16=s16,
                      skip=None if t["sk"] is None else (t["sk"], None),
                      skip_weight=ops.pack_skip_weight(wsk) if wsk is not None else None,
                      raw_amax=amax if s16 is not None else None, ups_subpixel=subpixel)


def _assert_route(c, t):
    """The case takes the kernel it is meant for, by the project's own predicates."""
    from ddnm_amd import ops
    B, H, W = t["a"].shape[:3]
    cin, cout, k = t["w"].shape[1], t["w"].shape[0], t["w"].shape[-1]
    if c["form"] in GATHER_FORMS:
        assert ops.conv_runs_s16_gather(B, H, W, cin, cout, ksize=k, stride=t["stride"])
        assert not (k == 3 and t["stride"] == 1 and ops.conv_runs_s16(B, H, W, cin, cout))
    elif c["form"] == "ups":
        assert ops.conv_runs_s16(B, 2 * H, 2 * W, cin, cout) and ops.conv_runs_ups_subpixel(B, H, W, cin, cout)
    else:
        assert ops.conv_runs_s16(B, H, W, cin, cout)
        if t["sk"] is not None:
            assert ops.conv_fuses_skip(B, H, W, cin, cout)


def _per_channel(out, y):
    """(r[o], e[o]): L2 error over (b, y, x) relative to the reference channel's norm, and unnormalised."""
    e = (out.double() - y).pow(2).sum((0, 1, 2)).sqrt()
    return e / y.pow(2).sum((0, 1, 2)).sqrt(), e


def _stats_errors(act, B):
    """GroupNorm partials against fp64 sums of the launch's own output: (the whole-tensor figure of tests/test_gpu_s16.py, the
    same per (image, channel), each channel normalised by its own size max(|s1|, sqrt(n s2)) resp. s2)."""
    o = act.t.double()
    n = o.shape[1] * o.shape[2]
    st = act.stats.view(B, act.tiles, -1, 2).double().sum(1)
    s1, s2 = o.sum((1, 2)), (o * o).sum((1, 2))
    d1, d2 = (st[..., 0] - s1).abs(), (st[..., 1] - s2).abs()
    whole = max((d1.max() / s1.abs().max()).item(), (d2.max() / s2.abs().max()).item())
    own = torch.maximum(s1.abs(), (n * s2).sqrt())
    live = s2 > 0
    chan = max((d1[live] / own[live]).max().item(), (d2[live] / s2[live]).max().item())
    return whole, chan


def _judge(label, act16, act32, y, bound, mag, B):
    """Assertions 1-5 of one split launch; returns (r16, relative-regime mask) for the sub-pixel comparison."""
    assert torch.isfinite(act16.t).all(), label
    rel = sm.channel_tiers(bound, mag)
    n, n_rel = rel.numel(), int(rel.sum())
    r16, e16 = _per_channel(act16.t, y)
    r32, e32 = _per_channel(act32.t, y)
    rmsb = bound.pow(2).sum((0, 2, 3)).sqrt()
    rel16 = ((act16.t.double() - y).norm() / y.norm()).item()
    rel32 = ((act32.t.double() - y).norm() / y.norm()).item()
    worst_rel = (r16 / r32)[rel].max().item() if n_rel else float("nan")
    worst_abs = (e16 / (2 * e32 + rmsb))[~rel].max().item() if n_rel < n else float("nan")
    stats = _stats_errors(act16, B) if act16.stats is not None else (float("nan"),) * 2
    print(f"{label}: tiers {n_rel} relative / {n - n_rel} absolute of {n}; worst r16/r32 (relative) {worst_rel:.3f}; "
          f"worst e16/(2 e32 + rmsb) (absolute) {worst_abs:.3f}; rel16 {rel16:.3e} rel32 {rel32:.3e}; "
          f"partials whole {stats[0]:.2e} per-channel {stats[1]:.2e}")
    if n_rel == n:
        assert rel16 <= 1.25 * rel32 + 2e-8, (label, rel16, rel32)
    assert bool((r16[rel] <= 2 * r32[rel]).all()), (label, worst_rel)
    assert bool((e16[~rel] <= 2 * e32[~rel] + rmsb[~rel]).all()), (label, worst_abs)
    if act16.stats is not None:
        assert act16.tiles > 0 and stats[0] < 2e-6 and stats[1] < 2e-6, (label, stats)
    return r16, rel


@pytest.mark.parametrize("c", sm.CASES, ids=lambda c: c["id"])
def test_split_launch_with_dynamic_range_inside_the_launch(c):
    """Measured on the MI355X (worst r16/r32 over relative-regime channels | worst e16/(2 e32 + rmsb) over absolute-regime
    channels): see DESIGN.md 3.0."""
    from ddnm_amd import ops
    t = sm.to(sm.build_case(c), DEV)
    B = t["a"].shape[0]
    _assert_route(c, t)
    raws = sm.raw_operands(t)
    amax = ops.amax_bound(*raws) if raws else None               # what the launch is given: an INPUT of the model
    amax_img = amax.view(B, ops.AMAX_N).amax(1).cpu() if raws else None
    y = sm.ref64(t)
    act32 = _launch(t, False, None)
    act16 = _launch(t, True, amax)
    bound, mag = sm.layer_bound(t, amax_img)
    r16, rel = _judge(c["id"], act16, act32, y, bound, mag, B)
    if c["form"] == "ups":
        sub = _launch(t, True, amax, subpixel=True)
        bound_s, mag_s = sm.layer_bound(t, amax_img, subpixel=True)
        r_sub, rel_s = _judge(c["id"] + " sub-pixel", sub, act32, y, bound_s, mag_s, B)
        assert sub.tiles == 4 * t["a"].shape[1] * t["a"].shape[2] // 256
        both = rel & rel_s                                        # one extra rounding of the pre-summed weights (test_gpu_s16_subpixel.py)
        print(f"{c['id']}: worst r_sub/r_ups over {int(both.sum())} channels {(r_sub / r16)[both].max().item():.3f}")
        assert bool((r_sub[both] <= 2 * r16[both]).all())


def _model_pair(sd):
    from oracle import cases
    from ddnm_amd.guided_diffusion.models import Model
    cfg = cases.weights.celeba_config(resolution=64, ch=128, ch_mult=(1, 2, 2), attn_resolutions=(16,))
    a, b = Model(cfg, device=DEV, split16=True), Model(cfg, device=DEV, split16=False)
    sd = sd(a)
    a.load_state_dict(sd)
    b.load_state_dict(sd)
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(4, 3, 64, 64, device=DEV, generator=g)
    t = torch.tensor([999.0, 500.0, 37.0, 0.0], device=DEV)
    ea, eb = a(x, t), b(x, t)
    assert torch.isfinite(ea).all()
    return a, ((ea - eb).double().norm() / eb.double().norm()).item()


def test_model_with_spec_weight_rows_keeps_every_split_launch():
    """Rows of every convolution rescaled over 1e-3 ... 1e1: inside the tested range, so nothing leaves the split engine."""
    a, d = _model_pair(lambda m: sm.spec_state_dict(m.random_state_dict(seed=7), 0))
    print(f"spec rows: split vs fp32-MFMA engine {d:.3e}")
    assert a.s16_dropped == []
    assert any(k.endswith(".s16") for k in a.w) and any(k.endswith(".s16_subpixel") for k in a.w)
    assert d < 3e-6


def test_model_with_outlier_weight_columns_sends_those_layers_to_the_fp32_kernel():
    """The same weights plus outlier columns in a conv1 and an upsample convolution: exactly those lose their split packings
    (Model._guard_weight_range; without the guard `s16_dropped` stays empty and this test fails)."""
    a, d = _model_pair(lambda m: sm.spec_state_dict(m.random_state_dict(seed=7), 0, sm.OUTLIER_LAYERS))
    print(f"spec rows + outlier columns in {sm.OUTLIER_LAYERS}: dropped {a.s16_dropped}; split vs fp32-MFMA engine {d:.3e}")
    assert sorted(a.s16_dropped) == sorted(sm.OUTLIER_LAYERS)
    for n in sm.OUTLIER_LAYERS:
        assert n + ".s16" not in a.w and n + ".s16_subpixel" not in a.w
    assert "up.2.upsample.conv.s16" in a.w and "down.1.block.0.conv2.s16" in a.w
    assert d < 3e-6
