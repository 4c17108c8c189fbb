"""Slices-on-waves form of the split-fp16 3x3 convolutions of the 8 x 8 level (ddnm_amd/csrc/conv_s16_wslice.hip, reached through
ddnm_conv_gather_s16_f32) on the GPU, at the smallest shapes that still walk every path of the kernel: 8 slices of equal and of
unequal length, fewer slices than waves, the four summation orders of the statistics tiles, a concat whose source boundary is a
chunk edge, GroupNorm affine with and without swish, a raw operand with its range guard, every epilogue term with and without
statistics (the two associations of the reduction launches it replaces), and the plans it must leave to the gather kernel.
Bars are the family's (tests/test_gpu_s16.py, gather cases): against torch fp64 the split result is fp32-grade and no worse than
the fp32 MFMA kernel, the emitted GroupNorm partials are the sums of the output.  Every case asserts what the query
(ddnm_conv_gather_s16_wslice) says about the launch and compares it with the gather kernel plus its reduction launch on the same
inputs (`one_tile=True` keeps the launch there): the two are equal bit for bit, output and statistics."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
H = 8


def _routes(B, C0, C1, Cout, stats, one_tile=False, H=H):
    from ddnm_amd import _lib
    d = _lib.ConvDesc()
    d.B, d.Hin, d.Win, d.C0, d.C1, d.Cout = B, H, H, C0, C1, Cout
    d.ksize, d.stride, d.pad, d.Ho, d.Wo = 3, 1, 1, H, H
    d.flags = 1 if one_tile else 0
    if stats:
        d.stats_out = 16                   # only compared with NULL by the query
    return _lib.lib().ddnm_conv_gather_s16_wslice(ctypes.byref(d))


# name: B, C0, C1, Cout, gn, silu, res, stats, badd (None / "row" = stride 0 / "image" = one row per image), image scales, routed
CASES = {
    # 1. ksplit = 8: 8 chunks on 8 slices; 12 chunks on 8 slices of 1 or 2 chunks (statistics of Cout 512: 2 pixel rows)
    "even8": (1, 256, 0, 64, True, True, False, True, None, None, 1),
    "uneven8_rows2": (8, 384, 0, 512, True, True, True, True, "image", None, 1),
    # 2. statistics summed in the orders of 1, 3 and >= 4 pixel rows of the reduction pass (256 / (Cout / 4))
    "rows1": (1, 256, 0, 576, True, False, True, True, None, None, 1),
    "rows3": (1, 256, 0, 320, True, True, True, True, "row", None, 1),
    "rows4": (1, 256, 0, 64, True, False, True, True, "row", None, 1),
    # 3. src0 || src1 with the source boundary at a chunk edge: 3 chunks on 3 slices, five waves without a slice
    "concat": (2, 64, 32, 64, True, True, False, True, None, None, 1),
    # 4. raw operand with its bound: one launch, image 0 scaled by 1e5 and image 1 by 1e-5
    "range": (2, 256, 0, 64, False, False, False, True, None, (1e5, 1e-5), 1),
    # 5. no statistics: the association of conv_splitk_reduce_kernel, every term
    "plain_res_badd_image": (2, 256, 0, 128, True, True, True, False, "image", None, 1),
    "plain_badd_row": (1, 256, 0, 64, True, True, False, False, "row", None, 1),
    "plain_bias_only": (1, 256, 0, 64, True, False, False, False, None, None, 1),
    # 6. plans the kernel cannot hold stay on the gather kernel: 12 slices, one slice
    "fallback_ksplit12": (1, 384, 0, 64, True, True, True, True, None, None, 0),
    "fallback_ksplit1": (1, 32, 0, 64, True, True, True, True, None, None, 0),
}
STATS_TILES = 16                           # per image, split plans: hw / 4

_cache = {}


def _case(name):
    """Inputs, the fp64 evaluation and the launches (new route twice, gather route, fp32 MFMA kernel) of a case, once."""
    if name in _cache:
        return _cache[name]
    from ddnm_amd import ops
    B, C0, C1, Cout, gn, silu, res, stats, badd, scales, _ = CASES[name]
    g = torch.Generator(device=DEV).manual_seed(29)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    cin = C0 + C1
    a, b = rn(B, H, H, C0) * 1.5, (rn(B, H, H, C1) * 1.5 if C1 else None)
    if scales is not None:
        a = a * torch.tensor(scales, device=DEV)[:, None, None, None]
    w = rn(Cout, cin, 3, 3) / (3 * cin ** 0.5)
    bias = rn(Cout)
    sc, sh = (rn(B, cin) * 0.3 + 1.0, rn(B, cin) * 0.3) if gn else (None, None)
    r = rn(B, H, H, Cout) * 2.0 if res else None
    ba = None if badd is None else (rn(Cout) if badd == "row" else rn(B, Cout))
    if scales is not None:                 # keep every term of an image on the image's scale (the bars are relative)
        bias = None
    # fp64 evaluation
    x = (a if b is None else torch.cat([a, b], 3)).double()
    if gn:
        x = x * sc.double()[:, None, None, :] + sh.double()[:, None, None, :]
        if silu:
            x = x * torch.sigmoid(x)
    y = F.conv2d(x.permute(0, 3, 1, 2), w.double(), None if bias is None else bias.double(), padding=1).permute(0, 2, 3, 1)
    if ba is not None:
        y = y + (ba.double() if badd == "row" else ba.double()[:, None, None, :])
    if res:
        y = y + r.double()
    w32, s = ops.pack_conv_weight(w), ops.s16_weight_scale(w)
    s16 = (ops.pack_conv_weight_s16(w, s), s, None)
    amax = None if gn else ops.amax_bound(a, b)

    def launch(split, one_tile=False):
        o = ops.conv2d(a, w32, Cout, 3, src1=b, bias=bias, badd=ba, badd_stride=(Cout if badd == "image" else 0), res=r,
                       gn=(sc, sh) if gn else None, gn_silu=silu, emit_stats=stats, weight_s16=s16 if split else None,
                       raw_amax=amax if split else None, one_tile=one_tile)
        return o if stats else ops.Act(o)
    assert ops.conv_runs_s16_gather(B, H, H, cin, Cout, ksize=3)
    _cache[name] = dict(y=y, new=launch(True), new2=launch(True), old=launch(True, one_tile=True), f32=launch(False),
                        stats=stats, shape=(B, C0, C1, Cout))
    return _cache[name]


def _rel(o, y):
    return ((o.double() - y).norm() / y.norm()).item()


@pytest.mark.parametrize("name", list(CASES))
def test_new_route_vs_fp64_fp32_kernel_and_gather_route(name):
    c = _case(name)
    B, C0, C1, Cout = c["shape"]
    assert _routes(B, C0, C1, Cout, c["stats"]) == CASES[name][-1]            # the launch under test takes the form it should ...
    assert _routes(B, C0, C1, Cout, c["stats"], one_tile=True) == 0           # ... and its partner is the gather kernel
    y, new, old, f32 = c["y"], c["new"].t, c["old"].t, c["f32"].t
    for i in range(B):                     # per image (the `range` case: the images differ by 1e10)
        e_new, e_f32, e_old = _rel(new[i], y[i]), _rel(f32[i], y[i]), _rel(old[i], y[i])
        print(f"{name} image {i}: rel-L2 vs fp64: slices on waves {e_new:.3e}, gather route {e_old:.3e}, fp32 MFMA {e_f32:.3e}; "
              f"slices on waves vs gather route {_rel(new[i], old[i].double()):.3e}")
        assert e_new < 8e-7, (name, i, e_new)
        assert e_new <= 1.25 * e_f32 + 2e-8, (name, i, e_new, e_f32)
    # equal, not close: the same products in the same order per element, the slices added in slice order, the epilogue terms
    # and the statistics in the association of the reduction pass (the runner replay pins outputs bit for bit)
    assert torch.equal(new, old), name
    if c["stats"]:
        assert torch.equal(c["new"].stats, c["old"].stats), name


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[7] and c[-1]])
def test_statistics_fill_the_layout_python_sized(name):
    c = _case(name)
    B, _, _, Cout = c["shape"]
    for act in (c["new"], c["old"]):       # the layout is the plan's: the same for both routes
        assert act.stats is not None and act.tiles == STATS_TILES, (name, act.tiles)
    act = c["new"]
    o = act.t.double()
    st = act.stats.view(B, act.tiles, Cout, 2).double()
    grp = o.view(B, act.tiles, H * H // act.tiles, Cout)                      # the pixel group of every tile
    for k, ref in ((0, grp.sum(2)), (1, (grp * grp).sum(2))):
        tot, rtot = st[..., k].sum(1), ref.sum(1)
        for i in range(B):                 # per image (the `range` case)
            assert ((st[i, :, :, k] - ref[i]).abs().max() / ref[i].abs().max()).item() < 2e-6, (name, "per tile", k, i)
            assert ((tot[i] - rtot[i]).abs().max() / rtot[i].abs().max()).item() < 2e-6, (name, "total", k, i)


@pytest.mark.parametrize("name", ["uneven8_rows2", "concat", "plain_res_badd_image"])
def test_two_launches_are_bit_identical(name):
    c = _case(name)
    assert torch.equal(c["new"].t, c["new2"].t)
    if c["stats"]:
        assert torch.equal(c["new"].stats, c["new2"].stats)


def test_route_is_refused_where_the_kernel_has_no_form():
    assert _routes(8, 512, 0, 512, True) == 1 and _routes(8, 512, 512, 512, True) == 1      # the network's launches at B = 8
    assert _routes(4, 512, 0, 512, True) == 0                 # B = 4: the plan has 16 slices
    assert _routes(8, 512, 0, 512, True, H=16) == 0           # 16 x 16 images: not routed
    assert _routes(2, 256, 0, 96, False) < 0                  # Cout % 64: not in the family
