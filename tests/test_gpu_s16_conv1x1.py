"""GEMM form of the split-fp16 1x1 convolutions (ddnm_amd/csrc/conv1x1_s16.hip, reached through ddnm_conv_gather_s16_f32) on the
GPU: the attention blocks' qkv / proj_out and the un-fused nin_shortcut forms at the smallest shapes that still walk every path
of the kernel -- a ragged last K step, a source boundary inside a K step, Cout that is no multiple of 128, several M tiles per
image, both statistics layouts.  Bars are the family's (tests/test_gpu_s16.py, gather cases): against torch fp64 the split result
is fp32-grade and no worse than the fp32 MFMA kernel, the emitted GroupNorm partials are the sums of the output.  Every case
asserts that the launch is one the new route takes (ddnm_conv_gather_s16_gemm1x1) and compares it with the gather kernel on the
same inputs (`one_tile=True` keeps the launch on it): the two are equal bit for bit, output and statistics."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _routes(B, H, C0, C1, Cout, stats, one_tile=False, flags=0):
    from ddnm_amd import _lib
    d = _lib.ConvDesc()
    d.B, d.Hin, d.Win, d.C0, d.C1, d.Cout = B, H, H, C0, C1, Cout
    d.ksize, d.stride, d.pad, d.Ho, d.Wo = 1, 1, 0, H, H
    d.flags = flags | (1 if one_tile else 0)
    if stats:
        d.stats_out = 16                   # only compared with NULL by the query
    return _lib.lib().ddnm_conv_gather_s16_gemm1x1(ctypes.byref(d))


# name: B, C0, C1, Cout, H, gn, silu, res, stats, badd (None / "row" = stride 0 / "image" = one row per image), image scales
CASES = {
    # 1. qkv form: Cin = 3 sub-rows (ragged last K step), Cout = 3 x 64
    "qkv_affine": (1, 96, 0, 192, 8, True, False, False, False, None, None),
    "qkv_swish": (1, 96, 0, 192, 8, True, True, False, False, None, None),
    # 2. proj_out form: raw operand, residual, statistics; the plan splits K for the first two (4-pixel statistics tiles of
    #    the reduction pass) and not for the third (one chunk: 64-pixel tiles of the epilogue)
    "proj_16": (2, 64, 0, 64, 16, False, False, True, True, None, None),
    "proj_8": (2, 64, 0, 64, 8, False, False, True, True, None, None),
    "proj_16_unsplit": (2, 32, 0, 64, 16, False, False, True, True, None, None),
    #    the statistics of a split plan are summed in the order of the reduction pass, whose workgroup holds 256 / (Cout / 4)
    #    pixel rows: 3, 2 and 1 here (16 and 8 above), each its own order over the four pixels of a tile
    "proj_8_rows3": (1, 64, 0, 320, 8, False, False, True, True, None, None),
    "proj_8_rows2": (1, 64, 0, 512, 8, False, False, True, True, None, None),
    "proj_8_rows1": (1, 64, 0, 576, 8, False, False, True, True, None, None),
    # 3. shortcut form: src0 || src1 with the source boundary inside a 64-channel K step
    "shortcut_32_64": (2, 32, 64, 64, 16, False, False, False, False, None, None),
    "shortcut_96_32": (2, 96, 32, 64, 16, False, False, False, False, None, None),
    # 4. operand range: one launch, image 0 scaled by 1e5 and image 1 by 1e-5
    "range": (2, 96, 0, 64, 16, False, False, False, True, None, (1e5, 1e-5)),
    # 5. per-sample addend, one row for all images (stride 0) and one row per image
    "badd_row": (2, 64, 0, 128, 8, False, False, True, False, "row", None),
    "badd_image": (2, 64, 0, 128, 8, False, False, True, False, "image", None),
}
STATS_TILES = {"proj_16": 64, "proj_8": 16, "proj_16_unsplit": 4, "proj_8_rows3": 16, "proj_8_rows2": 16, "proj_8_rows1": 16,
               "range": 64}      # per image: hw / 4 (split plan), hw / 64

_cache = {}


def _case(name):
    """Inputs, the fp64 evaluation and the three launches (new route, gather kernel, fp32 MFMA kernel) of a case, once."""
    if name in _cache:
        return _cache[name]
    from ddnm_amd import ops
    B, C0, C1, Cout, H, gn, silu, res, stats, badd, scales = CASES[name]
    g = torch.Generator(device=DEV).manual_seed(23)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    cin = C0 + C1
    a, b = rn(B, H, H, C0) * 1.5, (rn(B, H, H, C1) * 1.5 if C1 else None)
    if scales is not None:
        a = a * torch.tensor(scales, device=DEV)[:, None, None, None]
    w = rn(Cout, cin, 1, 1) / cin ** 0.5
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
    y = F.conv2d(x.permute(0, 3, 1, 2), w.double(), None if bias is None else bias.double()).permute(0, 2, 3, 1)
    if ba is not None:
        y = y + (ba.double() if badd == "row" else ba.double()[:, None, None, :])
    if res:
        y = y + r.double()
    w32, s = ops.pack_conv_weight(w), ops.s16_weight_scale(w)
    s16 = (ops.pack_conv_weight_s16(w, s), s, None)
    amax = None if gn else ops.amax_bound(a, b)

    def launch(split, one_tile=False):
        o = ops.conv2d(a, w32, Cout, 1, src1=b, bias=bias, badd=ba, badd_stride=(Cout if badd == "image" else 0), res=r,
                       gn=(sc, sh) if gn else None, gn_silu=silu, emit_stats=stats, weight_s16=s16 if split else None,
                       raw_amax=amax if split else None, one_tile=one_tile)
        return o if stats else ops.Act(o)
    assert ops.conv_runs_s16_gather(B, H, H, cin, Cout, ksize=1)
    _cache[name] = dict(y=y, new=launch(True), new2=launch(True), old=launch(True, one_tile=True), f32=launch(False),
                        stats=stats, shape=(B, H, C0, C1, Cout))
    return _cache[name]


def _rel(o, y):
    return ((o.double() - y).norm() / y.norm()).item()


@pytest.mark.parametrize("name", list(CASES))
def test_new_route_vs_fp64_fp32_kernel_and_gather_kernel(name):
    c = _case(name)
    B, H, C0, C1, Cout = c["shape"]
    assert _routes(B, H, C0, C1, Cout, c["stats"]) == 1                       # the launch under test is the GEMM form ...
    assert _routes(B, H, C0, C1, Cout, c["stats"], one_tile=True) == 0        # ... and its partner the gather kernel
    y, new, old, f32 = c["y"], c["new"].t, c["old"].t, c["f32"].t
    for i in range(B):                     # per image (case 4: the images differ by 1e10)
        e_new, e_f32, e_old = _rel(new[i], y[i]), _rel(f32[i], y[i]), _rel(old[i], y[i])
        print(f"{name} image {i}: rel-L2 vs fp64: GEMM form {e_new:.3e}, gather kernel {e_old:.3e}, fp32 MFMA {e_f32:.3e}; "
              f"GEMM form vs gather kernel {_rel(new[i], old[i].double()):.3e}")
        assert e_new < 8e-7, (name, i, e_new)
        assert e_new <= 1.25 * e_f32 + 2e-8, (name, i, e_new, e_f32)
        # 7. both routes are within 8e-7 of fp64, so within 1.6e-6 of each other ...
        assert _rel(new[i], old[i].double()) < 1.6e-6, (name, i)
    # ... and in fact equal: the GEMM form adds in the gather route's order, slice by slice where that route splits K, and
    # its statistics in the order of that route's reduction pass (the runner replay pins outputs bit for bit)
    assert torch.equal(new, old), name
    if c["stats"]:
        assert torch.equal(c["new"].stats, c["old"].stats), name


@pytest.mark.parametrize("name", list(STATS_TILES))
def test_statistics_fill_the_layout_python_sized(name):
    c = _case(name)
    B, H, _, _, Cout = c["shape"]
    for act in (c["new"], c["old"]):       # the layout is the plan's: the same for both routes
        assert act.stats is not None and act.tiles == STATS_TILES[name], (name, act.tiles)
    act = c["new"]
    o = act.t.double()
    st = act.stats.view(B, act.tiles, Cout, 2).double()
    grp = o.view(B, act.tiles, H * H // act.tiles, Cout)                      # the pixel group of every tile
    for k, ref in ((0, grp.sum(2)), (1, (grp * grp).sum(2))):
        tot, rtot = st[..., k].sum(1), ref.sum(1)
        for i in range(B):                 # per image (the `range` case)
            assert ((st[i, :, :, k] - ref[i]).abs().max() / ref[i].abs().max()).item() < 2e-6, (name, "per tile", k, i)
            assert ((tot[i] - rtot[i]).abs().max() / rtot[i].abs().max()).item() < 2e-6, (name, "total", k, i)


@pytest.mark.parametrize("name", ["qkv_swish", "proj_16", "proj_16_unsplit", "shortcut_96_32"])
def test_two_launches_are_bit_identical(name):
    c = _case(name)
    assert torch.equal(c["new"].t, c["new2"].t)
    if c["stats"]:
        assert torch.equal(c["new"].stats, c["new2"].stats)


def test_route_is_refused_where_the_kernel_has_no_form():
    assert _routes(2, 16, 64, 0, 64, False) == 1
    assert _routes(2, 16, 512, 0, 64, False) == 1 and _routes(2, 16, 512, 32, 64, False) == 0      # K beyond the measured rule ...
    assert _routes(2, 16, 512, 512, 64, False, flags=4) == 1                 # ... which DDNM_CONV_GEMM1X1 overrides (A/B timing),
    assert _routes(2, 16, 512, 512, 64, False, flags=4, one_tile=True) == 0  # DDNM_CONV_ONE_TILE still wins,
    assert _routes(2, 16, 1024, 512, 64, False, flags=4) == 0                # and never beyond what one workgroup owns
    assert _routes(2, 32, 64, 0, 64, True) == 0               # split plan whose statistics tiles are 8 pixels
    assert _routes(2, 16, 64, 0, 96, False) < 0               # Cout % 64: not in the family
