"""Host half of the fp16-activation convolution edge tests (tests/conv16_model.py; the GPU half is
test_gpu_conv16_edges.py): every exact case of the table meets the conditions that make a bit-exact comparison legitimate,
every case lands on the plan cell its record names (asked of the library's host queries: no device), the table covers
every entry of COVERAGE below, the float64 reference agrees with an independent loop formulation, and the reference is
sensitive, in every pixel tile, to the addressing errors the GPU comparison is meant to catch.  A change to the planner
that moves a case off its cell fails here instead of silently turning a GPU test into a duplicate of another."""
import ctypes

import pytest
import torch

from tests import conv16_model as CM


@pytest.fixture(scope="module")
def plans():
    from ddnm_amd import build
    build.build()
    return {c.name: CM.plan_of(c) for c in CM.CASES}


def test_case_names_are_unique():
    assert len(CM.BY_NAME) == len(CM.CASES)
    assert len(CM.REAL_CASES) <= 6


@pytest.mark.parametrize("case", CM.CASES, ids=lambda c: c.name)
def test_case_lands_on_its_cell(plans, case):
    plan = plans[case.name]
    assert CM.cell_of(case, plan) == case.cell
    assert CM.tile_width_is_the_widest(case, plan)
    if case.skip:
        assert plan["kernel"] == "k9" and not case.ups              # what a fused shortcut needs
    if case.k == 1:
        # the documented tile rule agrees with the query wherever the query can see the tile (an unsplit copy whose tile
        # divides the image reports H W / (64 MT) statistics tiles)
        assert CM.gemm_tile_rule(case.B, case.H * case.W, case.Cout) == plan["MT"]
        assert case.gn == "none" and not case.ups
    if plan["ksplit"] > 1 and not plan["fin"]:
        assert plan["stats_tiles"] == CM.splitk_tiles(case)
    if case.fin:
        assert plan["fin"] == int(case.H * case.W <= 1024)           # the query declines images of more than 1024 pixels
    assert (plan["stats_tiles"] > 0) == (not case.out_nchw and not (case.k == 1 and plan["ksplit"] == 1
                                                                     and (case.H * case.W) % plan["BM"]))


@pytest.mark.parametrize("case", CM.EXACT_CASES, ids=lambda c: c.name)
def test_exactness_preconditions(plans, case):
    t = CM.make_inputs(case)
    plan = plans[case.name]
    assert CM.exactness_violations(case, t, plan) == []
    if case.gn == "affine":
        assert bool((t["shift"] != 0).all()) and bool((t["scale"] != 0).all())
        assert case.B == 1 or not torch.equal(t["scale"][0], t["scale"][1])
    ref = CM.reference(case, t)
    assert torch.equal(ref.half().double(), ref) or case.out_nchw
    if plan["ksplit"] > 1:                                           # the slices' partial sums add up to the products
        assert torch.equal(sum(CM.slice_partials(case, t, plan)), CM.conv_part(case, t))


@pytest.mark.parametrize("case", CM.REAL_CASES, ids=lambda c: c.name)
def test_real_cases_have_an_exact_affine(case):
    """Every operand is an fp16 number, scale * x + shift is an fp32 number inside the interval E_ACT was measured on."""
    t = CM.make_inputs(case)
    for name in ("x0", "x1", "w", "res"):
        assert t[name] is None or torch.equal(t[name].half().float(), t[name]), name
    x = t["x0"] if t["x1"] is None else torch.cat([t["x0"], t["x1"]], 1)
    v64 = CM.affine_arg(case, t)
    v32 = x * t["scale"][:, :, None, None] + t["shift"][:, :, None, None]
    assert torch.equal(v32.double(), v64)
    assert torch.equal((x * t["scale"][:, :, None, None]).double() + t["shift"].double()[:, :, None, None], v64)
    assert CM.V_RANGE[0] <= float(v64.min()) and float(v64.max()) <= CM.V_RANGE[1]
    assert case.k == 3 and not case.skip


# ----------------------------------------------------------------------------- the coverage list, as data
# (label, requirements on conv16_model.features(case, plan)).  "has": options that are on; every other key: equality.
# A third element (key, n): the matching cases take at least n distinct values of `key`.
COVERAGE = [
    # 3x3 unsplit
    ("MT2/TW32, one tile with all four borders", dict(kernel="k9", shape=(1, 4, 32, 64, 64), MT=2, TW=32, m_tiles=1, split=False)),
    ("MT2/TW32, seams on both axes", dict(kernel="k9", shape=(1, 8, 64, 64, 64), MT=2, TW=32, tiles_x=2, tile_rows=2)),
    ("MT2/TW16", dict(kernel="k9", shape=(1, 8, 16, 64, 64), MT=2, TW=16, split=False)),
    ("MT2/TW16, 2 x 3 tiles, Cout 192", dict(kernel="k9", shape=(1, 16, 48, 64, 192), MT=2, TW=16, tiles_x=3, tile_rows=2, cout_tail=192)),
    ("MT4/TW32 at the 200-tile threshold", dict(kernel="k9", shape=(1, 200, 256, 64, 64), MT=4, TW=32, m_tiles=200)),
    ("... and 192 tiles stay on MT2", dict(kernel="k9", shape=(1, 192, 256, 64, 64), MT=2, m_tiles=384)),
    ("MT4/TW16", dict(kernel="k9", shape=(1, 240, 240, 64, 64), MT=4, TW=16)),
    ("n128/TW32", dict(kernel="n128", shape=(1, 200, 256, 64, 128), TW=32)),
    ("n128/TW16, two chunks", dict(kernel="n128", shape=(1, 240, 240, 128, 128), TW=16, nchunks=2)),
    ("... with a fused shortcut: conv16_kernel<9,4,4>", dict(kernel="k9", MT=4, shape=(1, 240, 240, 128, 128), has=("skip",))),
    ("... with Cout 256: conv16_kernel<9,4,4>", dict(kernel="k9", MT=4, shape=(1, 240, 240, 128, 256))),
    ("unsplit 3x3: affine + concat", dict(kernel="k9", split=False, has=("gn", "concat"))),
    ("unsplit 3x3: nearest x2 + affine, non-square", dict(kernel="k9", split=False, has=("gn", "ups"), square=False)),
    ("unsplit 3x3: res_ups + shortcut over a concat", dict(kernel="k9", split=False, has=("res_ups", "skip"))),
    ("n128: affine + concat", dict(kernel="n128", has=("gn", "concat"))),
    ("n128: residual", dict(kernel="n128", has=("res",))),
    # channel tiles and workgroup order
    ("two channel tiles, wmajor: Cout 320", dict(shape=(1, 32, 32, 64, 320), n_tiles=2, wmajor=1, cout_tail=64)),
    ("two channel tiles, wmajor: Cout 512", dict(shape=(1, 16, 16, 128, 512), n_tiles=2, wmajor=1)),
    ("two channel tiles, pixel-major", dict(shape=(2, 32, 32, 64, 320), n_tiles=2, wmajor=0)),
    ("grid of 1", dict(grid=1)), ("grid of 3", dict(grid=3)), ("grid of 6", dict(grid=6)), ("grid of 9", dict(grid=9)),
    # 3x3 split
    ("ks2", dict(kernel="k9", shape=(1, 8, 16, 256, 64), ksplit=2, slab=16, opts=frozenset({"bias"}))),
    ("5 chunks over 2", dict(kernel="k9", shape=(1, 8, 16, 320, 64), ksplit=2, uneven_slices=True, C0=320)),
    ("... with the concat boundary inside slice 1", dict(kernel="k9", shape=(1, 8, 16, 320, 64), C0=192, concat_inside_slice=True)),
    ("7 chunks over 3, 192-channel reduction slab", dict(kernel="k9", shape=(1, 8, 16, 448, 192), ksplit=3, uneven_slices=True)),
    ("ks8: the last fp16-slab split", dict(kernel="k9", shape=(1, 8, 16, 1024, 64), ksplit=8, slab=16)),
    ("ks9: the first fp32-slab split", dict(kernel="k9", shape=(1, 8, 16, 1152, 64), ksplit=9, slab=32, opts=frozenset({"bias"}))),
    ("ks32: the cap", dict(kernel="k9", shape=(1, 16, 16, 4096, 64), ksplit=32, slab=32)),
    ("ks4 with a two-chunk shortcut: two idle slices", dict(kernel="k9", shape=(2, 16, 16, 512, 128), ksplit=4, skip_idle_slices=2)),
    ("split: res", dict(kernel="k9", split=True, fin=0, has=("res",))),
    ("split: res_ups", dict(kernel="k9", split=True, fin=0, has=("res_ups",))),
    ("split: ups", dict(kernel="k9", split=True, has=("ups",))),
    ("split: affine", dict(kernel="k9", split=True, has=("gn",))),
    ("split: Cout 320, reduction slabs of 256 + 64", dict(kernel="k9", split=True, Cout=320, fin=0)),
    # fin
    ("fin: Cout 128, slabs of 16", dict(fin=1, Cout=128, fin_slab=16)),
    ("fin: Cout 256, slabs of 16", dict(fin=1, Cout=256, fin_slab=16, k=3)),
    ("fin: Cout 384, slabs of 24", dict(fin=1, Cout=384, fin_slab=24)),
    ("fin: Cout 1024, slabs of 32", dict(fin=1, Cout=1024, fin_slab=32)),
    ("fin: FiLM", dict(fin=1, has=("film",))),
    ("fin: res_ups", dict(fin=1, has=("res_ups",))),
    ("fin: fp32 slabs", dict(fin=1, slab=32)),
    ("fin: the GEMM form", dict(fin=1, k=1)),
    ("fin declined at 2048 pixels", dict(fin=0, fin_asked=True, pixels=2048, split=True)),
    # 1x1
    ("1x1 MT4 ragged: 64 of 256 rows", dict(kernel="k1", shape=(1, 8, 8, 64, 64), MT=4, rows_last=64, stats_tiles=0)),
    ("1x1 MT4 ragged: 100 rows", dict(kernel="k1", shape=(1, 10, 10, 128, 64), MT=4, rows_last=100, stats_tiles=0)),
    ("1x1 MT1 whole tiles", dict(kernel="k1", shape=(3, 8, 8, 64, 64), MT=1, ragged=False, stats_tiles=1)),
    ("1x1 MT1 ragged + ks2 + fp16 slabs", dict(kernel="k1", shape=(2, 5, 13, 256, 64), MT=1, ragged=True, ksplit=2, slab=16)),
    ("1x1 MT4 ragged + ks18 + fp32 slabs", dict(kernel="k1", shape=(1, 8, 8, 2304, 256), MT=4, ragged=True, ksplit=18, slab=32, fin=0)),
    ("1x1 MT2 whole tiles", dict(kernel="k1", shape=(5, 64, 64, 64, 64), MT=2, ragged=False)),
    ("1x1 MT2 ragged last tile", dict(kernel="k1", shape=(1, 129, 129, 64, 64), MT=2, ragged=True, stats_tiles=0)),
    ("1x1 MT4 whole tiles", dict(kernel="k1", shape=(13, 64, 64, 64, 64), MT=4, ragged=False)),
    ("1x1 MT1, 12 channel tiles, wmajor", dict(kernel="k1", shape=(3, 8, 8, 1024, 3072), MT=1, n_tiles=12, wmajor=1)),
    ("1x1 with a residual: unsplit and split", dict(kernel="k1", has=("res",)), ("split", 2)),
    ("1x1 split with res_ups (the reduction maps it)", dict(kernel="k1", split=True, has=("res_ups",))),
    # conv16_out
    *[(f"conv16_out {shape} {'with' if bias else 'without'} bias", dict(kernel="out", shape=shape, opts=frozenset({"out_nchw"} | ({"bias"} if bias else set()))))
      for shape in ((1, 8, 32, 64, 3), (2, 16, 64, 128, 6), (1, 8, 32, 64, 32), (1, 8, 32, 64, 1)) for bias in (True, False)],
    ("conv16_out with the affine", dict(kernel="out", has=("gn",))),
    # swish
    ("real: unsplit MT2 with concat", dict(kernel="k9", MT=2, split=False, has=("swish", "concat"))),
    ("real: unsplit through ups", dict(kernel="k9", split=False, has=("swish", "ups"))),
    ("real: n128", dict(kernel="n128", has=("swish",))),
    ("real: split fp16 slabs with res", dict(kernel="k9", slab=16, has=("swish", "res"))),
    ("real: split fp32 slabs", dict(kernel="k9", slab=32, has=("swish",))),
    ("real: conv16_out", dict(kernel="out", has=("swish",))),
]


def _matches(f, spec):
    for k, v in spec.items():
        if k == "has":
            if not set(v) <= f["opts"]:
                return False
        elif f.get(k) != v:
            return False
    return True


@pytest.mark.parametrize("entry", COVERAGE, ids=lambda e: e[0])
def test_table_covers_the_cell(plans, entry):
    label, spec = entry[0], entry[1]
    hits = [f for f in (CM.features(c, plans[c.name]) for c in CM.CASES) if _matches(f, spec)]
    assert hits, f"no case covers: {label}"
    if len(entry) > 2:
        key, n = entry[2]
        assert len({f.get(key) for f in hits}) >= n, f"{label}: {[(f['name'], f.get(key)) for f in hits]}"


def test_every_case_serves_the_coverage_list(plans):
    """No dead weight in the GPU file: a case that matches no entry is a duplicate (or the list lacks its cell)."""
    idle = [c.name for c in CM.CASES if not any(_matches(CM.features(c, plans[c.name]), e[1]) for e in COVERAGE)]
    assert idle == []


def test_some_grid_is_no_multiple_of_eight_in_every_kernel(plans):
    feats = [CM.features(c, plans[c.name]) for c in CM.CASES]
    assert {f["kernel"] for f in feats if f["grid_mod8"]} == {"k9", "n128", "k1", "out"}


@pytest.mark.parametrize("name", ["k9_ups_gn_unsplit", "k9_res_ups_skip_cat_unsplit", "k9_ks2_uneven_5_cat_192_128",
                                  "k1_mt1_ragged_ks2", "real_k9_mt2_cat"])
def test_reference_agrees_with_explicit_loops(name):
    """nearest x2 of the activated operand + affine; res_ups + the fused shortcut over a concat; a concat; the GEMM form;
    swish."""
    case = CM.BY_NAME[name]
    t = CM.make_inputs(case)
    ref, slow = CM.reference(case, t), CM.slow_reference(case, t)
    if case.real:
        assert float((ref - slow).abs().max()) <= 1e-12 * float(CM.conv_part(case, t, mag=True).max() + 10.0)
    else:
        assert torch.equal(ref, slow)


def test_stats_reference_layout():
    """stats_reference on a hand-made image: 2-D patches, flat runs, the reduction's strips, one tile per image."""
    case = CM.BY_NAME["k9_mt2_tw16_2x3_cout192"]                          # 16 x 48, patches of 8 x 16, tiles_x 3, two tile rows
    plan = {"fin": 0, "ksplit": 1, "BM": 128, "TW": 16, "tiles_x": 3, "stats_tiles": 6}
    out = torch.zeros(2, case.Cout, case.H, case.W, dtype=torch.float64)
    case2 = case._replace(B=2)
    out[1, 5, 8:16, 32:48] = 3.0                                          # image 1, patch (1, 2) = tile 5, channel 5
    out[0, 2, 0, 16] = 2.0                                                # image 0, patch (0, 1) = tile 1, channel 2
    st = CM.stats_reference(case2, out, plan)
    want = torch.zeros(12, case.Cout, 2, dtype=torch.float64)
    want[6 + 5, 5] = torch.tensor([384.0, 1152.0])
    want[1, 2] = torch.tensor([2.0, 4.0])
    assert torch.equal(st, want)
    flat = CM.stats_reference(case2._replace(k=1), out, plan)             # flat runs of 128 pixels: 2 2/3 rows each
    # run 3 = pixels 384..511: rows 8, 9 and x < 32 of row 10 -> 32 of the patch's pixels; runs 4 and 5: 48 each
    assert float(flat[0, 2, 0]) == 2.0 and [float(flat[6 + i, 5, 0]) for i in (2, 3, 4, 5)] == [0.0, 96.0, 144.0, 144.0]
    tpi = CM.splitk_tiles(case2)
    assert tpi == 64                                                      # strips of 12 consecutive pixels
    strips = CM.stats_reference(case2, out, dict(plan, ksplit=2, stats_tiles=tpi))
    assert strips.shape == (2 * tpi, case.Cout, 2) and float(strips[1, 2, 0]) == 2.0
    # row 8, x 32..47 = pixels 416..431: 4 of them in strip 34 (408..419), 12 in strip 35
    assert float(strips[tpi:, 5, 0].sum()) == 384.0 and [float(strips[tpi + i, 5, 0]) for i in (34, 35, 36)] == [12.0, 36.0, 0.0]
    one = CM.stats_reference(case2, out, dict(plan, fin=1, ksplit=2, stats_tiles=1))
    assert one.shape == (2, case.Cout, 2) and torch.equal(one[1, 5], torch.tensor([384.0, 1152.0], dtype=torch.float64))


# ----------------------------------------------------------------------------- sensitivity
def _every_tile_differs(case, plan, a, b, tiles=None):
    """`a` and `b` [B, Cout, H, W] differ in at least one element of every pixel tile (of `tiles`: those it concerns)."""
    tmap = CM.pixel_tiles(case, plan)
    diff = (a != b).any(dim=1)
    hit = set(tmap[diff].tolist())
    want = set(tmap.flatten().tolist()) if tiles is None else set(tiles)
    return want <= hit, sorted(want - hit)


SENSITIVE = ["k9_gn_cat_unsplit", "k9_ks4_skip_two_idle_slices", "k1_mt1_ragged_ks2"]


@pytest.mark.parametrize("name", SENSITIVE)
def test_reference_is_sensitive_to_addressing_errors(plans, name):
    """An unsplit 3x3 launch with the affine and a concat, a split 3x3 launch with a fused shortcut, a ragged split GEMM: the
    reference of each changes, in every pixel tile concerned, when one tap is read one pixel off, two 64-channel chunks
    trade places, one slice's chunk range is dropped, two images trade GroupNorm parameters, the shift leaks into the zero
    padding, or one statistics tile lands in its neighbour's slot -- the data are not degenerate."""
    case, plan = CM.BY_NAME[name], plans[name]
    t = CM.make_inputs(case)
    act, ref = CM.activation(case, t), CM.reference(case, t)
    ran = []
    if case.k == 3:                                                      # tap (2, 2) read where tap (2, 1) belongs
        w = t["w"].clone()
        w[:, :, 2, 1] += w[:, :, 2, 2]
        w[:, :, 2, 2] = 0
        ok, miss = _every_tile_differs(case, plan, CM.add_epilogue(case, t, CM.conv_part(case, t, act, w=w)), ref)
        assert ok, f"shifted tap: tiles {miss} unchanged"
        ran.append("tap")
    if plan["nchunks"] >= 2:                                             # chunks 0 and 1 of the operand trade places
        sw = torch.cat([act[:, CM.KC:2 * CM.KC], act[:, :CM.KC], act[:, 2 * CM.KC:]], 1)
        ok, miss = _every_tile_differs(case, plan, CM.add_epilogue(case, t, CM.conv_part(case, t, sw)), ref)
        assert ok, f"swapped chunks: tiles {miss} unchanged"
        ran.append("chunks")
    if plan["ksplit"] > 1:                                               # every slice in turn contributes nothing
        for s, part in enumerate(CM.slice_partials(case, t, plan, act)):
            ok, miss = _every_tile_differs(case, plan, ref - part, ref)
            assert ok, f"dropped slice {s}: tiles {miss} unchanged"
        ran.append("slice")
    if case.gn == "affine":
        tm = CM.pixel_tiles(case, plan)
        sw = {**t, "scale": t["scale"].flip(0), "shift": t["shift"].flip(0)}     # the images trade parameters
        ok, miss = _every_tile_differs(case, plan, CM.reference(case, sw), ref)
        assert ok, f"swapped GroupNorm parameters: tiles {miss} unchanged"
        leak = torch.nn.functional.pad(torch.cat([t["x0"], t["x1"]], 1).double(), (1, 1, 1, 1))   # padded BEFORE the affine
        leak = leak * t["scale"].double()[:, :, None, None] + t["shift"].double()[:, :, None, None]
        out = torch.nn.functional.conv2d(leak, t["w"].double())
        border = torch.zeros(case.H, case.W, dtype=torch.bool)
        border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
        ok, miss = _every_tile_differs(case, plan, CM.add_epilogue(case, t, out), ref, tiles=tm[:, border].flatten().tolist())
        assert ok, f"shift in the padding: border tiles {miss} unchanged"
        ran += ["gn", "padding"]
    st = CM.stats_reference(case, ref, plan).reshape(case.B, plan["stats_tiles"], case.Cout, 2)
    assert plan["stats_tiles"] >= 2
    same = (st[:, 1:] == st[:, :-1]).all(dim=3).all(dim=2)               # neighbouring tiles with identical partials
    assert not bool(same.any()), "two neighbouring statistics tiles hold the same partials"
    ran.append("stats")
    assert set(ran) >= {"chunks", "stats"}


def test_the_three_sensitivity_cases_run_every_mutation(plans):
    c = [CM.BY_NAME[n] for n in SENSITIVE]
    p = [plans[n] for n in SENSITIVE]
    assert c[0].k == 3 and p[0]["ksplit"] == 1 and c[0].gn == "affine" and c[0].C1 and c[0].B >= 2
    assert c[1].k == 3 and p[1]["ksplit"] > 1 and c[1].skip
    assert c[2].k == 1 and p[2]["ksplit"] > 1 and (c[2].B * c[2].H * c[2].W) % p[2]["BM"]


# ----------------------------------------------------------------------------- rejections
def _query(**kw):
    from ddnm_amd._lib import Conv16Desc, lib
    d = Conv16Desc()
    d.src = d.weight = d.out = 0x1000
    d.B, d.H, d.W, d.Cin, d.Cout, d.ksize = 1, 16, 32, 64, 64, 3
    for k, v in kw.items():
        setattr(d, k, v)
    return lib().ddnm_conv16_supported(ctypes.byref(d))


def test_planner_rejections(plans):
    assert _query() == 1
    assert _query(W=24) == 0                                             # no tile width of 32 / 16 divides it
    assert _query(H=12, W=40) == 0
    assert _query(Cin=96) == 0 and _query(Cin=32) == 0
    assert _query(Cout=96) == 0 and _query(Cout=33) == 0
    assert _query(ksize=1) == 1
    assert _query(ksize=1, ups=1) == 0
    assert _query(ksize=1, skip0=0x1000, skip_weight=0x1000, SC0=64) == 0
    assert _query(ksize=5) == 0
    # res_ups in the GEMM form: the split-K reductions map the residual through the nearest x2, the unsplit epilogue reads
    # it at the output pixel's own index -- past the end of a quarter-size tensor -- so the planner refuses that launch
    assert _query(ksize=1, res=0x1000) == 1 and _query(ksize=1, res=0x1000, res_ups=1) == 0
    assert _query(ksize=1, res_ups=1) == 1                               # (no residual: the flag is idle)
    assert _query(ksize=3, res=0x1000, res_ups=1) == 1
    assert plans["k1_mt4_ragged_ks18"]["ksplit"] > 1 and CM.BY_NAME["k1_mt4_ragged_ks18"].res_ups
    # conv16_out: Cout <= 32, W % 32 == 0, H % 8 == 0
    assert _query(out_nchw_f32=1, Cout=6, H=8) == 1 and _query(out_nchw_f32=1, Cout=32, H=8) == 1
    assert _query(out_nchw_f32=1, Cout=33, H=8) == 0
    assert _query(out_nchw_f32=1, Cout=6, H=8, W=48) == 0
    assert _query(out_nchw_f32=1, Cout=6, H=12) == 0
    assert _query(out_nchw_f32=1, Cout=6, H=8, res=0x1000) == 0 and _query(out_nchw_f32=1, Cout=6, H=8, ksize=1) == 0
