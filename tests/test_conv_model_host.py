"""Host half of the exact-fp32 convolution edge tests (tests/conv_model.py; the GPU half is test_gpu_conv_f32_edges.py):
every case of the table meets the conditions that make a bit-exact comparison legitimate, lands on the plan cell its
record names (asked of the library's host queries: no device), the table covers every cell of COVERAGE below, and the
float64 reference agrees with an independent loop formulation.  A change to the planner that moves a case off its cell
fails here instead of silently turning a GPU test into a duplicate of another."""
import pytest
import torch

from tests import conv_model as CM


@pytest.fixture(scope="module")
def plans():
    from ddnm_amd import build
    build.build()
    return {c.name: CM.plan_of(c) for c in CM.CASES}


def test_case_names_are_unique():
    assert len(CM.BY_NAME) == len(CM.CASES)


@pytest.mark.parametrize("case", CM.EXACT_CASES, ids=lambda c: c.name)
def test_exactness_preconditions(plans, case):
    """Integer-valued tensors; conv(|act|, |w|) + |addends| < 2^24 per element; sum |v|, sum v^2 < 2^24 per statistics
    tile and channel; a shift that is never 0 (the padding sentinel)."""
    t = CM.make_inputs(case)
    assert CM.exactness_violations(case, t, plans[case.name]) == []
    if case.gn:
        assert bool((t["shift"] != 0).all()) and bool((t["scale"] != 0).all())
    assert case.K <= 9 * 640 + 96


@pytest.mark.parametrize("case", CM.REAL_CASES, ids=lambda c: c.name)
def test_real_cases_have_an_exact_affine(case):
    """scale * x + shift of the real-valued cases is an fp32 number (so the swish is the prologue's only rounding), the
    shift sits around +3, and K stays small."""
    t = CM.make_inputs(case)
    x = t["x0"] if t["x1"] is None else torch.cat([t["x0"], t["x1"]], 1)
    v64 = x.double() * t["scale"].double()[:, :, None, None] + t["shift"].double()[:, :, None, None]
    v32 = x * t["scale"][:, :, None, None] + t["shift"][:, :, None, None]
    assert torch.equal(v32.double(), v64) and torch.equal((x * t["scale"][:, :, None, None]).double() + t["shift"].double()[:, :, None, None], v64)
    assert float((t["shift"] - 3.0).abs().max()) <= 0.5 and case.Cin <= 64
    if case.ident:
        assert torch.equal(CM.reference(case, t), CM.activation(case, t)[:, :case.Cout])


@pytest.mark.parametrize("case", CM.CASES, ids=lambda c: c.name)
def test_case_lands_on_its_cell(plans, case):
    plan = plans[case.name]
    assert CM.cell_of(case, plan) == case.cell
    assert CM.tile_width_is_the_widest(case, plan)
    if plan["family"] == "f32" and case.tile:
        assert plan["tile"] == case.tile
    if case.skip:
        assert plan["kernel"] == "halo" and not case.ups          # what a fused shortcut needs
    if case.nchw and plan["family"] == "f32":
        assert plan["ksplit"] == 1 and not case.res and not case.stats


# ----------------------------------------------------------------------------- the coverage list, as data
# (label, requirements on conv_model.features(case, plan)).  "has": options that are on; "only": the exact option set;
# every other key: equality.  A third element (key, n): the matching cases take at least n distinct values of `key`.
def _opt(name, has, **kw):
    """An option of the halo kernel: on an unsplit launch, on a split launch, and on two different tiles."""
    base = dict(kernel="halo", has=has, **kw)
    return [(f"{name}: unsplit", dict(base, split=False)), (f"{name}: split", dict(base, split=True)),
            (f"{name}: two tiles", base, ("tile", 2))]


COVERAGE = [
    # halo kernel geometry: forced tile x TW, bias only
    ("halo tile 2, TW 8", dict(kernel="halo", tile=2, TW=8, hw=(8, 8), bias_only=True, split=False)),
    ("halo tile 2, TW 16", dict(kernel="halo", tile=2, TW=16, hw=(4, 16), bias_only=True, split=False)),
    ("halo tile 2, TW 32: 136 halo rows", dict(kernel="halo", tile=2, TW=32, hw=(2, 32), halo_rows_full=True, bias_only=True)),
    ("halo tile 1, TW 8", dict(kernel="halo", tile=1, TW=8, hw=(16, 8), bias_only=True, split=False)),
    ("halo tile 1, TW 16", dict(kernel="halo", tile=1, TW=16, hw=(8, 16), bias_only=True, split=False)),
    ("halo tile 1, TW 32: 204 halo rows, Cout 96 on the 128 tile, grid 6, split 2",
     dict(kernel="halo", tile=1, TW=32, halo_rows_full=True, Cout=96, cout_mod_bn=True, grid=6, grid_mod8=True, ksplit=2)),
    ("halo tile 3, NHWC", dict(kernel="halo", tile=3, nchw=False, bias_only=True)),
    ("igemm NCHW store, Cout 3, declined by small_cout", dict(kernel="halo", nchw=True, Cout=3, small_cout_ok=False), ("tile", 2)),
    ("igemm NCHW store, Cout 6 at 8x16", dict(kernel="halo", nchw=True, Cout=6, hw=(8, 16), small_cout_ok=False)),
    ("igemm NCHW store, Cout 5", dict(kernel="halo", nchw=True, Cout=5, small_cout_ok=False)),
    ("16x24: TW 8, tiles_x 3, two tile rows, grid 12", dict(kernel="halo", hw=(16, 24), TW=8, tiles_x=3, tile_rows=2, grid=12)),
    ("24x16 with Cout 96", dict(kernel="halo", hw=(24, 16), Cout=96, tile_rows=6)),
    ("64x96 on tile 1: tiles_x 3, 96 tiles, unsplit", dict(kernel="halo", tile=1, hw=(64, 96), tiles_x=3, grid=96, split=False)),
    ("unsplit chunk loop, Cout % 4 != 0", dict(kernel="halo", split=False, multi_chunk=True, Cout=66, bias_only=True, nchw=False)),
    ("unsplit chunk loop, 192 tiles on tile 2", dict(kernel="halo", tile=2, grid=192, split=False, multi_chunk=True, bias_only=True)),
    # options on the halo kernel
    *_opt("concat with C0 != C1", ("concat",), C0_ne_C1=True),
    ("concat 32 + 64", dict(kernel="halo", only=("concat",), C0=32)), ("concat 64 + 32", dict(kernel="halo", only=("concat",), C0=64)),
    *_opt("integer affine alone", (), only=("gn",)),
    *_opt("integer affine with concat", (), only=("gn", "concat")),
    *_opt("nearest x2 alone, non-square", (), only=("ups",), square=False),
    *_opt("nearest x2 with concat and the affine, non-square", (), only=("ups", "gn", "concat"), square=False),
    *_opt("badd as an offset view", (), only=("badd",)),
    *_opt("res", (), only=("res",)),
    *_opt("res_ups on a non-square output", (), only=("res_ups",), square=False),
    ("fused shortcut over a concat: unsplit", dict(kernel="halo", has=("skip_concat",), split=False)),
    ("fused shortcut over a concat: split", dict(kernel="halo", has=("skip_concat",), split=True)),
    ("fused shortcut: two tiles", dict(kernel="halo", has=("skip",)), ("tile", 2)),
    ("fused shortcut: one chunk under a 6-way split", dict(kernel="halo", has=("skip",), ksplit=6, skip_chunks_lt_slices=True)),
    ("fused shortcut with statistics: unsplit", dict(kernel="halo", has=("skip", "stats"), split=False)),
    ("fused shortcut with statistics: split", dict(kernel="halo", has=("skip", "stats"), split=True)),
    # split-K
    ("one chunk per slice: 5 of 5", dict(hw=(8, 16), Cin=160, ksplit=5, one_chunk_per_slice=True)),
    ("uneven slices: 6 chunks over 4", dict(B=5, Cin=192, Cout=512, tile=2, ksplit=4, uneven_slices=True)),
    ("the cap: 20 chunks over 16 slices", dict(Cin=640, ksplit=16, capped=True, uneven_slices=True)),
    ("plain reduction: bias", dict(split=True, bias_only=True)),
    ("plain reduction: badd", dict(split=True, only=("badd",))),
    ("plain reduction: res", dict(split=True, only=("res",))),
    ("plain reduction: res_ups", dict(split=True, only=("res_ups",))),
    # statistics from the reduction pass
    ("stats reduction: bias", dict(split=True, only=("stats",))),
    ("stats reduction: badd", dict(split=True, only=("stats", "badd"))),
    ("stats reduction: res", dict(split=True, only=("stats", "res"))),
    ("stats reduction: res_ups", dict(split=True, only=("stats", "res_ups"))),
    ("stats reduction: Cout 96, 24 columns", dict(split=True, has=("stats",), Cout=96, columns=24, cols_divide_256=False)),
    ("stats reduction: Cout 160, 40 columns", dict(split=True, has=("stats",), Cout=160, columns=40, cols_divide_256=False)),
    ("stats reduction: 8x8, 16 strips of 4 pixels < rows per block",
     dict(split=True, has=("stats",), hw=(8, 8), stats_tiles=16, strip_shorter_than_rows=True)),
    ("stats reduction: 32x32, 128 strips", dict(split=True, has=("stats",), hw=(32, 32), stats_tiles=128)),
    ("stats reduction: 24x24, the walk ends at 96", dict(split=True, has=("stats",), hw=(24, 24), stats_tiles=96)),
    ("stats reduction: 16x12, 48 strips", dict(split=True, has=("stats",), hw=(16, 12), stats_tiles=48)),
    ("stats reduction: several images on tile 1", dict(split=True, has=("stats",), tile=1, B=3)),
    # statistics from the kernels' own epilogue
    ("epilogue stats: halo, every tile", dict(kernel="halo", split=False, has=("stats",)), ("tile", 3)),
    ("epilogue stats: halo, every tile width", dict(kernel="halo", split=False, has=("stats",)), ("TW", 3)),
    ("epilogue stats: tiles_x 3, two tile rows, two images", dict(split=False, has=("stats",), tiles_x=3, tile_rows=2, B=2)),
    ("epilogue stats: Cout 96 on the 128 tile", dict(split=False, has=("stats",), tile=1, cout_mod_bn=True)),
    ("epilogue stats: gather 1x1", dict(kernel="gather", k=1, split=False, has=("stats",))),
    # gather kernel
    ("1x1: grid 9", dict(kernel="gather", k=1, B=3, Cin=96, Cout=160, grid=9, grid_mod8=True)),
    ("1x1: tile 1", dict(kernel="gather", k=1, tile=1)), ("1x1: tile 3", dict(kernel="gather", k=1, tile=3)),
    ("1x1: affine and concat", dict(kernel="gather", k=1, only=("gn", "concat"))),
    ("1x1: res_ups", dict(kernel="gather", k=1, only=("res_ups",)), ("split", 2)),
    ("1x1: NCHW store", dict(kernel="gather", k=1, nchw=True)),
    ("1x1: flat strips 16x12", dict(kernel="gather", k=1, flat=True, hw=(16, 12), Cin=64)),
    ("3x3 stride 2: (2,32,64,8x16)", dict(kernel="gather", stride=2, B=2, Cin=32, Cout=64, hw=(8, 16), bias_only=True)),
    ("3x3 stride 2: tile 1", dict(kernel="gather", stride=2, tile=1, Cin=64, Cout=128, hw=(16, 8))),
    ("3x3 stride 2: integer affine (padding sentinel)", dict(kernel="gather", stride=2, only=("gn",)), ("split", 2)),
    ("3x3 stride 2: statistics", dict(kernel="gather", stride=2, has=("stats",))),
    ("3x3 flat fallback: tile 2, affine, unsplit statistics on flat strips",
     dict(kernel="gather", k=3, stride=1, flat=True, tile=2, hw=(16, 12), only=("gn", "stats"), split=False, stats_tiles=3)),
    ("3x3 flat fallback: affine, split", dict(kernel="gather", k=3, stride=1, flat=True, only=("gn",), split=True)),
    # small_cout: every instance at every shape, with and without the affine
    *[(f"small_cout Cout {co} at {B}x{cin} {hw} {'affine' if gn else 'plain'}",
       dict(family="small_cout", Cout=co, B=B, Cin=cin, hw=hw, only=("nchw", "gn") if gn else ("nchw",)))
      for co in (1, 2, 3, 4) for B, cin, hw in ((1, 32, (8, 32)), (2, 96, (16, 64)), (1, 32, (8, 64))) for gn in (False, True)],
    # swish on real-valued data
    ("real: halo tile 2", dict(kernel="halo", tile=2, has=("real", "gn"), ident=False)),
    ("real: halo tile 1 with ups and concat", dict(kernel="halo", tile=1, has=("real", "gn", "ups", "concat"))),
    ("real: gather stride 2", dict(kernel="gather", stride=2, has=("real", "gn"))),
    ("real: small_cout", dict(family="small_cout", has=("real", "gn"), ident=False)),
    ("real identity: gather 1x1", dict(kernel="gather", k=1, has=("real", "ident"))),
    ("real identity: halo", dict(kernel="halo", has=("real", "ident"))),
    ("real identity: small_cout", dict(family="small_cout", has=("real", "ident"))),
]


def _matches(f, spec):
    for k, v in spec.items():
        if k == "has":
            if not set(v) <= f["opts"]:
                return False
        elif k == "only":
            if f["opts"] != frozenset(v):
                return False
        elif f.get(k) != v:
            return False
    return True


@pytest.mark.parametrize("entry", COVERAGE, ids=lambda e: e[0])
def test_table_covers_the_cell(plans, entry):
    label, spec = entry[0], entry[1]
    feats = [CM.features(c, plans[c.name]) for c in CM.CASES]
    hits = [f for f in feats if _matches(f, spec)]
    assert hits, f"no case covers: {label}"
    if len(entry) > 2:
        key, n = entry[2]
        assert len({f.get(key) for f in hits}) >= n, f"{label}: {[(f['name'], f.get(key)) for f in hits]}"


def test_every_case_serves_the_coverage_list(plans):
    """No dead weight in the GPU file: a case that matches no entry is a duplicate (or the list lacks its cell)."""
    idle = [c.name for c in CM.CASES
            if not any(_matches(CM.features(c, plans[c.name]), e[1]) for e in COVERAGE)]
    assert idle == []


def test_igemm_nchw_cases_and_small_cout_cannot_trade_places(plans):
    small = [c for c in CM.CASES if plans[c.name]["family"] == "small_cout"]
    igemm = [c for c in CM.CASES if c.nchw and plans[c.name]["family"] == "f32"]
    assert len(small) >= 24 and len(igemm) >= 5
    assert {c.Cout for c in small} == {1, 2, 3, 4}
    assert all(plans[c.name]["small_cout_ok"] for c in small)
    assert not any(plans[c.name]["small_cout_ok"] for c in igemm)
    assert any(c.Cout <= 4 for c in igemm)              # declined for its shape, not for its channel count


@pytest.mark.parametrize("name", ["ups_gn_cat_unsplit_t1", "gs2_gn_unsplit", "g1x1_res_ups_unsplit", "skip_unsplit_t2", "real_gs2"])
def test_reference_agrees_with_explicit_loops(name):
    """nearest x2 + concat (+ affine); stride 2 with the prologue (padding stays zero); res_ups on a non-square image; the
    fused shortcut; swish."""
    case = CM.BY_NAME[name]
    t = CM.make_inputs(case)
    ref, slow = CM.reference(case, t), CM.slow_reference(case, t)
    if case.real:
        assert float((ref - slow).abs().max()) <= 1e-12 * float(CM.magnitude(case, t).max())
    else:
        assert torch.equal(ref, slow)


def test_stats_reference_layout():
    """stats_reference on a hand-made image: tile rectangles, flat strips and the reduction's strips, channel-major pairs."""
    case = CM.BY_NAME["stats_t2_16x24"]                                  # 2 images, TW 8, tiles_x 3, two tile rows, unsplit
    plan = {"ksplit": 1, "flat": False, "BM": 64, "TW": 8, "tiles_x": 3, "stats_tiles": 6}
    out = torch.zeros(case.B, case.Cout, case.Ho, case.Wo, dtype=torch.float64)
    out[1, 5, 8:16, 16:24] = 3.0                                         # image 1, tile (1, 2) = tile 5, channel 5
    out[0, 2, 0, 8] = 2.0                                                # image 0, tile (0, 1) = tile 1, channel 2
    st = CM.stats_reference(case, out, plan)
    want = torch.zeros(12, case.Cout, 2, dtype=torch.float64)
    want[6 + 5, 5] = torch.tensor([192.0, 576.0])
    want[1, 2] = torch.tensor([2.0, 4.0])
    assert torch.equal(st, want)
    strips = CM.stats_reference(case, out, dict(plan, ksplit=2, stats_tiles=96))     # 4 consecutive pixels each
    assert strips.shape == (192, case.Cout, 2)
    assert torch.equal(strips[2, 2], torch.tensor([2.0, 4.0], dtype=torch.float64))  # pixel 8 of image 0: strip 2
    assert float(strips[96:, 5, 0].sum()) == 192.0 and float(strips[96 + 8 * 6 + 4, 5, 0]) == 12.0   # row 8, x 16..19
    flat = CM.stats_reference(case, out, dict(plan, flat=True, TW=0, tiles_x=0))     # 64 consecutive pixels each
    assert float(flat[0, 2, 0]) == 2.0 and float(flat[6 + 3, 5, 0]) == 3.0 * 8 * 2   # pixels 192..255: rows 8, 9 and x < 16 of row 10
