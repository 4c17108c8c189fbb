"""The conditions the GPU GroupNorm edge tests (test_gpu_groupnorm_edges.py) rely on, asserted on the CPU for every
case's own inputs (tests/gn_model.py):

  1. a numpy replay of the route's summation (fp32 runs in pixel order, fp64 combine, var clamped at 0; float64 up to but
     not including the final fp32 roundings) stays within ONE QUARTER of every bar -- a kernel inside its contract has
     room, a bar that the contract itself would reach is derived wrongly;
  2. no bar exceeds 1e-2 of the magnitude it bounds -- a bar looser than that could not see a subtle error.  The groups
     with mean / sigma = 30 are the exception: rstd's bar is 2 n u (1 + 2 r^2) of rstd there, 1.4e-2 at the 64-pixel run
     of gn_stats_kernel (the one-pass var = E[x^2] - mean^2 loses r^2 to cancellation); they are held to that figure
     (gn_model.loose_limit) instead, and scale / shift inherit it.

Also: the launch geometry each GPU case is meant to reach, and the closed form of the backward against float64 autograd."""
import pytest
import torch

from tests import gn_model as GM

QUARTER = 0.25


def _assert_conditions(c, rep, n, what):
    w_rep, w_tight, w_loose = GM.conditions(c["ref"], c["bars"], rep, c["r_nom"], c["gamma"])
    print(f"{what}: replay / bar {w_rep:.3f}, bar / magnitude {w_tight:.2e} (r = 30 groups {w_loose:.2e})")
    assert w_rep <= QUARTER, (what, w_rep)
    assert w_tight <= 1e-2, (what, w_tight)
    assert w_loose <= GM.loose_limit(n), (what, w_loose, GM.loose_limit(n))


# ----------------------------------------------------------------------------- inputs
def test_builder_covers_every_pair_and_one_constant_group():
    x, r = GM.make_x(2, 8, 8, 256, 32)
    v = x.double().reshape(2, 64, 32, 8)
    for b in range(2):
        cg = GM.const_group(b, 32)
        assert bool((v[b, :, cg, :] == 0.5).all()) and bool(torch.isnan(r[b, cg]))
        seen = {(float(r[b, g]), round(float(v[b, :, g, :].std()) / s, 0) * s) for g in range(32) if g != cg
                for s in (1e-3, 1.0, 50.0) if 0.5 * s < float(v[b, :, g, :].std()) < 2.0 * s}
        assert seen == set(GM.PAIRS)
    # realised |mean| / std follows the nominal r at this group size (512 elements)
    m, sd = v.mean(dim=(1, 3)), v.std(dim=(1, 3))
    ok = ~torch.isnan(r)
    assert float(((m / sd)[ok] - r[ok]).abs().max()) < 0.15 * 30
    xh, _ = GM.make_x(2, 8, 8, 256, 32, half=True)
    assert float(xh.abs().max()) < 65504.0 and torch.equal(xh.half().float(), xh)
    _, _, s, _ = GM.make_affine(2, 256, True)
    assert bool(((1.0 + s) < 0).any())


def test_film_rows_layout():
    _, _, s, t = GM.make_affine(2, 32, True)
    buf, off, stride = GM.film_rows(s, t)
    assert stride > 2 * 32 and off > 0
    view = buf[:, off:]
    assert torch.equal(view[:, :32], s) and torch.equal(view[:, 32:64], t)


# ----------------------------------------------------------------------------- launch geometry
def test_f32_cases_reach_their_branches():
    geo = {c: GM.f32_route(c[3] * c[4], c[1] + c[2]) for c in GM.F32_CASES}
    g = geo[(2, 32, 0, 4, 4, 32)]
    assert g["rows"] == 32 and 16 < g["rows"]                                   # HW < rows
    assert geo[(1, 192, 0, 8, 8, 32)]["idle"] == 16
    assert (21 * 3 < 64 < 22 * 3)                                               # group 21 of C = 96 spans both sources
    g = geo[(1, 1024, 0, 9, 8, 32)]
    assert (g["block"], g["nchunk"], g["last"], g["n"]) == (256, 2, 8, 64)
    g = geo[(1, 1024, 512, 9, 8, 32)]
    assert (g["block"], g["idle"], g["nchunk"], g["last"]) == (512, 128, 2, 8) and 21 * 48 < 1024 < 22 * 48
    g = geo[(1, 1152, 1024, 4, 5, 32)]
    assert (g["block"], g["rows"]) == (1024, 1) and 2176 // 4 == 544
    g = geo[(1, 4096, 0, 2, 2, 32)]
    assert (g["block"], g["idle"]) == (1024, 0)
    g = geo[(1, 128, 0, 64, 65, 32)]
    # 8 rows x 64 pixels per chunk: 9 chunks (8 full, 64 pixels in the last), so lane 0 of finalize's `ch += 4` loop adds
    # three chunks and lanes 1 .. 3 two
    assert (g["rows"], g["nchunk"], g["last"], g["n"]) == (8, 9, 64, 64) and g["nchunk"] % 4 == 1


def test_h16_cases_pick_the_listed_tiles():
    for B, C, H, W, groups in GM.H16_CASES:
        assert GM.stats16_tiles(H * W) == GM.H16_TILES[(H, W)]
    assert (2056 // 8 + 255) // 256 == 2 and 2056 // 8 - 256 == 1              # second blockIdx.y, one live thread
    assert (2080 // 8 + 255) // 256 == 2 and 2080 // 32 <= 256 and 2056 // 8 > 256


def test_bwd_cases_reach_their_branches():
    geo = {c: GM.f32_route(c[2] * c[3], c[1], GM.GNB_PIX_PER_THREAD) for c in GM.BWD_CASES}
    assert geo[GM.BWD_CASES[2]]["idle"] == 64
    g = geo[GM.BWD_CASES[3]]
    assert (g["block"], g["nchunk"], g["last"]) == (512, 3, 8)
    assert geo[GM.BWD_CASES[4]]["block"] == 1024
    g = geo[GM.BWD_CASES[5]]
    assert (g["rows"], g["nchunk"], g["last"]) == (4, 5, 16)
    for c in GM.BWD_CASES:
        assert c[1] % (c[4] * 4) == 0 and (not (c[6] or c[8]) or (c[2] % 2 == 0 and c[3] % 2 == 0))


# ----------------------------------------------------------------------------- the two conditions, forward
@pytest.mark.parametrize("film", [False, True], ids=["plain", "film"])
@pytest.mark.parametrize("case", GM.F32_CASES, ids=GM.case_id)
def test_f32_route_conditions(case, film):
    c = GM.f32_case(case, film)
    rep = GM.replay_runs(c["x"], case[5], c["route"]["runs"])
    GM.replay_affine(rep, case[5], c["gamma"], c["beta"], c["s"], c["t"])
    _assert_conditions(c, rep, c["route"]["n"], f"gn_stats_f32 {case}")


@pytest.mark.parametrize("film", [False, True], ids=["plain", "film"])
@pytest.mark.parametrize("case", GM.TILE_CASES, ids=GM.case_id)
def test_tile_partials_conditions(case, film):
    c = GM.tile_case(case, film)
    rep = GM.replay_partials(c["parts"], case[5], case[6])
    GM.replay_affine(rep, case[5], c["gamma"], c["beta"], c["s"], c["t"])
    _assert_conditions(c, rep, 1, f"gn_finalize_tiles {case}")
    # the amax bound the GPU test asserts is consistent: sqrt(max tile sumsq) >= max |x| of the group
    if case[5] == 32:
        B, C0, _, C1, _, groups, HW = case
        q = torch.cat([p[..., 1].double().amax(dim=1) for p in c["parts"]], dim=1)                  # [B, C]
        qg = q.reshape(B, groups, -1).amax(dim=2)
        assert bool((torch.sqrt(qg) * (1.0 + 2.0 ** -9) >= c["ref"]["amax"]).all())


@pytest.mark.parametrize("case", [c for c in GM.H16_CASES if c[4]], ids=GM.case_id)
def test_h16_route_conditions(case):
    c = GM.h16_case(case)
    rep = GM.replay_runs(c["x"], case[4], c["route"]["runs"])
    GM.replay_affine(rep, case[4], c["gamma"], c["beta"], c["s"], c["t"])
    _assert_conditions(c, rep, c["route"]["n"], f"gn_stats_h16 {case}")


@pytest.mark.parametrize("case", GM.H16_CASES, ids=GM.case_id)
def test_h16_partials_replay(case):
    """The (tile, channel) partials themselves: an fp32 replay within a quarter of 4 n u sum |x| / 4 n u sum x^2."""
    import numpy as np
    c = GM.h16_case(case)
    B, C, H, W, _ = case
    xs = c["x"].numpy().reshape(B, c["tiles"], -1, C)
    rep = np.stack([np.cumsum(xs, axis=2, dtype=np.float32)[:, :, -1], np.cumsum(xs * xs, axis=2, dtype=np.float32)[:, :, -1]], axis=-1)
    bar = c["part_bar"].clamp_min(1e-300)
    w = GM.worst(torch.from_numpy(rep), c["part_ref"], bar)
    print(f"gn_stats_h16 partials {case}: replay / bar {w:.3f}")
    assert w <= QUARTER


# ----------------------------------------------------------------------------- backward
@pytest.mark.parametrize("half", [False, True], ids=["f32", "h16"])
@pytest.mark.parametrize("case", GM.BWD_CASES, ids=GM.case_id)
def test_bwd_chain_conditions(case, half):
    """The closed form of backward.hip equals float64 autograd (to 1e-9 of the term magnitudes: both are float64), the fp32
    replay of the P1 / P2 summation is within a quarter of the coef bars, and no bar exceeds 1e-2 of its magnitude."""
    B, C, H, W, groups, silu, dA_ups, add, add_ups, film = case
    c = GM.bwd_case(case, half)
    ch = c["chain"]
    auto = GM.bwd_autograd(c["x"], groups, c["gamma"], c["beta"], c["s"], c["t"], silu, c["dA"], dA_ups, c["add"], add_ups)
    gap = float(((auto - ch["dx"]).abs() / ch["mag"]["dx"]).max())
    const = torch.isnan(c["r_nom"])                      # x - mean = 0 there: c2 is identically 0 and has no magnitude
    assert bool((ch["coef"][..., 1][const] == 0).all())
    rep = GM.replay_bwd_coef(c["x"], c["ref"], ch)
    w_rep = GM.worst(rep, ch["coef"], ch["e_coef"])
    r_dx = float((ch["e_dx"] / ch["mag"]["dx"]).max())
    r_coef = max(float((ch["e_coef"][..., 0] / ch["mag"]["coef"][..., 0]).max()),
                 float((ch["e_coef"][..., 1] / ch["mag"]["coef"][..., 1])[~const].max()))
    print(f"gn_bwd {case} half={half}: autograd gap {gap:.2e}, coef replay / bar {w_rep:.3f}, bar / magnitude dx {r_dx:.2e} "
          f"coef {r_coef:.2e}")
    assert gap <= 1e-9
    assert w_rep <= QUARTER
    assert r_dx <= 1e-2 and r_coef <= 1e-2
