"""The GroupNorm kernels at their edges, one route at a time: ddnm_gn_stats_f32 + ddnm_gn_finalize_f32,
ddnm_gn_finalize_tiles_amax_f32 on synthetic partials, ddnm_gn_stats_h16, ddnm_gn_bwd_f32 / _h16, and what the launchers
refuse.  Inputs, float64 references and the derivation of every bar are in tests/gn_model.py; test_gn_model_host.py
asserts on the CPU that a replay of each route's summation stays within a quarter of these bars and that no bar is
looser than 1e-2 of what it bounds (1.4e-2 for the mean / sigma = 30 groups at a 64-pixel run).

Every comparison is per element against a bar built from the reference's own magnitudes; output buffers are filled with
NaN before the launch (where the ops wrapper allocates them itself, a NaN block of the same size is handed back to the
caching allocator first); each test prints its worst |err| / bar."""
import pytest
import torch

from tests import gn_model as GM

pytestmark = pytest.mark.gpu

NAN = float("nan")
E_BADARG, E_SHAPE = -1, -2


def _p(t):
    return None if t is None else t.data_ptr()


def _film(c):
    """Device FiLM rows inside a wider NaN-padded buffer: (view at a column offset, row stride > 2C), or (None, 0)."""
    if c["s"] is None:
        return None, 0
    buf, off, stride = GM.film_rows(c["s"], c["t"])
    return buf.cuda()[:, off:], stride


def _forward_worst(c, sc, sh, mr):
    ref, bars = c["ref"], c["bars"]
    w = {"scale": GM.worst(sc, ref["scale"], bars["scale"]), "shift": GM.worst(sh, ref["shift"], bars["shift"])}
    if mr is not None:
        w["mean"] = GM.worst(mr[..., 0], ref["mean"], bars["mean"])
        w["rstd"] = GM.worst(mr[..., 1], ref["rstd"], bars["rstd"])
    return w


def _fmt(w):
    return ", ".join(f"{k} {v:.4f}" for k, v in w.items())


def _affine_via_ops(c, src0, src1, B, C, groups, partial_doubles):
    """ops.group_norm_affine twice: into a NaN-filled workspace (scale, shift), then with keep= (mean_rstd; its scale and
    shift must be the same bits: the kernels are deterministic)."""
    from ddnm_amd import ops
    ws = ops.GroupNormWorkspace("cuda", B, C, max(partial_doubles, 1))
    ws.partial.fill_(NAN), ws.scale.fill_(NAN), ws.shift.fill_(NAN)
    film, stride = _film(c)
    gamma, beta = c["gamma"].cuda(), c["beta"].cuda()
    sc, sh = ops.group_norm_affine(src0, src1, gamma, beta, GM.EPS, ws, groups=groups, film=film, film_stride=stride)
    sc, sh = sc[:B * C].reshape(B, C).cpu(), sh[:B * C].reshape(B, C).cpu()
    part = ws.partial[:partial_doubles].cpu()
    poison = [torch.full((n,), NAN, device="cuda") for n in (B * C, B * C, B * groups * 2)]
    del poison                                                 # the blocks keep= is about to be given
    keep = {}
    ops.group_norm_affine(src0, src1, gamma, beta, GM.EPS, ws, groups=groups, film=film, film_stride=stride, keep=keep)
    torch.cuda.synchronize()
    mr = keep["mean_rstd"].reshape(B, groups, 2).cpu()
    assert torch.equal(keep["scale"].reshape(B, C).cpu(), sc) and torch.equal(keep["shift"].reshape(B, C).cpu(), sh)
    return sc, sh, mr, part


# ----------------------------------------------------------------------------- 1. stats_f32 + finalize_f32
@pytest.mark.parametrize("film", [False, True], ids=["plain", "film"])
@pytest.mark.parametrize("case", GM.F32_CASES, ids=GM.case_id)
def test_stats_f32_and_finalize(hip, case, film):
    """ddnm_gn_stats_f32 + ddnm_gn_finalize_f32 through ops.group_norm_affine: block sizes 256 / 512 / 1024, idle threads,
    HW < rows, a ragged last chunk, groups straddling the two sources, groups = 1 and 64, 9 chunks over finalize's four
    lanes.  scale, shift, mean and rstd per element against gn_model.forward_bars; every partial slot is written."""
    from ddnm_amd import ops
    B, C0, C1, H, W, groups = case
    C = C0 + C1
    c = GM.f32_case(case, film)
    nchunk = ops.gn_nchunk(H * W, C)
    assert nchunk == c["route"]["nchunk"]
    x = c["x"]
    src0 = x[..., :C0].contiguous().cuda()
    src1 = x[..., C0:].contiguous().cuda() if C1 else None
    sc, sh, mr, part = _affine_via_ops(c, src0, src1, B, C, groups, B * nchunk * groups * 2)
    w = _forward_worst(c, sc, sh, mr)
    print(f"gn_stats_f32 {case} film={film}: worst |err| / bar {_fmt(w)}")
    assert bool(torch.isfinite(part).all())
    assert all(bool(torch.isfinite(t).all()) for t in (sc, sh, mr))
    assert all(v <= 1.0 for v in w.values()), w


# ----------------------------------------------------------------------------- 2. finalize from tile partials
@pytest.mark.parametrize("want_mr", [False, True], ids=["nomr", "mr"])
@pytest.mark.parametrize("film", [False, True], ids=["plain", "film"])
@pytest.mark.parametrize("case", GM.TILE_CASES, ids=GM.case_id)
def test_finalize_tiles_on_synthetic_partials(hip, case, film, want_mr):
    """ddnm_gn_finalize_tiles_amax_f32 on (sum, sumsq) partials taken from the float64 reference and rounded once (n = 1:
    the bars isolate the finalize kernel): two tilings, a group straddling part0 / part1, a group wholly in part1
    (n0 = 0), cpg = 1 and 256.  With groups = AMAX_N the operand bound is requested too:
    max |x| of the group <= amax <= sqrt(largest tile sumsq of the group) (1 + 2^-9)."""
    from ddnm_amd import ops
    from ddnm_amd._lib import check
    B, C0, tpi0, C1, tpi1, groups, HW = case
    C = C0 + C1
    c = GM.tile_case(case, film)
    parts = [p.cuda() for p in c["parts"]]
    film_v, stride = _film(c)
    gamma, beta = c["gamma"].cuda(), c["beta"].cuda()
    sc = torch.full((B, C), NAN, device="cuda")
    sh = torch.full((B, C), NAN, device="cuda")
    mr = torch.full((B, groups, 2), NAN, device="cuda") if want_mr else None
    amax = torch.full((B, groups), NAN, device="cuda") if groups == ops.AMAX_N else None
    check(hip.ddnm_gn_finalize_tiles_amax_f32(_p(parts[0]), tpi0, C0, _p(parts[1]) if C1 else None, tpi1, C1, _p(gamma),
                                              _p(beta), B, HW, groups, GM.EPS, _p(sc), _p(sh), _p(film_v), stride, _p(mr),
                                              _p(amax), ops._stream()), "ddnm_gn_finalize_tiles_amax_f32")
    torch.cuda.synchronize()
    sc, sh = sc.cpu(), sh.cpu()
    w = _forward_worst(c, sc, sh, None if mr is None else mr.cpu())
    print(f"gn_finalize_tiles {case} film={film} mr={want_mr}: worst |err| / bar {_fmt(w)}")
    assert bool(torch.isfinite(sc).all()) and bool(torch.isfinite(sh).all())
    assert mr is None or bool(torch.isfinite(mr).all())
    assert all(v <= 1.0 for v in w.values()), w
    if amax is not None:
        q = torch.cat([p[..., 1].double().amax(dim=1) for p in c["parts"]], dim=1).reshape(B, groups, -1).amax(dim=2)
        a = amax.double().cpu()
        lo, hi = float((a / c["ref"]["amax"]).min()), float((a / (torch.sqrt(q) * (1.0 + 2.0 ** -9))).max())
        print(f"    amax / max|x| >= {lo:.6f}, amax / (sqrt(max sumsq) (1 + 2^-9)) <= {hi:.6f}")
        assert bool((a >= c["ref"]["amax"]).all()) and bool((a <= torch.sqrt(q) * (1.0 + 2.0 ** -9)).all())


# ----------------------------------------------------------------------------- 3. stats_h16
@pytest.mark.parametrize("case,film", [(c, f) for c in GM.H16_CASES for f in (False, True) if c[4] or not f],
                         ids=lambda v: GM.case_id(v) if isinstance(v, tuple) else ("film" if v else "plain"))
def test_stats_h16(hip, case, film):
    """ddnm_gn_stats_h16 with the tile count ops.gn_stats16 picks (16, 4, 4, 1, 4, 2): every (tile, channel) partial
    against the float64 sums of the fp16-rounded values (bars 4 n u sum |x|, 4 n u sum x^2, n = HW / tiles), C = 2056 and
    2080 with a second, nearly empty block along the channels; then the affine through ops.group_norm_affine.  C = 2056
    has no group count that finalize-from-tiles accepts (8 x 257 channels), so it stops at the partials."""
    from ddnm_amd import ops
    from ddnm_amd._lib import check
    B, C, H, W, groups = case
    c = GM.h16_case(case, film)
    tiles = c["tiles"]
    x16 = c["x"].half().cuda()
    stats = torch.full((B, tiles, C, 2), NAN, device="cuda")
    check(hip.ddnm_gn_stats_h16(_p(x16), _p(stats), B, H * W, C, tiles, ops._stream()), "ddnm_gn_stats_h16")
    act = ops.gn_stats16(x16)
    torch.cuda.synchronize()
    assert act.tiles == tiles == GM.H16_TILES[(H, W)]
    st = stats.cpu()
    assert bool(torch.isfinite(st).all()) and torch.equal(act.stats.reshape(st.shape).cpu(), st)
    bar = c["part_bar"] + 2.0 ** -149                                   # an all-zero column: exact, 0 <= tiny
    w = {"partials": GM.worst(st, c["part_ref"], bar)}
    if groups:
        sc, sh, mr, _ = _affine_via_ops(c, x16, None, B, C, groups, 0)
        w.update(_forward_worst(c, sc, sh, mr))
        assert all(bool(torch.isfinite(t).all()) for t in (sc, sh, mr))
    print(f"gn_stats_h16 {case} film={film} tiles={tiles}: worst |err| / bar {_fmt(w)}")
    assert all(v <= 1.0 for v in w.values()), w


# ----------------------------------------------------------------------------- 4. backward
@pytest.mark.parametrize("half", [False, True], ids=["f32", "h16"])
@pytest.mark.parametrize("case", GM.BWD_CASES, ids=GM.case_id)
def test_gn_backward_edges(hip, case, half):
    """ddnm_gn_bwd_f32 / _h16 against float64 autograd of act(GN(x) (1 + s) + t) (avg_pool2d(2) behind it when dA_ups), on
    the offset / spread inputs: H != W with half-resolution dA and add, no silu and no add, half-resolution dA with a
    full-resolution add, blocks of 512 and 1024 threads, idle threads, a ragged last chunk, groups = 64.  scale, shift and
    mean_rstd are the float64 reference rounded to fp32, so a forward error can neither mask nor fake a backward one.  dx
    and coef = (P1 / cnt, rstd^2 P2 / cnt) per element against the chain written out in gn_model.bwd_chain."""
    from ddnm_amd import ops
    from ddnm_amd._lib import check
    B, C, H, W, groups, silu, dA_ups, add, add_ups, film = case
    c = GM.bwd_case(case, half)
    ref, ch = c["ref"], c["chain"]
    dx_ref = GM.bwd_autograd(c["x"], groups, c["gamma"], c["beta"], c["s"], c["t"], silu, c["dA"], dA_ups, c["add"], add_ups)
    dev = (lambda t: t.half().cuda()) if half else (lambda t: t.cuda())
    x, dA = dev(c["x"]), dev(c["dA"])
    ad = None if c["add"] is None else dev(c["add"])
    sc, sh = ref["scale"].float().cuda(), ref["shift"].float().cuda()
    mr = torch.stack([ref["mean"], ref["rstd"]], dim=-1).float().cuda()
    nchunk = hip.ddnm_gn_bwd_nchunk(H * W, C)
    assert nchunk == GM.f32_route(H * W, C, GM.GNB_PIX_PER_THREAD)["nchunk"]
    partial = torch.full((B * nchunk * groups * 2,), NAN, dtype=torch.float64, device="cuda")
    coef = torch.full((B, groups, 2), NAN, device="cuda")
    dx = torch.full((B, H, W, C), NAN, device="cuda", dtype=torch.float16 if half else torch.float32)
    fn = hip.ddnm_gn_bwd_h16 if half else hip.ddnm_gn_bwd_f32
    check(fn(_p(x), _p(dA), int(dA_ups), _p(sc), _p(sh), _p(mr), int(silu), _p(ad), int(add_ups), B, H, W, C, groups,
             _p(partial), nchunk, _p(coef), _p(dx), ops._stream()), "ddnm_gn_bwd")
    torch.cuda.synchronize()
    dx, coef = dx.cpu(), coef.cpu()
    floor = 2.0 ** -149                                            # c2 of the constant group: 0 against 0
    w = {"dx": GM.worst(dx, dx_ref, ch["e_dx"]), "c1": GM.worst(coef[..., 0], ch["coef"][..., 0], ch["e_coef"][..., 0]),
         "c2": GM.worst(coef[..., 1], ch["coef"][..., 1], ch["e_coef"][..., 1] + floor)}
    print(f"gn_bwd {case} half={half}: worst |err| / bar {_fmt(w)}")
    assert bool(torch.isfinite(partial).all()) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(coef).all())
    assert all(v <= 1.0 for v in w.values()), w


# ----------------------------------------------------------------------------- 5. rejections
def test_launchers_refuse_bad_geometry(hip):
    """Return codes only: each call below is refused by its launcher before anything is launched (every pointer is a valid
    sentinel-filled buffer that must come back untouched)."""
    from ddnm_amd import ops
    buf = torch.full((4096,), 7.0, device="cuda", dtype=torch.float64)
    p, s = buf.data_ptr(), ops._stream()
    L = hip

    def stats(C0, C1, groups, HW=16, nchunk=None):
        n = L.ddnm_gn_nchunk(HW, C0 + C1) if nchunk is None else nchunk
        return L.ddnm_gn_stats_f32(p, p, 1, HW, C0, C1, groups, p, n, s)

    def tiles(C0, groups, amax=None):
        return L.ddnm_gn_finalize_tiles_amax_f32(p, 1, C0, None, 0, 0, p, p, 1, 16, groups, GM.EPS, p, p, None, 0, None, amax, s)

    def bwd(fn, C, H, W, groups, dA_ups=0, add_ups=0, nchunk=None):
        n = L.ddnm_gn_bwd_nchunk(H * W, C) if nchunk is None else nchunk
        return fn(p, p, dA_ups, p, p, p, 1, p, add_ups, 1, H, W, C, groups, p, n, p, p, s)

    assert L.ddnm_gn_nchunk(16, 4100) == E_SHAPE and L.ddnm_gn_bwd_nchunk(16, 4100) == E_SHAPE        # C / 4 > 1024
    assert stats(4100, 0, 1, nchunk=1) == E_SHAPE
    assert stats(2048, 2052, 1, nchunk=1) == E_SHAPE
    assert stats(260, 0, 65) == E_SHAPE                                                               # groups > 64
    assert L.ddnm_gn_finalize_f32(p, 1, p, p, 1, 16, 260, 65, GM.EPS, p, p, None, 0, None, s) == E_SHAPE
    assert stats(128, 0, 32, nchunk=L.ddnm_gn_nchunk(16, 128) + 1) == E_BADARG                        # a wrong nchunk
    assert stats(128, 0, 32, HW=600, nchunk=1) == E_BADARG
    assert tiles(514, 2) == E_SHAPE                                                                   # C / groups > 256
    assert tiles(128, 16, amax=p) == E_SHAPE                                                          # amax, groups != AMAX_N
    assert L.ddnm_gn_stats_h16(p, p, 1, 16, 12, 4, s) == E_SHAPE                                      # C % 8
    assert L.ddnm_gn_stats_h16(p, p, 1, 10, 16, 4, s) == E_SHAPE                                      # HW % tiles
    for fn in (L.ddnm_gn_bwd_f32, L.ddnm_gn_bwd_h16):
        assert bwd(fn, 4100, 4, 4, 1, nchunk=1) == E_SHAPE                                            # C / 4 > 1024
        assert bwd(fn, 260, 4, 4, 65, nchunk=1) == E_BADARG                                           # groups > 64
        assert bwd(fn, 96, 4, 4, 32) == E_SHAPE                                                       # C % (groups * 4)
        assert bwd(fn, 128, 5, 4, 32, dA_ups=1) == E_SHAPE                                            # odd H, dA_ups
        assert bwd(fn, 128, 4, 5, 32, add_ups=1) == E_SHAPE                                           # odd W, add_ups
        assert bwd(fn, 128, 4, 4, 32, nchunk=L.ddnm_gn_bwd_nchunk(16, 128) + 1) == E_BADARG           # a wrong nchunk
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
