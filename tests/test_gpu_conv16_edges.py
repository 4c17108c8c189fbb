"""The fp16-activation convolution engine (csrc/conv16.hip: conv16_kernel<TAPS, MT, WNW>, conv16_n128_kernel, the split-K
reductions and the reduction that finalizes the consumer's GroupNorm) per tile, tile width, split, slab format and fused
option, through ops.conv16 / ops.conv16_out; and the operand helpers of csrc/act16.hip (ops.gn_apply16, ops.im2col16,
ops.nchw_to_nhwc16) per element.  Cases, inputs, float64 references and the conditions that make the comparison legitimate
are in tests/conv16_model.py; test_conv16_model_host.py asserts on the CPU that every case lands on the plan cell it names,
that the table covers the coverage list and that the references notice a misplaced tap, chunk, slice, image or tile.

Exact cases: integer-valued fp16 data whose every intermediate is an integer its format holds (<= 2048 where it is rounded
to fp16, < 2^24 where it stays fp32), so the output and the GroupNorm partials must equal the float64 reference BIT FOR BIT
in any summation order: no tolerance; a misplaced element, tap, channel, image, slice or statistics tile is a mismatch at a
known index.  The output is a view into a NaN-filled fp16 buffer with 4096 elements of guard on both sides, the per-stream
split-K scratch is NaN-filled THROUGH AN fp16 VIEW before every split launch (an fp32 NaN reads as one NaN half and one
zero half: half of an fp16 slab would read as harmless zeros), and a NaN block of the statistics' size is handed back to
the caching allocator before a launch that emits them.  Launches that finalize the consumer's GroupNorm are exact in the
output and the per-image partials; their scale / shift are held per (image, channel) to gn_model.forward_bars with n = 1
(the sums are exact) against a float64 GroupNorm (+ FiLM) of the exact output.

Swish cases: per element
    |got - ref| <= ((2^-11 + E_ACT) + (K + 8) 2^-24) (conv(|act|, |w|) + skip(|s|, |w_s|)) + r 2^-11 (|ref| + |res|) + 2^-24
(conv16_model.real_bound; E_ACT is the relative error of the engines' common swish measured by
test_gpu_conv_f32_edges.py for arguments in [-5.3, 10.9], and the host test keeps the arguments inside).
Worst |err| / bound observed on the MI355X: real_k9_mt2_cat 0.206, real_k9_ups 0.156, real_n128 0.166, real_ks2_res 0.116,
real_ks9_fp32_slab 0.024, real_out 0.078 (the rounding of the activated operand and of the result to fp16 dominate; the
(K + 8) 2^-24 term is a worst case over summation orders); ops.gn_apply16 with swish 0.980 of (2^-11 + E_ACT) |ref| + 2^-24
(a result half an fp16 ulp from a value just above a power of two); the finalized scale / shift of the fin cases 0.12 .. 0.23
of their bars."""
import ctypes
import functools

import pytest
import torch

from tests import conv16_model as CM
from tests import gn_model as GM
from tests.test_gpu_conv_f32_edges import E_ACT

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 4096
U16 = 2.0 ** -11


def _nhwc16(x):
    return None if x is None else x.permute(0, 2, 3, 1).contiguous().half().cuda()


def _dev(x):
    return None if x is None else x.contiguous().cuda()


@functools.lru_cache(maxsize=None)
def _host(name):
    """(case, inputs, plan, float64 reference): computed once per case, shared, never modified."""
    case = CM.BY_NAME[name]
    t = CM.make_inputs(case)
    return case, t, CM.plan_of(case), CM.reference(case, t)


def _poison(numel, dtype):
    """Hands a NaN block of the size the launcher is about to ask the caching allocator for back to it."""
    block = torch.full((int(numel),), NAN, dtype=dtype, device="cuda")
    del block


def _launch(hip, case, t, plan):
    """One launch of the case -> (NCHW float32 result on the CPU, Act or None, GroupNorm workspace or None)."""
    from ddnm_amd import ops
    x0, w = _nhwc16(t["x0"]), ops.pack_conv_weight16(t["w"].cuda())
    gn = (_dev(t["scale"]), _dev(t["shift"])) if case.gn != "none" else None
    n = case.B * case.Cout * case.H * case.W
    if case.out_nchw:
        _poison(n, torch.float32)
        got = ops.conv16_out(x0, w, case.Cout, bias=_dev(t["bias"]), gn=gn, gn_silu=case.real)
        torch.cuda.synchronize()
        assert got.shape == (case.B, case.Cout, case.H, case.W) and got.dtype == torch.float32
        return got.cpu(), None, None
    kw = dict(src1=_nhwc16(t["x1"]), gn=gn, gn_silu=case.real, bias=_dev(t["bias"]), res=_nhwc16(t["res"]), res_ups=case.res_ups,
              ups=case.ups, emit_stats=case.stats)
    if case.skip:
        sc = sum(case.skip)
        kw["skip"] = (_nhwc16(t["skip0"]), _nhwc16(t["skip1"]))
        kw["skip_weight"] = ops.pack_conv_weight16(t["skip_w"].cuda()).reshape(-1, sc).contiguous()
    ws = None
    if case.fin:
        ws = ops.GroupNormWorkspace("cuda", case.B, case.Cout, 16)
        ws.scale.fill_(NAN)
        ws.shift.fill_(NAN)
        film = CM.film_rows(t).cuda() if case.fin == "film" else None
        kw["fin"] = ("gn", _dev(t["gamma"]), _dev(t["beta"]), film, 0 if film is None else film.shape[1], 1e-5, ws)
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float16, device="cuda")
    out = buf[GUARD:GUARD + n].view(case.B, case.H, case.W, case.Cout)
    need = int(hip.ddnm_conv16_workspace_floats(ctypes.byref(CM.desc_of(case))))
    if plan["ksplit"] > 1:
        # the scratch ops keeps per (device, stream), obtained as ops._launch_conv obtains it, poisoned as a whole
        assert need == plan["ksplit"] * n
        ops._conv_workspace(out.device, need).view(torch.float16).fill_(NAN)
    else:
        assert need == 0
    if plan["stats_tiles"] > 0 and case.stats:
        _poison(case.B * plan["stats_tiles"] * case.Cout * 2, torch.float32)
    act = ops.conv16(x0, w, case.Cout, case.k, out=out, **kw)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert bool(torch.isnan(got[:GUARD]).all()), f"{case.name}: store in front of the output"
    assert bool(torch.isnan(got[GUARD + n:]).all()), f"{case.name}: store behind the output"
    return got[GUARD:GUARD + n].view(case.B, case.H, case.W, case.Cout).permute(0, 3, 1, 2).float(), act, ws


def _assert_bits(got, want, what, names):
    """torch.equal with a report: how many elements differ (NaN counts), and the first few with their indices."""
    if got.shape == want.shape and torch.equal(got, want):
        return
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()
    first = "; ".join(f"{dict(zip(names, i.tolist()))}: got {float(got[tuple(i)])}, expected {float(want[tuple(i)])}" for i in idx[:6])
    raise AssertionError(f"{what}: {idx.shape[0]} of {got.numel()} elements differ ({int(torch.isnan(got).sum())} NaN): {first}")


def _check_stats(case, plan, act, out64):
    """The partials against the sums of `out64` in the kernel's tile layout; absent exactly when the plan has no tiles."""
    tiles = plan["stats_tiles"]
    assert act.tiles == tiles
    if tiles == 0:
        assert act.stats is None
        return None
    assert act.stats is not None and act.stats.numel() == case.B * tiles * case.Cout * 2
    stats = act.stats.cpu().reshape(case.B * tiles, case.Cout, 2)
    _assert_bits(stats, CM.stats_reference(case, out64, plan).float(), f"{case.name} statistics ({tiles} tiles per image)",
                 ("tile", "channel", "sum|sumsq"))
    return stats


def _check_exact(hip, name):
    case, t, plan, ref = _host(name)
    want = ref.float()
    assert torch.equal(want.double(), ref)                         # (the preconditions: asserted in the host test)
    got, act, ws = _launch(hip, case, t, plan)
    _assert_bits(got, want, f"{name} output", ("img", "channel", "y", "x"))
    if case.out_nchw:
        return got, None
    stats = _check_stats(case, plan, act, ref)
    if not plan["fin"]:
        assert act.gn is None
        return got, stats
    assert act.gn is not None and act.gn[2] == "gn", "this case must take the finalizing reduction"
    B, C = case.B, case.Cout
    sc, sh = ws.scale[:B * C].reshape(B, C).cpu(), ws.shift[:B * C].reshape(B, C).cpu()
    g = GM.gn_reference(ref.permute(0, 2, 3, 1), 32, t["gamma"], t["beta"], t["film_s"], t["film_t"])
    bars = GM.forward_bars(g, 1, t["gamma"], t["beta"], t["film_s"], t["film_t"])     # n = 1: the kernel's sums are exact here
    w_sc, w_sh = GM.worst(sc, g["scale"], bars["scale"]), GM.worst(sh, g["shift"], bars["shift"])
    print(f"{name}: finalized scale / shift, worst |err| / bar {w_sc:.3f} / {w_sh:.3f}")
    assert bool(torch.isfinite(sc).all()) and bool(torch.isfinite(sh).all())
    bad = ((sc.double() - g["scale"]).abs() > bars["scale"]) | ((sh.double() - g["shift"]).abs() > bars["shift"])
    assert not bool(bad.any()), f"{name}: (image, channel) over the bar: {bad.nonzero()[:6].tolist()} (worst {w_sc:.3f} / {w_sh:.3f})"
    return got, stats


@pytest.mark.parametrize("name", [c.name for c in CM.EXACT_CASES])
def test_exact(hip, name):
    _check_exact(hip, name)


@pytest.mark.parametrize("name", ["k9_ks4_skip_two_idle_slices", "fin_cout384_res_ups", "k1_mt1_ragged_ks2"])
def test_second_run_is_bit_identical(hip, name):
    """A split launch with a fused shortcut, a finalizing one and a ragged split GEMM, run again with the scratch re-poisoned."""
    (a, sa), (b, sb) = _check_exact(hip, name), _check_exact(hip, name)
    assert torch.equal(a, b) and torch.equal(sa, sb)


@pytest.mark.parametrize("name", [c.name for c in CM.REAL_CASES])
def test_real(hip, name):
    case, t, plan, ref = _host(name)
    got, act, _ = _launch(hip, case, t, plan)
    err, bound = (got.double() - ref).abs(), CM.real_bound(case, t, E_ACT, plan)
    assert bool(torch.isfinite(got).all())
    ratio = err / bound
    print(f"{name}: worst |err| / bound {float(ratio.max()):.4f} (K = {case.K}, r = {0 if case.out_nchw else (2 if plan['ksplit'] == 1 else 1)})")
    over = (err > bound).nonzero()
    assert over.shape[0] == 0, f"{name}: {over.shape[0]} elements over the bound, first (img, channel, y, x) {over[:6].tolist()}"
    if not case.out_nchw:
        # the partials describe the values the launch wrote: fp32 sums of at most 256 fp16 numbers per tile
        st = act.stats.cpu().reshape(case.B * plan["stats_tiles"], case.Cout, 2).double()
        want = CM.stats_reference(case, got.double(), plan)
        n = case.H * case.W // plan["stats_tiles"]
        bar = 4.0 * n * CM.U * CM.stats_reference(case, got.double().abs(), plan)
        assert bool(((st - want).abs() <= bar + 1e-30).all()), f"{name}: partials off the written values"


# ----------------------------------------------------------------------------- the operand helpers (csrc/act16.hip)
def _affine_ints(g, B, C):
    scale = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (B, C), generator=g)]
    shift = torch.randint(1, 4, (B, C), generator=g).float() * (2.0 * torch.randint(0, 2, (B, C), generator=g).float() - 1.0)
    return scale, shift


def _apply_ref(x, scale, shift, silu=False, pool=False):
    """float64 NCHW: scale x + shift (+ swish) (+ 2x2 mean)."""
    v = x.double()
    if scale is not None:
        v = v * scale.double()[:, :, None, None] + shift.double()[:, :, None, None]
    if silu:
        v = v * torch.sigmoid(v)
    if pool:
        v = (v[:, :, 0::2, 0::2] + v[:, :, 0::2, 1::2] + v[:, :, 1::2, 0::2] + v[:, :, 1::2, 1::2]) / 4.0
    return v


@pytest.mark.parametrize("B,H,W,C0,C1,pool,gn", [(2, 3, 5, 8, 8, False, True), (1, 1, 1, 8, 0, False, True), (2, 2, 6, 8, 8, True, True),
                                                 (2, 2, 6, 8, 8, True, False), (1, 4, 4, 16, 0, False, False)])
def test_gn_apply16_integer_affine_is_exact(hip, B, H, W, C0, C1, pool, gn):
    """Integer affine without swish, bit for bit: a concat of 8 + 8 channels, a launch of ONE thread, 2x2 pooling of a 2 x 6
    image (every 2x2 sum a multiple of 4: the means are integers), the raw pooling / plain concat without parameters."""
    from ddnm_amd import ops
    g = torch.Generator().manual_seed(1601 + 10 * H + W + pool)
    C = C0 + C1
    x = torch.randint(-8, 9, (B, C, H, W), generator=g).float()
    if pool:
        x[:, :, 1::2, 1::2] -= (x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2] + x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2]) % 4
    scale, shift = _affine_ints(g, B, C) if gn else (None, None)
    ref = _apply_ref(x, scale, shift, pool=pool)
    assert torch.equal(ref, ref.round()) and float(ref.abs().max()) <= 2048
    Ho, Wo = ref.shape[2:]
    _poison(B * Ho * Wo * C, torch.float16)
    got = ops.gn_apply16(_nhwc16(x[:, :C0]), _nhwc16(x[:, C0:]) if C1 else None, (_dev(scale), _dev(shift)) if gn else None, False,
                         pool=pool)
    torch.cuda.synchronize()
    assert got.shape == (B, Ho, Wo, C) and got.dtype == torch.float16
    _assert_bits(got.cpu().permute(0, 3, 1, 2).float(), ref.float(), "gn_apply16", ("img", "channel", "y", "x"))


def test_gn_apply16_grid_stride_second_trip(hip):
    """256 * 32768 + 8 threads' worth of work: the grid is capped at 32768 workgroups and the first 8 threads take a second
    trip.  67 M elements: the integer affine is taken in fp32 on the device (exact) and compared there."""
    from ddnm_amd import ops
    B, H, W, C0, C1 = 1, 17, 61681, 32, 32
    assert B * H * W * (C0 + C1) // 8 == 256 * 32768 + 8
    g = torch.Generator(device="cuda").manual_seed(1602)
    x0 = torch.randint(-8, 9, (B, H, W, C0), generator=g, device="cuda", dtype=torch.int8).half()
    x1 = torch.randint(-8, 9, (B, H, W, C1), generator=g, device="cuda", dtype=torch.int8).half()
    scale, shift = _affine_ints(torch.Generator().manual_seed(1603), B, C0 + C1)
    _poison(B * H * W * (C0 + C1), torch.float16)
    got = ops.gn_apply16(x0, x1, (scale.cuda(), shift.cuda()), False)
    want = (torch.cat([x0, x1], 3).float() * scale.cuda()[:, None, None, :] + shift.cuda()[:, None, None, :]).half()
    torch.cuda.synchronize()
    bad = (got != want) | torch.isnan(got)
    n_bad = int(bad.sum())
    assert n_bad == 0, f"gn_apply16: {n_bad} elements differ, first (img, y, x, channel) {bad.nonzero()[:6].tolist()}"


def test_gn_apply16_swish_per_element(hip):
    """|got - ref| <= (2^-11 + E_ACT) |ref| + 2^-24 per element: the swish and one rounding to fp16 (+ subnormal results)."""
    from ddnm_amd import ops
    g = torch.Generator().manual_seed(1604)
    B, H, W, C0, C1 = 2, 4, 6, 8, 8
    x = CM._grid(torch.randn(B, C0 + C1, H, W, generator=g).clamp(-3.6875, 3.6875))
    scale = torch.tensor([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0])[torch.randint(0, 6, (B, C0 + C1), generator=g)]
    shift = 3.0 + CM._grid(torch.rand(B, C0 + C1, generator=g) - 0.5)
    v = x.double() * scale.double()[:, :, None, None] + shift.double()[:, :, None, None]
    assert torch.equal((x * scale[:, :, None, None] + shift[:, :, None, None]).double(), v)
    assert CM.V_RANGE[0] <= float(v.min()) and float(v.max()) <= CM.V_RANGE[1]
    ref = _apply_ref(x, scale, shift, silu=True)
    got = ops.gn_apply16(_nhwc16(x[:, :C0]), _nhwc16(x[:, C0:]), (_dev(scale), _dev(shift)), True)
    torch.cuda.synchronize()
    err = (got.cpu().permute(0, 3, 1, 2).double() - ref).abs()
    bound = (U16 + E_ACT) * ref.abs() + CM.U
    print(f"gn_apply16 swish: worst |err| / bound {float((err / bound).max()):.4f}")
    over = (err > bound).nonzero()
    assert over.shape[0] == 0, f"{over.shape[0]} elements over the bound, first (img, channel, y, x) {over[:6].tolist()}"


def test_im2col16_per_element(hip):
    """1 x 3 x 5 image, 8 + 16 channels, integer affine with a shift that is never zero: col[b, y, x, tap * C + c] is the
    activated pixel under the tap, and exactly zero where the tap falls outside the image (zero padding AFTER the
    activation); bit for bit."""
    import torch.nn.functional as F
    from ddnm_amd import ops
    g = torch.Generator().manual_seed(1605)
    B, H, W, C0, C1 = 1, 3, 5, 8, 16
    C = C0 + C1
    x = torch.randint(-8, 9, (B, C, H, W), generator=g).float()
    scale, shift = _affine_ints(g, B, C)
    act = _apply_ref(x, scale, shift)
    ref = torch.zeros(B, H, W, 9, C, dtype=torch.float64)
    for tap in range(9):
        ref[:, :, :, tap] = F.pad(act, (1, 1, 1, 1))[:, :, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W].permute(0, 2, 3, 1)
    for gn in ((_dev(scale), _dev(shift)), None):
        want = ref if gn is not None else torch.stack([F.pad(x.double(), (1, 1, 1, 1))[:, :, k // 3:k // 3 + H, k % 3:k % 3 + W]
                                                       .permute(0, 2, 3, 1) for k in range(9)], 3)
        _poison(B * H * W * 9 * C, torch.float16)
        got = ops.im2col16(_nhwc16(x[:, :C0]), _nhwc16(x[:, C0:]), gn, False)
        torch.cuda.synchronize()
        assert got.shape == (B, H, W, 9 * C)
        _assert_bits(got.cpu().float().reshape(B, H, W, 9, C), want.float(), f"im2col16 gn={gn is not None}", ("img", "y", "x", "tap", "channel"))


@pytest.mark.parametrize("C,cpad", [(3, 64), (6, 8)])
def test_nchw_to_nhwc16_per_element(hip, C, cpad):
    """Values bit-equal to x.half(), the channel padding exactly zero (the output block is NaN before the launch)."""
    from ddnm_amd import ops
    g = torch.Generator().manual_seed(1606 + C)
    B, H, W = 2, 4, 5
    x = torch.randn(B, C, H, W, generator=g) * 3.0
    _poison(B * H * W * cpad, torch.float16)
    got = ops.nchw_to_nhwc16(x.cuda(), cpad)
    torch.cuda.synchronize()
    assert got.shape == (B, H, W, cpad) and got.dtype == torch.float16
    want = torch.zeros(B, H, W, cpad, dtype=torch.float16)
    want[..., :C] = x.half().permute(0, 2, 3, 1)
    _assert_bits(got.cpu(), want, f"nchw_to_nhwc16 C={C} cpad={cpad}", ("img", "y", "x", "channel"))
