"""The exact-fp32 convolution kernels (ddnm_conv2d_f32: halo and gather kernel, their split-K reductions;
ddnm_conv3x3_small_cout_f32) per tile, tile width, split and fused option, through ops.conv2d.  Cases, inputs, float64
references and the conditions that make the comparison legitimate are in tests/conv_model.py; test_conv_model_host.py
asserts on the CPU that every case lands on the plan cell it names and that the table covers the coverage list.

Exact cases: integer-valued data whose every intermediate is an integer below 2^24, so the output and the GroupNorm
partials must equal the float64 reference BIT FOR BIT: no tolerance; a misplaced element, tap, channel, image, slice or
statistics tile is a mismatch at a known index.  The output is a view into a NaN-filled buffer with 4096 floats of guard
on both sides (unwritten elements and stray stores show), the per-stream split-K scratch is NaN-filled before every split
launch (a slab element no slice writes surfaces as NaN), and a NaN block of the statistics' size is handed back to the
caching allocator before a launch that emits them.

Real-valued cases (swish prologue): per element
    |got - ref| <= ((K + 8) 2^-24 + E_ACT) (conv(|act|, |w|) + |addends|)
E_ACT is the relative error of the kernels' swish (v_rcp_f32 of 1 + __expf(-v)), measured against float64 swish on the
CPU with the identity launches below (they return the activation itself: every other product is an exact zero) over the
tests' own activation values, v = scale x + shift in [-5.3, 10.9].  Measured on the MI355X: 2.420e-07 (gather 1x1),
2.038e-07 (halo), 1.912e-07 (small_cout); E_ACT is twice the largest (the factor 2: values the probe did not visit).
The identity launches are bounded by E_ACT alone.  With it the four real-valued cases sit at 0.003 .. 0.005 of their
bound (K = 576: the (K + 8) 2^-24 term is a worst case over summation orders)."""
import ctypes
import functools

import pytest
import torch

from tests import conv_model as CM

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 4096
E_ACT = 2 * 2.420e-07


def _nhwc(x):
    return None if x is None else x.permute(0, 2, 3, 1).contiguous().cuda()


def _dev(x):
    return None if x is None else x.contiguous().cuda()


@functools.lru_cache(maxsize=None)
def _host(name):
    """(case, inputs, plan, float64 reference): computed once per case, shared, never modified."""
    case = CM.BY_NAME[name]
    t = CM.make_inputs(case)
    return case, t, CM.plan_of(case), CM.reference(case, t)


def _launch(hip, case, t, plan):
    """One ops.conv2d launch of the case into a guarded NaN buffer -> (NCHW result on the CPU, Act or None)."""
    from ddnm_amd import ops
    shape = (case.B, case.Cout, case.Ho, case.Wo) if case.nchw else (case.B, case.Ho, case.Wo, case.Cout)
    n = case.B * case.Cout * case.Ho * case.Wo
    kw = dict(src1=_nhwc(t["x1"]), bias=_dev(t["bias"]), stride=case.stride, pad=case.pad, ups=case.ups, out_nchw=case.nchw,
              out_hw=(case.Ho, case.Wo), tile=case.tile, emit_stats=case.stats, gn_silu=case.real)
    if case.gn:
        kw["gn"] = (_dev(t["scale"]), _dev(t["shift"]))
    if case.badd:
        kw["badd"], kw["badd_stride"] = _dev(t["badd_rows"])[:, CM.BADD_OFFSET:], CM.badd_stride(case)
    if case.res:
        kw["res"], kw["res_ups"] = _nhwc(t["res"]), case.res_ups
    if case.skip:
        kw["skip"], kw["skip_weight"] = (_nhwc(t["skip0"]), _nhwc(t["skip1"])), ops.pack_skip_weight(t["skip_w"].cuda())
    x0, w = _nhwc(t["x0"]), ops.pack_conv_weight(t["w"].cuda())
    buf = torch.full((n + 2 * GUARD,), NAN, device="cuda")
    out = buf[GUARD:GUARD + n].view(shape)
    if plan["ksplit"] > 1:
        # the scratch ops keeps per (device, stream), obtained as ops._launch_conv obtains it, poisoned as a whole
        need = int(hip.ddnm_conv2d_f32_workspace_floats(ctypes.byref(CM.desc_of(case))))
        assert need == plan["ksplit"] * n
        ops._conv_workspace(out.device, need).fill_(NAN)
    if case.stats:
        poison = torch.full((case.B * plan["stats_tiles"] * case.Cout * 2,), NAN, device="cuda")
        del poison                                                 # the block the statistics tensor is about to be given
    r = ops.conv2d(x0, w, case.Cout, case.k, out=out, **kw)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert bool(torch.isnan(got[:GUARD]).all()), f"{case.name}: store in front of the output"
    assert bool(torch.isnan(got[GUARD + n:]).all()), f"{case.name}: store behind the output"
    got = got[GUARD:GUARD + n].view(shape)
    return (got if case.nchw else got.permute(0, 3, 1, 2)), (r if case.stats else None)


def _assert_bits(got, want, what, names):
    """torch.equal with a report: how many elements differ (NaN counts), and the first few with their indices."""
    if got.shape == want.shape and torch.equal(got, want):
        return
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()
    first = "; ".join(f"{dict(zip(names, i.tolist()))}: got {float(got[tuple(i)])}, expected {float(want[tuple(i)])}" for i in idx[:6])
    raise AssertionError(f"{what}: {idx.shape[0]} of {got.numel()} elements differ ({int(torch.isnan(got).sum())} NaN): {first}")


def _check_exact(hip, name):
    case, t, plan, ref = _host(name)
    want = ref.float()
    assert torch.equal(want.double(), ref)                         # (the preconditions: asserted in the host test)
    got, act = _launch(hip, case, t, plan)
    _assert_bits(got, want, f"{name} output", ("img", "channel", "y", "x"))
    stats = None
    if case.stats:
        tiles = plan["stats_tiles"]
        assert act.tiles == tiles and act.stats is not None
        stats = act.stats.cpu().reshape(case.B * tiles, case.Cout, 2)
        _assert_bits(stats, CM.stats_reference(case, ref, plan).float(), f"{name} statistics ({tiles} tiles per image)",
                     ("tile", "channel", "sum|sumsq"))
    return got, stats


@pytest.mark.parametrize("name", [c.name for c in CM.EXACT_CASES])
def test_exact(hip, name):
    _check_exact(hip, name)


@pytest.mark.parametrize("name", ["skip_stats_split", "split_uneven_6_over_4", "stats_t2_16x24"])
def test_second_run_is_bit_identical(hip, name):
    """A split launch with statistics, the largest split launch and an unsplit one, run again with the scratch re-poisoned."""
    (a, sa), (b, sb) = _check_exact(hip, name), _check_exact(hip, name)
    assert torch.equal(a, b)
    assert (sa is None and sb is None) or torch.equal(sa, sb)


def _rolled(t, j):
    """The inputs with the channels rotated so that channels 4j .. 4j + 3 come first (small_cout has 4 outputs at most)."""
    r = dict(t)
    r["x0"], r["scale"], r["shift"] = (torch.roll(t[k], -4 * j, 1) for k in ("x0", "scale", "shift"))
    return r


@pytest.mark.parametrize("name", [c.name for c in CM.REAL_CASES if c.ident])
def test_swish_of_identity_launch(hip, name):
    """1x1 with W = I on the gather kernel, 3x3 with the centre tap = I on the halo kernel and small_cout: the launch returns
    swish(scale x + shift) of channels 0 .. Cout - 1; relative error against float64 swish <= E_ACT."""
    case, t, plan, _ = _host(name)
    worst, lo, hi = 0.0, 0.0, 0.0
    for j in range(case.Cin // case.Cout):                         # one launch, except small_cout: 4 channels at a time
        tj = _rolled(t, j)
        ref = CM.reference(case, tj)
        got, _ = _launch(hip, case, tj, plan)
        err = (got.double() - ref).abs()
        nz = ref != 0
        worst = max(worst, float((err[nz] / ref[nz].abs()).max()))
        bound = CM.real_bound(case, tj, E_ACT)
        v = (torch.cat([tj["x0"], tj["x1"]], 1) if tj["x1"] is not None else tj["x0"]).double()
        v = v * tj["scale"].double()[:, :, None, None] + tj["shift"].double()[:, :, None, None]
        lo, hi = min(lo, float(v.min())), max(hi, float(v.max()))
        print(f"{name} channels {4 * j}..: largest relative error so far {worst:.3e} (E_ACT {E_ACT:.3e}), v in [{lo:.2f}, {hi:.2f}]")
        assert bool((err <= bound).all()), f"{name}: {int((err > bound).sum())} elements over E_ACT, worst relative {worst:.3e}"


@pytest.mark.parametrize("name", [c.name for c in CM.REAL_CASES if not c.ident])
def test_swish_prologue(hip, name):
    case, t, plan, ref = _host(name)
    got, _ = _launch(hip, case, t, plan)
    err, bound = (got.double() - ref).abs(), CM.real_bound(case, t, E_ACT)
    assert bool(torch.isfinite(got).all())
    print(f"{name}: worst |err| / bound {float((err / bound).max()):.4f} (K = {case.K})")
    assert bool((err <= bound).all()), f"{name}: {int((err > bound).sum())} elements over the bound"
