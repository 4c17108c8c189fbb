"""Dynamic range INSIDE one split-fp16 launch, on the CPU: the error model of tests/s16_model.py is pinned against an emulation
of the documented arithmetic (operands split with torch fp16, the three products exact in fp64) for every case of
tests/test_gpu_s16_dynamic_range.py at that test's shapes; the tier split of every case is checked against the caps that make
the GPU test exercise what it claims to; and ops.s16_weight_row_bound -- the quantity Model.load_state_dict guards -- separates
the generators exactly where the tiers do.  Conditions on the model and the inputs, not measurements of a kernel."""
import pytest
import torch

from ddnm_amd import ops
from tests import s16_model as sm

_cache = {}


def _case(c):
    """(layer, amax, [(label, bound, mag, emulated error)]) of a case, computed once; the `ups` form also in its sub-pixel variant."""
    if c["id"] not in _cache:
        t = sm.build_case(c)
        amax = sm.exact_amax(t)
        forms = [("", False)] + ([("sub-pixel", True)] if c["form"] == "ups" else [])
        _cache[c["id"]] = (t, amax, [(lab, *sm.layer_bound(t, amax, sp), sm.emulated_error(t, amax, sp)) for lab, sp in forms])
    return _cache[c["id"]]


def test_element_model():
    v = torch.tensor([0.0, 1e-9, -0.2499, 0.25, -3.0, 2.0 ** 14], dtype=torch.float64)
    want = torch.tensor([0.0, 2.0 ** -25, 2.0 ** -25, 2.0 ** -24, 3 * 2.0 ** -22, 2.0 ** -8], dtype=torch.float64)
    assert torch.equal(sm.elem_eps(v), want)
    # ... and it does bound the split of torch's fp16 (subnormals honoured) over the whole scaled range, sign included
    g = torch.Generator().manual_seed(0)
    x = 2.0 ** (torch.rand(200000, generator=g, dtype=torch.float64) * 45.0 - 30.0)            # 2^-30 ... 2^15
    x = torch.cat([x, -x, torch.tensor([0.25, 0.2499999, 2.0 ** -24, 2.0 ** -26, 32767.9], dtype=torch.float64)])
    hi = x.half().double()
    lo = (x - hi).half().double()
    assert bool(((hi + lo - x).abs() <= sm.elem_eps(x)).all())


def test_operand_scale_rule():
    for m in (3e-9, 0.02, 1.0, 16384.0, 40000.0, 3e7):
        s = sm.operand_scale(m, down_only=False)
        assert 2.0 ** 14 <= m * s < 2.0 ** 15
        assert sm.operand_scale(m, down_only=True) == min(s, 1.0)
    assert sm.operand_scale(0.0, False) == 2.0 ** 94 and sm.operand_scale(1e-30, False) == 2.0 ** 94      # the kernel's clamp
    assert sm.operand_scale(1e30, False) == 2.0 ** -66


@pytest.mark.parametrize("c", sm.CASES, ids=lambda c: c["id"])
def test_emulated_split_arithmetic_stays_inside_the_bound(c):
    for label, bound, mag, err in _case(c)[2]:
        assert bound.shape == err.shape == mag.shape
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{c['id']} {label}: worst emulated error / bound = {worst:.3f}")
        assert bool((err <= bound).all()), (label, worst)
        assert worst > 1e-3, "a bound this loose pins nothing"


@pytest.mark.parametrize("c", sm.CASES, ids=lambda c: c["id"])
def test_tier_caps(c):
    for label, bound, mag, _ in _case(c)[2]:
        rel = sm.channel_tiers(bound, mag)
        n, n_rel = rel.numel(), int(rel.sum())
        print(f"{c['id']} {label}: {n_rel}/{n} channels in the relative regime")
        if c["tier"] == "rel":
            assert n_rel == n, (label, n_rel, n)
        else:
            assert n_rel >= c["tier"][0] * n and n - n_rel >= c["tier"][1] * n, (label, n_rel, n)


def _row_bound(w, *more):
    return ops.s16_weight_row_bound(ops.s16_weight_scale(w, *more), w, *more)


@pytest.mark.parametrize("shape", [(128, 128, 3), (256, 256, 3), (128, 64, 3), (1536, 512, 1), (256, 512, 1), (192, 160, 3)])
def test_weight_row_bound_separates_the_generators(shape):
    cout, cin, k = shape
    lim = ops.S16_WEIGHT_ROW_LIMIT
    assert lim == 2.0 ** -21
    for kind in ("control", "spec", "student_t"):
        v = _row_bound(sm.weights(kind, cout, cin, k, 0))
        assert 2.0 ** -22 * (1 - 1e-12) <= v <= lim, (kind, v)
    for kind in ("outlier_cols", "beyond"):
        v = _row_bound(sm.weights(kind, cout, cin, k, 0))
        assert v > lim, (kind, v)


def test_weight_row_bound_definition():
    # relative regime: exactly 2^-22; zero rows (Cout padding) are skipped, zero ELEMENTS cost nothing
    w = torch.tensor([[1.0, -0.5, 0.0, 0.25], [0.0, 0.0, 0.0, 0.0], [2.0, 1.0, 1.0, -1.0]]).view(3, 4, 1, 1)
    s = ops.s16_weight_scale(w)
    assert ops.s16_weight_row_bound(s, w) == 2.0 ** -22
    assert ops.s16_weight_row_bound(s, ops.pack_conv_weight(w)) == 2.0 ** -22          # 125 rows of padding
    assert ops.s16_weight_row_bound(1.0, torch.zeros(4, 4, 1, 1)) == 0.0
    # one row far below the launch's maximum: its elements keep 2^-25 absolute
    w2 = w.clone()
    w2[1] = torch.tensor([1.0, 1.0, 1.0, 1.0]).view(4, 1, 1) * 2.0 ** -20
    s2 = ops.s16_weight_scale(w2)                                                       # 2^12: the row becomes 2^-8
    assert ops.s16_weight_row_bound(s2, w2) == 2.0 ** -25 / 2.0 ** -8
    # tensors that share the accumulator are judged per row over both
    wsk = torch.ones(3, 2, 1, 1) * 2.0
    assert ops.s16_weight_row_bound(ops.s16_weight_scale(w2, wsk), w2, wsk) == pytest.approx(
        (4 * 2.0 ** -25 + 2 * 2.0 ** 13 * 2.0 ** -22) / (4 * 2.0 ** -8 + 2 * 2.0 ** 13))
    # the phase tensor of an upsample convolution: one row per (phase, output channel)
    wu = sm.weights("control", 64, 32, 3, 0)
    wu[7, :, 0, 0] *= 2.0 ** -24                              # phase (0, 0), tap (0, 0) is ky = kx = 0 alone
    wp = ops.upsample_phase_weights(wu)
    sp = ops.s16_weight_scale(wp)
    rows = (wp.flatten(0, 2).flatten(1).abs() * sp)
    want = float((sm.elem_eps(rows).sum(1) / rows.sum(1)).max())
    assert ops.s16_weight_row_bound(sp, wp) == want


def test_random_state_dict_trips_no_weight_guard():
    """The weights the benchmark and the model tests run on are in the relative regime: the guard changes no launch there."""
    from oracle import cases
    from ddnm_amd.guided_diffusion.models import Model
    cfg = cases.weights.celeba_config(resolution=64, ch=128, ch_mult=(1, 2, 2), attn_resolutions=(16,))
    sd = Model(cfg, device="cpu", split16=True).random_state_dict(seed=7)
    for k, v in sd.items():
        if k.endswith(".weight") and v.dim() == 4 and v.shape[1] % 32 == 0:
            assert _row_bound(v) <= ops.S16_WEIGHT_ROW_LIMIT, k
            if v.shape[-1] == 3:
                wp = ops.upsample_phase_weights(v)
                assert ops.s16_weight_row_bound(ops.s16_weight_scale(wp), wp) <= ops.S16_WEIGHT_ROW_LIMIT, k


def test_loader_guard_drops_exactly_the_layers_with_outlier_columns():
    """Model._guard_weight_range on the state dicts of the model-level GPU test (packing is host code: no GPU needed)."""
    from oracle import cases
    from ddnm_amd.guided_diffusion.models import Model
    cfg = cases.weights.celeba_config(resolution=64, ch=128, ch_mult=(1, 2, 2), attn_resolutions=(16,))
    m = Model(cfg, device="cpu", split16=True)
    sd = m.random_state_dict(seed=7)
    m.load_state_dict(sm.spec_state_dict(sd, 0))
    assert m.s16_dropped == []
    n_s16 = sum(1 for k in m.w if k.endswith((".s16", ".s16_subpixel")))
    m.load_state_dict(sm.spec_state_dict(sd, 0, sm.OUTLIER_LAYERS))
    assert sorted(m.s16_dropped) == sorted(sm.OUTLIER_LAYERS)
    gone = [n + s for n in sm.OUTLIER_LAYERS for s in (".s16", ".s16_subpixel")]
    assert not any(k in m.w for k in gone)
    assert sum(1 for k in m.w if k.endswith((".s16", ".s16_subpixel"))) == n_s16 - 3      # conv1: one packing, upsample: two
    # conv2 and its fused shortcut share a scale: outlier columns in the SHORTCUT drop both packings of the pair
    sd2 = sm.spec_state_dict(sd, 0, ("down.1.block.0.nin_shortcut",))
    m.load_state_dict(sd2)
    assert "down.1.block.0.conv2" in m.s16_dropped
    assert "down.1.block.0.conv2.s16" not in m.w and "down.1.block.0.nin_shortcut.s16" not in m.w
    assert "down.1.block.0.conv1.s16" in m.w
