"""attn16.hip, attn16_bwd.hip and attn_d512.hip at their tiling and softmax edges, judged PER BLOCK: the maximum over
(batch, head, 32-row block) of ||got - ref|| / ||ref|| -- the 32 rows one wave owns -- never one norm over the tensor.

References are float64 on the CPU (tests/attn_model.py): the exact softmax attention and its autograd, and the fp64 model
of the kernels' documented roundings from which the Gaussian and drift bars are DERIVED (twice the model's own worst
per-block error on the same inputs; the factor 2 covers the fp32 accumulation order and the one-ulp v_exp_f32, which the
model does not reproduce).  tests/test_attn_model_host.py asserts, without a GPU, the conditions the cases rely on.

Every test prints its figures before it asserts (pytest -s)."""
import functools
import math

import pytest
import torch

from tests import attn_model as AM

pytestmark = pytest.mark.gpu

B = 2
ATTN16_SHAPES = [(T, C) for T in (64, 128, 192, 320, 384) for C in (64, 192)]
FUSED_SHAPES = [(T, C) for C in (128, 256, 384, 512) for T in (32, 96, 160, 224, 256)]
RESOLVED = 1e-2        # a block whose MODEL error is below this is resolved by the fp16 operands (see _bars)


def _hw(T):
    side = math.isqrt(T)
    return (side, side) if side * side == T else (T // 8, 8)


# ----------------------------------------------------------------------------- attn16: CPU side (cached, never modified)
def _case16(kind, T, nh, bwd=False):
    lead = (B, nh)
    if kind == "gauss":
        return AM.gaussian_case(T, 64, 0.8 if bwd else 1.5, lead=lead)        # amplitudes of the existing tests
    if kind in ("rising", "falling"):
        return AM.drift_case(T, 64, kind == "rising", lead=lead)
    if kind == "perm":
        return AM.permutation_case(T, 64, 8.0, 0.125, lead=lead)
    if kind == "large":
        return AM.permutation_case(T, 64, 62.5, 0.125, lead=lead)
    if kind == "flat":
        return AM.flat_case(T, 64, lead=lead)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _fwd_ref(kind, T, nh, bwd=False):
    """(exact o, exact lse, model o, model lse, worst per-block model error, worst model lse error)."""
    cs = _case16(kind, T, nh, bwd)
    o, lse = AM.exact_attention(cs["q"], cs["k"], cs["v"], 0.125)
    om, lm = AM.attn16_model_fwd(cs["q"], cs["k"], cs["v"])
    return o, lse, om, lm, AM.worst_block(om, o), float((lm - lse).abs().max())


def _bars(model, exact):
    """(bar over all blocks, mask of resolved blocks, bar over the resolved blocks) = twice the model's worst per-block
    error, over all blocks and over those the model resolves.  A drift case leaves key blocks whose probabilities all
    underflow fp16: their dk / dv are rounding residue of norm ~ 1e-10 with a relative model error of order 1, which
    would make the bar over all blocks vacuous on its own."""
    e = AM.block_errors(model, exact)
    ok = e < RESOLVED
    return 2.0 * float(e.max()), ok, 2.0 * float(e[ok].max()) if bool(ok.any()) else 0.0


@functools.lru_cache(maxsize=None)
def _bwd_ref(kind, T, nh, expo=0):
    """Exact gradients for dO 2^expo and the model's, from the model's own forward (o, lse)."""
    cs = _case16(kind, T, nh, bwd=True)
    dO = AM.grad_case(T, 64, lead=(B, nh)) * 2.0 ** expo
    _, _, om, lm, _, _ = _fwd_ref(kind, T, nh, True)
    exact = AM.exact_attention_grads(cs["q"], cs["k"], cs["v"], dO, 0.125)
    *model, ds = AM.attn16_model_bwd(cs["q"], cs["k"], cs["v"], om, lm, dO, return_ds=True)
    return dO, exact, tuple(model), ds


# ----------------------------------------------------------------------------- attn16: GPU side
def _gpu_fwd(cs, nh, lse=True):
    from ddnm_amd import ops
    T = cs["q"].shape[-2]
    C = 64 * nh
    qd = AM.pack_legacy(cs["q"], cs["k"], cs["v"]).half().view(B, *_hw(T), 3 * C).cuda()
    l = torch.empty(B, nh, T, device="cuda") if lse else None
    o = ops.attn16(qd, C, lse=l)
    torch.cuda.synchronize()
    return qd, o, l


def _heads(t, nh):
    Bn = t.shape[0]
    return AM.tokens_to_heads(t.cpu().double().reshape(Bn, -1, 64 * nh), nh)


def _gpu_bwd(cs, nh, dO):
    from ddnm_amd import ops
    T = cs["q"].shape[-2]
    qd, o, l = _gpu_fwd(cs, nh)
    g = AM.heads_to_tokens(dO).half().view(B, *_hw(T), 64 * nh).cuda()
    assert torch.equal(g.cpu().double().view(B, T, -1), AM.heads_to_tokens(dO))          # dO is fp16-exact
    d = ops.attn16_bwd(qd, o, g, l)
    torch.cuda.synchronize()
    return AM.unpack_legacy(d.cpu().double().view(B, T, -1), nh), o


@pytest.mark.parametrize("kind", ["gauss", "rising", "falling"])
@pytest.mark.parametrize("T,C", ATTN16_SHAPES)
def test_attn16_per_block_against_exact(hip, T, C, kind):
    """ddnm_attn16_d64_lse (and ddnm_attn16_d64: same bits) per 32-query block against the exact float64 attention of the
    fp16 inputs.  T % 128 != 0 runs attn16_d64_kernel<2> with up to five key tiles (cross-tile prefetch of k0..k3 / v0..v3,
    alpha rescale), T % 128 == 0 the 4-wave kernel.  gauss: amplitude 1.5 as test_attn16_matches_legacy_qkv_attention;
    rising / falling: the row maximum of every query lies in the last / first key tile (alpha << 1 resp. exp2 underflow
    below fp16 in every later tile).

    bar = 2 x the worst per-block error of attn16_model against the exact reference on the same inputs.  Measured model
    errors over the ten shapes (CPU):  gauss 2.27e-4 .. 2.45e-4  -> bars 4.5e-4 .. 4.9e-4;  rising 2.57e-4 .. 2.78e-4,
    falling 2.55e-4 .. 2.81e-4  -> bars 5.1e-4 .. 5.6e-4.  All per-block bars lie BELOW the whole-tensor 2e-3 of the
    existing test.  lse: twice the model's worst |lse - exact| (model 1.3e-4 .. 2.8e-4, from summing the rounded P).
    Measured on the MI355X: the kernel's worst per-block error is the model's to within 0.5 % in all thirty cases, its
    lse error the model's to within 4 %."""
    nh = C // 64
    o, lse, _, _, e_model, l_model = _fwd_ref(kind, T, nh)
    cs = _case16(kind, T, nh)
    _, got, l = _gpu_fwd(cs, nh)
    _, got2, _ = _gpu_fwd(cs, nh, lse=False)
    got_h = _heads(got, nh)
    err = AM.worst_block(got_h, o)
    l_err = float((l.cpu().double() - lse).abs().max())
    print(f"attn16 {kind} T={T} C={C}: per-block {err:.3e} (model {e_model:.3e}, bar {2 * e_model:.3e}); "
          f"lse {l_err:.3e} (model {l_model:.3e})")
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(l).all())
    assert torch.equal(got, got2)
    assert err <= 2.0 * e_model, (err, e_model)
    assert l_err <= 2.0 * l_model, (l_err, l_model)


@pytest.mark.parametrize("kind", ["perm", "large"])
@pytest.mark.parametrize("T,C", ATTN16_SHAPES)
def test_attn16_one_hot_rows_return_the_target_value(hip, T, C, kind):
    """Keys of +-1, q_i = c k_pi(i), pi(i) = (77 i + 13) mod T: out[i] = v[pi(i)] to one fp16 ulp per element, which
    pins every key position of the V^T image ([0-3, 8-11, 4-7, 12-15] inside a group of 16) and every tile.  Every
    off-target probability rounds to zero in fp16, the target's is exactly 1, and partial sums of earlier tiles are scaled
    by alpha <= 2^-39 against |v| ratios of at most 4.  perm: c = 8 (target logit 64 nats, margin >= 28); large: c = 62.5
    (target logit 500 nats, all others >= 218 nats below): no NaN / inf.  lse = the exact base-2 log-sum-exp to
    2^-20 max(1, |lse|).  Measured on the MI355X: the match is BIT-EXACT for every shape of both kinds."""
    nh = C // 64
    cs = _case16(kind, T, nh)
    want = cs["v"][..., cs["pi"], :]
    _, lse_ref = AM.exact_attention(cs["q"], cs["k"], cs["v"], 0.125)
    _, got, l = _gpu_fwd(cs, nh)
    got_h, l = _heads(got, nh), l.cpu().double()
    diff = (got_h - want).abs()
    l_err = ((l - lse_ref).abs() / lse_ref.abs().clamp_min(1.0)).max()
    print(f"attn16 {kind} T={T} C={C}: bit-exact {bool(torch.equal(got_h, want))}, max |diff| / ulp "
          f"{float((diff / AM.ulp16(want)).max()):.2f}, lse rel {float(l_err):.3e} (bar {2.0 ** -20:.3e})")
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(l).all())
    assert bool((diff <= AM.ulp16(want)).all())
    assert float(l_err) <= 2.0 ** -20


@pytest.mark.parametrize("T,C", ATTN16_SHAPES)
def test_attn16_flat_rows_return_the_mean(hip, T, C):
    """q = 0: every probability is exactly 1 in the kernel's running sums, every output row is the fp16 rounding of the
    mean of v over the tokens (to one fp16 ulp) and lse = log2 T to 2^-20.  Measured on the MI355X: every element equals the
    rounded mean bit for bit; |lse - log2 T| = 0 (T = 64, 128), 1.3e-7 (192), 7.1e-8 (320), 6.1e-7 (384) against 9.5e-7."""
    nh = C // 64
    cs = _case16("flat", T, nh)
    _, got, l = _gpu_fwd(cs, nh)
    got_h = _heads(got, nh)
    mean = AM.r16(cs["v"].mean(dim=-2, keepdim=True)).expand_as(got_h)
    diff = (got_h - mean).abs()
    l_err = float((l.cpu().double() - math.log2(T)).abs().max())
    print(f"attn16 flat T={T} C={C}: max |diff| / ulp {float((diff / AM.ulp16(mean)).max()):.2f}, lse {l_err:.3e}")
    assert bool((diff <= AM.ulp16(mean)).all())
    assert l_err <= 2.0 ** -20


def test_attn16_rejects_a_token_count_that_is_no_multiple_of_the_tile(hip):
    """T = 96: the shape error through ops.attn16, and nothing is launched (the output of the C entry point stays as it
    was)."""
    from ddnm_amd import ops
    from ddnm_amd._lib import DDNMHipError
    qd = torch.zeros(1, 12, 8, 192, dtype=torch.float16, device="cuda")
    with pytest.raises(DDNMHipError, match="shape"):
        ops.attn16(qd, 64)
    with pytest.raises(DDNMHipError, match="shape"):
        ops.attn16(qd, 64, lse=torch.empty(1, 1, 96, device="cuda"))
    out = torch.full((1, 96, 64), 7.0, dtype=torch.float16, device="cuda")
    lse = torch.full((1, 1, 96), 7.0, device="cuda")
    code = hip.ddnm_attn16_d64_lse(qd.data_ptr(), out.data_ptr(), lse.data_ptr(), 1, 96, 64, ops._stream())
    dq = torch.full((1, 96, 192), 7.0, dtype=torch.float16, device="cuda")
    code_b = hip.ddnm_attn16_d64_bwd(qd.data_ptr(), out.data_ptr(), out.data_ptr(), lse.data_ptr(), lse.data_ptr(),
                                     dq.data_ptr(), 1, 96, 64, ops._stream())
    torch.cuda.synchronize()
    assert code != 0 and code_b != 0
    assert bool((out == 7.0).all()) and bool((lse == 7.0).all()) and bool((dq == 7.0).all())


# ----------------------------------------------------------------------------- attn16_bwd
def _judge_bwd(tag, got, exact, model, scale=1.0):
    worst = {}
    for name, g, e, m in zip(("dq", "dk", "dv"), got, exact, model):
        bar_all, ok, bar_ok = _bars(m, e)
        errs = AM.block_errors(g, e * scale)
        e_all, e_ok = float(errs.max()), float(errs[ok].max())
        print(f"{tag} {name}: per-block {e_all:.3e} (bar {bar_all:.3e}); resolved blocks {int(ok.sum())}/{ok.numel()} "
              f"{e_ok:.3e} (bar {bar_ok:.3e})")
        worst[name] = (e_all, bar_all, e_ok, bar_ok)
    for name, (e_all, bar_all, e_ok, bar_ok) in worst.items():
        assert e_all <= bar_all and e_ok <= bar_ok, (tag, name, e_all, bar_all, e_ok, bar_ok)


@pytest.mark.parametrize("kind", ["gauss", "rising", "falling"])
@pytest.mark.parametrize("T,C", ATTN16_SHAPES)
def test_attn16_bwd_per_block_against_autograd(hip, T, C, kind):
    """ddnm_attn16_d64_bwd with lse and o from the forward launch (as the classifier does): dq, dk, dv separately, per
    32-row block (32 queries of the dq kernel, 32 keys of the dk / dv kernel), against float64 autograd on the fp16 inputs.
    T % 128 != 0 runs attn16_bwd_dq_kernel<2> / attn16_bwd_dkv_kernel<2> for up to five trips of their loops.

    bar = 2 x the worst per-block error of attn16_model (forward + backward) against the exact gradients.  Measured model
    errors over the ten shapes (CPU), gauss (amplitude 0.8 as test_attention16_backward): dq 3.02e-4 .. 3.17e-4,
    dk 3.00e-4 .. 3.24e-4, dv 2.91e-4 .. 3.22e-4 -> bars 5.8e-4 .. 6.5e-4, BELOW the whole-tensor 4e-3.  Drift: dq
    5.7e-4 .. 1.7e-3 -> bars 1.1e-3 .. 3.4e-3 (dS has a handful of significant keys per query, each rounded to fp16).  For
    T >= 128 the dk / dv blocks of keys whose probabilities all underflow fp16 are rounding residue (model error of order
    1: the bar over all blocks, 2.0 .. 3.3, is ABOVE the 4e-3 of the existing test and says nothing); the blocks the model
    resolves (model error < 1e-2; there dk <= 1.2e-3, dv <= 4.6e-3) are therefore held to twice the model's worst error
    among them as well.  Measured on the MI355X: error / bar between 0.50 and 0.52 for dq, dk and dv in all thirty cases."""
    nh = C // 64
    dO, exact, model, _ = _bwd_ref(kind, T, nh)
    got, _ = _gpu_bwd(_case16(kind, T, nh, bwd=True), nh, dO)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    _judge_bwd(f"attn16_bwd {kind} T={T} C={C}", got, exact, model)


@pytest.mark.parametrize("T,C", ATTN16_SHAPES)
def test_attn16_bwd_one_hot_rows(hip, T, C):
    """Permutation case (c = 8): P is the permutation matrix, so dv[pi(i)] = dO[i] to one fp16 ulp, and dq, dk vanish in
    exact arithmetic (dP = D on the target, P = 0 elsewhere).  What is left is the difference of the two 64-term fp32 dot
    products dP and D over the same products:  |dq_i| <= 2 * 64 * 2^-24 * sum_d |dO[i,d] v[pi(i),d]| * max|k| / 8, and
    |dk_pi(i)| <= the same with max|q| = 8 for max|k| = 1, each plus half an fp16 ulp of the bound for the final rounding."""
    nh = C // 64
    cs = _case16("perm", T, nh, bwd=True)
    dO = AM.grad_case(T, 64, lead=(B, nh))
    (dq, dk, dv), o = _gpu_bwd(cs, nh, dO)
    pi = cs["pi"]
    assert torch.equal(_heads(o, nh), cs["v"][..., pi, :])           # the forward is bit-exact here: D is the exact sum
    ddv = (dv[..., pi, :] - dO).abs()
    core = 2.0 * 64.0 * 2.0 ** -24 * (dO * cs["v"][..., pi, :]).abs().sum(dim=-1, keepdim=True) / 8.0
    bq = core * 1.0
    bk = torch.empty_like(core)
    bk[..., pi, :] = core * 8.0
    bq, bk = bq + 0.5 * AM.ulp16(bq), bk + 0.5 * AM.ulp16(bk)
    print(f"attn16_bwd perm T={T} C={C}: dv bit-exact {bool(torch.equal(dv[..., pi, :], dO))}; max |dq| / bound "
          f"{float((dq.abs() / bq).max()):.3f}, max |dk| / bound {float((dk.abs() / bk).max()):.3f}")
    assert bool((ddv <= AM.ulp16(dO)).all())
    assert bool((dq.abs() <= bq).all()) and bool((dk.abs() <= bk).all())


@pytest.mark.parametrize("expo", [-6, 6])
def test_attn16_bwd_is_linear_in_the_output_gradient(hip, expo):
    """The classifier pre-scales its gradient by 2^10; here dO 2^-6 and dO 2^6 at T = 192, C = 64 (Gaussian case), judged
    against the same exact gradients scaled, with the bars of the unscaled case: the model shows no fp16 overflow of dS
    (max |dS| 2^6 = 50 << 65504) and no effect of underflow (model errors at 2^-6: dq 3.02e-4, dk 3.07e-4, dv 2.91e-4
    against 3.03e-4, 3.06e-4, 2.91e-4 unscaled).  By the same criteria (errors within 5 % of the unscaled ones, dS finite
    in fp16) the model supports 2^-8 .. 2^12; at 2^-9 the subnormal dS raise its dq / dk errors by 21 %, and beyond 2^12
    dO itself (|dO| < 7.5 here) leaves fp16."""
    T, nh = 192, 1
    dO0, exact0, model0, _ = _bwd_ref("gauss", T, nh)
    dO, exact, model, ds = _bwd_ref("gauss", T, nh, expo)
    assert float(ds.abs().max()) < 65504.0
    for m, e, m0, e0 in zip(model, exact, model0, exact0):
        assert AM.worst_block(m, e) <= 1.05 * AM.worst_block(m0, e0)
    got, _ = _gpu_bwd(_case16("gauss", T, nh, bwd=True), nh, dO)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    _judge_bwd(f"attn16_bwd dO*2^{expo}", got, exact0, model0, scale=2.0 ** expo)


# ----------------------------------------------------------------------------- attn_fused (attn_d512.hip)
def _tight(t):
    """Largest power of two s with max|t| s < 2^15."""
    m = float(t.abs().max())
    e = math.floor(15.0 - math.log2(m))
    if m * 2.0 ** e >= 2.0 ** 15:
        e -= 1
    return 2.0 ** e


def _scale_sets(qk, v):
    """tight, and loose = tight / 2^6 (a static per-checkpoint bound is loose in production)."""
    return [("tight", _tight(qk), _tight(v)), ("loose", _tight(qk) / 64.0, _tight(v) / 64.0)]


def _fused(cs, s_qk, s_v, C):
    from ddnm_amd import ops
    T = cs["q"].shape[-2]
    qkv = torch.cat([cs["q"], cs["k"], cs["v"]], dim=-1).float().cuda().contiguous()
    got = ops.attn_fused(qkv, B, T, C, s_qk, s_v, float(int(C) ** (-0.5)))
    torch.cuda.synchronize()
    return qkv, got


def _three_launch(qkv, T, C):
    from ddnm_amd import ops
    S = torch.empty(B, T, T, device="cuda")
    f = qkv.view(-1)
    ops.bgemm(f[0:], f[C:], S, T, T, C, lda=3 * C, ldb=3 * C, ldc=T, transb=True, batch=B, sA=(T * 3 * C, 0), sB=(T * 3 * C, 0),
              sC=(T * T, 0))
    ops.softmax_rows_(S, B * T, T, T, float(int(C) ** (-0.5)))
    o3 = torch.empty(B, T, C, device="cuda")
    ops.bgemm(S, f[2 * C:], o3, T, C, T, lda=T, ldb=3 * C, ldc=C, transb=False, batch=B, sA=(T * T, 0), sB=(T * 3 * C, 0),
              sC=(T * C, 0))
    torch.cuda.synchronize()
    return o3


@functools.lru_cache(maxsize=None)
def _fused_gauss_case(T, C):
    """The construction of test_fused_single_head_attention: Gaussian of magnitude mag, q and k brought to scores of a few
    units; mag cycles through 1, 40, 1e-3 over the grid."""
    mag = (1.0, 40.0, 1e-3)[(T // 32 + C // 128) % 3]
    g = torch.Generator().manual_seed(T + C)
    qkv = (torch.randn(B, T, 3 * C, generator=g) * mag)
    qkv[..., :2 * C] *= (4.0 / (mag * C ** 0.25))
    q, k, v = (qkv[..., i * C:(i + 1) * C].double() for i in range(3))
    return {"q": q, "k": k, "v": v, "scale": C ** -0.5}


def _judge_fused(tag, cs, T, C, bar=2e-6):
    want, _ = AM.exact_attention(cs["q"], cs["k"], cs["v"], C ** -0.5)
    qk = torch.cat([cs["q"], cs["k"]], dim=-1)
    res = []
    for name, s_qk, s_v in _scale_sets(qk, cs["v"]):
        qkv, got = _fused(cs, s_qk, s_v, C)
        e_f = AM.block_errors(got.cpu(), want)
        e_3 = AM.block_errors(_three_launch(qkv, T, C).cpu(), want)
        print(f"{tag} T={T} C={C} {name} (s_qk 2^{math.log2(s_qk):.0f}, s_v 2^{math.log2(s_v):.0f}): per-block fused "
              f"{float(e_f.max()):.3e}, three-launch {float(e_3.max()):.3e}, worst (e_f - 2 e_3) {float((e_f - 2 * e_3).max()):.3e}")
        res.append((name, bool(torch.isfinite(got).all()), e_f, e_3))
    for name, finite, e_f, e_3 in res:
        assert finite, name
        assert float(e_f.max()) < bar, (name, float(e_f.max()), bar)
        assert bool((e_f <= 2.0 * e_3 + 3e-7).all()), (name, float((e_f - 2 * e_3).max()))


@pytest.mark.parametrize("T,C", FUSED_SHAPES)
def test_fused_attention_gaussian_per_block(hip, T, C):
    """ddnm_attn_fused_f32 per (image, 32-query block = one workgroup) against fp64, all four attn_d512_kernel<NB>
    (C = 128 NB), T = 32 (three of the four waves skip phase 1), odd tile counts T = 160, 224 (the `two` branch taken by
    some waves only), with tight and loose operand scales: under the existing 2e-6, and e_f <= 2 e_3 + 3e-7 against the
    three-launch route per block.  Measured on the MI355X over the twenty shapes: worst per-block e_f 2.6e-7 .. 5.8e-7,
    e_3 3.9e-7 .. 7.8e-7, identical for the two scale sets; worst e_f - 2 e_3 = -4.2e-7."""
    _judge_fused("fused gauss", _fused_gauss_case(T, C), T, C)


@pytest.mark.parametrize("rising", [True, False])
def test_fused_attention_drift(hip, rising):
    """Row maximum in the last / first keys at T = 256, C = 512; per block against the three-launch route as in the
    Gaussian case (e_f <= 2 e_3 + 3e-7).  The absolute bar is the existing 2e-6 scaled by the size of the logits: the
    scores live in fp32 (in LDS here, in HBM on the three-launch route), the relative error of a probability is the
    ABSOLUTE error of its logit, and that grows with the logit's magnitude (fp32 spacing).  2e-6 is the bar of the Gaussian
    construction, whose largest |logit| at this shape is L_g = 3.2 nats; the drift cases reach L_d = 40.4 nats, so
    bar = 2e-6 L_d / L_g = 2.6e-5.  Measured on the MI355X: fused 7.1e-6 / 7.4e-6, three-launch 1.28e-5 / 1.17e-5."""
    T, C = 256, 512
    cs = AM.drift_case(T, C, rising, scale=C ** -0.5, sigma=4.0 / C ** 0.25, lead=(B,), half=False)
    gs = _fused_gauss_case(T, C)
    L_g = float(AM.exact_logits(gs["q"], gs["k"], C ** -0.5).abs().max())
    L_d = float(AM.exact_logits(cs["q"], cs["k"], C ** -0.5).abs().max())
    print(f"fused drift rising={rising}: largest |logit| {L_d:.2f} nats against {L_g:.2f} of the Gaussian case -> bar {2e-6 * L_d / L_g:.3e}")
    _judge_fused(f"fused drift rising={rising}", cs, T, C, bar=2e-6 * L_d / L_g)


@pytest.mark.parametrize("T,C", FUSED_SHAPES)
def test_fused_attention_one_hot_rows(hip, T, C):
    """Permutation case with c = 4 (d = C, scale C^-0.5) and v = Gaussian x {1e-3, 1, 40}:
    |out[i] - v[pi(i)]| <= 2^-21 max|v| + (off-target mass of the fp64 reference) max|v| element-wise (2^-22 is the
    documented hi/lo operand error; the off-target probabilities times 2^14 lie below half the smallest fp16 subnormal).
    At T = 224 pi is 7-to-1, which this forward-only statement does not mind.  Measured on the MI355X: worst
    |diff| / bound 0.11 .. 0.25."""
    worst = []
    for vmag in (1e-3, 1.0, 40.0):
        cs = AM.permutation_case(T, C, 4.0, C ** -0.5, lead=(B,), vkind="gauss", vmag=vmag)
        want = cs["v"][..., cs["pi"], :]
        _, _, mass = AM.permutation_margins(cs)
        vmax = cs["v"].abs().amax(dim=(-1, -2), keepdim=True)
        bound = (2.0 ** -21 + mass) * vmax
        for name, s_qk, s_v in _scale_sets(torch.cat([cs["q"], cs["k"]], dim=-1), cs["v"]):
            _, got = _fused(cs, s_qk, s_v, C)
            ratio = float(((got.cpu().double() - want).abs() / bound).max())
            print(f"fused perm T={T} C={C} v x {vmag:g} {name}: max |diff| / bound {ratio:.3f}")
            worst.append((vmag, name, bool(torch.isfinite(got).all()), ratio))
    for vmag, name, finite, ratio in worst:
        assert finite and ratio <= 1.0, (vmag, name, ratio)


@pytest.mark.parametrize("T,C", FUSED_SHAPES)
def test_fused_attention_flat_rows(hip, T, C):
    """q = 0: every row is the mean of v, per block under the same 2e-6 (measured on the MI355X: 4.0e-8 .. 1.5e-7)."""
    cs = AM.flat_case(T, C, lead=(B,), half=False)
    mean = cs["v"].mean(dim=-2, keepdim=True).expand_as(cs["v"])
    for name, s_qk, s_v in _scale_sets(cs["k"], cs["v"]):
        _, got = _fused(cs, s_qk, s_v, C)
        err = AM.worst_block(got.cpu(), mean)
        print(f"fused flat T={T} C={C} {name}: per-block {err:.3e}")
        assert bool(torch.isfinite(got).all()) and err < 2e-6, (name, err)


@pytest.mark.parametrize("T,C", [(48, 128), (288, 128), (64, 64), (64, 640)])
def test_fused_attention_rejects_unsupported_shapes(hip, T, C):
    from ddnm_amd import ops
    from ddnm_amd._lib import DDNMHipError
    assert ops.attn_fused_supported(T, C) is False
    qkv = torch.zeros(1, T, 3 * C, device="cuda")
    out = torch.full((1, T, C), 7.0, device="cuda")
    with pytest.raises(DDNMHipError, match="shape"):
        ops.attn_fused(qkv, 1, T, C, 1.0, 1.0, C ** -0.5, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
