"""The AttentionPool2d chain of the classifier (csrc/backward.hip) and its two row kernels, one entry point at a time,
called through `_lib.lib()` and `check` like test_gn_backward_kernel.  References are float64 torch expressions of
AttentionPool2d (guided_diffusion/unet.py:22-51) and their autograd.

Tolerances.  The kernels are plain fp32 with sums of at most 1024 terms, so no flat constant: an element produced by a
reduction of n terms t_i may be off by   4 n 2^-24 sum_i |t_i|   with the |t_i| taken from the float64 reference
(`_red`).  Where an element is a chain of reductions the bars are chained the same way (an input bar e of a factor x
enters the next stage as e |y| for the other factor y); the chain is written out next to each test.  Outputs rounded to
fp16 get half an fp16 ulp on top; 2^-126 is added wherever a probability may be an fp32 subnormal that the hardware may
flush."""
import math

import pytest
import torch

from tests import attn_model as AM

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
FLOOR = 2.0 ** -126


def _red(n, abs_sum):
    return 4.0 * n * EPS * abs_sum


def _p(t):
    return t.data_ptr()


def _worst(got, ref, bar):
    return float(((got.double().cpu() - ref).abs() / bar).max())


# ----------------------------------------------------------------------------- tokens
def _token_case(HW, C, half):
    g = torch.Generator().manual_seed(1000 * HW + C + int(half))
    Bn = 2
    h = torch.randn(Bn, HW, C, generator=g)
    if half:
        h = h.half().float()
    sc, sh = torch.randn(Bn, C, generator=g), torch.randn(Bn, C, generator=g)
    pos = torch.randn(C, HW + 1, generator=g) / C ** 0.5
    return Bn, h, sc, sh, pos


@pytest.mark.parametrize("half", [False, True], ids=["f32", "h16"])
@pytest.mark.parametrize("C", [64, 192, 512])
@pytest.mark.parametrize("HW", [1, 4, 64, 256])
def test_pool_tokens(hip, HW, C, half):
    """ddnm_pool_tokens_f32 / _h16: X[b][1 + p] = act + pos[:, 1 + p], X[b][0] = mean_p act + pos[:, 0] with
    act = silu(h a + t0), random per-(b, c) scale a and shift t0, pos of layout [C][HW + 1].  C = 192 leaves 64 of the 256
    threads idle, C = 512 gives every thread two channels.  The h16 variant reads fp16 h (reference on the same rounded
    values); the tokens stay fp32.
    Bars: act is a chain of 3 terms (h a, t0 and the activation itself; silu is 1.1-Lipschitz):
    e_act = _red(3, |h a| + |t0| + |act|); a token adds the 2-term sum act + pos; the class token the (HW + 1)-term sum
    of act / HW and pos, plus the mean of e_act."""
    from ddnm_amd import ops
    from ddnm_amd._lib import check
    Bn, h, sc, sh, pos = _token_case(HW, C, half)
    hd, a, t0 = h.double(), sc.double()[:, None, :], sh.double()[:, None, :]
    act = torch.nn.functional.silu(hd * a + t0)
    posT = pos.double().t()                                                   # [T][C]
    ref = torch.cat([act.mean(dim=1, keepdim=True), act], dim=1) + posT[None]
    e_act = _red(3, (hd * a).abs() + t0.abs() + act.abs())
    bar = torch.cat([e_act.mean(dim=1, keepdim=True) + _red(HW + 1, act.abs().mean(dim=1, keepdim=True) + posT[None, :1].abs()),
                     e_act + _red(2, act.abs() + posT[None, 1:].abs())], dim=1)
    X = torch.full((Bn, HW + 1, C), float("nan"), device="cuda")
    hg, scg, shg, posg = (h.half() if half else h).cuda(), sc.cuda(), sh.cuda(), pos.cuda()
    fn = hip.ddnm_pool_tokens_h16 if half else hip.ddnm_pool_tokens_f32
    check(fn(_p(hg), _p(scg), _p(shg), _p(posg), _p(X), Bn, HW, C, ops._stream()), "ddnm_pool_tokens")
    torch.cuda.synchronize()
    w = _worst(X, ref, bar)
    print(f"pool_tokens HW={HW} C={C} half={half}: worst |err| / bar {w:.3f}")
    assert bool(torch.isfinite(X).all()) and w <= 1.0


@pytest.mark.parametrize("half", [False, True], ids=["f32", "h16"])
@pytest.mark.parametrize("C", [64, 192, 512])
@pytest.mark.parametrize("HW", [1, 4, 64, 256])
def test_pool_tokens_bwd(hip, HW, C, half):
    """ddnm_pool_tokens_bwd_f32 / _h16: d act[b][p] = dX[b][1 + p] + dX[b][0] / HW, a 2-term sum; the h16 output is rounded
    once (half an fp16 ulp on top)."""
    from ddnm_amd import ops
    from ddnm_amd._lib import check
    g = torch.Generator().manual_seed(7 * HW + C)
    Bn = 2
    dX = torch.randn(Bn, HW + 1, C, generator=g)
    d = dX.double()
    ref = d[:, 1:] + d[:, :1] / HW
    bar = _red(2, d[:, 1:].abs() + d[:, :1].abs() / HW)
    if half:
        bar = bar + 0.5 * AM.ulp16(ref)
    out = torch.full((Bn, HW, C), float("nan"), device="cuda", dtype=torch.float16 if half else torch.float32)
    fn = hip.ddnm_pool_tokens_bwd_h16 if half else hip.ddnm_pool_tokens_bwd_f32
    dXg = dX.cuda()
    check(fn(_p(dXg), _p(out), Bn, HW, C, ops._stream()), "ddnm_pool_tokens_bwd")
    torch.cuda.synchronize()
    w = _worst(out, ref, bar)
    print(f"pool_tokens_bwd HW={HW} C={C} half={half}: worst |err| / bar {w:.3f}")
    assert bool(torch.isfinite(out).all()) and w <= 1.0


# ----------------------------------------------------------------------------- the class-token attention
def _attn_case(T, C, heads):
    """qkv [3][T][3C] (q | k | v blocks of C, head-major inside).  Image 0: Gaussian; image 1: a flat query (q of the class
    token = 0); image 2: a one-hot query (q of the class token = 8 k of token T // 2, a margin of tens of nats)."""
    g = torch.Generator().manual_seed(31 * T + C + heads)
    qkv = torch.randn(3, T, 3 * C, generator=g)
    qkv[1, 0, :C] = 0.0
    qkv[2, 0, :C] = 8.0 * qkv[2, T // 2, C:2 * C]
    da0 = torch.randn(3, C, generator=g)
    return qkv, da0


def _attn_ref(qkv, heads):
    """P [B][heads][T] and a0 [B][C] of the class token, float64, differentiable in qkv."""
    Bn, T, C3 = qkv.shape
    C = C3 // 3
    ch = C // heads
    q0 = qkv[:, 0, :C].reshape(Bn, heads, ch)
    k = qkv[:, :, C:2 * C].reshape(Bn, T, heads, ch)
    v = qkv[:, :, 2 * C:].reshape(Bn, T, heads, ch)
    P = torch.softmax(torch.einsum("bhc,bshc->bhs", q0, k) / math.sqrt(ch), dim=-1)
    return P, torch.einsum("bhs,bshc->bhc", P, v).reshape(Bn, C), (q0, k, v)


@pytest.mark.parametrize("C,heads", [(64, 1), (128, 4), (256, 2), (512, 8)])
@pytest.mark.parametrize("T", [1, 2, 63, 65, 257, 1024])
def test_pool_attention_forward_and_backward(hip, T, C, heads):
    """ddnm_pool_attn_fwd_f32 (P, a0) and ddnm_pool_attn_bwd_f32 (all of dqkv) for head widths ch = 32, 64, 128, T = 1,
    around the 64-lane stride (63, 65), 257 and the bound T = 1024 of the 1024-entry LDS array; Gaussian, flat and one-hot
    class-token queries.  dqkv is pre-filled with NaN: the result is finite and the dq rows of tokens >= 1 are exactly 0.
    The backward launch gets the reference P rounded to fp32 (a relative 2^-24, inside the bars).

    Bars (s = ch^-1/2; |.| sums from the float64 reference):
      logit  A_s = s sum_c |q_c k_sc|;  P_s relative: _red(ch, A_s + max A) + _red(T, 1)   (its logit, the row maximum, the
             T-term normaliser);  a0_c: _red(T, sum_s |P_s v_sc|) + sum_s e_P,s |v_sc|
      dp_s:  e_dp = _red(ch, sum_c |g_c v_sc|);  dot = sum_s dp_s P_s: e_dot = _red(T, sum |dp P|) + sum_s P_s e_dp,s
      ds_s = s P_s (dp_s - dot):  e_ds = s P_s (e_dp,s + e_dot) + _red(2, s P_s (|dp_s| + |dot|))
      dk_sc = ds_s q_c: e_ds |q_c| + _red(1, |ds q|);  dv_sc = P_s g_c: _red(1, |P g|);
      dq_c = sum_s ds_s k_sc: _red(T, sum_s |ds_s k_sc|) + sum_s e_ds,s |k_sc|."""
    from ddnm_amd import ops
    from ddnm_amd._lib import check
    qkv, da0 = _attn_case(T, C, heads)
    Bn, ch = qkv.shape[0], C // heads
    s = 1.0 / math.sqrt(ch)
    x = qkv.double().requires_grad_(True)
    P, a0, (q0, k, v) = _attn_ref(x, heads)
    (a0 * da0.double()).sum().backward()
    dref = x.grad
    P, a0, q0, k, v = (t.detach() for t in (P, a0, q0, k, v))
    A = s * torch.einsum("bhc,bshc->bhs", q0.abs(), k.abs())
    e_P = P * (_red(ch, A + A.amax(dim=-1, keepdim=True)) + _red(T, 1.0)) + FLOOR
    e_a0 = (_red(T, torch.einsum("bhs,bshc->bhc", P, v.abs())) + torch.einsum("bhs,bshc->bhc", e_P, v.abs())).reshape(Bn, C)

    qg = qkv.cuda()
    Pg = torch.full((Bn, heads, T), float("nan"), device="cuda")
    a0g = torch.full((Bn, C), float("nan"), device="cuda")
    check(hip.ddnm_pool_attn_fwd_f32(_p(qg), _p(Pg), _p(a0g), Bn, T, C, heads, ops._stream()), "ddnm_pool_attn_fwd_f32")
    P32, da0g = P.float().cuda().contiguous(), da0.cuda()
    dg = torch.full((Bn, T, 3 * C), float("nan"), device="cuda")
    check(hip.ddnm_pool_attn_bwd_f32(_p(qg), _p(P32), _p(da0g), _p(dg), Bn, T, C, heads, ops._stream()),
          "ddnm_pool_attn_bwd_f32")
    torch.cuda.synchronize()

    g = da0.double().reshape(Bn, heads, ch)
    dp = torch.einsum("bhc,bshc->bhs", g, v)
    e_dp = _red(ch, torch.einsum("bhc,bshc->bhs", g.abs(), v.abs()))
    dot = (dp * P).sum(dim=-1, keepdim=True)
    e_dot = _red(T, (dp * P).abs().sum(dim=-1, keepdim=True)) + (P * e_dp).sum(dim=-1, keepdim=True)
    ds = s * P * (dp - dot)
    e_ds = s * P * (e_dp + e_dot) + _red(2, s * P * (dp.abs() + dot.abs())) + FLOOR
    e_dk = torch.einsum("bhs,bhc->bshc", e_ds, q0.abs()) + _red(1, torch.einsum("bhs,bhc->bshc", ds.abs(), q0.abs())) + FLOOR
    e_dv = _red(1, torch.einsum("bhs,bhc->bshc", P, g.abs())) + FLOOR
    e_dq = _red(T, torch.einsum("bhs,bshc->bhc", ds.abs(), k.abs())) + torch.einsum("bhs,bshc->bhc", e_ds, k.abs()) + FLOOR
    d = dg.cpu()
    w = {"P": _worst(Pg, P, e_P), "a0": _worst(a0g, a0, e_a0),
         "dq": _worst(d[:, 0, :C], dref[:, 0, :C], e_dq.reshape(Bn, C)),
         "dk": _worst(d[:, :, C:2 * C], dref[:, :, C:2 * C], e_dk.reshape(Bn, T, C)),
         "dv": _worst(d[:, :, 2 * C:], dref[:, :, 2 * C:], e_dv.reshape(Bn, T, C))}
    print(f"pool_attn T={T} C={C} heads={heads}: worst |err| / bar " + ", ".join(f"{n} {x:.3f}" for n, x in w.items()))
    assert bool(torch.isfinite(Pg).all()) and bool(torch.isfinite(a0g).all()) and bool(torch.isfinite(dg).all())
    assert float((Pg.double().sum(dim=-1) - 1.0).abs().max()) <= _red(T, 1.0)
    if T > 1:
        assert bool((d[:, 1:, :C] == 0).all())
        assert float(Pg[2, :, T // 2].min()) > 0.999 and float((Pg[1] - 1.0 / T).abs().max()) <= _red(T, 1.0) / T
    assert all(x <= 1.0 for x in w.values()), w


def test_pool_attention_rejects_more_tokens_than_its_lds_array(hip):
    """T = 1025: the bad-argument error from both entry points, nothing launched (1024-entry LDS arrays)."""
    from ddnm_amd import ops
    from ddnm_amd._lib import DDNMHipError, check
    T, C, heads = 1025, 64, 1
    qkv = torch.zeros(1, T, 3 * C, device="cuda")
    P = torch.full((1, heads, T), 7.0, device="cuda")
    a0 = torch.full((1, C), 7.0, device="cuda")
    dq = torch.full((1, T, 3 * C), 7.0, device="cuda")
    with pytest.raises(DDNMHipError, match="bad argument"):
        check(hip.ddnm_pool_attn_fwd_f32(_p(qkv), _p(P), _p(a0), 1, T, C, heads, ops._stream()), "ddnm_pool_attn_fwd_f32")
    with pytest.raises(DDNMHipError, match="bad argument"):
        check(hip.ddnm_pool_attn_bwd_f32(_p(qkv), _p(P), _p(a0), _p(dq), 1, T, C, heads, ops._stream()), "ddnm_pool_attn_bwd_f32")
    torch.cuda.synchronize()
    assert bool((P == 7.0).all()) and bool((a0 == 7.0).all()) and bool((dq == 7.0).all())


# ----------------------------------------------------------------------------- row kernels
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_softmax_bwd_rows(hip, n):
    """ddnm_softmax_bwd_rows_f32 in place on dP: dS = scale P (dP - rowsum(dP P)), rows = 37 (no multiple of the 4 rows per
    block), ld = n + 3 with a sentinel in the padding columns of dP that must survive (and NaN in those of P, which must not
    be read).  Bars: dot is an n-term sum, e_dot = _red(n, sum |dP P|); element: scale P e_dot + _red(2, scale P (|dP| + |dot|))."""
    from ddnm_amd import ops
    from ddnm_amd._lib import check
    rows, ld, scale = 37, n + 3, 0.125
    g = torch.Generator().manual_seed(n)
    P = torch.softmax(2.0 * torch.randn(rows, n, generator=g).double(), dim=-1).float()
    dP = torch.randn(rows, n, generator=g)
    Pp = torch.full((rows, ld), float("nan"))
    Pp[:, :n] = P
    dPp = torch.full((rows, ld), -12345.0)
    dPp[:, :n] = dP
    p64, d64 = P.double(), dP.double()
    dot = (d64 * p64).sum(dim=-1, keepdim=True)
    ref = scale * p64 * (d64 - dot)
    bar = scale * p64 * _red(n, (d64 * p64).abs().sum(dim=-1, keepdim=True)) + _red(2, scale * p64 * (d64.abs() + dot.abs())) + FLOOR
    Pg, dg = Pp.cuda(), dPp.cuda()
    check(hip.ddnm_softmax_bwd_rows_f32(_p(Pg), _p(dg), rows, n, ld, scale, ops._stream()), "ddnm_softmax_bwd_rows_f32")
    torch.cuda.synchronize()
    out = dg.cpu()
    w = _worst(out[:, :n], ref, bar)
    print(f"softmax_bwd_rows n={n}: worst |err| / bar {w:.3f}")
    assert bool((out[:, n:] == -12345.0).all())
    assert bool(torch.isfinite(out).all()) and w <= 1.0


@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_logsoftmax_grad(hip, N):
    """ddnm_logsoftmax_grad_f32: dlogits = onehot(y) - softmax(logits), B = 3: one row of logits around +80, one around
    -80 (the maximum must be subtracted), one wide; labels 0, N - 1 and the middle.  Bars: softmax_j relative
    _red(N + |l_j - max| + 1, 1) (N-term normaliser, exponent argument), the label entry adds the 2-term sum
    _red(2, 1 + p).  Every row sums to zero within N 2^-23."""
    from ddnm_amd import ops
    from ddnm_amd._lib import check
    g = torch.Generator().manual_seed(N)
    logits = torch.stack([80.0 + torch.randn(N, generator=g), -80.0 + torch.randn(N, generator=g), 3.0 * torch.randn(N, generator=g)])
    y = torch.tensor([0, N - 1, N // 2], dtype=torch.int64)
    l64 = logits.double()
    p = torch.softmax(l64, dim=-1)
    onehot = torch.nn.functional.one_hot(y, N).double()
    ref = onehot - p
    bar = p * 4.0 * (N + (l64 - l64.amax(dim=-1, keepdim=True)).abs() + 1.0) * EPS + onehot * _red(2, 1.0 + p) + FLOOR
    out = torch.full((3, N), float("nan"), device="cuda")
    lg, yg = logits.cuda(), y.cuda()
    check(hip.ddnm_logsoftmax_grad_f32(_p(lg), _p(yg), _p(out), 3, N, ops._stream()), "ddnm_logsoftmax_grad_f32")
    torch.cuda.synchronize()
    w = _worst(out, ref, bar)
    rs = float(out.double().sum(dim=-1).abs().max())
    print(f"logsoftmax_grad N={N}: worst |err| / bar {w:.3f}, worst |row sum| {rs:.3e} (bar {N * 2.0 ** -23:.3e})")
    assert bool(torch.isfinite(out).all()) and w <= 1.0
    assert rs <= N * 2.0 ** -23
