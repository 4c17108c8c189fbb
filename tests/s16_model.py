"""The documented error model of the split-fp16 convolutions, in fp64, on whatever device its inputs live on.

Element model (csrc/conv_common.h::split_store): a scaled operand value v is carried as hi = rn16(v),
lo = rn16(v - hi) with |hi + lo - v| <= 2^-25 for |v| < 0.25 and <= 2^-22 |v| above; a product is hi.hi' + hi.lo' + lo.hi',
each exact in the fp32 accumulator, the dropped lo.lo' is <= 2^-22 |v||v'|.  The launch's scales are reproduced from the
project's own rules: ops.s16_weight_scale (max|W| into [2^13, 2^14)), conv_common.h::s16_operand_scale (a raw operand's
bound into [2^14, 2^15) per image, `down_only` next to a GroupNorm'd operand), ops._s16_act_scale() for GroupNorm'd operands.

From these `layer_bound` gives a per-output-element bound of the split arithmetic's error.  It predicts no bits of a kernel's
output: the order of the fp32 accumulation is not modelled, which is why the GPU tests add the fp32 kernel's own error.

Shared by tests/test_s16_dynamic_range_host.py (the model against an emulation of the arithmetic, CPU) and
tests/test_gpu_s16_dynamic_range.py (the kernels against the model): operands are drawn on the CPU from a seeded generator,
so both see the same numbers.  A helper module, not a conftest."""
import math

import torch
import torch.nn.functional as F

from ddnm_amd import ops

U = 2.0 ** -22                  # relative error of hi + lo, and of the dropped lo.lo' product
REL_TIER = 4 * U                # channel_tiers: weight term <= 2 (the loader guard's 2^-21), activation term 1, product 1


# ------------------------------------------------------------------ element model and bound
def elem_eps(v):
    a = v.abs()
    return torch.where(a == 0, torch.zeros_like(a), torch.where(a < 0.25, torch.full_like(a, 2.0 ** -25), U * a))


def _subpixel_conv(x, wp):
    """Four 2x2 convolutions on the low-resolution grid (ops.upsample_phase_weights): out[2y + py][2x + px]."""
    B, _, h, w = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_zeros(B, wp.shape[2], 2 * h, 2 * w)
    for py in range(2):
        for px in range(2):
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + h + 1, px:px + w + 1], wp[py, px])
    return out


def conv(x, w, stride=1, ups=False):
    """The layer's convolution, NCHW fp64: 3x3 / 1x1 "same" at stride 1 (behind a nearest x2 when `ups`), pad (0, 1, 0, 1) at
    stride 2; `w` with six dimensions is the sub-pixel form's phase tensor [py][px][O][I][a][b]."""
    if w.dim() == 6:
        return _subpixel_conv(x, w)
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if stride == 2:
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    return F.conv2d(x, w, padding=w.shape[-1] // 2)


def conv_bound(A, W, **conv_kwargs):
    """(bound, mag) per output element for already scaled fp64 operands: mag = conv(|A|, |W|),
    bound = conv(eps(A), |W|) + conv(|A|, eps(W)) + conv(eps(A), eps(W)) + 2^-22 mag."""
    aA, aW, eA, eW = A.abs(), W.abs(), elem_eps(A), elem_eps(W)
    mag = conv(aA, aW, **conv_kwargs)
    bound = conv(eA, aW + eW, **conv_kwargs) + conv(aA, eW, **conv_kwargs) + U * mag
    return bound, mag


def channel_tiers(bound, mag):
    """[Cout] bool over NCHW tensors: True = relative regime, max over (b, y, x) of bound / mag <= 4 * 2^-22."""
    ratio = torch.where(mag > 0, bound / mag.clamp_min(1e-300), torch.zeros_like(mag))
    return ratio.amax((0, 2, 3)) <= REL_TIER


def operand_scale(amax, down_only):
    """conv_common.h::s16_operand_scale for one image: `amax` = the largest of the image's DDNM_AMAX_N bound words."""
    e = math.frexp(float(amax))[1] - 1 if amax > 0 and math.isfinite(amax) else -80
    k = 14 - min(max(e, -80), 80)
    return 2.0 ** (min(k, 0) if down_only else k)


# ------------------------------------------------------------------ a layer: operands, reference, bound
def layer(a, w, *, b=None, bias=None, sc=None, sh=None, gn_silu=True, res=None, sk=None, wsk=None, badd=None, ups=False,
          stride=1):
    """One launch's fp32 inputs (NHWC activations, OIHW weights), None where the layer has no such input."""
    return dict(a=a, b=b, w=w, bias=bias, sc=sc, sh=sh, gn_silu=gn_silu, res=res, sk=sk, wsk=wsk, badd=badd, ups=ups,
                stride=stride)


def to(t, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in t.items()}


def operand64(t):
    """The operand the kernel splits (GroupNorm affine and swish applied), NCHW fp64."""
    x = t["a"] if t["b"] is None else torch.cat([t["a"], t["b"]], 3)
    x = x.double()
    if t["sc"] is not None:
        x = x * t["sc"].double()[:, None, None, :] + t["sh"].double()[:, None, None, :]
        if t["gn_silu"]:
            x = x * torch.sigmoid(x)
    return x.permute(0, 3, 1, 2)


def ref64(t):
    """fp64 evaluation of the layer, NHWC."""
    y = conv(operand64(t), t["w"].double(), stride=t["stride"], ups=t["ups"])
    if t["bias"] is not None:
        y = y + t["bias"].double()[None, :, None, None]
    if t["sk"] is not None:
        y = y + F.conv2d(t["sk"].double().permute(0, 3, 1, 2), t["wsk"].double())
    y = y.permute(0, 2, 3, 1)
    if t["badd"] is not None:
        y = y + t["badd"].double()[:, None, None, :]
    if t["res"] is not None:
        y = y + t["res"].double()
    return y


def raw_operands(t):
    """The tensors the launch reads raw (ops.conv2d: the main operand without GroupNorm, the fused shortcut's input always)."""
    if t["sk"] is not None:
        return (t["sk"],)
    if t["sc"] is None:
        return (t["a"],) if t["b"] is None else (t["a"], t["b"])
    return ()


def exact_amax(t):
    """What ops.amax_bound returns for plain tensors (tests/test_gpu_s16.py::test_operand_bound_kernels): the per-image maximum."""
    raws = raw_operands(t)
    return None if not raws else torch.stack([r.abs().amax((1, 2, 3)) for r in raws]).amax(0)


def scaled_operands(t, amax=None, subpixel=False):
    """[(A, W)] of the products that share the accumulator, scaled as the launch scales them, and unscale[B] = 1 / (weight
    scale * operand scale).  `amax` [B]: the per-image operand bound the launch is given (an input of the model)."""
    B = t["a"].shape[0]
    if subpixel:
        W = ops.upsample_phase_weights(t["w"])
        sw = float(ops.upsample_weight_s16(t["w"])[1])
    else:
        W = t["w"].double()
        sw = float(ops.s16_weight_scale(*([t["w"]] + ([t["wsk"]] if t["wsk"] is not None else []))))
    if raw_operands(t):
        sa = torch.tensor([operand_scale(float(amax[i]), down_only=t["sk"] is not None) for i in range(B)],
                          dtype=torch.float64, device=t["a"].device)
    else:
        sa = torch.full((B,), float(ops._s16_act_scale()), dtype=torch.float64, device=t["a"].device)
    pairs = [(operand64(t) * sa[:, None, None, None], W * sw)]
    if t["sk"] is not None:
        pairs.append((t["sk"].double().permute(0, 3, 1, 2) * sa[:, None, None, None], t["wsk"].double() * sw))
    return pairs, 1.0 / (sw * sa)


def _kwargs(t, i):
    return dict(stride=t["stride"], ups=t["ups"]) if i == 0 else {}


def layer_bound(t, amax=None, subpixel=False):
    """(bound, mag), NCHW fp64 in the OUTPUT's units: the split error of every product in the accumulator (3x3 and fused 1x1)."""
    pairs, unscale = scaled_operands(t, amax, subpixel)
    bound = mag = 0.0
    for i, (A, W) in enumerate(pairs):
        b_, m_ = conv_bound(A, W, **_kwargs(t, i))
        bound, mag = bound + b_, mag + m_
    u = unscale[:, None, None, None]
    return bound * u, mag * u


def emulated_error(t, amax=None, subpixel=False):
    """|emulated - exact| NCHW fp64 in the output's units: operands split with torch fp16, the three products formed and summed
    in fp64 (each fp16 x fp16 product is exact there)."""
    pairs, unscale = scaled_operands(t, amax, subpixel)
    err = 0.0
    for i, (A, W) in enumerate(pairs):
        kw = _kwargs(t, i)
        ah, wh = A.half().double(), W.half().double()
        al, wl = (A - ah).half().double(), (W - wh).half().double()
        assert bool(torch.isfinite(ah).all()) and bool(torch.isfinite(wh).all()), "scaled operand left fp16 range"
        err = err + conv(ah, wh, **kw) + conv(ah, wl, **kw) + conv(al, wh, **kw) - conv(A, W, **kw)
    return err.abs() * unscale[:, None, None, None]


# ------------------------------------------------------------------ operand generators (CPU, seeded)
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _loguniform(g, n, lo, hi):
    return torch.exp(torch.rand(n, generator=g) * (math.log(hi) - math.log(lo)) + math.log(lo))


def _student_t(g, shape, df=2.5):
    z = torch.randn(*shape, generator=g)
    chi2 = 2.0 * torch._standard_gamma(torch.full(shape, df / 2.0), generator=g)
    return z / torch.sqrt(chi2 / df)


def _outlier_cols(w):
    w[:, 5::32] *= 2.0 ** 6
    return w


def weights(kind, cout, cin, k, seed):
    """OIHW fp32.  control: randn / (k sqrt(Cin)); spec: rows of it scaled log-uniformly over 1e-3 ... 1e1; student_t: df 2.5;
    outlier_cols: spec with every 32nd input column x 2^6; beyond: rows spread over 2^-20, the same outlier columns."""
    g = _gen(1000 + seed)
    base = 1.0 / (k * cin ** 0.5)
    if kind == "student_t":
        return _student_t(g, (cout, cin, k, k)) * base
    w = torch.randn(cout, cin, k, k, generator=g) * base
    if kind in ("spec", "outlier_cols"):
        w = w * _loguniform(g, cout, 1e-3, 1e1)[:, None, None, None]
    elif kind == "beyond":
        w = w * (2.0 ** (-20.0 * torch.arange(cout, dtype=torch.float32) / (cout - 1)))[:, None, None, None]
    elif kind != "control":
        raise ValueError(kind)
    return _outlier_cols(w) if kind in ("outlier_cols", "beyond") else w


WEIGHT_KINDS = ("control", "spec", "student_t", "outlier_cols", "beyond")
ACT_OF = {"control": "control", "spec": "spec", "student_t": "student_t", "outlier_cols": "spec", "beyond": "spec"}


def raw_acts(kind, B, H, W, C, seed):
    """NHWC fp32 raw operand.  control: 1.5 randn; spec: channels of randn scaled log-uniformly over 1e-4 ... 1e4; student_t."""
    g = _gen(2000 + seed)
    if kind == "student_t":
        return _student_t(g, (B, H, W, C))
    x = torch.randn(B, H, W, C, generator=g)
    if kind == "control":
        return x * 1.5
    if kind == "spec":
        return x * _loguniform(g, C, 1e-4, 1e4)
    raise ValueError(kind)


def gn_affine(kind, B, C, seed):
    """(sc, sh) [B, C] of a GroupNorm'd operand.  control: tests/test_gpu_s16.py::_make; gn_heavy: sc log-uniform over
    1e-2 ... 1e1 per channel, sh ~ N(-1, 2) -- with 1.5 randn underneath it the operand stays far inside fp16 range, which
    an UNSCALED operand has to (Model._guard_normalised_operands)."""
    g = _gen(3000 + seed)
    if kind == "control":
        return torch.randn(B, C, generator=g) * 0.3 + 1.0, torch.randn(B, C, generator=g) * 0.3
    if kind == "gn_heavy":
        sc = _loguniform(g, C, 1e-2, 1e1)[None, :].expand(B, C).contiguous()
        return sc, torch.randn(B, C, generator=g) * 2.0 - 1.0
    raise ValueError(kind)


# ------------------------------------------------------------------ the cases of the GPU test (and of the host test)
# id -> (form, (B, C0, C1, Cout, H[, W]), operands).  `tier`: "rel" = every channel must be in the relative regime, else the
# (min relative, min absolute) fractions of the host test's caps.
def _c(form, shape, kind, tier="rel", seed=0):
    return dict(id=f"{form}-{kind}", form=form, shape=shape, kind=kind, tier=tier, seed=seed)


_TIER = {"control": "rel", "spec": "rel", "student_t": "rel", "gn_heavy": "rel", "outlier_cols": (0.5, 0.10),
         "beyond": (0.25, 0.25)}
CASES = (
    [_c("halo_raw", (2, 128, 0, 128, 32), k, _TIER[k]) for k in WEIGHT_KINDS] +
    [_c("halo_gn_badd_res", (2, 128, 0, 128, 32), k, _TIER[k]) for k in WEIGHT_KINDS] +
    [_c("concat_gn", (2, 128, 128, 128, 32), "outlier_channels")] +
    [_c("fused_shortcut", (2, 128, 0, 256, 32), "spec")] +
    [_c("splitk_stats", (2, 256, 0, 256, 16), k, _TIER[k]) for k in ("spec", "outlier_cols")] +
    [_c("ups", (2, 64, 0, 128, 8, 32), k, _TIER[k]) for k in ("spec", "student_t", "outlier_cols")] +
    [_c("down", (2, 128, 0, 128, 32), k, _TIER[k]) for k in ("spec", "outlier_cols")] +
    [_c("qkv_1x1_gn", (2, 512, 0, 1536, 16), "spec"), _c("nin_1x1_concat", (2, 256, 256, 256, 16), "spec")] +
    [_c("level8_gn", (1, 160, 0, 192, 8), k, _TIER[k]) for k in ("spec", "outlier_cols")]
)


def build_case(c):
    """The layer of case `c` on the CPU.  Forms whose operand is GroupNorm'd take the `gn_heavy` affine as their activation
    side (an unscaled operand cannot carry `spec`'s 1e4 channels: they leave fp16 range, and the loader drops such a layer);
    `kind` then names the weights."""
    form, kind, seed = c["form"], c["kind"], c["seed"]
    B, C0, C1, Cout, H = c["shape"][:5]
    W = c["shape"][5] if len(c["shape"]) > 5 else H
    cin = C0 + C1
    g = _gen(4000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    plain = lambda C: raw_acts("control", B, H, W, C, seed)  # noqa: E731
    if form == "halo_raw":
        return layer(raw_acts(ACT_OF[kind], B, H, W, C0, seed), weights(kind, Cout, cin, 3, seed), bias=rn(Cout))
    if form == "halo_gn_badd_res":
        sc, sh = gn_affine("gn_heavy", B, cin, seed)
        return layer(plain(C0), weights(kind, Cout, cin, 3, seed), bias=rn(Cout), sc=sc, sh=sh, res=rn(B, H, W, Cout) * 2.0,
                     badd=rn(B, Cout))
    if form == "concat_gn":
        b = raw_acts("control", B, H, W, C1, seed + 1)
        b[..., 3::16] *= 2.0 ** 10
        sc, sh = gn_affine("control", B, cin, seed)
        return layer(plain(C0), weights("control", Cout, cin, 3, seed), b=b, bias=rn(Cout), sc=sc, sh=sh)
    if form == "fused_shortcut":
        sc, sh = gn_affine("control", B, cin, seed)
        return layer(plain(C0), weights("spec", Cout, cin, 3, seed), bias=rn(Cout), sc=sc, sh=sh,
                     sk=raw_acts("spec", B, H, W, 64, seed + 1), wsk=weights("spec", Cout, 64, 1, seed + 1))
    if form == "splitk_stats":
        return layer(raw_acts(ACT_OF[kind], B, H, W, C0, seed), weights(kind, Cout, cin, 3, seed), bias=rn(Cout),
                     res=rn(B, H, W, Cout) * 2.0)
    if form == "ups":
        return layer(raw_acts(ACT_OF[kind], B, H, W, C0, seed), weights(kind, Cout, cin, 3, seed), bias=rn(Cout), ups=True)
    if form == "down":
        return layer(raw_acts(ACT_OF[kind], B, H, W, C0, seed), weights(kind, Cout, cin, 3, seed), bias=rn(Cout), stride=2)
    if form == "qkv_1x1_gn":
        sc, sh = gn_affine("gn_heavy", B, cin, seed)
        return layer(plain(C0), weights(kind, Cout, cin, 1, seed), bias=rn(Cout), sc=sc, sh=sh, gn_silu=False)
    if form == "nin_1x1_concat":
        return layer(raw_acts("spec", B, H, W, C0, seed), weights(kind, Cout, cin, 1, seed), b=raw_acts("spec", B, H, W, C1, seed + 1),
                     bias=rn(Cout))
    if form == "level8_gn":
        sc, sh = gn_affine("gn_heavy", B, cin, seed)
        return layer(plain(C0), weights(kind, Cout, cin, 3, seed), bias=rn(Cout), sc=sc, sh=sh)
    raise ValueError(form)


# ------------------------------------------------------------------ model level: a state dict with dynamic range in every launch
OUTLIER_LAYERS = ("down.1.block.0.conv1", "up.1.upsample.conv")      # a ResnetBlock conv1 and an upsample conv (both packings)


def spec_state_dict(sd, seed=0, outlier_layers=()):
    """`sd` with the rows of EVERY convolution weight rescaled by `spec` row scales (log-uniform 1e-3 ... 1e1), and the outlier
    columns (every 32nd input column x 2^6) in the named layers."""
    g = _gen(5000 + seed)
    out = {}
    for k, v in sd.items():
        if k.endswith(".weight") and v.dim() == 4:
            v = v * _loguniform(g, v.shape[0], 1e-3, 1e1).to(v)[:, None, None, None]
            if k[:-len(".weight")] in outlier_layers:
                v = _outlier_cols(v.clone())
        out[k] = v
    return out
