"""Case table, inputs, float64 references and plan queries shared by the fp16-activation convolution edge tests
(test_conv16_model_host.py without a GPU, test_gpu_conv16_edges.py on one).

The kernels under test (csrc/conv16.hip: conv16_kernel<TAPS, MT, WNW> in six instantiations, conv16_n128_kernel, the two
split-K reductions, the reduction that finalizes the consumer's GroupNorm) multiply fp16 operands on
v_mfma_f32_32x32x16_f16, accumulate in fp32, keep split-K partial sums in fp16 slabs (up to 8 slices) or fp32 slabs, round
the result to fp16 and sum the GroupNorm partials of the rounded values in fp32.  Fed integer-valued fp16 tensors whose
every intermediate is an integer that its format holds exactly (|v| <= 2048 wherever a value is rounded to fp16, below
2^24 wherever it stays fp32), they have one representable answer in ANY summation order, so the GPU tests compare bit for
bit with the float64 reference below (`exactness_violations` is the condition; the host test asserts it on every case).
Value ranges of the exact cases: activations in {-a..a} with a = 3, 2 or 1 by the length of the sum, dense weights in
{-1, 0, 1}, bias / residual in {-8..8}, shortcut input like the activations, GroupNorm scale in {-2, -1, 1, 2} and shift
in {-3..3} \\ {0}, distinct per image (the affine of a zero-padded pixel is then never zero: a kernel that pads BEFORE the
prologue adds w * shift along the border).

Swish cannot be exact: the `swish` cases use fp16 data on a 2^-7 grid (standard normal, clamped to +-3.6875), scale in
{+-0.5, +-1, +-2} and shift = 3 + a multiple of 2^-7 in [-0.5, 0.5], so that scale * x + shift is an fp32 number however
the kernel forms it, stays inside [-5.3, 10.9] (the interval the swish's relative error E_ACT was measured on) and the
only inexact steps of the prologue are the swish and the rounding of the activated operand to fp16.

A case names the plan cell it is meant to hit as `cell` = (kernel, MT, TW, ksplit, slab, statistics tiles, fin) with kernel
"k9" (conv16_kernel<9, MT, 4>) / "n128" / "k1" (conv16_kernel<1, MT, 4>) / "out" (conv16_kernel<9, 1, 1>), TW = 0 for the
flat rows of the 1x1 form, slab = 0 (unsplit) / 16 / 32 bits; `plan_of` asks the library's host queries.
All tensors here are NCHW float32 holding fp16-representable values; the GPU test converts."""
import ctypes
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

KC = 64                                   # channels per K chunk
BN = 256                                  # output channels per workgroup tile
LIMIT = float(2 ** 24)
H16_INT = 2048.0                          # every integer up to here is an fp16 number
U = 2.0 ** -24
U16 = 2.0 ** -11
V_RANGE = (-5.3, 10.9)                    # swish arguments E_ACT covers (tests/test_gpu_conv_f32_edges.py)


class Case(NamedTuple):
    name: str
    B: int
    H: int                                # output height / width (the source is H / 2 x W / 2 when `ups`)
    W: int
    C0: int
    C1: int
    Cout: int
    k: int
    ups: bool = False                     # nearest x2 read of the (activated) operand
    res: bool = False
    res_ups: bool = False                 # the residual is read through a nearest x2 upsample
    skip: Optional[Tuple[int, int]] = None      # fused 1x1 shortcut over (SC0, SC1) raw channels
    bias: bool = True
    gn: str = "none"                      # "none" / "affine" (integer, exact) / "swish" (real-valued, bounded)
    stats: bool = True                    # emit_stats (ops.conv16's default); conv16_out emits none
    fin: str = ""                         # "" / "gn" / "film": the consumer GroupNorm the reduction is asked to finalize
    out_nchw: bool = False                # ops.conv16_out: fp32 NCHW, Cout <= 32
    cell: tuple = ()                      # (kernel, MT, TW, ksplit, slab, stats tiles, fin)

    @property
    def Cin(self):
        return self.C0 + self.C1

    @property
    def src_hw(self):
        return (self.H // 2, self.W // 2) if self.ups else (self.H, self.W)

    @property
    def K(self):
        return self.k * self.k * self.Cin + (sum(self.skip) if self.skip else 0)

    @property
    def real(self):
        return self.gn == "swish"


def _c(name, B, H, W, cin, cout, k, cell, **kw):
    c0, c1 = cin if isinstance(cin, tuple) else (cin, 0)
    return Case(name, B, H, W, c0, c1, cout, k, cell=tuple(cell), **kw)


def _out_cases():
    out = []
    for B, H, W, cin, co in ((1, 8, 32, 64, 3), (2, 16, 64, 128, 6), (1, 8, 32, 64, 32), (1, 8, 32, 64, 1)):
        for bias in (True, False):
            out.append(_c(f"out_{B}x{cin}_{H}x{W}_co{co}{'' if bias else '_nobias'}", B, H, W, cin, co, 3,
                          ("out", 1, 32, 1, 0, 0, 0), bias=bias, stats=False, out_nchw=True))
    out.append(_c("out_2x128_16x64_co6_gn", 2, 16, 64, 128, 6, 3, ("out", 1, 32, 1, 0, 0, 0), gn="affine", stats=False, out_nchw=True))
    return out


CASES = [
    # ---- 3x3 unsplit: tile x tile width
    _c("k9_mt2_tw32_one_tile", 1, 4, 32, 64, 64, 3, ("k9", 2, 32, 1, 0, 1, 0)),                 # all four borders in one tile; grid 1
    _c("k9_mt2_tw32_seams", 1, 8, 64, 64, 64, 3, ("k9", 2, 32, 1, 0, 4, 0)),                    # interior seams on both axes
    _c("k9_mt2_tw16", 1, 8, 16, 64, 64, 3, ("k9", 2, 16, 1, 0, 1, 0)),
    _c("k9_mt2_tw16_2x3_cout192", 1, 16, 48, 64, 192, 3, ("k9", 2, 16, 1, 0, 6, 0)),            # grid 6; one idle 64-channel wave column
    _c("k9_mt4_tw32_200_tiles", 1, 200, 256, 64, 64, 3, ("k9", 4, 32, 1, 0, 200, 0)),           # the threshold
    _c("k9_mt2_192_tiles", 1, 192, 256, 64, 64, 3, ("k9", 2, 32, 1, 0, 384, 0)),                # its pair: 192 < 200 -> MT2
    _c("k9_mt4_tw16", 1, 240, 240, 64, 64, 3, ("k9", 4, 16, 1, 0, 225, 0)),
    _c("n128_tw32", 1, 200, 256, 64, 128, 3, ("n128", 4, 32, 1, 0, 200, 0)),
    _c("n128_tw16_two_chunks", 1, 240, 240, 128, 128, 3, ("n128", 4, 16, 1, 0, 225, 0), res=True),
    _c("k9_mt4_tw16_skip_not_n128", 1, 240, 240, 128, 128, 3, ("k9", 4, 16, 1, 0, 225, 0), skip=(64, 0)),
    _c("k9_mt4_tw16_cout256", 1, 240, 240, 128, 256, 3, ("k9", 4, 16, 1, 0, 225, 0)),
    # ---- options on the unsplit 3x3 kernel
    _c("k9_gn_cat_unsplit", 2, 16, 32, (64, 64), 64, 3, ("k9", 2, 32, 1, 0, 4, 0), gn="affine", res=True),
    _c("k9_ups_gn_unsplit", 2, 8, 32, 64, 64, 3, ("k9", 2, 32, 1, 0, 2, 0), ups=True, gn="affine"),
    _c("k9_res_ups_skip_cat_unsplit", 2, 8, 16, 64, 128, 3, ("k9", 2, 16, 1, 0, 1, 0), res=True, res_ups=True, skip=(64, 64)),
    _c("n128_gn_cat", 1, 200, 256, (64, 64), 128, 3, ("n128", 4, 32, 1, 0, 200, 0), gn="affine"),
    # ---- channel tiles and workgroup order
    _c("k9_two_ntiles_wmajor_cout320", 1, 32, 32, 64, 320, 3, ("k9", 2, 32, 1, 0, 8, 0)),
    _c("k9_two_ntiles_wmajor_cout512", 1, 16, 16, 128, 512, 3, ("k9", 2, 16, 1, 0, 2, 0)),
    _c("k9_two_ntiles_mmajor_cout320", 2, 32, 32, 64, 320, 3, ("k9", 2, 32, 1, 0, 8, 0)),
    # ---- 3x3 split
    _c("k9_ks2", 1, 8, 16, 256, 64, 3, ("k9", 2, 16, 2, 16, 32, 0)),
    _c("k9_ks2_uneven_5", 1, 8, 16, 320, 64, 3, ("k9", 2, 16, 2, 16, 32, 0)),
    _c("k9_ks2_uneven_5_cat_192_128", 1, 8, 16, (192, 128), 64, 3, ("k9", 2, 16, 2, 16, 32, 0)),  # concat boundary inside slice 1
    _c("k9_ks3_7_chunks_cout192", 1, 8, 16, 448, 192, 3, ("k9", 2, 16, 3, 16, 32, 0)),
    _c("k9_ks8_last_fp16_slab", 1, 8, 16, 1024, 64, 3, ("k9", 2, 16, 8, 16, 32, 0)),
    _c("k9_ks9_first_fp32_slab", 1, 8, 16, 1152, 64, 3, ("k9", 2, 16, 9, 32, 32, 0)),            # grid 9
    _c("k9_ks32_cap", 1, 16, 16, 4096, 64, 3, ("k9", 2, 16, 32, 32, 64, 0)),
    _c("k9_ks4_skip_two_idle_slices", 2, 16, 16, 512, 128, 3, ("k9", 2, 16, 4, 16, 64, 0), skip=(64, 64)),
    _c("k9_ks2_res", 1, 8, 16, 256, 64, 3, ("k9", 2, 16, 2, 16, 32, 0), res=True),
    _c("k9_ks2_res_ups", 2, 8, 16, 256, 64, 3, ("k9", 2, 16, 2, 16, 32, 0), res=True, res_ups=True),
    _c("k9_ks2_ups", 1, 8, 16, 256, 64, 3, ("k9", 2, 16, 2, 16, 32, 0), ups=True),
    _c("k9_ks2_gn", 2, 8, 16, (128, 128), 64, 3, ("k9", 2, 16, 2, 16, 32, 0), gn="affine"),
    _c("k9_ks2_cout320", 1, 8, 16, 256, 320, 3, ("k9", 2, 16, 2, 16, 32, 0), bias=False),       # reduction slabs of 256 + 64
    # ---- the reduction that finalizes the consumer's GroupNorm
    _c("fin_cout128", 2, 8, 16, 256, 128, 3, ("k9", 2, 16, 2, 16, 1, 1), fin="gn"),             # channel slabs of 16
    _c("fin_cout256_film", 1, 16, 16, 256, 256, 3, ("k9", 2, 16, 2, 16, 1, 1), fin="film", res=True),
    _c("fin_cout384_res_ups", 2, 8, 16, 256, 384, 3, ("k9", 2, 16, 2, 16, 1, 1), fin="gn", res=True, res_ups=True),   # slabs of 24
    _c("fin_cout1024_fp32_slab", 1, 8, 16, 1152, 1024, 3, ("k9", 2, 16, 9, 32, 1, 1), fin="gn"),                      # slabs of 32
    _c("fin_declined_2048_pixels", 1, 32, 64, 256, 128, 3, ("k9", 2, 32, 2, 16, 64, 0), fin="gn"),
    _c("fin_k1_im2col", 2, 8, 8, 2304, 256, 1, ("k1", 4, 0, 18, 32, 1, 1), fin="film"),
    # ---- 1x1 / GEMM form
    _c("k1_mt4_ragged_64_of_256", 1, 8, 8, 64, 64, 1, ("k1", 4, 0, 1, 0, 0, 0)),
    _c("k1_mt4_ragged_100", 1, 10, 10, 128, 64, 1, ("k1", 4, 0, 1, 0, 0, 0), res=True),
    _c("k1_mt1_whole", 3, 8, 8, 64, 64, 1, ("k1", 1, 0, 1, 0, 1, 0)),                          # grid 3
    _c("k1_mt1_ragged_ks2", 2, 5, 13, 256, 64, 1, ("k1", 1, 0, 2, 16, 13, 0), res=True),
    _c("k1_mt4_ragged_ks18", 1, 8, 8, 2304, 256, 1, ("k1", 4, 0, 18, 32, 16, 0), res=True, res_ups=True),   # (the reduction maps res_ups)
    _c("k1_mt2_whole", 5, 64, 64, 64, 64, 1, ("k1", 2, 0, 1, 0, 32, 0)),
    _c("k1_mt2_ragged_last", 1, 129, 129, 64, 64, 1, ("k1", 2, 0, 1, 0, 0, 0)),
    _c("k1_mt4_whole", 13, 64, 64, 64, 64, 1, ("k1", 4, 0, 1, 0, 16, 0), res=True),
    _c("k1_mt1_12_ntiles_wmajor", 3, 8, 8, 1024, 3072, 1, ("k1", 1, 0, 1, 0, 1, 0)),
] + _out_cases() + [
    # ---- swish prologue on real-valued data
    _c("real_k9_mt2_cat", 2, 8, 32, (64, 64), 64, 3, ("k9", 2, 32, 1, 0, 2, 0), gn="swish", res=True),
    _c("real_k9_ups", 1, 16, 32, 64, 128, 3, ("k9", 2, 32, 1, 0, 4, 0), gn="swish", ups=True),
    _c("real_n128", 1, 200, 256, 64, 128, 3, ("n128", 4, 32, 1, 0, 200, 0), gn="swish"),
    _c("real_ks2_res", 2, 8, 16, 256, 64, 3, ("k9", 2, 16, 2, 16, 32, 0), gn="swish", res=True),
    _c("real_ks9_fp32_slab", 1, 8, 16, 1152, 64, 3, ("k9", 2, 16, 9, 32, 32, 0), gn="swish"),
    _c("real_out", 2, 16, 64, 128, 6, 3, ("out", 1, 32, 1, 0, 0, 0), gn="swish", stats=False, out_nchw=True),
]
BY_NAME = {c.name: c for c in CASES}
EXACT_CASES = [c for c in CASES if not c.real]
REAL_CASES = [c for c in CASES if c.real]
FILM_EXTRA = 40                           # the FiLM rows are 2 * Cout + 40 floats wide, NaN beyond [s | t]


# ----------------------------------------------------------------------------- inputs
def _gen(case, salt):
    h = salt
    for ch in case.name:
        h = (h * 1000003 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(h)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)


def _grid(x, step=2.0 ** -7):
    return torch.round(x / step) * step


def act_range(case):
    """Activations of an exact case are drawn from {-a..a}: 3 for short sums, 1 for the longest."""
    return 3 if case.K <= 2400 else (2 if case.K <= 9300 else 1)


def make_inputs(case):
    """The fp32 tensors of a case (NCHW, every value an fp16 number except bias / scale / shift / gamma / beta / FiLM, which
    the kernels read as fp32): x0, x1, w, bias, res, scale, shift, skip0, skip1, skip_w, gamma, beta, film_s, film_t; None
    where the case has none."""
    g = _gen(case, 1)
    B, (hs, ws) = case.B, case.src_hw
    a = act_range(case)
    t = dict.fromkeys(("x1", "bias", "res", "scale", "shift", "skip0", "skip1", "skip_w", "gamma", "beta", "film_s", "film_t"))
    if case.real:
        draw = lambda *s: _grid(torch.randn(*s, generator=g).clamp(-3.6875, 3.6875))
        t["x0"] = draw(B, case.C0, hs, ws)
        if case.C1:
            t["x1"] = draw(B, case.C1, hs, ws)
        t["w"] = (torch.randn(case.Cout, case.Cin, case.k, case.k, generator=g) * float(case.K) ** -0.5).half().float()
        if case.bias:
            t["bias"] = torch.randn(case.Cout, generator=g)
        t["scale"] = torch.tensor([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0])[torch.randint(0, 6, (B, case.Cin), generator=g)]
        t["shift"] = 3.0 + _grid(torch.rand(B, case.Cin, generator=g) - 0.5)
        addend = lambda *s: torch.randn(*s, generator=g).half().float()
    else:
        t["x0"] = _ints(g, -a, a, B, case.C0, hs, ws)
        if case.C1:
            t["x1"] = _ints(g, -a, a, B, case.C1, hs, ws)
        t["w"] = _ints(g, -1, 1, case.Cout, case.Cin, case.k, case.k)
        if case.bias:
            t["bias"] = _ints(g, -8, 8, case.Cout)
        if case.gn == "affine":
            t["scale"] = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (B, case.Cin), generator=g)]
            sh = _ints(g, 1, 3, B, case.Cin)
            t["shift"] = sh * (2.0 * torch.randint(0, 2, (B, case.Cin), generator=g).float() - 1.0)
        addend = lambda *s: _ints(g, -8, 8, *s)
    if case.res:
        t["res"] = addend(B, case.Cout, *((case.H // 2, case.W // 2) if case.res_ups else (case.H, case.W)))
    if case.skip:
        sc0, sc1 = case.skip
        t["skip0"] = _ints(g, -a, a, B, sc0, case.H, case.W)
        if sc1:
            t["skip1"] = _ints(g, -a, a, B, sc1, case.H, case.W)
        t["skip_w"] = _ints(g, -1, 1, case.Cout, sc0 + sc1, 1, 1)
    if case.fin:
        t["gamma"] = 1.0 + 0.5 * torch.randn(case.Cout, generator=g)
        t["beta"] = 0.5 * torch.randn(case.Cout, generator=g)
        if case.fin == "film":
            t["film_s"] = 0.5 * torch.randn(B, case.Cout, generator=g)
            t["film_t"] = 0.5 * torch.randn(B, case.Cout, generator=g)
            t["film_s"][:, 1] = -1.75                                    # a negative 1 + s
    return t


def film_rows(t):
    """[B, 2 Cout + FILM_EXTRA]: [s | t | NaN]; its row length is the stride the launch gets."""
    B, C = t["film_s"].shape
    rows = torch.full((B, 2 * C + FILM_EXTRA), float("nan"))
    rows[:, :C], rows[:, C:2 * C] = t["film_s"], t["film_t"]
    return rows


# ----------------------------------------------------------------------------- float64 reference
def _up2(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def affine_arg(case, t):
    """float64 [B, Cin, Hs, Ws]: concat and GroupNorm affine (the swish's argument for the swish cases)."""
    x = t["x0"].double() if t["x1"] is None else torch.cat([t["x0"], t["x1"]], 1).double()
    if case.gn != "none":
        x = x * t["scale"].double()[:, :, None, None] + t["shift"].double()[:, :, None, None]
    return x


def activation(case, t):
    """float64 [B, Cin, H, W]: concat, GroupNorm affine (+ swish), nearest x2 of the ACTIVATED operand -- what the taps read
    where they do not fall on the zero padding."""
    x = affine_arg(case, t)
    if case.real:
        x = x * torch.sigmoid(x)
    return _up2(x) if case.ups else x


def conv_part(case, t, act=None, chunks=None, skip_chunks=None, mag=False, w=None):
    """The products alone, float64 [B, Cout, H, W]: main operand chunks [c0, c1) (64 channels each; None: all) through the
    k x k weights with zero padding AFTER the activation, plus shortcut chunks [s0, s1) through the 1x1 shortcut weights.
    `mag`: the same over absolute values."""
    f = (lambda v: v.double().abs()) if mag else (lambda v: v.double())
    act = activation(case, t) if act is None else act
    w = t["w"] if w is None else w
    c0, c1 = (0, case.Cin // KC) if chunks is None else chunks
    p = case.k // 2
    out = torch.zeros(case.B, case.Cout, case.H, case.W, dtype=torch.float64)
    if c1 > c0:
        out = out + F.conv2d(F.pad(f(act[:, c0 * KC:c1 * KC]), (p, p, p, p)), f(w[:, c0 * KC:c1 * KC]))
    if case.skip:
        s0, s1 = (0, sum(case.skip) // KC) if skip_chunks is None else skip_chunks
        if s1 > s0:
            s = t["skip0"] if t["skip1"] is None else torch.cat([t["skip0"], t["skip1"]], 1)
            out = out + F.conv2d(f(s[:, s0 * KC:s1 * KC]), f(t["skip_w"][:, s0 * KC:s1 * KC]))
    return out


def residual(case, t):
    if not case.res:
        return None
    r = t["res"].double()
    return _up2(r) if case.res_ups else r


def add_epilogue(case, t, acc):
    """+ bias + res (nearest x2 when res_ups)."""
    if t["bias"] is not None:
        acc = acc + t["bias"].double()[None, :, None, None]
    r = residual(case, t)
    return acc if r is None else acc + r


def reference(case, t):
    """float64 [B, Cout, H, W]."""
    return add_epilogue(case, t, conv_part(case, t))


def slow_reference(case, t):
    """The same result by explicit loops over images, taps and pixels in float64 (no F.conv2d, no F.pad, no
    repeat_interleave): an independent formulation for the host test, for tiny cases only."""
    B, Cout, H, W, k = case.B, case.Cout, case.H, case.W, case.k
    w, p = t["w"].double(), case.k // 2
    out = torch.zeros(B, Cout, H, W, dtype=torch.float64)
    for b in range(B):
        for oy in range(H):
            for ox in range(W):
                acc = t["bias"].double().clone() if t["bias"] is not None else torch.zeros(Cout, dtype=torch.float64)
                for ky in range(k):
                    for kx in range(k):
                        iy, ix = oy - p + ky, ox - p + kx
                        if not (0 <= iy < H and 0 <= ix < W):
                            continue                                       # padding: contributes nothing, affine or not
                        sy, sx = (iy // 2, ix // 2) if case.ups else (iy, ix)
                        v = t["x0"][b, :, sy, sx].double()
                        if t["x1"] is not None:
                            v = torch.cat([v, t["x1"][b, :, sy, sx].double()])
                        if case.gn != "none":
                            v = v * t["scale"][b].double() + t["shift"][b].double()
                            if case.real:
                                v = v / (1.0 + torch.exp(-v))
                        acc = acc + w[:, :, ky, kx] @ v
                if case.skip:
                    s = t["skip0"][b, :, oy, ox].double()
                    if t["skip1"] is not None:
                        s = torch.cat([s, t["skip1"][b, :, oy, ox].double()])
                    acc = acc + t["skip_w"].double()[:, :, 0, 0] @ s
                if case.res:
                    acc = acc + (t["res"][b, :, oy // 2, ox // 2] if case.res_ups else t["res"][b, :, oy, ox]).double()
                out[b, :, oy, ox] = acc
    return out


# ----------------------------------------------------------------------------- plans
_DUMMY = 0x1000


def _lib():
    from ddnm_amd import _lib as L
    return L.lib()


def desc_of(case):
    """The shape fields of the descriptor ops.conv16 / ops.conv16_out fill for this case; every pointer the launch would
    carry is a non-null dummy (the planner looks at some of them).  For the host queries only."""
    from ddnm_amd._lib import Conv16Desc
    d = Conv16Desc()
    d.src = d.weight = d.out = _DUMMY
    if case.bias:
        d.bias = _DUMMY
    if case.C1:
        d.src1, d.C0 = _DUMMY, case.C0
    if case.gn != "none":
        d.gn_scale = d.gn_shift = _DUMMY
        d.gn_silu = int(case.real)
    if case.res:
        d.res, d.res_ups = _DUMMY, int(case.res_ups)
    if case.skip:
        d.skip0 = d.skip_weight = _DUMMY
        d.SC0, d.SC1 = case.skip
        if case.skip[1]:
            d.skip1 = _DUMMY
    if case.fin:
        d.fin_gamma = d.fin_beta = d.fin_scale = d.fin_shift = _DUMMY
        d.fin_eps, d.fin_groups = 1e-5, 32
        if case.fin == "film":
            d.fin_film, d.fin_film_stride = _DUMMY, 2 * case.Cout + FILM_EXTRA
    d.B, d.H, d.W, d.Cin, d.Cout, d.ksize = case.B, case.H, case.W, case.Cin, case.Cout, case.k
    d.ups, d.out_nchw_f32 = int(case.ups), int(case.out_nchw)
    return d


def _copy(d, **fields):
    c = type(d).from_buffer_copy(d)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def gemm_tile_rule(B, hw, cout):
    """The documented tile rule of the 1x1 form (plan16): 256 rows unless that gives fewer than 200 workgroups and 128 rows
    give more; from 128 down to 64 rows where 128 give at most 128 workgroups and 64 give more."""
    M, nt = B * hw, (cout + BN - 1) // BN
    tiles = {mt: (M + 64 * mt - 1) // (64 * mt) * nt for mt in (1, 2, 4)}
    best = 2 if tiles[4] < 200 and tiles[2] > tiles[4] else 4
    return 1 if best == 2 and tiles[2] <= 128 and tiles[1] > tiles[2] else best


def splitk_tiles(case):
    """Pixel tiles per image of the plain split-K reduction (splitk_tiles16)."""
    hw = case.H * case.W
    tpi = max(1, min(512 // (case.B * ((case.Cout + 255) // 256)), hw // 4, 64))
    while tpi > 1 and hw % tpi:
        tpi -= 1
    return tpi


def plan_of(case):
    """The launch plan of a case from the library's host queries (no device needed).

    ksplit is ddnm_conv16_workspace_floats / (B H W Cout), fin is ddnm_conv16_fuses_fin, stats_tiles is
    ddnm_conv16_stats_tiles.  No query reports the pixel tile of a split launch, and the tile choice does not depend on Cin:
    a copy of the descriptor with Cin = 64, no fin and no residual (an unsplit 1x1 launch
    with res_ups is refused) is unsplit, and its stats_tiles is H W / (64 MT) (3x3 always; 1x1 when
    the tile divides the image).  Where that query returns 0 -- a GEMM tile that does not divide the image, so that tiles
    span images -- MT comes from the documented rule instead (`gemm_tile_rule`); the host test checks that the rule agrees
    with the query wherever the query can see the tile.  TW, n128, wmajor and slab16 restate the rules of plan16 /
    ddnm_conv16; TW is cross-checked by `tile_width_is_the_widest` and, on the GPU, by the per-tile statistics."""
    L = _lib()
    d = desc_of(case)
    q = ctypes.byref(d)
    assert L.ddnm_conv16_supported(q) == 1, case.name
    hw, M = case.H * case.W, case.B * case.H * case.W
    ws = int(L.ddnm_conv16_workspace_floats(q))
    assert ws >= 0 and ws % (M * case.Cout) == 0, (case.name, ws)
    ksplit = max(1, ws // (M * case.Cout))
    fin = int(L.ddnm_conv16_fuses_fin(q))
    stats_tiles = int(L.ddnm_conv16_stats_tiles(q))
    if case.out_nchw:
        mt, bm, kernel = 1, 256, "out"
    else:
        probe = int(L.ddnm_conv16_stats_tiles(ctypes.byref(_copy(d, Cin=KC, src1=None, C0=0, fin_gamma=None, res=None))))
        assert probe >= 0 and (probe > 0 or case.k == 1), (case.name, probe)
        mt = hw // (64 * probe) if probe > 0 else gemm_tile_rule(case.B, hw, case.Cout)
        assert mt in (1, 2, 4) and (probe == 0 or hw == 64 * mt * probe), (case.name, probe)
        bm, kernel = 64 * mt, ("k9" if case.k == 3 else "k1")
    n_tiles = (case.Cout + BN - 1) // BN
    if case.k == 3:
        tw = 32
        while tw >= 16 and (case.W % tw or case.H % (bm // tw)):
            tw >>= 1
        assert tw >= 16, case.name
        m_tiles, tiles_x, tpi = M // bm, case.W // tw, hw // bm
    else:
        tw, tiles_x, tpi, m_tiles = 0, 0, 0, (M + bm - 1) // bm
    if kernel == "k9" and mt == 4 and ksplit == 1 and not case.skip and m_tiles >= 128 and case.Cout == 128:
        kernel, n_tiles = "n128", 1
    slab16 = ksplit <= 8
    return {"kernel": kernel, "MT": mt, "BM": bm, "TW": tw, "tiles_x": tiles_x, "tiles_per_img": tpi, "m_tiles": m_tiles,
            "n_tiles": n_tiles, "ksplit": ksplit, "slab16": slab16, "slab": 0 if ksplit == 1 else (16 if slab16 else 32),
            "stats_tiles": stats_tiles, "fin": fin, "grid": m_tiles * n_tiles * ksplit,
            "wmajor": int(case.Cout * case.k * case.k > M and m_tiles <= 8) if kernel in ("k9", "k1") else 0,
            "nchunks": case.Cin // KC, "nsk": sum(case.skip) // KC if case.skip else 0}


def cell_of(case, plan):
    """The plan in the form of Case.cell."""
    return (plan["kernel"], plan["MT"], plan["TW"], plan["ksplit"], plan["slab"], plan["stats_tiles"], plan["fin"])


def tile_width_is_the_widest(case, plan):
    """The recorded TW tiles the image (W % TW == 0, H % (BM / TW) == 0) and 32 does not where 16 is recorded."""
    if case.k != 3:
        return plan["TW"] == 0
    bm = plan["BM"]
    ok = lambda tw: case.W % tw == 0 and case.H % (bm // tw) == 0
    return ok(plan["TW"]) and (plan["TW"] == 32 or not ok(32))


def slice_ranges(n, ksplit):
    """Chunk range [begin, end) of every split-K slice: n * s / ksplit."""
    return [(n * s // ksplit, n * (s + 1) // ksplit) for s in range(ksplit)]


def slice_partials(case, t, plan, act=None):
    """float64 partial sum of every slice (main chunks and shortcut chunks of its ranges): what a slab holds."""
    act = activation(case, t) if act is None else act
    main, skip = slice_ranges(plan["nchunks"], plan["ksplit"]), slice_ranges(plan["nsk"], plan["ksplit"])
    return [conv_part(case, t, act, chunks=m, skip_chunks=s) for m, s in zip(main, skip)]


def pixel_tiles(case, plan):
    """[B, H, W] long: the pixel tile (m_tile of the convolution kernel) every output pixel belongs to."""
    B, H, W, bm = case.B, case.H, case.W, plan["BM"]
    if case.k == 3:
        th, tw = bm // plan["TW"], plan["TW"]
        t = (torch.arange(H) // th)[:, None] * plan["tiles_x"] + (torch.arange(W) // tw)[None, :]
        return torch.arange(B)[:, None, None] * plan["tiles_per_img"] + t[None]
    return (torch.arange(B * H * W) // bm).reshape(B, H, W)


# ----------------------------------------------------------------------------- statistics
def stats_pixels(case, plan):
    """[tiles per image][pixels per tile] flat pixel indices (y * W + x) of every statistics tile of one image:
    fin: one tile; split: splitk_tiles16 flat runs; 3x3 unsplit: patches of 64 MT / TW rows x TW columns, row-major over the
    image; 1x1 unsplit: flat runs of 64 MT pixels."""
    hw, tiles = case.H * case.W, plan["stats_tiles"]
    if plan["fin"]:
        assert tiles == 1
        return torch.arange(hw).reshape(1, hw)
    if plan["ksplit"] > 1:
        assert tiles == splitk_tiles(case) and hw % tiles == 0
        return torch.arange(hw).reshape(tiles, hw // tiles)
    bm = plan["BM"]
    assert tiles == hw // bm and hw % bm == 0
    if case.k == 1:
        return torch.arange(hw).reshape(tiles, bm)
    tw, tx = plan["TW"], plan["tiles_x"]
    th = bm // tw
    t = torch.arange(tiles)
    y0, x0 = (t // tx) * th, (t % tx) * tw
    r = torch.arange(bm)
    return (y0[:, None] + (r // tw)[None, :]) * case.W + x0[:, None] + (r % tw)[None, :]


def stats_reference(case, out, plan):
    """float64 [B * tiles][Cout][2]: (sum, sum of squares) of `out` [B, Cout, H, W] (the fp16-rounded output) per statistics
    tile and channel, in the layout the kernels write: stats[(m * Cout + n) * 2 + {0, 1}], m = img * tiles + t."""
    pix = stats_pixels(case, plan)
    v = out.double().reshape(case.B, case.Cout, -1)[:, :, pix]           # [B][Cout][tiles][P]
    s, q = v.sum(-1), (v * v).sum(-1)
    return torch.stack([s, q], -1).permute(0, 2, 1, 3).reshape(case.B * pix.shape[0], case.Cout, 2)


# ----------------------------------------------------------------------------- conditions and bounds
def exactness_violations(case, t=None, plan=None):
    """Why the bit-exact comparison would NOT be justified for this case (empty: it is).  Every tensor integer-valued; the
    activated operand, the output, the output before the residual is added (the unsplit epilogue rounds there) and, with
    fp16 slabs, every slice's partial sum of magnitude <= 2048; sum |a||w| + |addends| < 2^24 per output element; the sum of
    squares (hence of magnitudes) of the outputs over every statistics tile < 2^24."""
    t = make_inputs(case) if t is None else t
    plan = plan_of(case) if plan is None else plan
    bad = []
    for name in ("x0", "x1", "w", "bias", "res", "scale", "shift", "skip0", "skip1", "skip_w"):
        v = t[name]
        if v is not None and not bool((v == v.round()).all()):
            bad.append(f"{name} is not integer-valued")
    act = activation(case, t)
    acc = conv_part(case, t, act)
    pre = acc if t["bias"] is None else acc + t["bias"].double()[None, :, None, None]
    ref = add_epilogue(case, t, acc)
    held = [("activated operand", act)]
    if not case.out_nchw:
        held += [("output", ref), ("output before the residual", pre)]
    if plan["ksplit"] > 1 and plan["slab16"]:
        held += [(f"partial sum of slice {s}", v) for s, v in enumerate(slice_partials(case, t, plan, act))]
    for name, v in held:
        if not float(v.abs().max()) <= H16_INT:
            bad.append(f"{name}: magnitude {float(v.abs().max()):.6g} > 2048")
    m = conv_part(case, t, act, mag=True)
    m = add_epilogue(case, {**t, "bias": None if t["bias"] is None else t["bias"].abs(), "res": None if t["res"] is None else t["res"].abs()}, m)
    if not float(m.max()) < LIMIT:
        bad.append(f"magnitude {float(m.max()):.4g} >= 2^24")
    if plan["stats_tiles"] > 0 and case.stats:
        s2 = float(stats_reference(case, ref, plan)[..., 1].max())
        if not s2 < LIMIT:
            bad.append(f"statistics: sum v^2 {s2:.4g} >= 2^24")
    return bad


def real_bound(case, t, e_act, plan=None):
    """Per-element bound of a swish case, float64 [B, Cout, H, W]:
        ((2^-11 + e_act) + (K + 8) 2^-24) (conv(|act|, |w|) + skip(|s|, |w_s|)) + r 2^-11 (|ref| + |res|) + 2^-24
    2^-11: the activated operand is rounded to fp16; e_act: the swish; (K + 8) 2^-24: a length-K fp32 sum in any order plus
    the handful of additions of the epilogue; r = 2 on the unsplit path (acc + bias is rounded to fp16, then rounded again
    after the residual is added), 1 on the reduction paths (one rounding), 0 for conv16_out (fp32 result); 2^-24: fp16
    subnormal results."""
    plan = plan_of(case) if plan is None else plan
    m = conv_part(case, t, mag=True)
    r = 0 if case.out_nchw else (2 if plan["ksplit"] == 1 else 1)
    ref = reference(case, t)
    rs = residual(case, t)
    tail = ref.abs() + (rs.abs() if rs is not None else 0.0)
    return ((U16 + e_act) + (case.K + 8) * U) * m + r * U16 * tail + U


# ----------------------------------------------------------------------------- what a case exercises (coverage list of the host test)
def features(case, plan):
    """Flat description of case + plan that the host test's coverage list matches against."""
    opts = {n for n in ("ups", "res", "res_ups", "bias", "out_nchw") if getattr(case, n)}
    opts -= {"res"} if case.res_ups else set()
    opts |= {"concat"} if case.C1 else set()
    opts |= {"skip"} if case.skip else set()
    opts |= {"gn"} if case.gn == "affine" else set()
    opts |= {"swish"} if case.real else set()
    opts |= {"film"} if case.fin == "film" else set()
    hw, ks, nch = case.H * case.W, plan["ksplit"], plan["nchunks"]
    f = {"name": case.name, "kernel": plan["kernel"], "k": case.k, "shape": (case.B, case.H, case.W, case.Cin, case.Cout),
         "B": case.B, "Cin": case.Cin, "Cout": case.Cout, "hw": (case.H, case.W), "square": case.H == case.W,
         "opts": frozenset(opts), "MT": plan["MT"], "TW": plan["TW"], "ksplit": ks, "split": ks > 1, "slab": plan["slab"],
         "fin": plan["fin"], "fin_asked": bool(case.fin), "stats_tiles": plan["stats_tiles"], "grid": plan["grid"],
         "grid_mod8": plan["grid"] % 8 != 0, "n_tiles": plan["n_tiles"], "wmajor": plan["wmajor"], "m_tiles": plan["m_tiles"],
         "cout_tail": case.Cout % BN, "nchunks": nch, "uneven_slices": ks > 1 and nch % ks != 0, "C0": case.C0,
         "concat_inside_slice": bool(case.C1) and ks > 1 and all(case.C0 // KC != b for b, _ in slice_ranges(nch, ks)),
         "ragged": case.k == 1 and (case.B * hw) % plan["BM"] != 0, "rows_last": (case.B * hw) % plan["BM"],
         "pixels": hw}
    if case.k == 3:
        th = plan["BM"] // plan["TW"]
        f.update(tiles_x=plan["tiles_x"], tile_rows=case.H // th)
    if case.skip:
        f["skip_idle_slices"] = sum(1 for a, b in slice_ranges(plan["nsk"], ks) if a == b)
    if plan["fin"]:
        cpg = case.Cout // 32
        cs = cpg
        while cs < 16:
            cs *= 2
        f["fin_slab"] = cs
    return f
