"""Case table, inputs, float64 references and plan queries shared by the exact-fp32 convolution edge tests
(test_conv_model_host.py without a GPU, test_gpu_conv_f32_edges.py on one).

The kernels under test (csrc/conv_igemm_f32.hip: halo and gather kernel on v_mfma_f32_32x32x2_f32, their split-K
reductions in csrc/conv_common.h; csrc/conv_small_f32.hip: fmaf chains) are fp32 multiply-add chains, fp32 slab sums and
fp32 statistics sums.  Fed integer-valued fp32 tensors whose every intermediate, in ANY summation order, is an integer
below 2^24, they have one representable answer, so the GPU tests compare bit for bit with the float64 reference below
(`exactness_violations` is the condition; the host test asserts it on every case).  Value ranges of the exact cases:
x in {-3..3}, w in {-2..2}, bias / badd / res / shortcut input in {-8..8} resp. {-3..3}, GroupNorm scale in {-2,-1,1,2},
shift in {-3..3} \\ {0} (the affine of a zero-padded pixel is then never zero: a kernel that pads BEFORE the prologue
adds w * shift along the border), no swish.  Cases that check statistics draw x, w from {-1, 0, 1}.

Swish cannot be exact: the `real` cases use data on a 2^-10 grid (standard normal, clamped to +-6), scale in
{+-0.5, +-1, +-2} and shift = 3 + a multiple of 2^-10 in [-0.5, 0.5], so that scale * x + shift is an fp32 number however
the kernel forms it (a multiple of 2^-11 below 16) and the only inexact step of the prologue is the swish itself.

A case names the plan cell it is meant to hit as `cell` = (kernel, tile, TW, ksplit[, statistics tiles]) with kernel
"halo" / "gather" / "small_cout" and TW = 0 for the gather kernel's flat strips; `plan_of` asks the library's host
queries.  The tile WIDTH has no query: the record states it, the host test checks that it is the widest of 32 / 16 / 8
that tiles the image (the rule in the kernel's header comment), and the per-tile statistics of the GPU test see it.
All tensors here are NCHW; the GPU test converts."""
import ctypes
import functools
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

KC = 32                                   # channels per K chunk
TILE_BM = {1: 128, 2: 64, 3: 128}         # output pixels / channels per workgroup tile (include/ddnm_hip.h: ddnm_conv_desc::tile)
TILE_BN = {1: 128, 2: 64, 3: 32}
BN_TILE = {128: 1, 64: 2, 32: 3}
LIMIT = float(2 ** 24)
U = 2.0 ** -24


class Case(NamedTuple):
    name: str
    B: int
    C0: int
    C1: int
    Cout: int
    Ho: int
    Wo: int
    cell: tuple                           # (kernel, tile, TW, ksplit[, stats tiles]) or ("small_cout",)
    k: int = 3
    stride: int = 1
    tile: int = 0                         # forced tile (0: the planner's choice)
    ups: bool = False                     # nearest x2 read of the sources
    gn: bool = False                      # GroupNorm affine prologue
    badd: bool = False                    # per-image addend, an offset view into wider rows
    res: bool = False
    res_ups: bool = False                 # the residual is read through a nearest x2 upsample
    nchw: bool = False
    skip: Optional[Tuple[int, int]] = None      # fused 1x1 shortcut over (SC0, SC1) raw channels
    stats: bool = False                   # emit_stats=True: x, w in {-1, 0, 1}
    real: bool = False                    # swish prologue on real-valued data (tolerance, not bits)
    ident: bool = False                   # real: identity weights (centre tap), the launch returns the activation

    @property
    def Cin(self):
        return self.C0 + self.C1

    @property
    def Hin(self):
        return self.Ho * self.stride

    @property
    def Win(self):
        return self.Wo * self.stride

    @property
    def pad(self):
        return self.k // 2 if self.stride == 1 else 0

    @property
    def src_hw(self):
        return (self.Hin // 2, self.Win // 2) if self.ups else (self.Hin, self.Win)

    @property
    def K(self):
        return self.k * self.k * self.Cin + (sum(self.skip) if self.skip else 0)


def _c(name, B, cin, cout, ho, wo, cell, **kw):
    c0, c1 = cin if isinstance(cin, tuple) else (cin, 0)
    return Case(name, B, c0, c1, cout, ho, wo, tuple(cell), **kw)


def _small_cout_cases():
    out = []
    for co in (1, 2, 3, 4):
        for B, cin, ho, wo in ((1, 32, 8, 32), (2, 96, 16, 64), (1, 32, 8, 64)):
            for gn in (False, True):
                out.append(_c(f"small_co{co}_{B}x{cin}_{ho}x{wo}{'_gn' if gn else ''}", B, cin, co, ho, wo, ("small_cout",),
                              nchw=True, gn=gn))
    return out


CASES = [
    # ---- halo kernel geometry: 3x3 / stride 1 / pad 1, bias only; forced tile x tile width
    _c("halo_t2_tw8", 1, 32, 64, 8, 8, ("halo", 2, 8, 1), tile=2),
    _c("halo_t2_tw16", 1, 32, 64, 4, 16, ("halo", 2, 16, 1), tile=2),
    _c("halo_t2_tw32", 1, 32, 64, 2, 32, ("halo", 2, 32, 1), tile=2),                # 4 x 34 = 136 halo rows exactly
    _c("halo_t1_tw8", 1, 32, 128, 16, 8, ("halo", 1, 8, 1), tile=1),
    _c("halo_t1_tw16", 1, 32, 128, 8, 16, ("halo", 1, 16, 1), tile=1),
    _c("halo_t1_tw32_cout96", 3, 64, 96, 8, 32, ("halo", 1, 32, 2), tile=1),         # 6 x 34 = 204 rows; Cout % 128; grid 6
    _c("halo_t3", 1, 64, 32, 16, 8, ("halo", 3, 8, 2)),
    _c("halo_t3_unsplit", 1, 32, 32, 16, 8, ("halo", 3, 8, 1)),
    _c("halo_t3_tw32", 1, 32, 32, 4, 32, ("halo", 3, 32, 1)),
    _c("halo_nchw_cout3", 3, 32, 3, 8, 8, ("halo", 2, 8, 1), nchw=True),              # small_cout declines: Win % 32
    _c("halo_nchw_cout6", 1, 32, 6, 8, 16, ("halo", 3, 16, 1), nchw=True),            # the ADM networks' output convolution
    _c("halo_nchw_cout5", 2, 64, 5, 8, 8, ("halo", 2, 8, 1), nchw=True),
    _c("halo_nchw_cout3_wide", 1, 32, 3, 4, 32, ("halo", 3, 32, 1), nchw=True),       # small_cout declines: Hin % 8
    _c("halo_16x24", 2, 64, 64, 16, 24, ("halo", 2, 8, 2)),                           # tiles_x 3, two tile rows, grid 12
    _c("halo_24x16_cout96", 1, 64, 96, 24, 16, ("halo", 2, 16, 2)),
    _c("halo_64x96_t1", 2, 32, 128, 64, 96, ("halo", 1, 32, 1), tile=1),              # tiles_x 3, 96 tiles
    _c("halo_cout66_two_chunks", 1, 64, 66, 8, 16, ("halo", 2, 16, 1)),               # Cout % 4: unsplit chunk loop
    _c("halo_32x32_t2_192tiles", 3, 64, 256, 32, 32, ("halo", 2, 32, 1), tile=2),
    # ---- options on the halo kernel: unsplit and split, two tiles each
    _c("cat_32_64_unsplit_t2", 1, (32, 64), 66, 8, 16, ("halo", 2, 16, 1)),
    _c("cat_64_32_split_t1", 1, (64, 32), 128, 16, 8, ("halo", 1, 8, 3), tile=1),
    _c("gn_unsplit_t1", 2, 32, 128, 8, 16, ("halo", 1, 16, 1), tile=1, gn=True),
    _c("gn_split_t2", 2, 64, 64, 8, 8, ("halo", 2, 8, 2), gn=True),
    _c("gn_cat_unsplit_t2", 2, (32, 64), 66, 8, 8, ("halo", 2, 8, 1), gn=True),
    _c("gn_cat_split_t1", 2, (64, 32), 128, 8, 16, ("halo", 1, 16, 3), tile=1, gn=True),
    _c("ups_unsplit_t2", 2, 32, 64, 8, 16, ("halo", 2, 16, 1), ups=True),
    _c("ups_split_t1", 1, 64, 128, 16, 8, ("halo", 1, 8, 2), tile=1, ups=True),
    _c("ups_gn_cat_unsplit_t1", 1, (32, 64), 130, 8, 16, ("halo", 1, 16, 1), tile=1, ups=True, gn=True),
    _c("ups_gn_cat_split_t2", 2, (64, 32), 64, 8, 24, ("halo", 2, 8, 3), ups=True, gn=True),
    _c("badd_unsplit_t2", 2, 32, 64, 8, 8, ("halo", 2, 8, 1), badd=True),
    _c("badd_split_t1", 2, 64, 128, 16, 8, ("halo", 1, 8, 2), tile=1, badd=True),
    _c("res_unsplit_t2", 2, 32, 64, 8, 16, ("halo", 2, 16, 1), res=True),
    _c("res_split_t1", 1, 64, 128, 8, 16, ("halo", 1, 16, 2), tile=1, res=True),
    _c("res_ups_unsplit_t1", 2, 32, 128, 8, 16, ("halo", 1, 16, 1), tile=1, res=True, res_ups=True),
    _c("res_ups_split_t2", 2, 64, 64, 8, 24, ("halo", 2, 8, 2), res=True, res_ups=True),
    _c("all_unsplit_t2", 3, (32, 64), 256, 32, 32, ("halo", 2, 32, 1), tile=2, ups=True, gn=True, badd=True, res=True),
    _c("skip_unsplit_t2", 1, 64, 66, 8, 16, ("halo", 2, 16, 1), gn=True, skip=(32, 64)),
    _c("skip_unsplit_t1", 2, 32, 128, 16, 8, ("halo", 1, 8, 1), tile=1, gn=True, skip=(64, 32)),
    _c("skip_split_t2", 2, 64, 64, 8, 8, ("halo", 2, 8, 2), gn=True, skip=(32, 32)),
    _c("skip_split_t1", 1, 96, 128, 8, 16, ("halo", 1, 16, 3), tile=1, gn=True, skip=(64, 32), res=True),
    _c("skip_one_chunk_six_slices", 1, 192, 64, 8, 8, ("halo", 2, 8, 6), gn=True, skip=(32, 0)),
    _c("skip_stats_unsplit", 2, 32, 64, 16, 8, ("halo", 2, 8, 1, 2), gn=True, skip=(32, 32), stats=True),
    _c("skip_stats_split", 1, 64, 96, 8, 8, ("halo", 2, 8, 2, 16), gn=True, skip=(32, 32), stats=True),
    # ---- split-K corners
    _c("split_one_chunk_per_slice", 1, 160, 64, 8, 16, ("halo", 2, 16, 5)),
    _c("split_uneven_6_over_4", 5, 192, 512, 16, 16, ("halo", 2, 16, 4), tile=2),
    _c("split_cap16", 1, 640, 64, 8, 8, ("halo", 2, 8, 16)),
    # ---- statistics: the reduction pass (split) ...
    _c("stats_split_bias_cout96_8x8", 1, 64, 96, 8, 8, ("halo", 2, 8, 2, 16), stats=True),        # 24 columns, 4-pixel strips
    _c("stats_split_badd_cout160_32x32", 1, 64, 160, 32, 32, ("halo", 2, 32, 2, 128), stats=True, badd=True),   # 40 columns
    _c("stats_split_res_24x24", 1, 64, 64, 24, 24, ("halo", 2, 8, 2, 96), stats=True, res=True),
    _c("stats_split_res_ups_16x12", 2, 64, 64, 16, 12, ("gather", 2, 0, 2, 48), stats=True, res=True, res_ups=True),
    _c("stats_split_t1_b3", 3, 64, 128, 16, 8, ("halo", 1, 8, 2, 32), tile=1, stats=True, gn=True),
    # ---- ... and the kernels' own epilogue (unsplit): every tile, every tile width, several tiles each way
    _c("stats_t2_16x24", 2, 32, 64, 16, 24, ("halo", 2, 8, 1, 6), stats=True, res=True),
    _c("stats_t2_tw16", 1, 32, 64, 8, 16, ("halo", 2, 16, 1, 2), stats=True, badd=True),
    _c("stats_t2_tw32", 2, 32, 64, 4, 64, ("halo", 2, 32, 1, 4), stats=True),
    _c("stats_t1_tw32_cout96", 2, 32, 96, 8, 64, ("halo", 1, 32, 1, 4), tile=1, stats=True, res=True, res_ups=True),
    _c("stats_t1_tw8", 1, 32, 128, 32, 8, ("halo", 1, 8, 1, 2), tile=1, stats=True),
    _c("stats_t3_tw16", 1, 32, 32, 8, 48, ("halo", 3, 16, 1, 3), stats=True),
    # ---- gather kernel: 1x1
    _c("g1x1_grid9", 3, 96, 160, 8, 8, ("gather", 2, 8, 3), k=1),
    _c("g1x1_t1", 1, 64, 128, 16, 8, ("gather", 1, 8, 2), k=1, tile=1),
    _c("g1x1_t3", 1, 32, 32, 16, 8, ("gather", 3, 8, 1), k=1, tile=3),
    _c("g1x1_gn_cat", 2, (32, 64), 64, 8, 8, ("gather", 2, 8, 3), k=1, gn=True),
    _c("g1x1_res_ups_split", 1, 64, 64, 8, 16, ("gather", 2, 16, 2), k=1, res=True, res_ups=True),
    _c("g1x1_res_ups_unsplit", 2, 32, 66, 8, 24, ("gather", 2, 8, 1), k=1, res=True, res_ups=True),
    _c("g1x1_nchw_cout6", 2, 32, 6, 8, 8, ("gather", 2, 8, 1), k=1, nchw=True),
    _c("g1x1_flat_16x12", 2, 64, 64, 16, 12, ("gather", 2, 0, 2), k=1),
    _c("g1x1_stats_t1", 2, 32, 128, 16, 16, ("gather", 1, 16, 1, 2), k=1, tile=1, stats=True),
    # ---- gather kernel: 3x3 stride 2, pad 0 (the bottom / right taps fall on padding)
    _c("gs2_8x16", 2, 32, 64, 8, 16, ("gather", 2, 16, 1), stride=2),
    _c("gs2_t1", 1, 64, 128, 16, 8, ("gather", 1, 8, 2), stride=2, tile=1),
    _c("gs2_gn_split", 2, 64, 64, 8, 8, ("gather", 2, 8, 2), stride=2, gn=True),
    _c("gs2_gn_unsplit", 1, 32, 64, 8, 24, ("gather", 2, 8, 1), stride=2, gn=True),
    _c("gs2_stats", 1, 32, 64, 16, 8, ("gather", 2, 8, 1, 2), stride=2, stats=True),
    # ---- gather kernel: the 3x3 stride-1 fallback on flat strips (Wo % 8 != 0)
    _c("g3x3_flat_gn_stats", 2, 32, 64, 16, 12, ("gather", 2, 0, 1, 3), tile=2, gn=True, stats=True),
    _c("g3x3_flat_gn_split", 1, 64, 64, 16, 12, ("gather", 2, 0, 2), tile=2, gn=True),
] + _small_cout_cases() + [
    # ---- swish prologue on real-valued data: identity launches (they return the activation) and one case per family
    _c("real_ident_g1x1", 2, 64, 64, 8, 8, ("gather", 2, 8, 2), k=1, gn=True, real=True, ident=True),
    _c("real_ident_halo", 2, 64, 64, 8, 8, ("halo", 2, 8, 2), gn=True, real=True, ident=True),
    _c("real_ident_small_cout", 1, 32, 4, 8, 32, ("small_cout",), nchw=True, gn=True, real=True, ident=True),
    _c("real_halo_t2", 2, 64, 64, 8, 16, ("halo", 2, 16, 2), gn=True, real=True, badd=True, res=True),
    _c("real_halo_t1_ups_cat", 1, (32, 32), 128, 8, 16, ("halo", 1, 16, 2), tile=1, gn=True, real=True, ups=True),
    _c("real_gs2", 2, 64, 64, 8, 8, ("gather", 2, 8, 2), stride=2, gn=True, real=True),
    _c("real_small_cout", 2, 64, 3, 8, 32, ("small_cout",), nchw=True, gn=True, real=True),
]
BY_NAME = {c.name: c for c in CASES}
EXACT_CASES = [c for c in CASES if not c.real]
REAL_CASES = [c for c in CASES if c.real]
BADD_OFFSET, BADD_EXTRA = 12, 20          # the addend starts 12 floats into rows of Cout + 20 (rounded up to 4) floats


def badd_stride(case):
    return (case.Cout + BADD_EXTRA + 3) // 4 * 4


# ----------------------------------------------------------------------------- inputs
def _gen(case, salt):
    h = salt
    for ch in case.name:
        h = (h * 1000003 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(h)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)


def _grid(x, step=2.0 ** -10):
    return torch.round(x / step) * step


def make_inputs(case):
    """The fp32 tensors of a case (NCHW): x0, x1, w, bias, badd_rows (the whole [B, stride] buffer, NaN outside the addend),
    res, scale, shift, skip0, skip1, skip_w; None where the case has none."""
    g = _gen(case, 1)
    B, hs, ws = case.B, *case.src_hw
    xa = 1 if case.stats else 3
    wa = 1 if case.stats else 2
    t = {"x1": None, "bias": None, "badd_rows": None, "res": None, "scale": None, "shift": None, "skip0": None, "skip1": None,
         "skip_w": None}
    if case.real:
        draw = lambda *s: _grid(torch.randn(*s, generator=g).clamp(-6.0, 6.0))
        t["x0"] = draw(B, case.C0, hs, ws)
        if case.C1:
            t["x1"] = draw(B, case.C1, hs, ws)
        if case.ident:
            w = torch.zeros(case.Cout, case.Cin, case.k, case.k)
            w[torch.arange(case.Cout), torch.arange(case.Cout), case.k // 2, case.k // 2] = 1.0
            t["w"] = w
        else:
            t["w"] = torch.randn(case.Cout, case.Cin, case.k, case.k, generator=g) * float(case.K) ** -0.5
            t["bias"] = torch.randn(case.Cout, generator=g)
        t["scale"] = torch.tensor([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0])[torch.randint(0, 6, (B, case.Cin), generator=g)]
        t["shift"] = 3.0 + _grid(torch.rand(B, case.Cin, generator=g) - 0.5)
        addend = lambda *s: torch.randn(*s, generator=g)
    else:
        t["x0"] = _ints(g, -xa, xa, B, case.C0, hs, ws)
        if case.C1:
            t["x1"] = _ints(g, -xa, xa, B, case.C1, hs, ws)
        t["w"] = _ints(g, -wa, wa, case.Cout, case.Cin, case.k, case.k)
        t["bias"] = _ints(g, -8, 8, case.Cout)
        if case.gn:
            t["scale"] = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (B, case.Cin), generator=g)]
            sh = _ints(g, 1, 3, B, case.Cin)
            t["shift"] = sh * (2.0 * torch.randint(0, 2, (B, case.Cin), generator=g).float() - 1.0)
        addend = lambda *s: _ints(g, -8, 8, *s)
    if case.badd:
        rows = torch.full((B, badd_stride(case)), float("nan"))
        rows[:, BADD_OFFSET:BADD_OFFSET + case.Cout] = addend(B, case.Cout)
        t["badd_rows"] = rows
    if case.res:
        t["res"] = addend(B, case.Cout, *((case.Ho // 2, case.Wo // 2) if case.res_ups else (case.Ho, case.Wo)))
    if case.skip:
        sc0, sc1 = case.skip
        t["skip0"] = _ints(g, -xa, xa, B, sc0, case.Ho, case.Wo)
        if sc1:
            t["skip1"] = _ints(g, -xa, xa, B, sc1, case.Ho, case.Wo)
        t["skip_w"] = _ints(g, -wa, wa, case.Cout, sc0 + sc1, 1, 1)
    return t


# ----------------------------------------------------------------------------- float64 reference
def _up2(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def activation(case, t):
    """float64 [B, Cin, Hin, Win]: concat, GroupNorm affine (+ swish for the real cases), nearest x2 -- what the taps read
    where they do not fall on the zero padding."""
    x = t["x0"].double() if t["x1"] is None else torch.cat([t["x0"], t["x1"]], 1).double()
    if case.gn:
        x = x * t["scale"].double()[:, :, None, None] + t["shift"].double()[:, :, None, None]
        if case.real:
            x = x * torch.sigmoid(x)
    return _up2(x) if case.ups else x


def _evaluate(case, t, mag):
    """The convolution with every option; `mag`: the same expression over absolute values (the magnitude every bound here
    is relative to)."""
    f = (lambda v: v.double().abs()) if mag else (lambda v: v.double())
    act = f(activation(case, t))
    p = case.pad
    pb = (case.Ho - 1) * case.stride + case.k - p - case.Hin             # zero padding AFTER the prologue
    pr = (case.Wo - 1) * case.stride + case.k - p - case.Win
    out = F.conv2d(F.pad(act, (p, pr, p, pb)), f(t["w"]), None if t["bias"] is None else f(t["bias"]), stride=case.stride)
    assert out.shape == (case.B, case.Cout, case.Ho, case.Wo), out.shape
    if case.skip:
        s = t["skip0"] if t["skip1"] is None else torch.cat([t["skip0"], t["skip1"]], 1)
        out = out + F.conv2d(f(s), f(t["skip_w"]))
    if case.badd:
        out = out + f(t["badd_rows"][:, BADD_OFFSET:BADD_OFFSET + case.Cout])[:, :, None, None]
    if case.res:
        r = f(t["res"])
        out = out + (_up2(r) if case.res_ups else r)
    return out


def reference(case, t):
    """float64 [B, Cout, Ho, Wo]."""
    return _evaluate(case, t, False)


def magnitude(case, t):
    """conv(|act|, |w|) + |bias| + |badd| + |res| (+ the shortcut's) per output element, float64."""
    return _evaluate(case, t, True)


def slow_reference(case, t):
    """The same result by explicit loops over images, taps and pixels in float64 (no F.conv2d, no F.pad, no
    repeat_interleave): an independent formulation for the host test, for tiny cases only."""
    B, Cout, Ho, Wo, k = case.B, case.Cout, case.Ho, case.Wo, case.k
    hs, ws = case.src_hw
    w = t["w"].double()
    out = torch.zeros(B, Cout, Ho, Wo, dtype=torch.float64)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                acc = t["bias"].double().clone() if t["bias"] is not None else torch.zeros(Cout, dtype=torch.float64)
                for ky in range(k):
                    for kx in range(k):
                        iy, ix = oy * case.stride - case.pad + ky, ox * case.stride - case.pad + kx
                        if not (0 <= iy < case.Hin and 0 <= ix < case.Win):
                            continue                                       # padding: contributes nothing, affine or not
                        sy, sx = (iy // 2, ix // 2) if case.ups else (iy, ix)
                        v = t["x0"][b, :, sy, sx].double()
                        if t["x1"] is not None:
                            v = torch.cat([v, t["x1"][b, :, sy, sx].double()])
                        if case.gn:
                            v = v * t["scale"][b].double() + t["shift"][b].double()
                            if case.real:
                                v = v / (1.0 + torch.exp(-v))
                        acc = acc + w[:, :, ky, kx] @ v
                if case.skip:
                    s = t["skip0"][b, :, oy, ox].double()
                    if t["skip1"] is not None:
                        s = torch.cat([s, t["skip1"][b, :, oy, ox].double()])
                    acc = acc + t["skip_w"].double()[:, :, 0, 0] @ s
                if case.badd:
                    acc = acc + t["badd_rows"][b, BADD_OFFSET:BADD_OFFSET + Cout].double()
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
    """The shape fields of the descriptor ops.conv2d fills for this case; every pointer the launch would carry is a
    non-null dummy (the planners look at some of them).  For the host queries only."""
    from ddnm_amd._lib import ConvDesc
    d = ConvDesc()
    d.src0 = d.weight = d.out = d.bias = _DUMMY
    if case.C1:
        d.src1 = _DUMMY
    if case.gn:
        d.gn_scale = d.gn_shift = _DUMMY
    if case.badd:
        d.badd, d.badd_stride = _DUMMY, badd_stride(case)
    if case.res:
        d.res, d.res_ups = _DUMMY, int(case.res_ups)
    if case.skip:
        d.skip0, d.skip_weight = _DUMMY, _DUMMY
        d.SC0, d.SC1 = case.skip
        if case.skip[1]:
            d.skip1 = _DUMMY
    d.B, d.Hin, d.Win, d.C0, d.C1, d.Cout = case.B, case.Hin, case.Win, case.C0, case.C1, case.Cout
    d.ksize, d.stride, d.pad, d.Ho, d.Wo = case.k, case.stride, case.pad, case.Ho, case.Wo
    d.ups, d.gn_silu, d.out_nchw, d.tile = int(case.ups), int(case.real), int(case.nchw), case.tile
    return d


def _copy(d, **fields):
    c = type(d).from_buffer_copy(d)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def plan_of(case):
    """The launch plan of a case from the library's host queries (no device needed):
    family, tile, BM, BN, kernel, flat, TW, tiles_x, ksplit, stats_tiles (per image), small_cout_ok."""
    L = _lib()
    d = desc_of(case)
    q = ctypes.byref(d)
    small_ok = L.ddnm_conv3x3_small_cout_f32_supported(q) == 1
    # ops._select_conv_family: NCHW launches of at most 4 output channels without a fused shortcut go to small_cout where it accepts
    if small_ok and case.nchw and case.Cout <= 4 and not case.skip:
        return {"family": "small_cout", "kernel": "small_cout", "small_cout_ok": True, "ksplit": 1, "stats_tiles": 0}
    bn = L.ddnm_conv2d_f32_tile_n(q)
    assert bn in BN_TILE, f"{case.name}: ddnm_conv2d_f32_tile_n = {bn}"
    tile = BN_TILE[bn]
    ws = int(L.ddnm_conv2d_f32_workspace_floats(q))
    per_slab = case.B * case.Ho * case.Wo * case.Cout
    assert ws >= 0 and ws % per_slab == 0, (case.name, ws)
    # the 2-D tiling exists exactly when the 3x3 / stride-1 / pad-1 launch of this output shape would run the halo kernel
    two_d = L.ddnm_conv2d_f32_fuses_skip(ctypes.byref(_copy(d, ksize=3, stride=1, pad=1, Hin=case.Ho, Win=case.Wo, ups=0))) == 1
    halo = case.k == 3 and case.stride == 1 and L.ddnm_conv2d_f32_fuses_skip(ctypes.byref(_copy(d, ups=0))) == 1
    tw = case.cell[2] if two_d else 0
    return {"family": "f32", "tile": tile, "BM": TILE_BM[tile], "BN": bn, "kernel": "halo" if halo else "gather",
            "flat": not two_d, "TW": tw, "tiles_x": case.Wo // tw if tw else 0, "ksplit": max(1, ws // per_slab),
            "stats_tiles": int(L.ddnm_conv2d_f32_stats_tiles(q)), "small_cout_ok": small_ok}


def cell_of(case, plan):
    """The plan in the form of Case.cell."""
    if plan["family"] == "small_cout":
        return ("small_cout",)
    cell = (plan["kernel"], plan["tile"], plan["TW"], plan["ksplit"])
    return cell + ((plan["stats_tiles"],) if case.stats else ())


def tile_width_is_the_widest(case, plan):
    """The recorded TW tiles the image (Wo % TW == 0, Ho % (BM / TW) == 0) and no wider one of 32 / 16 does."""
    if plan["family"] != "f32" or plan["flat"]:
        return True
    bm = plan["BM"]
    ok = lambda tw: tw <= bm and case.Wo % tw == 0 and case.Ho % (bm // tw) == 0
    return ok(plan["TW"]) and not any(ok(tw) for tw in (32, 16) if tw > plan["TW"])


# ----------------------------------------------------------------------------- statistics
def stats_pixels(case, plan):
    """[tiles per image][pixels per tile] flat pixel indices (oy * Wo + ox) of every statistics tile of one image."""
    hw = case.Ho * case.Wo
    tiles = plan["stats_tiles"]
    if plan["ksplit"] > 1 or plan["flat"]:
        # the reduction pass (tiles strips of hw / tiles consecutive pixels) / the gather kernel's flat strips of BM pixels
        assert hw % tiles == 0 and (plan["ksplit"] > 1 or hw // tiles == plan["BM"])
        return torch.arange(hw).reshape(tiles, hw // tiles)
    bm, tw, tx = plan["BM"], plan["TW"], plan["tiles_x"]
    th = bm // tw
    assert tiles == hw // bm and tx * tw == case.Wo and case.Ho % th == 0
    t = torch.arange(tiles)
    y0, x0 = (t // tx) * th, (t % tx) * tw
    r = torch.arange(bm)
    oy, ox = y0[:, None] + (r // tw)[None, :], x0[:, None] + (r % tw)[None, :]
    return oy * case.Wo + ox


def stats_reference(case, out, plan=None):
    """float64 [B * tiles][Cout][2]: (sum, sum of squares) of `out` [B, Cout, Ho, Wo] per statistics tile and channel, in
    the layout the kernels write: stats[(m * Cout + n) * 2 + {0, 1}], m = img * tiles + t."""
    plan = plan_of(case) if plan is None else plan
    pix = stats_pixels(case, plan)                                       # [tiles][P]
    v = out.double().reshape(case.B, case.Cout, -1)[:, :, pix]           # [B][Cout][tiles][P]
    s, q = v.sum(-1), (v * v).sum(-1)
    return torch.stack([s, q], -1).permute(0, 2, 1, 3).reshape(case.B * pix.shape[0], case.Cout, 2)


# ----------------------------------------------------------------------------- conditions and bounds
def exactness_violations(case, t=None, plan=None):
    """Why the bit-exact comparison would NOT be justified for this case (empty: it is).  Per output element
    conv(|act|, |w|) + |addends| < 2^24 and every tensor integer-valued; per statistics tile and channel
    sum |v| < 2^24 and sum v^2 < 2^24."""
    t = make_inputs(case) if t is None else t
    bad = []
    for name, v in t.items():
        if v is not None and name != "badd_rows" and not bool((v == v.round()).all()):
            bad.append(f"{name} is not integer-valued")
    if t["badd_rows"] is not None:
        v = t["badd_rows"][:, BADD_OFFSET:BADD_OFFSET + case.Cout]
        if not bool((v == v.round()).all()):
            bad.append("badd is not integer-valued")
    m = float(magnitude(case, t).max())
    if not m < LIMIT:
        bad.append(f"magnitude {m:.4g} >= 2^24")
    if case.stats:
        ref = reference(case, t)
        s1 = float(stats_reference(case, ref.abs(), plan)[..., 0].max())
        s2 = float(stats_reference(case, ref, plan)[..., 1].max())
        if not (s1 < LIMIT and s2 < LIMIT):
            bad.append(f"statistics: sum |v| {s1:.4g}, sum v^2 {s2:.4g} (limit 2^24)")
    return bad


def real_bound(case, t, e_act):
    """Per-element bound of a real-valued case: ((K + 8) 2^-24 + e_act) (conv(|act|, |w|) + |addends|): the first term
    bounds a length-K fp32 sum in any order (plus the handful of additions of the epilogue), the second the swish.
    Identity launches have one non-zero product per output: e_act alone."""
    m = magnitude(case, t)
    return (e_act if case.ident else (case.K + 8) * U + e_act) * m


# ----------------------------------------------------------------------------- what a case exercises (coverage list of the host test)
def features(case, plan):
    """Flat description of case + plan that the host test's coverage list matches against."""
    opts = {n for n in ("ups", "gn", "badd", "res", "nchw", "stats", "real", "ident") if getattr(case, n)}
    opts -= {"res"} if case.res_ups else set()
    opts |= {"res_ups"} if case.res_ups else set()
    opts |= {"concat"} if case.C1 else set()
    opts |= {"skip"} if case.skip else set()
    opts |= {"skip_concat"} if case.skip and case.skip[1] else set()
    f = {"name": case.name, "family": plan["family"], "kernel": plan["kernel"], "k": case.k, "stride": case.stride, "B": case.B,
         "Cout": case.Cout, "Cin": case.Cin, "hw": (case.Ho, case.Wo), "square": case.Ho == case.Wo, "opts": frozenset(opts),
         "bias_only": not (opts - {"nchw"}), "C0_ne_C1": case.C1 > 0 and case.C0 != case.C1, "C0": case.C0, "nchw": case.nchw,
         "ident": case.ident}
    if plan["family"] != "f32":
        return f
    nchunks, ks, bm, bn = case.Cin // KC, plan["ksplit"], plan["BM"], plan["BN"]
    hw = case.Ho * case.Wo
    grid = case.B * (hw // bm) * ((case.Cout + bn - 1) // bn)
    f.update(tile=plan["tile"], TW=plan["TW"], flat=plan["flat"], ksplit=ks, split=ks > 1, nchunks=nchunks, grid=grid,
             grid_mod8=grid % 8 != 0, cout_mod_bn=case.Cout % bn != 0, tiles_x=plan["tiles_x"],
             tile_rows=(case.Ho * plan["TW"] // bm if plan["TW"] else 0), multi_chunk=nchunks > 1,
             one_chunk_per_slice=ks > 1 and ks == nchunks, uneven_slices=ks > 1 and nchunks % ks != 0,
             capped=ks == 16 and nchunks > 16, small_cout_ok=plan["small_cout_ok"])
    if plan["kernel"] == "halo":
        th = bm // plan["TW"]
        f["halo_rows_full"] = (th + 2) * (plan["TW"] + 2) == (204 if bm == 128 else 136)
    if case.skip:
        f["skip_chunks_lt_slices"] = sum(case.skip) // KC < ks
    if case.stats:
        f["stats_tiles"] = plan["stats_tiles"]
        if ks > 1:
            c4n = case.Cout // 4
            f["columns"] = c4n                                            # float4 columns of the reduction pass
            f["cols_divide_256"] = 256 % c4n == 0
            f["strip_shorter_than_rows"] = hw // plan["stats_tiles"] < 256 // c4n
    return f
