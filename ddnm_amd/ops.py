"""Tensor-level wrappers over the C ABI (ddnm_amd/_lib.py).

PyTorch-ROCm is used here only as the owner of device memory and of the HIP
stream; every computation below is a hand-written HIP kernel from
ddnm_amd/csrc.  Nothing in this module falls back to torch ops.
"""
import ctypes
import math
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import Conv16Desc, ConvDesc, GemmDesc, StepScalars, check


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"{name}: expected a contiguous float32 device tensor, got {t.dtype} "
                         f"contiguous={t.is_contiguous()} device={t.device}")
    return t


# ----------------------------------------------------------------------------- kernel timing hook
class KernelTimer:
    """Optional per-launch timing of the convolution kernel with HIP events on the launch stream
    (used by bench.py for the roofline figure; off in normal operation)."""

    def __init__(self):
        self.records = []          # (variant, flops, start_event, end_event)
        self.shapes = []           # per record: (B, Ho, Wo, Cin, Cout, k, stride, ups, skipC, gn, res)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for variant, flops, e0, e1 in self.records:
            r = out.setdefault(variant, {"launches": 0, "flops": 0.0, "ms": 0.0})
            r["launches"] += 1
            r["flops"] += flops
            r["ms"] += e0.elapsed_time(e1)
        return out


_timer = None


def set_kernel_timer(t):
    global _timer
    _timer = t


def _launch(fn, d, label, record):
    """Checked launch of `fn(descriptor, stream)`.  With a `KernelTimer` installed the launch is bracketed by two events
    on the launch stream and recorded: `record()` -> (variant, flops, shape tuple of KernelTimer.shapes) is called only
    then (resolving the variant of some kernel families costs an extra library call)."""
    if _timer is None:
        check(fn(ctypes.byref(d), _stream()), label)
        return
    variant, flops, shape = record()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(fn(ctypes.byref(d), _stream()), label)
    e1.record()
    _timer.records.append((variant, flops, e0, e1))
    _timer.shapes.append(shape)


def max_launch_batch(per_image_bytes, margin=2):
    """Largest batch whose biggest activation stays `margin` times below the 2 GiB one convolution launch can address
    (32-bit byte offsets of the raw buffer descriptors, csrc/conv_common.h::conv_sizes_addressable): the models split a
    larger batch into chunks of this size INSIDE forward() instead of refusing it (the reference: "you may increase the
    batch_size to accelerate evaluation", README.md:89).  Margin 2 = half of the addressable limit (32 images for the celeba
    `Model` and the fp16-activation ADM UNet at 256 x 256, 16 for the fp32 ADM UNet): the 32-image BASELINE configurations run
    as ONE launch per layer (round 5's margin of 4 split them into two chunks plus a concat copy)."""
    return max(1, (1 << 31) // int(per_image_bytes) // margin)


# ----------------------------------------------------------------------------- convolution
CONV_COUT_ALIGN = 128

# Module switches: tests and tools set them ON THE MODULE (monkeypatch / a script's assignment), so every use below reads
# them at call time.
_NO_FUSED_GN = False            # A/B profiling: convolutions emit no GroupNorm partials
FORCE_ONE_TILE = False          # A/B timing: every split-fp16 3x3 launch on the one-tile kernel
_NO_S16_GATHER = False          # A/B: gather-form launches stay on the fp32 MFMA kernel
_S16_CHECK = False              # debugging: assert finiteness after every split-fp16 launch (synchronises)
_F16_PREPASS_MIN_COUT = 256     # first-generation fp16 3x3 launches of at least this many output channels take the GroupNorm pre-pass

_conv_ws = {}


def _conv_workspace(device, floats):
    """Split-K scratch, one buffer per (device, stream), grown on demand: stream order makes reuse safe within a
    stream, and the two half-batch streams of a captured forward (ddnm_amd/graph.py) must not share one."""
    key = (device, _stream())
    ws = _conv_ws.get(key)
    if ws is None or ws.numel() < floats:
        ws = torch.empty(int(floats), dtype=torch.float32, device=device)
        _conv_ws[key] = ws
    return ws


def pack_conv_weight(w, cin_pad=None):
    """OIHW [Cout,Cin,k,k] -> (O, ky, kx, I) with Cout padded to 128 and Cin to `cin_pad`."""
    cout, cin, kh, kw = w.shape
    cin_pad = cin if cin_pad is None else cin_pad
    cout_pad = (cout + CONV_COUT_ALIGN - 1) // CONV_COUT_ALIGN * CONV_COUT_ALIGN
    out = torch.zeros(cout_pad, kh * kw, cin_pad, dtype=torch.float32, device=w.device)
    out[:cout, :, :cin] = w.float().permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
    return out.contiguous()


class Act:
    """An NHWC activation plus, when its producer could emit them, the GroupNorm partials of it
    (per-(M tile, channel) sum / sum of squares written by the convolution epilogue)."""
    __slots__ = ("t", "stats", "tiles", "gn")

    def __init__(self, t, stats=None, tiles=0, gn=None):
        self.t, self.stats, self.tiles = t, stats, tiles
        # (scale, shift, name): the affine of the consumer GroupNorm `name`, already finalized by the producing launch
        # (split-K reduction pass, ddnm_conv16_desc::fin_*); valid until the next finalize reuses the workspace
        self.gn = gn


def tensor_of(x):
    """The tensor of an `Act`; a tensor (or None) as it is."""
    return x.t if isinstance(x, Act) else x


def _shape_desc(B, H, W, cin, cout, ksize=3, stride=1):
    """Shape-only `ConvDesc` of a one-source conv over a [B, H, W, cin] INPUT ("same" padding at stride 1, none at
    stride 2), for the planners' support queries."""
    d = ConvDesc()
    d.B, d.Hin, d.Win, d.C0, d.C1, d.Cout = B, H, W, cin, 0, cout
    d.ksize, d.stride, d.pad, d.Ho, d.Wo = ksize, stride, (ksize // 2 if stride == 1 else 0), H // stride, W // stride
    return d


def conv_fuses_skip(B, H, W, cin, cout):
    """True when a 3x3 / stride-1 conv of this shape runs on the halo kernel, i.e. can take a fused shortcut."""
    return _lib.lib().ddnm_conv2d_f32_fuses_skip(ctypes.byref(_shape_desc(B, H, W, cin, cout))) == 1


def pack_skip_weight(w, f16=False):
    """1x1 shortcut weights [Cout, Cin, 1, 1] -> [Cout_pad][Cin] (fp32, or fp16 for the fp16-operand kernel)."""
    p = pack_conv_weight(w).reshape(-1, w.shape[1]).contiguous()
    return p.to(torch.float16) if f16 else p


def pack_conv_weight_f16(w, cin_pad=None):
    """OIHW fp32/fp16 -> (O, ky, kx, I) IEEE fp16, Cout padded to 128 (operands of ddnm_conv3x3_f16_f32)."""
    return pack_conv_weight(w, cin_pad=cin_pad).to(torch.float16).contiguous()


def s16_weight_scale(*ws):
    """The power of two 2^s that brings max|W| of a launch's weight tensors (3x3 kernel + fused shortcut: they share
    one accumulator) into [2^13, 2^14): fp16 `hi` parts stay far from 65504 and the `lo` parts of all but negligible
    weights are normal fp16 numbers (include/ddnm_hip.h::ddnm_conv3x3_s16_f32)."""
    m = max(float(w.abs().max()) for w in ws)
    if not (m > 0.0) or not math.isfinite(m):
        return 1.0
    return 2.0 ** (13 - math.floor(math.log2(m)))


def s16_weight_row_bound(scale, *ws):
    """Worst output row's relative split error of a launch's weights: max_o sum_k eps(scale W[o, k]) / sum_k |scale W[o, k]|
    over ALL tensors that share the accumulator (3x3 kernel + fused shortcut), with the element model of
    csrc/conv_common.h::split_store: eps(v) = 0 for v = 0, 2^-25 for |v| < 0.25 (`lo` is a subnormal fp16 number), 2^-22 |v|
    above.  Exactly 2^-22 while every weight of every row is carried relatively; it grows when a row lies so far below the
    launch's maximum that its weights keep the ABSOLUTE 2^-25 only.  All-zero rows (Cout padding) are skipped.  A phase tensor
    [py][px][O][I][a][b] (upsample_phase_weights) is judged per (phase, output channel): each phase has its own accumulator."""
    num = den = None
    for w in ws:
        v = w.detach().to(torch.float64)
        v = (v.flatten(0, 2) if v.dim() == 6 else v).flatten(1).abs() * float(scale)       # [rows][everything a row sums over]
        eps = torch.where(v == 0, torch.zeros_like(v), torch.where(v < 0.25, torch.full_like(v, 2.0 ** -25), v * 2.0 ** -22))
        n, d_ = eps.sum(1), v.sum(1)
        num, den = (n, d_) if num is None else (num + n, den + d_)
    live = den > 0
    if not bool(live.any()):
        return 0.0
    return float((num[live] / den[live]).max())


# Weight-range limit of the split-fp16 launches (Model.load_state_dict): a launch whose s16_weight_row_bound exceeds it runs
# the exact-fp32 kernel.  In units of 2^-22 a product's relative error is (weight term) + (activation term: 1 for an operand
# carried relatively) + (dropped lo.lo': 1); an all-relative weight row has weight term 1, and allowing it to DOUBLE -- 2^-21 --
# keeps an output channel within 4 . 2^-22 of its own magnitude sum |w||a| (the row sum weighs every k alike, i.e. activations of
# comparable size over k; the tier definition of tests/s16_model.py weighs them as they are), the order of the fp32 kernel's
# own accumulation error.  Beyond it a row keeps only an absolute bound (relative to the launch's largest row).  Not tuned.
S16_WEIGHT_ROW_LIMIT = 2.0 ** -21


def pack_conv_weight_s16(w, scale):
    """OIHW fp32 -> the split packing of ddnm_conv3x3_s16_f32: (O, ky, kx, I) with Cout padded to 128, every 32-channel
    chunk stored as 32 hi halfs then 32 lo halfs of scale * W (hi = rn16, lo = rn16(residual)); returned as an fp16
    tensor [Cout_pad][taps][Cin/32][2][32] (= the byte size of the fp32 packing)."""
    p = pack_conv_weight(w) * float(scale)                      # [Cout_pad][taps][Cin], power-of-two scaling: exact
    cp, taps, cin = p.shape
    if cin % 32:
        raise ValueError("split packing needs Cin % 32 == 0")
    hi = p.to(torch.float16)
    lo = (p - hi.float()).to(torch.float16)
    hi, lo = hi.view(cp, taps, cin // 32, 1, 32), lo.view(cp, taps, cin // 32, 1, 32)
    return torch.cat([hi, lo], 3).contiguous()


def upsample_phase_weights(w):
    """OIHW 3x3 weights of `nearest x2 -> conv3x3(pad 1)` -> the four 2x2 kernels Wp[py][px][O][I][a][b] (fp64) that give the
    same output on the LOW-resolution grid: out[2y + py][2x + px] = sum_ab Wp[py][px][a][b] . X[y + py - 1 + a][x + px - 1 + b].
    Row phase 0 sends ky = 0 to offset -1 and ky = 1, 2 to 0; phase 1 sends ky = 0, 1 to 0 and ky = 2 to +1; columns alike."""
    w = w.detach().to(torch.float64)
    # sel[p][a][k] = 1 when tap k of phase p lands on 2x2 position a
    sel = torch.tensor([[[1, 0, 0], [0, 1, 1]], [[1, 1, 0], [0, 0, 1]]], dtype=torch.float64, device=w.device)
    return torch.einsum("pak,qbl,oikl->pqoiab", sel, sel, w)


UPS_SUBPIXEL = 2          # include/ddnm_hip.h::DDNM_CONV_UPS_SUBPIXEL


def pack_upsample_conv_weight_s16(w, scale):
    """Phase packing of an upsample convolution for ddnm_conv3x3_s16_f32 with DDNM_CONV_UPS_SUBPIXEL: scale * Wp (summed in fp64,
    `scale` = s16_weight_scale of the SUMMED tensor: |Wp| reaches 4 max|W|) split into hi / lo fp16, as an fp16 tensor
    [4 Cout][4 steps (a, b)][Cin / 32][2][32] with row ((cb * 2 + py) * 2 + px) * 64 + c for output channel cb * 64 + c."""
    cout, cin = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3) or cin % 32 or cout % 64:
        raise ValueError("phase packing needs 3x3 weights, Cin % 32 == 0 and Cout % 64 == 0")
    wp = upsample_phase_weights(w) * float(scale)                # [py][px][O][I][a][b], power-of-two scaling: exact
    wp = wp.reshape(2, 2, cout // 64, 64, cin, 4).permute(2, 0, 1, 3, 5, 4).reshape(4 * cout, 4, cin)
    hi = wp.to(torch.float16)
    lo = (wp - hi.double()).to(torch.float16)
    hi, lo = hi.view(4 * cout, 4, cin // 32, 1, 32), lo.view(4 * cout, 4, cin // 32, 1, 32)
    return torch.cat([hi, lo], 3).contiguous()


def upsample_weight_s16(w):
    """(packed, scale, None) of pack_upsample_conv_weight_s16 with the scale of the summed tensor: `weight_s16` of
    conv2d(..., ups=True, ups_subpixel=True)."""
    sc = s16_weight_scale(upsample_phase_weights(w))
    return (pack_upsample_conv_weight_s16(w, sc), sc, None)


def conv_runs_ups_subpixel(B, H, W, cin, cout):
    """True when `nearest x2 -> 3x3` over a [B, H, W, cin] LOW-resolution input can take the sub-pixel form."""
    d = _shape_desc(B, 2 * H, 2 * W, cin, cout)
    d.ups, d.flags = 1, UPS_SUBPIXEL
    return _lib.lib().ddnm_conv3x3_s16_ups_subpixel_supported(ctypes.byref(d)) == 1


def conv_runs_s16(B, H, W, cin, cout, ups=False):
    """True when a 3x3 / stride-1 conv of this OUTPUT shape takes the split-fp16 kernel (given split-packed weights)."""
    return _lib.lib().ddnm_conv3x3_s16_supported(ctypes.byref(_shape_desc(B, H, W, cin, cout))) == 1


def conv_runs_s16_gather(B, H, W, cin, cout, ksize=3, stride=1):
    """True when a conv of this INPUT shape takes the gather form of the split-fp16 arithmetic (no fused shortcut)."""
    if _NO_S16_GATHER:
        return False
    return _lib.lib().ddnm_conv_gather_s16_supported(ctypes.byref(_shape_desc(B, H, W, cin, cout, ksize, stride))) == 1


_S16_ACT_SCALE = None


def _s16_act_scale():
    global _S16_ACT_SCALE
    if _S16_ACT_SCALE is None:
        _S16_ACT_SCALE = float(_lib.lib().ddnm_conv3x3_s16_act_scale())
    return _S16_ACT_SCALE


def conv_runs_f16(B, H, W, cin, cout, ksize=3):
    """True when a stride-1 conv of this shape takes the fp16-operand kernel (given packed fp16 weights)."""
    L = _lib.lib()
    d = _shape_desc(B, H, W, cin, cout, ksize)
    return (L.ddnm_conv3x3_f16_supported if ksize == 3 else L.ddnm_conv1x1_f16_supported)(ctypes.byref(d)) == 1


_f16_scratch_buf = {}


def _f16_scratch(device, numel, slot=0):
    """fp16 activation scratch of the GroupNorm pre-pass (slot 0) / the im2col matrix (slot 1); stream order makes
    reuse safe."""
    key = (device, slot, _stream())
    buf = _f16_scratch_buf.get(key)
    if buf is None or buf.numel() < numel:
        buf = torch.empty(numel, dtype=torch.float16, device=device)
        _f16_scratch_buf[key] = buf
    return buf


AMAX_N = 32          # include/ddnm_hip.h::DDNM_AMAX_N


def amax_bound(a0, a1=None):
    """[B][AMAX_N] per-image upper bounds of |concat(a0, a1)| for the operand-range guard of the split-fp16 kernels
    (ddnm_conv_desc::amax_in): from the producers' GroupNorm partials when the `Act`s carry them (a few KB ... 2 MB read),
    otherwise from the tensors themselves.  One small launch, no host synchronisation."""
    def src(a):
        if a is None:
            return None, 0, 0
        if isinstance(a, Act) and a.stats is not None:
            B = a.t.shape[0]
            return a.stats, a.stats.numel() // B, 1
        t = tensor_of(a)
        return _f32c(t, "amax source"), t.numel() // t.shape[0], 0
    t0 = tensor_of(a0)
    B = t0.shape[0]
    p0, n0, k0 = src(a0)
    p1, n1, k1 = src(a1)
    out = torch.empty(B * AMAX_N, dtype=torch.float32, device=t0.device)
    check(_lib.lib().ddnm_amax_bound_f32(_p(p0), n0, k0, _p(p1), n1, k1, _p(out), B, _stream()), "ddnm_amax_bound_f32")
    return out


class ConvFamily(NamedTuple):
    """One kernel family of the convolution launchers.  Entry points are NAMES, resolved on the loaded library at call time."""
    name: str
    run: str
    stats_tiles: Optional[str]          # None: the family emits no GroupNorm partials ...
    workspace_floats: Optional[str]     # ... / takes no workspace
    variant: Callable                   # (library, descriptor) -> `KernelTimer` variant label; asked only under a timer
    pack: str = "f32"                   # which of conv2d's weight packs the launch reads: "f32" / "s16" / "f16"
    label: str = "ddnm_conv2d"          # what a refused launch is reported under
    strict: bool = False                # True: a negative planner answer raises under the planner's name; False: the
    #                                     launch goes on and the launcher refuses the descriptor under `label`


def _f32_variant(L, d):
    kind = "conv3x3_halo_f32" if (d.ksize == 3 and d.stride == 1) else "conv_gather_f32"
    return kind + {128: "<128x128>", 64: "<64x64>", 32: "<128x32>"}[L.ddnm_conv2d_f32_tile_n(ctypes.byref(d))]


def _s16_variant(L, d):
    persistent = L.ddnm_conv3x3_s16_persistent(ctypes.byref(d)) == 1
    return "conv3x3_s16_persist<256x128>" if persistent else "conv3x3_halo_s16<256x128>"


CONV_FAMILIES = {f.name: f for f in (
    # the network's 3-channel output convolution: HBM-bound vector-ALU kernel (csrc/conv_small_f32.hip)
    ConvFamily("small_cout", "ddnm_conv3x3_small_cout_f32", None, None, lambda L, d: "conv3x3_small_cout_f32",
               label="ddnm_conv3x3_small_cout_f32"),
    # split-fp16 arithmetic (fp32-grade products on the fp16 matrix pipe): the sub-pixel form of an upsample convolution,
    # the 3x3 / stride-1 halo kernel, and the per-tap gather form for 1x1 / strided / 8x8-level launches (no fused shortcut)
    ConvFamily("s16_subpixel", "ddnm_conv3x3_s16_f32", "ddnm_conv3x3_s16_stats_tiles", "ddnm_conv3x3_s16_workspace_floats",
               lambda L, d: "conv2x2x4_s16_subpixel<256x128>", pack="s16"),
    ConvFamily("s16", "ddnm_conv3x3_s16_f32", "ddnm_conv3x3_s16_stats_tiles", "ddnm_conv3x3_s16_workspace_floats",
               _s16_variant, pack="s16"),
    ConvFamily("s16_gather", "ddnm_conv_gather_s16_f32", "ddnm_conv_gather_s16_stats_tiles",
               "ddnm_conv_gather_s16_workspace_floats", lambda L, d: "conv_gather_s16", pack="s16"),
    # first-generation fp16-operand engine (the reference's use_fp16 torso): halo kernel, and one GEMM (1x1, im2col'd 3x3)
    ConvFamily("f16_3x3", "ddnm_conv3x3_f16_f32", "ddnm_conv3x3_f16_stats_tiles", "ddnm_conv3x3_f16_workspace_floats",
               lambda L, d: "conv3x3_halo_f16<256x128>", pack="f16"),
    ConvFamily("f16_1x1", "ddnm_conv1x1_f16_f32", "ddnm_conv1x1_f16_stats_tiles", "ddnm_conv1x1_f16_workspace_floats",
               lambda L, d: "conv1x1_f16<256x128>", pack="f16"),
    # exact fp32: everything else
    ConvFamily("f32", "ddnm_conv2d_f32", "ddnm_conv2d_f32_stats_tiles", "ddnm_conv2d_f32_workspace_floats", _f32_variant),
    # fp16-activation path (csrc/conv16.hip; descriptor: Conv16Desc)
    ConvFamily("conv16", "ddnm_conv16", "ddnm_conv16_stats_tiles", "ddnm_conv16_workspace_floats",
               lambda L, d: f"conv16<{d.ksize}x{d.ksize}>", pack="h16", label="ddnm_conv16", strict=True),
    ConvFamily("conv16_out", "ddnm_conv16", None, None, lambda L, d: "conv16<out>", pack="h16", label="ddnm_conv16(out)"),
)}


def _desc_copy(d, **fields):
    """A copy of descriptor `d` with `fields` replaced: what a planner is asked about an alternative form of the launch."""
    c = type(d).from_buffer_copy(d)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def _f16_im2col(L, d, src0, src1, gn_silu):
    """Lowest-resolution 3x3 launches of the first-generation engine (a 256-pixel tile would span several images): im2col
    with the GroupNorm prologue, then ONE fp16 GEMM with K = 9*Cin -- the (O,ky,kx,I)-packed weights are its matrix.
    Returns the GEMM's descriptor once the im2col launch is issued, None when the launch does not qualify."""
    B, Hs, Ws, _ = src0.shape
    if d.stride != 1 or d.ups or d.skip0 or d.out_nchw or d.res_ups or Hs * Ws >= 256 or (d.C0 | d.C1) % 8:
        return None
    cin = d.C0 + d.C1
    g = _desc_copy(d, ksize=1, pad=0, C0=9 * cin, C1=0, gn_scale=None, gn_shift=None)
    if L.ddnm_conv1x1_f16_supported(ctypes.byref(g)) != 1:
        return None
    col = _f16_scratch(src0.device, B * Hs * Ws * 9 * cin, slot=1)
    check(L.ddnm_im2col3x3_f16(_p(src0), _p(src1), d.gn_scale, d.gn_shift, col.data_ptr(), B, Hs, Ws, d.C0, d.C1,
                               int(gn_silu), _stream()), "ddnm_im2col3x3_f16")
    g.src0, g.src1, g.src_f16 = col.data_ptr(), None, 1
    return g


def _f16_gn_prepass(L, d, src0, src1, gn_silu):
    """GroupNorm (+ swish) once per element into an fp16 scratch tensor instead of once per (128-output-channel tile x
    halo overlap) inside the conv's loader; returns the descriptor that reads the scratch tensor."""
    B, Hs, Ws, _ = src0.shape
    cin = d.C0 + d.C1
    h16 = _f16_scratch(src0.device, B * Hs * Ws * cin)
    check(L.ddnm_gn_apply_f16(_p(src0), _p(src1), d.gn_scale, d.gn_shift, h16.data_ptr(), B, Hs * Ws, d.C0, d.C1,
                              int(gn_silu), _stream()), "ddnm_gn_apply_f16")
    return _desc_copy(d, src0=h16.data_ptr(), src1=None, C0=cin, C1=0, gn_scale=None, gn_shift=None, src_f16=1)


def _select_f16(L, d, src0, src1, gn, gn_silu):
    """The first-generation fp16-operand engine's part of _select_conv_family (packed fp16 weights are on offer): the
    halo kernel or the GEMM where the shape qualifies, with their pre-passes issued; the exact-fp32 kernels otherwise."""
    fam, launch = CONV_FAMILIES["f32"], d
    if d.ksize == 3:
        if L.ddnm_conv3x3_f16_supported(ctypes.byref(d)) == 1:
            fam = CONV_FAMILIES["f16_3x3"]
        else:
            g = _f16_im2col(L, d, src0, src1, gn_silu)
            if g is not None:
                return CONV_FAMILIES["f16_1x1"], g, None          # (the im2col launch has applied the GroupNorm)
    elif d.ksize == 1 and not d.skip0:
        g = _desc_copy(d, gn_scale=None, gn_shift=None)           # the GEMM kernel has no fused prologue: always the pre-pass
        if L.ddnm_conv1x1_f16_supported(ctypes.byref(g)) == 1:
            fam, launch = CONV_FAMILIES["f16_1x1"], g
    if fam.pack == "f16" and gn is not None and (fam.name == "f16_1x1" or d.Cout >= _F16_PREPASS_MIN_COUT):
        launch = _f16_gn_prepass(L, d, src0, src1, gn_silu)
    return fam, launch, gn


def _select_conv_family(L, d, src0, src1, gn, gn_silu, weight_s16, weight_f16):
    """The kernel family of the filled descriptor `d`, given the packs on offer -> (family, descriptor to launch, the
    GroupNorm affine the launch still applies).  Precedence: small_cout; the split-fp16 families (sub-pixel or 3x3, then
    gather); with `weight_f16` the first-generation engine INSTEAD of those; exact fp32.  Every planner sees `d` as the
    launch will: the fused-shortcut fields are filled (some planners key on the pointer, some on the channel counts; ADVICE
    r3 / r4) and `weight` is still the fp32 pack -- the chosen pack's pointers are set by conv2d afterwards."""
    q, fused = ctypes.byref(d), bool(d.skip0)
    if (d.out_nchw and d.Cout <= 4 and not fused and weight_f16 is None
            and L.ddnm_conv3x3_small_cout_f32_supported(q) == 1):
        return CONV_FAMILIES["small_cout"], d, gn
    if weight_f16 is not None:
        return _select_f16(L, d, src0, src1, gn, gn_silu)
    if weight_s16 is not None:
        if d.flags == UPS_SUBPIXEL:                               # (conv2d has checked that the launch qualifies)
            return CONV_FAMILIES["s16_subpixel"], d, gn
        if (d.ksize == 3 and d.stride == 1
                and (not fused or (weight_s16[2] is not None and gn is not None and d.SC0 % 32 == 0 and d.SC1 % 32 == 0))
                and L.ddnm_conv3x3_s16_supported(q) == 1):
            return CONV_FAMILIES["s16"], d, gn
        if not fused and not _NO_S16_GATHER and L.ddnm_conv_gather_s16_supported(q) == 1:
            return CONV_FAMILIES["s16_gather"], d, gn
    return CONV_FAMILIES["f32"], d, gn


def _launch_conv(L, fam, d, out, emit_stats, record):
    """The tail of every convolution launch: the GroupNorm-partials tensor where the plan emits them, the split-K
    workspace, the checked launch -> Act(out, stats, tiles)."""
    stats, tiles = None, 0
    if emit_stats and fam.stats_tiles is not None:
        tiles = getattr(L, fam.stats_tiles)(ctypes.byref(d))
        if tiles < 0 and fam.strict:
            check(tiles, fam.stats_tiles)
        if tiles > 0:
            stats = torch.empty(d.B * tiles * d.Cout * 2, dtype=torch.float32, device=out.device)
            d.stats_out = stats.data_ptr()
    if fam.workspace_floats is not None:
        need = getattr(L, fam.workspace_floats)(ctypes.byref(d))
        if need < 0 and fam.strict:
            check(int(need), fam.workspace_floats)
        if need > 0:
            ws = _conv_workspace(out.device, need)
            d.workspace, d.workspace_floats = ws.data_ptr(), ws.numel()
    _launch(getattr(L, fam.run), d, fam.label, record)
    return Act(out, stats, tiles)


def conv2d(src0, weight, cout, ksize, *, src1=None, bias=None, badd=None, badd_stride=0, res=None, res_ups=False,
           gn=None, gn_silu=True, stride=1, pad=None, ups=False, out=None, out_nchw=False, out_hw=None, tile=0,
           emit_stats=False, weight_f16=None, skip=None, skip_weight=None, skip_weight_f16=None, weight_s16=None,
           raw_amax=None, one_tile=False, ups_subpixel=False):
    """NHWC implicit-GEMM convolution; see include/ddnm_hip.h::ddnm_conv_desc.
    ups_subpixel=True (with ups=True): `weight_s16` is the PHASE packing (upsample_weight_s16) and the launch runs the
    sub-pixel form of the split-fp16 kernel; a launch that does not qualify is an error.
    one_tile=True: the split-fp16 3x3 launch runs the one-tile-per-workgroup kernel where the persistent form would apply
    (same results bit for bit; A/B timing and the bit-identity tests).
    With emit_stats=True returns an `Act` (tensor + GroupNorm partials when the launch can produce them).
    weight_f16 (packed fp16 weights): the fp16-operand MFMA path (the reference's use_fp16 torso) where the shape qualifies.
    weight_s16 = (packed, scale, packed_skip or None) from pack_conv_weight_s16: 3x3 / stride-1 launches whose shape
    qualifies then run the split-fp16 kernel (fp32-grade products on the fp16 matrix pipe) instead of the fp32 one.
    Operands such a launch reads RAW (no GroupNorm: the main operand when gn is None, the fused shortcut's input always)
    are range-guarded: `raw_amax` = their [B][AMAX_N] bound (amax_bound / group_norm_affine(want_amax=True)); when it is
    not supplied it is computed here from the producers' partials or the tensors."""
    a_src0, a_src1 = src0, src1                 # (possibly `Act`s: their partials feed the operand bound)
    src0, src1, res = tensor_of(src0), tensor_of(src1), tensor_of(res)
    B, Hs, Ws, C0 = src0.shape
    C1 = 0 if src1 is None else src1.shape[3]
    Hin, Win = (2 * Hs, 2 * Ws) if ups else (Hs, Ws)
    if pad is None:
        pad = ksize // 2
    Ho, Wo = (Hin // stride, Win // stride) if out_hw is None else out_hw
    if out is None:
        shape = (B, cout, Ho, Wo) if out_nchw else (B, Ho, Wo, cout)
        out = torch.empty(shape, dtype=torch.float32, device=src0.device)
    d = ConvDesc()
    d.src0, d.src1, d.weight = _p(_f32c(src0, "src0")), _p(src1), _p(_f32c(weight, "weight"))
    d.bias, d.badd, d.res = _p(bias), _p(badd), _p(res)
    d.gn_scale, d.gn_shift = (None, None) if gn is None else (_p(gn[0]), _p(gn[1]))
    d.out = _p(out)
    d.B, d.Hin, d.Win, d.C0, d.C1, d.Cout = B, Hin, Win, C0, C1, cout
    d.ksize, d.stride, d.pad, d.Ho, d.Wo = ksize, stride, pad, Ho, Wo
    d.ups, d.gn_silu, d.out_nchw = int(ups), int(gn_silu), int(out_nchw)
    d.badd_stride, d.tile, d.res_ups = badd_stride, tile, int(res_ups)
    d.flags = UPS_SUBPIXEL if ups_subpixel else (1 if (one_tile or FORCE_ONE_TILE) else 0)
    if skip is not None:
        # fused 1x1 shortcut (the caller has checked `conv_fuses_skip`): filled BEFORE any support query; its weight
        # pointer follows below, once the kernel family is known
        s0, s1 = tensor_of(skip[0]), tensor_of(skip[1])
        d.skip0, d.skip1 = _p(s0), _p(s1)
        d.SC0, d.SC1 = s0.shape[3], (0 if s1 is None else s1.shape[3])
    L = _lib.lib()
    if ups_subpixel and (not ups or weight_s16 is None or weight_f16 is not None or skip is not None
                         or L.ddnm_conv3x3_s16_ups_subpixel_supported(ctypes.byref(d)) != 1):
        raise ValueError(f"ups_subpixel: launch (B={B}, {Hs}x{Ws} -> {Ho}x{Wo}, Cin={C0 + C1}, Cout={cout}) does not "
                         "qualify (ddnm_conv3x3_s16_ups_subpixel_supported)")
    fam, d, gn = _select_conv_family(L, d, src0, src1, gn, gn_silu, weight_s16, weight_f16)
    if fam.pack == "s16":
        d.weight = weight_s16[0].data_ptr()
        d.acc_scale = 1.0 / (float(weight_s16[1]) * _s16_act_scale())
        if gn is None or skip is not None:
            # operand-range guard: a raw operand may have ANY fp32 magnitude; the kernel scales it per image by a power
            # of two derived on the device from this bound (include/ddnm_hip.h::ddnm_conv_desc::amax_in)
            if raw_amax is None:
                raw_amax = amax_bound(*skip) if skip is not None else amax_bound(a_src0, a_src1)
            d.amax_in = raw_amax.data_ptr()
    elif fam.pack == "f16":
        d.weight = weight_f16.data_ptr()
    if skip is not None:
        if fam.pack == "f16" and skip_weight_f16 is None:
            raise ValueError("fp16 launch with a fused shortcut needs skip_weight_f16")
        d.skip_weight = _p(skip_weight_f16 if fam.pack == "f16" else weight_s16[2] if fam.pack == "s16" else skip_weight)

    def record():
        flops = 2.0 * B * Ho * Wo * cout * (ksize * ksize * (C0 + C1) + d.SC0 + d.SC1)      # + fused 1x1 shortcut
        if ups_subpixel:
            flops *= 16.0 / 36.0                       # 4 of 9 taps per output pixel: the FLOPs the launch issues
        return fam.variant(L, d), flops, (B, Ho, Wo, C0 + C1, cout, ksize, stride, int(ups), d.SC0 + d.SC1, gn is not None,
                                          res is not None)
    act = _launch_conv(L, fam, d, out, emit_stats and not _NO_FUSED_GN, record)
    if _S16_CHECK and fam.pack == "s16" and not bool(torch.isfinite(out).all()):
        raise FloatingPointError(f"split-fp16 launch produced non-finite values (B={B}, {Hin}x{Win}, Cin={C0 + C1}, "
                                 f"Cout={cout}, k={ksize}): an operand left fp16 range; DDNM_CONV_F32=mfma32 selects the "
                                 "all-fp32 engine")
    return act if emit_stats else out


# ----------------------------------------------------------------------------- fp16-activation path (csrc/conv16.hip)
CONV16_COUT_ALIGN = 256


def _f16c(t, name):
    if t.dtype != torch.float16 or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"{name}: expected a contiguous float16 device tensor, got {t.dtype} "
                         f"contiguous={t.is_contiguous()} device={t.device}")
    return t


def pack_conv_weight16(w, cin_pad=None):
    """OIHW (or OI for Conv1d k=1 / Linear-like) -> fp16 (O, ky, kx, I) with Cout padded to 256, Cin to `cin_pad`."""
    if w.dim() == 2:
        w = w[:, :, None, None]
    cout, cin, kh, kw = w.shape
    cin_pad = cin if cin_pad is None else cin_pad
    cout_pad = (cout + CONV16_COUT_ALIGN - 1) // CONV16_COUT_ALIGN * CONV16_COUT_ALIGN
    out = torch.zeros(cout_pad, kh * kw, cin_pad, dtype=torch.float16, device=w.device)
    out[:cout, :, :cin] = w.float().permute(0, 2, 3, 1).reshape(cout, kh * kw, cin).to(torch.float16)
    return out.contiguous()


def _conv16_desc(src, weight, cout, ksize, *, H, W, ups=False, skip=None, skip_weight=None, bias=None, res=None,
                 res_ups=False, src1=None, gn=None, gn_silu=True):
    B = src.shape[0]
    d = Conv16Desc()
    d.src, d.weight, d.bias, d.res = _p(_f16c(src, "src")), _p(_f16c(weight, "weight")), _p(bias), _p(res)
    cin = src.shape[-1]
    if src1 is not None:
        d.src1, d.C0 = _p(_f16c(src1, "src1")), cin
        cin += src1.shape[-1]
    if gn is not None:
        d.gn_scale, d.gn_shift, d.gn_silu = _p(gn[0]), _p(gn[1]), int(gn_silu)
    d.B, d.H, d.W, d.Cin, d.Cout, d.ksize = B, H, W, cin, cout, ksize
    d.ups, d.res_ups = int(ups), int(res_ups)
    if skip is not None:
        s0, s1 = skip
        d.skip0, d.skip1, d.skip_weight = _p(_f16c(s0, "skip0")), _p(s1), _p(_f16c(skip_weight, "skip_weight"))
        d.SC0, d.SC1 = s0.shape[-1], (0 if s1 is None else s1.shape[-1])
    return d


def conv16_supported(B, H, W, cin, cout, ksize, ups=False):
    d = Conv16Desc()
    d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.ups = B, H, W, cin, cout, ksize, int(ups)
    return _lib.lib().ddnm_conv16_supported(ctypes.byref(d)) == 1


def conv16(src, weight, cout, ksize, *, src1=None, gn=None, gn_silu=True, bias=None, res=None, res_ups=False, ups=False,
           skip=None, skip_weight=None, emit_stats=True, out=None, fin=None):
    """fp16 NHWC convolution of the `use_fp16` torso (include/ddnm_hip.h::ddnm_conv16_desc).  The operand is
    concat_c(src, src1) [B,Hs,Ws,Cin] fp16: raw with `gn` = (scale, shift) (3x3 only: GroupNorm affine + swish fused,
    applied in LDS) or already activated.  Returns an `Act` whose tensor is fp16 [B,H,W,cout] and whose GroupNorm
    partials (when the launch can emit them) describe exactly those rounded values."""
    src, src1, res = tensor_of(src), tensor_of(src1), tensor_of(res)
    B, Hs, Ws, _ = src.shape
    H, W = (2 * Hs, 2 * Ws) if ups else (Hs, Ws)
    if skip is not None:
        skip = tuple(tensor_of(s) for s in skip)
    d = _conv16_desc(src, weight, cout, ksize, H=H, W=W, ups=ups, skip=skip, skip_weight=skip_weight, bias=bias, res=res,
                     res_ups=res_ups, src1=src1, gn=gn, gn_silu=gn_silu)
    L = _lib.lib()
    if out is None:
        out = torch.empty(B, H, W, cout, dtype=torch.float16, device=src.device)
    d.out = _p(_f16c(out, "out"))
    fused_fin = False
    if fin is not None and emit_stats:
        # fin = (name, gamma, beta, film or None, film_stride, eps, workspace): the GroupNorm that will consume `out`
        name, gamma, beta, film, film_stride, eps, ws = fin
        d.fin_gamma, d.fin_beta, d.fin_film = _p(gamma), _p(beta), _p(film)
        d.fin_scale, d.fin_shift = _p(ws.scale), _p(ws.shift)
        d.fin_eps, d.fin_film_stride, d.fin_groups = eps, film_stride, 32
        fused_fin = ws.scale.numel() >= B * cout and L.ddnm_conv16_fuses_fin(ctypes.byref(d)) == 1
        if not fused_fin:
            d.fin_gamma = None
        else:
            ws.generation += 1
    fam = CONV_FAMILIES["conv16"]
    act = _launch_conv(L, fam, d, out, emit_stats,
                       lambda: (fam.variant(L, d), 2.0 * B * H * W * cout * (ksize * ksize * d.Cin + d.SC0 + d.SC1),
                                (B, H, W, d.Cin, cout, ksize, 1, int(ups), d.SC0 + d.SC1, False, res is not None)))
    if fused_fin:
        act.gn = (fin[6].scale, fin[6].shift, fin[0], fin[6], fin[6].generation)
    return act


def conv16_out(src, weight, cout, bias=None, gn=None, gn_silu=True):
    """The network's output convolution on the fp16 path: 3x3, cout <= 32, fp32 NCHW result (unet.py:627-631,664);
    `gn` = (scale, shift) fuses the GroupNorm affine + swish of `out.0/out.1` into its loader like `conv16`."""
    src = tensor_of(src)
    B, H, W, _ = src.shape
    d = _conv16_desc(src, weight, cout, 3, H=H, W=W, bias=bias, gn=gn, gn_silu=gn_silu)
    d.out_nchw_f32 = 1
    out = torch.empty(B, cout, H, W, dtype=torch.float32, device=src.device)
    d.out = out.data_ptr()
    L, fam = _lib.lib(), CONV_FAMILIES["conv16_out"]
    _launch_conv(L, fam, d, out, False, lambda: (fam.variant(L, d), 2.0 * B * H * W * cout * 9 * d.Cin,
                                                 (B, H, W, d.Cin, cout, 3, 1, 0, 0, False, False)))
    return out


def gn_apply16(src0, src1, gn, silu, pool=False):
    """fp16 operand of the next convolution: act(concat_c(src0, src1) * scale + shift), optionally 2x2 average-pooled
    (gn=None: plain concat / pooling of the raw tensors)."""
    src0, src1 = tensor_of(src0), tensor_of(src1)
    B, H, W, C0 = src0.shape
    C1 = 0 if src1 is None else src1.shape[3]
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    out = torch.empty(B, Ho, Wo, C0 + C1, dtype=torch.float16, device=src0.device)
    sc, sh = (None, None) if gn is None else gn
    check(_lib.lib().ddnm_gn_apply_h16(_p(_f16c(src0, "src0")), _p(src1), _p(sc), _p(sh), _p(out), B, H, W, C0, C1,
                                       int(silu), int(pool), _stream()), "ddnm_gn_apply_h16")
    return out


def im2col16(src0, src1, gn, silu):
    src0, src1 = tensor_of(src0), tensor_of(src1)
    B, H, W, C0 = src0.shape
    C1 = 0 if src1 is None else src1.shape[3]
    out = torch.empty(B, H, W, 9 * (C0 + C1), dtype=torch.float16, device=src0.device)
    sc, sh = (None, None) if gn is None else gn
    check(_lib.lib().ddnm_im2col3x3_h16(_p(_f16c(src0, "src0")), _p(src1), _p(sc), _p(sh), _p(out), B, H, W, C0, C1,
                                        int(silu), _stream()), "ddnm_im2col3x3_h16")
    return out


def nchw_to_nhwc16(x, cpad):
    B, C, H, W = x.shape
    out = torch.empty(B, H, W, cpad, dtype=torch.float16, device=x.device)
    check(_lib.lib().ddnm_nchw_to_nhwc_h16(_p(_f32c(x, "x")), _p(out), B, C, H * W, cpad, _stream()),
          "ddnm_nchw_to_nhwc_h16")
    return out


def gn_stats16(t):
    """GroupNorm partials of an fp16 NHWC tensor whose producer could not emit them."""
    B, H, W, C = t.shape
    hw = H * W
    tiles = 1
    for cand in (64, 32, 16, 8, 4, 2):
        if hw % cand == 0 and hw // cand >= 4:
            tiles = cand
            break
    stats = torch.empty(B * tiles * C * 2, dtype=torch.float32, device=t.device)
    check(_lib.lib().ddnm_gn_stats_h16(_p(_f16c(t, "t")), _p(stats), B, hw, C, tiles, _stream()), "ddnm_gn_stats_h16")
    return Act(t, stats, tiles)


def attn16(qkv, C, lse=None):
    """Fused multi-head attention (head dim 64) over the legacy-ordered fp16 qkv tensor [B,H,W,3C] -> [B,H,W,C].
    `lse` (fp32 [B, C/64, H*W], optional) receives the per-query base-2 log-sum-exp the backward pass needs."""
    B, H, W, C3 = qkv.shape
    assert C3 == 3 * C
    out = torch.empty(B, H, W, C, dtype=torch.float16, device=qkv.device)
    if lse is None:
        check(_lib.lib().ddnm_attn16_d64(_p(_f16c(qkv, "qkv")), _p(out), B, H * W, C, _stream()), "ddnm_attn16_d64")
    else:
        if lse.dtype != torch.float32 or lse.numel() != B * (C // 64) * H * W or not lse.is_contiguous():
            raise ValueError("attn16: lse must be a contiguous float32 tensor [B, C/64, H*W]")
        check(_lib.lib().ddnm_attn16_d64_lse(_p(_f16c(qkv, "qkv")), _p(out), _p(lse), B, H * W, C, _stream()),
              "ddnm_attn16_d64_lse")
    return out


def attn16_bwd(qkv, o, dO, lse):
    """Input gradient of `attn16`: dqkv fp16 [B,H,W,3C] from qkv, the forward output o, its gradient dO and lse; the
    probabilities are recomputed tile by tile (csrc/attn16_bwd.hip), nothing of size [T][T] is stored."""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    dqkv = torch.empty_like(qkv)
    dsum = torch.empty_like(lse)
    check(_lib.lib().ddnm_attn16_d64_bwd(_p(_f16c(qkv, "qkv")), _p(_f16c(o, "o")), _p(_f16c(dO, "dO")), _p(lse), _p(dsum),
                                         _p(dqkv), B, H * W, C, _stream()), "ddnm_attn16_d64_bwd")
    return dqkv


# ----------------------------------------------------------------------------- GroupNorm
class GroupNormWorkspace:
    """Scratch shared by every GroupNorm of a forward pass (stream order makes reuse safe)."""

    def __init__(self, device, max_batch, max_channels, max_partial_doubles):
        self.partial = torch.empty(max_partial_doubles, dtype=torch.float64, device=device)
        self.scale = torch.empty(max_batch * max_channels, dtype=torch.float32, device=device)
        self.shift = torch.empty(max_batch * max_channels, dtype=torch.float32, device=device)
        # bumped by every launch that writes scale / shift (finalize kernels, the fused `fin` pass of conv16): a consumer
        # that was handed "already finalized" buffers checks that nobody has overwritten them since (Act.gn)
        self.generation = 0


def gn_nchunk(hw, c):
    n = _lib.lib().ddnm_gn_nchunk(hw, c)
    if n <= 0:
        check(n, "ddnm_gn_nchunk")
    return n


def group_norm_affine(src0, src1, gamma, beta, eps, ws, groups=32, film=None, film_stride=0, keep=None, want_amax=False):
    """(scale, shift) [B][C] such that GN(x)[b,:,c] = x*scale + shift; no normalised tensor is written.
    `film` (rows [s | t], row stride film_stride) folds the FiLM modulation GN(x)*(1+s)+t into the affine.
    src0 / src1 may be tensors or `Act`s; when every source carries conv-epilogue partials the statistics
    come from those (no pass over the activation), otherwise from the stand-alone statistics kernel."""
    # keep: optional dict that receives private copies of (scale, shift, mean_rstd) for a backward pass
    # want_amax: also return the [B][AMAX_N] operand bound of concat(src0, src1) (a third value), emitted by the same
    # finalize launch when the statistics come from tile partials (groups == AMAX_N), by amax_bound otherwise
    a0 = src0 if isinstance(src0, Act) else Act(src0)
    a1 = None if src1 is None else (src1 if isinstance(src1, Act) else Act(src1))
    if a0.t.dtype == torch.float16:          # fp16-activation path: statistics always come as tile partials
        if a0.stats is None:
            a0 = gn_stats16(a0.t)
        if a1 is not None and a1.stats is None:
            a1 = gn_stats16(a1.t)
    src0, src1 = a0.t, (None if a1 is None else a1.t)
    B, H, W, C0 = src0.shape
    C1 = 0 if src1 is None else src1.shape[3]
    C, HW = C0 + C1, H * W
    sc_buf, sh_buf, mr = ws.scale, ws.shift, None
    if keep is None:
        ws.generation += 1
    if keep is not None:
        sc_buf = torch.empty(B * C, dtype=torch.float32, device=src0.device)
        sh_buf = torch.empty(B * C, dtype=torch.float32, device=src0.device)
        mr = torch.empty(B * groups * 2, dtype=torch.float32, device=src0.device)
        keep.update(scale=sc_buf, shift=sh_buf, mean_rstd=mr, groups=groups)
    if a0.stats is not None and (a1 is None or a1.stats is not None):
        if sc_buf.numel() < B * C:
            raise ValueError("GroupNorm workspace too small")
        amax = None
        if want_amax and groups == AMAX_N:
            amax = torch.empty(B * AMAX_N, dtype=torch.float32, device=src0.device)
        check(_lib.lib().ddnm_gn_finalize_tiles_amax_f32(_p(a0.stats), a0.tiles, C0, None if a1 is None else _p(a1.stats),
                                                         0 if a1 is None else a1.tiles, C1, _p(gamma), _p(beta), B, HW,
                                                         groups, eps, _p(sc_buf), _p(sh_buf), _p(film), film_stride,
                                                         _p(mr), _p(amax), _stream()), "ddnm_gn_finalize_tiles_amax_f32")
        if want_amax:
            return sc_buf, sh_buf, (amax if amax is not None else amax_bound(a0, a1))
        return sc_buf, sh_buf
    nchunk = gn_nchunk(HW, C)
    need = B * nchunk * groups * 2
    if ws.partial.numel() < need or sc_buf.numel() < B * C:
        raise ValueError("GroupNorm workspace too small")
    L = _lib.lib()
    check(L.ddnm_gn_stats_f32(_p(src0), _p(src1), B, HW, C0, C1, groups, _p(ws.partial), nchunk, _stream()),
          "ddnm_gn_stats_f32")
    check(L.ddnm_gn_finalize_f32(_p(ws.partial), nchunk, _p(gamma), _p(beta), B, HW, C, groups, eps, _p(sc_buf),
                                 _p(sh_buf), _p(film), film_stride, _p(mr), _stream()), "ddnm_gn_finalize_f32")
    if want_amax:
        return sc_buf, sh_buf, amax_bound(a0, a1)
    return sc_buf, sh_buf


# ----------------------------------------------------------------------------- GEMM / softmax / linear
def bgemm(A, Bm, C, M, N, K, *, lda, ldb, ldc, transb, batch=1, inner=1, sA=(0, 0), sB=(0, 0), sC=(0, 0),
          D=None, ldd=0, sD=(0, 0), alpha=1.0, beta=0.0, transa=False):
    d = GemmDesc()
    d.A, d.Bm, d.D, d.C = _p(A), _p(Bm), _p(D), _p(C)
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.ldd = M, N, K, lda, ldb, ldc, ldd
    d.transb, d.batch, d.inner = int(transb), batch, inner
    d.sAo, d.sAi, d.sBo, d.sBi, d.sCo, d.sCi, d.sDo, d.sDi = sA[0], sA[1], sB[0], sB[1], sC[0], sC[1], sD[0], sD[1]
    d.alpha, d.beta, d.transa = alpha, beta, int(transa)
    # (timed too: FLOP accounting of an instrumented pass -- bench.py counts the classifier's work)
    _launch(_lib.lib().ddnm_bgemm_f32, d, "ddnm_bgemm_f32",
            lambda: ("bgemm_f32", 2.0 * M * N * K * batch, (batch, M, N, K, 0, 1, 1, 0, 0, False, False)))
    return C


def attn_fused_supported(T, C):
    return _lib.lib().ddnm_attn_fused_supported(int(T), int(C)) == 1


def attn_fused(qkv, B, T, C, s_qk, s_v, scale, out=None):
    """Single-head self-attention over qkv [B, T, 3C] fp32 (q | k | v per token) in ONE launch (csrc/attn_d512.hip): the two
    torch.bmm and the softmax of guided_diffusion/models.py:171-185.  s_qk / s_v: power-of-two operand scales (see
    models.Model: a static bound per checkpoint)."""
    if out is None:
        out = torch.empty(B, T, C, dtype=torch.float32, device=qkv.device)
    check(_lib.lib().ddnm_attn_fused_f32(_p(_f32c(qkv, "qkv")), _p(out), B, T, C, float(s_qk), float(s_v), float(scale), _stream()),
          "ddnm_attn_fused_f32")
    return out


def softmax_rows_(x, rows, n, ld, scale):
    check(_lib.lib().ddnm_softmax_rows_f32(_p(x), rows, n, ld, scale, _stream()), "ddnm_softmax_rows_f32")
    return x


def linear(x, W, bias, silu_in=False, out=None):
    B, K = x.shape
    N = W.shape[0]
    if out is None:
        out = torch.empty(B, N, dtype=torch.float32, device=x.device)
    check(_lib.lib().ddnm_linear_f32(_p(x), _p(W), _p(bias), _p(out), B, K, N, int(silu_in), _stream()),
          "ddnm_linear_f32")
    return out


def timestep_embedding(t, freq, order):
    B, half = t.shape[0], freq.shape[0]
    emb = torch.empty(B, 2 * half, dtype=torch.float32, device=t.device)
    check(_lib.lib().ddnm_timestep_embedding_f32(_p(t), _p(freq), _p(emb), B, half, order, _stream()),
          "ddnm_timestep_embedding_f32")
    return emb


def avgpool2_nhwc(x, gn=None, silu=False):
    B, H, W, C = x.shape
    out = torch.empty(B, H // 2, W // 2, C, dtype=torch.float32, device=x.device)
    sc, sh = (None, None) if gn is None else gn
    check(_lib.lib().ddnm_avgpool2_nhwc_f32(_p(_f32c(x, "x")), _p(sc), _p(sh), int(silu), _p(out), B, H // 2, W // 2, C,
                                            _stream()), "ddnm_avgpool2_nhwc_f32")
    return out


def embedding_add_(emb, table, idx):
    idx = idx.to(device=emb.device, dtype=torch.int64).contiguous()
    if idx.numel() != emb.shape[0]:
        raise ValueError("embedding_add_: one index per row expected")
    check(_lib.lib().ddnm_embedding_add_f32(_p(emb), _p(table), _p(idx), emb.shape[0], emb.shape[1], table.shape[0],
                                            _stream()), "ddnm_embedding_add_f32")
    return emb


def nchw_to_nhwc_pad(x, cpad):
    B, C, H, W = x.shape
    out = torch.empty(B, H, W, cpad, dtype=torch.float32, device=x.device)
    check(_lib.lib().ddnm_nchw_to_nhwc_pad_f32(_p(_f32c(x, "x")), _p(out), B, C, H * W, cpad, _stream()),
          "ddnm_nchw_to_nhwc_pad_f32")
    return out


def nchw_im2col3x3_pad(x, cpad):
    """[B,C,H,W] -> NHWC [B,H,W,cpad] holding the 9*C taps of the 3x3 / pad 1 input convolution (C = 3: one K chunk)."""
    B, C, H, W = x.shape
    out = torch.empty(B, H, W, cpad, dtype=torch.float32, device=x.device)
    check(_lib.lib().ddnm_nchw_im2col3x3_pad_f32(_p(_f32c(x, "x")), _p(out), B, C, H, W, cpad, _stream()),
          "ddnm_nchw_im2col3x3_pad_f32")
    return out


def pack_conv_in_weight_im2col(w, cpad):
    """conv_in weights [Cout, C, 3, 3] -> the 1x1 form over the im2col'ed input: [Cout_pad][1][cpad], entry
    (ky*3+kx)*C + c (the order ddnm_nchw_im2col3x3_pad_f32 writes)."""
    cout, cin = w.shape[0], w.shape[1]
    flat = w.float().permute(0, 2, 3, 1).reshape(cout, 9 * cin)
    cout_pad = (cout + CONV_COUT_ALIGN - 1) // CONV_COUT_ALIGN * CONV_COUT_ALIGN
    out = torch.zeros(cout_pad, 1, cpad, dtype=torch.float32, device=w.device)
    out[:cout, 0, :9 * cin] = flat
    return out.contiguous()


# ----------------------------------------------------------------------------- sampler step
class PhiloxNoise:
    """In-kernel noise of one sampling run (include/ddnm_hip.h::ddnm_step_scalars::rng_*): instead of a tensor, the step
    kernels get (seed, loop iteration, global index of the batch's first image) and draw N(0, I) themselves -- Philox4x32-10
    + Box-Muller, counter = (element / 4, iteration, image), so the values do not depend on batch size or rank count.
    `tensor(k, B, shape)` materialises the SAME values (x_T: iteration 0xFFFFFFFF; time-travel re-noise; DDNM+)."""
    XT_ITER = 0xFFFFFFFF

    def __init__(self, seed, image_base=0):
        self.seed_lo, self.seed_hi = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
        self.image_base = int(image_base)

    def stamp(self, s, k):
        s.rng_on, s.rng_seed_lo, s.rng_seed_hi, s.rng_iter, s.rng_image_base = 1, self.seed_lo, self.seed_hi, int(k), self.image_base
        return s

    def kernel_arg(self, s, k):
        """What a step kernel takes as `noise` for loop iteration k: None, with the draw stamped into `s`."""
        self.stamp(s, k)

    def tensor(self, k, like):
        B = like.shape[0]
        out = torch.empty(like.shape, dtype=torch.float32, device=like.device)
        check(_lib.lib().ddnm_randn_philox_f32(_p(out), B, out.numel() // B, self.seed_lo, self.seed_hi, int(k) & 0xFFFFFFFF,
                                               self.image_base, _stream()), "ddnm_randn_philox_f32")
        return out


class KeyedPhiloxNoise:
    """Per-image in-kernel noise: image b of the batch draws with its own 64-bit key `keys[b]` and image counter
    `image_ctrs[b]` (include/ddnm_hip.h::ddnm_randn_philox_keyed_f32), so that images from different loader batches --
    different seeds -- share one sampler call and each still gets the noise it gets when restored alone.  The step
    kernels' keyed entry points read the table [B][4] uint32 {key_lo, key_hi, image_ctr, 0}; `tensor(k, like)`
    materialises the same values for any per-image length (also lengths that are not a multiple of 4)."""
    XT_ITER = PhiloxNoise.XT_ITER

    def __init__(self, keys, image_ctrs):
        keys, image_ctrs = [int(k) for k in keys], [int(c) for c in image_ctrs]
        if not keys or len(keys) != len(image_ctrs):
            raise ValueError(f"KeyedPhiloxNoise: {len(keys)} keys for {len(image_ctrs)} image counters")
        self.keys, self.image_ctrs = keys, image_ctrs
        rows = [[k & 0xFFFFFFFF, (k >> 32) & 0xFFFFFFFF, c & 0xFFFFFFFF, 0] for k, c in zip(keys, image_ctrs)]
        # uint32 bit patterns in an int32 tensor (the kernels only read the table)
        self._host = torch.from_numpy(np.array(rows, dtype=np.uint32).view(np.int32))
        self._dev = {}

    @classmethod
    def from_sources(cls, pairs):
        """[(PhiloxNoise, image index within that source's batch), ...] -> one key row per pair: the fused batch of the
        per-loader-batch sources, each image keeping its (seed, image_base + index) draw."""
        pairs = list(pairs)
        return cls([(p.seed_hi << 32) | p.seed_lo for p, _ in pairs], [p.image_base + int(i) for p, i in pairs])

    concat = from_sources

    def __len__(self):
        return len(self.keys)

    def table(self, device):
        """The device key table (one host-to-device copy per device, kept for the life of the object)."""
        device = torch.device(device)
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = self._host.to(device)
        return t

    def stamp(self, s, k):
        s.rng_on, s.rng_iter = 1, int(k)
        return s

    def kernel_arg(self, s, k):
        """What a step kernel takes as `noise` for loop iteration k: this object (the key table), `s` stamped."""
        self.stamp(s, k)
        return self

    def _check_batch(self, B):
        if B != len(self.keys):
            raise ValueError(f"KeyedPhiloxNoise holds {len(self.keys)} image keys, the batch has {B} images")

    def tensor(self, k, like):
        B = like.shape[0]
        self._check_batch(B)
        out = torch.empty(like.shape, dtype=torch.float32, device=like.device)
        check(_lib.lib().ddnm_randn_philox_keyed_f32(_p(out), B, out.numel() // B, _p(self.table(like.device)),
                                                     int(k) & 0xFFFFFFFF, _stream()), "ddnm_randn_philox_keyed_f32")
        return out


def step_noise_args(name, noise, like):
    """(entry point, noise argument) of step kernel `name` (e.g. "ddnm_step_color_f32") for `noise`: a tensor or None
    (the unkeyed entry point, in-kernel draw per ddnm_step_scalars::rng_*), or a KeyedPhiloxNoise (the `_keyed_f32`
    entry point with the device key table)."""
    if isinstance(noise, KeyedPhiloxNoise):
        noise._check_batch(like.shape[0])
        return name[:-len("_f32")] + "_keyed_f32", _p(noise.table(like.device))
    return name, _p(noise)


def call(name, *args):
    """Checked call of the library's entry point `name` on the current stream (its last parameter)."""
    check(getattr(_lib.lib(), name)(*args, _stream()), name)


def step_call(name, xt, et, noise, y, *between_and_s):
    """Checked launch of a fused sampler step `name(xt, et, et batch stride, noise, y, *between, &s, stream)`: validates
    et's layout, picks the keyed or unkeyed entry point for `noise` (step_noise_args); the last argument is the StepScalars."""
    *between, s = between_and_s
    ep, es = _et_args(et)
    fn, nz = step_noise_args(name, noise, xt)
    check(getattr(_lib.lib(), fn)(_p(xt), ep, es, nz, _p(y), *between, ctypes.byref(s), _stream()), fn)


def step_scalars(at, at_next, eta, lam=1.0, gamma=1.0):
    """Host-side scalar terms of one reverse step, evaluated in fp32 exactly like the reference
    (functions/svd_ddnm.py:57,63-65): `at`, `at_next` are fp32 torch scalars (alpha-bar)."""
    s = StepScalars()
    at = at.float()
    at_next = at_next.float()
    s.sqrt_1m_at = float((1 - at).sqrt())
    s.sqrt_at = float(at.sqrt())
    s.sqrt_at_next = float(at_next.sqrt())
    c1 = (1 - at_next).sqrt() * eta
    c2 = (1 - at_next).sqrt() * ((1 - eta ** 2) ** 0.5)
    if gamma != 1.0:
        c1, c2 = gamma * c1, gamma * c2
    s.c1, s.c2, s.lam = float(c1), float(c2), float(lam)
    return s


def _et_args(et):
    """et may be a [B,3,H,W] view of a [B,6,H,W] learn_sigma output (svd_ddnm.py:54-55)."""
    if et.dim() != 4 or et.stride(3) != 1 or et.stride(2) != et.shape[3] or et.stride(1) != et.shape[2] * et.shape[3]:
        raise ValueError("et must be channel-contiguous NCHW")
    return et.data_ptr(), et.stride(0)


def step_x0(xt, et, s, out=None):
    B = xt.shape[0]
    chw = xt.numel() // B
    out = torch.empty_like(xt) if out is None else out
    ep, es = _et_args(et)
    check(_lib.lib().ddnm_step_x0_f32(_p(xt), ep, es, _p(out), B, chw, ctypes.byref(s), _stream()), "ddnm_step_x0_f32")
    return out


def step_combine(x0, proj, apy, noise, et, s, out=None):
    B = x0.shape[0]
    chw = x0.numel() // B
    out = torch.empty_like(x0) if out is None else out
    ep, es = _et_args(et)
    fn, nz = step_noise_args("ddnm_step_combine_f32", noise, x0)
    check(getattr(_lib.lib(), fn)(_p(x0), _p(proj), _p(apy), nz, ep, es, _p(out), B, chw, ctypes.byref(s), _stream()), fn)
    return out


def step_plus_spectral(xt_hat, et_hat, y_hat, gains, gains_cstride, noise, s, sigma_y, sigma_t, eta, out=None):
    """The fused DDNM+ step in the spectral planes (include/ddnm_hip.h::ddnm_step_plus_spectral_f32): `xt_hat`, `et_hat`,
    `y_hat` are [B, C, d, d]; `gains` the thresholded gain table, [C][d*d] with channel stride `gains_cstride` (0: one
    plane for all channels); `noise` a tensor, None (in-kernel draw per ddnm_step_scalars::rng_*) or a KeyedPhiloxNoise.
    `out` may be `xt_hat`."""
    B, C = xt_hat.shape[0], xt_hat.shape[1]
    plane = xt_hat.numel() // (B * C)
    out = torch.empty_like(xt_hat) if out is None else out
    for name, t in (("xt_hat", xt_hat), ("et_hat", et_hat), ("y_hat", y_hat), ("out", out)):
        if _f32c(t, name).numel() != B * C * plane:
            raise ValueError(f"step_plus_spectral: {name} has {t.numel()} entries, expected {B * C * plane}")
    if _f32c(gains, "gains").numel() < (C - 1) * gains_cstride + plane:
        raise ValueError("step_plus_spectral: the gain table is shorter than (C - 1) * gains_cstride + plane")
    if noise is not None and not isinstance(noise, KeyedPhiloxNoise) and _f32c(noise, "noise").numel() != B * C * plane:
        raise ValueError("step_plus_spectral: the noise tensor must have one entry per spectral entry")
    fn, nz = step_noise_args("ddnm_step_plus_spectral_f32", noise, xt_hat)
    check(getattr(_lib.lib(), fn)(_p(xt_hat), _p(et_hat), _p(y_hat), _p(gains), gains_cstride, nz, _p(out), B, C, plane,
                                  float(sigma_y), float(sigma_t), float(eta), ctypes.byref(s), _stream()), fn)
    return out


def step_plus_cs_pre(xt, et, noise, aty, s, coef, x0_out, xt_next, w, ps):
    """First kernel of the fused DDNM+ step of block-based CS (include/ddnm_hip.h::ddnm_step_plus_cs_pre_f32): `xt`,
    `aty` (= A^+ y), `x0_out`, `xt_next` are [B, C, D, D], `et` the same or the [:, :3] view of a 6-channel output, `w` the
    patch matrix [B*C*(D/ps)^2, ps*ps]; `coef` = svd_operators.cs_plus_coefficients(...); `noise` a tensor, None
    (in-kernel draw per ddnm_step_scalars::rng_*) or a KeyedPhiloxNoise."""
    if xt.dim() != 4 or xt.shape[2] != xt.shape[3] or tuple(et.shape) != tuple(xt.shape):
        raise ValueError(f"step_plus_cs_pre: xt / et must be [B, C, D, D], got {tuple(xt.shape)} / {tuple(et.shape)}")
    B, C, D = xt.shape[0], xt.shape[1], xt.shape[3]
    n = B * C * D * D
    for name, t in (("xt", xt), ("aty", aty), ("x0_out", x0_out), ("xt_next", xt_next), ("w", w)):
        if _f32c(t, name).numel() != n:
            raise ValueError(f"step_plus_cs_pre: {name} has {t.numel()} entries, expected {n}")
    if noise is not None and not isinstance(noise, KeyedPhiloxNoise) and _f32c(noise, "noise").numel() != n:
        raise ValueError("step_plus_cs_pre: the noise tensor must have one entry per pixel")
    if et.dtype != torch.float32 or et.stride(0) < C * D * D:
        raise ValueError("step_plus_cs_pre: et must be fp32 with a batch stride of at least C*D*D")
    al, d1n, d2n, dd1, dd2 = (float(v) for v in coef)
    ep, es = _et_args(et)
    fn, nz = step_noise_args("ddnm_step_plus_cs_pre_f32", noise, xt)
    check(getattr(_lib.lib(), fn)(_p(xt), ep, es, nz, _p(aty), _p(x0_out), _p(xt_next), _p(w), B, C, D, int(ps), al, d1n,
                                  d2n, dd1, dd2, ctypes.byref(s), _stream()), fn)


def step_plus_cs_post(P, xt_next, ps):
    """Last kernel of that step (ddnm_step_plus_cs_post_f32): xt_next [B, C, D, D] += the patch matrix `P`
    [B*C*(D/ps)^2, ps*ps] scattered back to image order."""
    if xt_next.dim() != 4 or xt_next.shape[2] != xt_next.shape[3]:
        raise ValueError(f"step_plus_cs_post: xt_next must be [B, C, D, D], got {tuple(xt_next.shape)}")
    B, C, D = xt_next.shape[0], xt_next.shape[1], xt_next.shape[3]
    if _f32c(P, "P").numel() != _f32c(xt_next, "xt_next").numel():
        raise ValueError(f"step_plus_cs_post: P has {P.numel()} entries, expected {xt_next.numel()}")
    check(_lib.lib().ddnm_step_plus_cs_post_f32(_p(P), _p(xt_next), B * C, D, int(ps), _stream()),
          "ddnm_step_plus_cs_post_f32")
    return xt_next


def fill_(t, value=0.0):
    """t[...] = value for a contiguous fp32 tensor (or contiguous slice) through ddnm_fill_f32."""
    if t.numel():
        check(_lib.lib().ddnm_fill_f32(_p(_f32c(t, "t")), t.numel(), float(value), _stream()), "ddnm_fill_f32")
    return t


def renoise(x0, noise, a, b, out=None):
    out = torch.empty_like(x0) if out is None else out
    check(_lib.lib().ddnm_renoise_f32(_p(x0), _p(noise), _p(out), x0.numel(), a, b, _stream()), "ddnm_renoise_f32")
    return out


def finalize_psnr(x, x_orig=None, want_img=True):
    """inverse_data_transform + per-image PSNR (datasets/__init__.py:218-227, diffusion.py:599-602)."""
    B = x.shape[0]
    chw = x.numel() // B
    img = torch.empty_like(x) if want_img else None
    sse = torch.empty(B, dtype=torch.float64, device=x.device) if x_orig is not None else None
    check(_lib.lib().ddnm_finalize_psnr_f32(_p(x), _p(x_orig), _p(img), _p(sse), B, chw, _stream()),
          "ddnm_finalize_psnr_f32")
    psnr = None
    if sse is not None:
        psnr = 10.0 * torch.log10(1.0 / (sse / chw))
    return img, psnr


def ssim(x, x_orig, transform=True):
    """Per-image SSIM of `x` against `x_orig` ([B, C, H, W], any C, H and W >= 11) as a float64 tensor [B]
    (csrc/metrics.hip): transform=True takes the sampler's [-1, 1] tensors exactly as `finalize_psnr` does,
    transform=False takes [0, 1] images."""
    if x.dim() != 4 or x.shape != x_orig.shape:
        raise ValueError(f"ssim: expected two [B, C, H, W] tensors of one shape, got {tuple(x.shape)} and "
                         f"{tuple(x_orig.shape)}")
    B, C, H, W = x.shape
    lib = _lib.lib()
    n = lib.ddnm_ssim_workspace_elems(B, C, H, W)
    if n < 0:
        check(int(n), "ddnm_ssim_workspace_elems")
    work = torch.empty(n, dtype=torch.float64, device=x.device)
    out = torch.empty(B, dtype=torch.float64, device=x.device)
    check(lib.ddnm_ssim_f32(_p(_f32c(x, "x")), _p(_f32c(x_orig, "x_orig")), _p(out), _p(work), n, B, C, H, W,
                            1 if transform else 0, _stream()), "ddnm_ssim_f32")
    return out


SAMPLE_LAYOUTS = ("samples_major", "images_major")


def sample_stats(x, n_images, n_samples, layout="samples_major", x_orig=None):
    """Per-pixel mean and standard deviation over the `n_samples` restorations of each of `n_images` images
    (csrc/metrics.hip::ddnm_sample_stats_f32).  `x` holds n_images * n_samples rows on the sampler's [-1, 1] scale:
    "samples_major" is [sample k][image j] (what a sampler call over K samples returns), "images_major" is
    [image j][sample k] (what rank 0 holds after the gather).  Returns (mean_img, std_img, psnr_mean, std_mean):
    the two [n_images, ...] fp32 images on the [0, 1] scale, the PSNR of mean_img against `x_orig` ([-1, 1] scale; None
    without it) as `finalize_psnr` computes it, and the per-image mean of the standard deviation, both float64
    [n_images]."""
    B, K = int(n_images), int(n_samples)
    if layout not in SAMPLE_LAYOUTS:
        raise ValueError(f"sample_stats: unknown layout {layout!r}; accepted values: {', '.join(SAMPLE_LAYOUTS)}")
    if B < 1 or K < 1:
        raise ValueError(f"sample_stats: need at least one image and one sample, got {B} images and {K} samples")
    if x.dim() < 2 or x.shape[0] != B * K:
        raise ValueError(f"sample_stats: x has {x.shape[0] if x.dim() else 0} rows, expected {B} images x {K} samples")
    chw = x.numel() // (B * K)
    if x_orig is not None and (x_orig.shape[0] != B or x_orig.numel() != B * chw):
        raise ValueError(f"sample_stats: x_orig is {tuple(x_orig.shape)}, expected {B} images of {chw} values")
    strides = (chw, B * chw) if layout == "samples_major" else (K * chw, chw)
    lib = _lib.lib()
    n = lib.ddnm_sample_stats_workspace_elems(B, chw)
    if n < 0:
        check(int(n), "ddnm_sample_stats_workspace_elems")
    shape = (B,) + tuple(x.shape[1:])
    mean_img = torch.empty(shape, dtype=torch.float32, device=x.device)
    std_img = torch.empty(shape, dtype=torch.float32, device=x.device)
    work = torch.empty(n, dtype=torch.float64, device=x.device)
    std_mean = torch.empty(B, dtype=torch.float64, device=x.device)
    sse = torch.empty(B, dtype=torch.float64, device=x.device) if x_orig is not None else None
    check(lib.ddnm_sample_stats_f32(_p(_f32c(x, "x")), strides[0], strides[1],
                                    _p(_f32c(x_orig, "x_orig")) if x_orig is not None else None, _p(mean_img),
                                    _p(std_img), _p(sse), _p(std_mean), _p(work), n, B, K, chw, _stream()),
          "ddnm_sample_stats_f32")
    psnr = 10.0 * torch.log10(1.0 / (sse / chw)) if sse is not None else None
    return mean_img, std_img, psnr, std_mean


def consistency(ax, y, counts=None):
    """Per-row norms of the residual `ax - y` of two [B, m] measurement tensors (csrc/metrics.hip::ddnm_consistency_f32):
    returns (l1, sse, maxabs) = (sum |d|, sum d^2, max |d|) over the first `counts[b]` entries of row b (all m without
    `counts`: a length-B sequence or int32 tensor inside [0, m]; a mask bank pads its rows) as float64 / float64 / float32
    tensors [B].  The differences are formed in fp64 (exact) and a row's values do not depend on the batch around it."""
    if not (torch.is_tensor(ax) and torch.is_tensor(y)) or ax.dim() != 2 or ax.shape != y.shape:
        raise ValueError("consistency: expected two [B, m] tensors of one shape, got "
                         f"{tuple(ax.shape) if torch.is_tensor(ax) else type(ax).__name__} and "
                         f"{tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")
    B, m = ax.shape
    if B < 1 or m < 1:
        raise ValueError(f"consistency: need at least one row and one entry, got {B} rows of {m}")
    if counts is not None:
        if torch.is_tensor(counts):
            if counts.dtype != torch.int32 or counts.dim() != 1:
                raise ValueError(f"consistency: counts must be a 1-D int32 tensor, got {counts.dtype} {tuple(counts.shape)}")
            host = counts.cpu().tolist()
        else:
            host = list(counts)
            if any(int(c) != c for c in host):
                raise ValueError(f"consistency: counts must be whole numbers, got {host}")
            host = [int(c) for c in host]
        if len(host) != B:
            raise ValueError(f"consistency: {len(host)} counts for {B} rows")
        if min(host) < 0 or max(host) > m:
            raise ValueError(f"consistency: counts must lie in [0, {m}], got {host}")
        if not (torch.is_tensor(counts) and counts.is_cuda and counts.is_contiguous()):
            counts = torch.tensor(host, dtype=torch.int32).to(ax.device)
    ax, y = _f32c(ax, "ax"), _f32c(y, "y")
    lib = _lib.lib()
    n = lib.ddnm_consistency_workspace_elems(B, m)
    if n < 0:
        check(int(n), "ddnm_consistency_workspace_elems")
    work = torch.empty(n, dtype=torch.float64, device=ax.device)
    l1 = torch.empty(B, dtype=torch.float64, device=ax.device)
    sse = torch.empty(B, dtype=torch.float64, device=ax.device)
    maxabs = torch.empty(B, dtype=torch.float32, device=ax.device)
    check(lib.ddnm_consistency_f32(_p(ax), _p(y), m, _p(counts), _p(l1), _p(sse), _p(maxabs), _p(work), n, B, m,
                                   _stream()), "ddnm_consistency_f32")
    return l1, sse, maxabs
