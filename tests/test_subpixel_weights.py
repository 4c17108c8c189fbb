"""Phase weights of the sub-pixel upsample convolution (ddnm_amd/ops.py::upsample_phase_weights, pack_upsample_conv_weight_s16):
`nearest x2 -> conv3x3(pad 1)` equals four 2x2 convolutions on the low-resolution grid with pre-summed weights.  CPU only."""
import torch
import torch.nn.functional as F

from ddnm_amd import ops

CIN, COUT, H, W = 32, 64, 5, 7           # odd, non-square: all four borders and both parities of both axes


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, CIN, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(COUT, CIN, 3, 3, generator=g, dtype=torch.float64) * 0.05
    return x, w


def _subpixel_conv(x, wp):
    """out[2y + py][2x + px] = sum_ab wp[py][px][a][b] . X[y + py - 1 + a][x + px - 1 + b], zero outside X."""
    B, _, h, w = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_zeros(B, wp.shape[2], 2 * h, 2 * w)
    for py in range(2):
        for px in range(2):
            o = F.conv2d(xp[:, :, py:py + h + 1, px:px + w + 1], wp[py, px])
            out[:, :, py::2, px::2] = o
    return out


def test_phase_weights_reproduce_upsample_then_conv():
    x, w = _inputs()
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    got = _subpixel_conv(x, ops.upsample_phase_weights(w))
    assert got.shape == ref.shape == (2, COUT, 2 * H, 2 * W)
    # fp64 rounding: 9 * CIN products per output, summed in a different order
    tol = 9 * CIN * 2.0 ** -52 * float((F.conv2d(F.interpolate(x.abs(), scale_factor=2, mode="nearest"), w.abs(), padding=1)).max())
    assert float((got - ref).abs().max()) <= tol, (float((got - ref).abs().max()), tol)


def test_packing_reproduces_the_scaled_phase_weights_in_the_specified_row_order():
    _, w = _inputs(1)
    cout = 128                                                       # two 64-channel blocks
    w = torch.cat([w, w.flip(0) * 0.5], 0).float()
    wp = ops.upsample_phase_weights(w)                               # [py][px][O][I][a][b] fp64
    scale = ops.s16_weight_scale(wp)
    assert 2.0 ** 13 <= float(wp.abs().max()) * scale < 2.0 ** 14    # the scale of the SUMMED tensor
    packed = ops.pack_upsample_conv_weight_s16(w, scale)
    assert packed.dtype == torch.float16 and tuple(packed.shape) == (4 * cout, 4, CIN // 32, 2, 32)
    back = (packed[:, :, :, 0].double() + packed[:, :, :, 1].double()).reshape(4 * cout, 4, CIN)     # hi + lo
    for cb in range(cout // 64):
        for py in range(2):
            for px in range(2):
                r0 = ((cb * 2 + py) * 2 + px) * 64
                for a in range(2):
                    for b in range(2):
                        want = wp[py, px, cb * 64:(cb + 1) * 64, :, a, b] * scale
                        got = back[r0:r0 + 64, a * 2 + b]
                        err = (got - want).abs()
                        # 2^-22 relative; below 2^-24 absolute the lo half is a subnormal fp16 number (scale * |Wp| < 2^14)
                        assert bool((err <= want.abs() * 2.0 ** -22 + 2.0 ** -25).all()), (cb, py, px, a, b, float(err.max()))


def test_upsample_weight_s16_uses_the_scale_of_the_summed_tensor():
    w = torch.ones(COUT, CIN, 3, 3)                                  # |Wp| = 4 max|W| at the (a, b) that collect four taps
    packed, scale, skip = ops.upsample_weight_s16(w)
    assert skip is None and scale == ops.s16_weight_scale(w) / 4
    assert float(packed.float().abs().max()) < 2.0 ** 14
