"""The first-generation sampler-step and operator kernels of csrc/ddnm_step.hip (the fused steps step_x0, step_combine,
step_sr4, step_color, step_inpaint shared / per image, step_denoise with their tensor, in-kernel and keyed noise; the
stand-alone operators and DDNM+ building blocks) held BIT FOR BIT to tests/step_model.py: the kernel's expression restated
in numpy float32, one rounding per operation, in the kernel's order.  Cases, inputs, the float64 twins and the planted
faults that show the comparison has teeth are in tests/step_model.py / tests/test_step_model_host.py.

Every output is a view into a NaN-filled buffer with 4096 elements of guard on both sides (both guards must survive, the
output may be NaN only where the model is); read-only operands are followed by 4096 NaN, index tables by entries that point
into those NaN, key tables by rows of another key.  A mismatch names the count and the first indices.  Every fused-step
case runs with its noise as a tensor, as the in-kernel draw and as keyed rows, with et contiguous and as the first half of
a six-channel tensor, with x0 requested and NULL; a keyed launch with different key rows equals B = 1 unkeyed launches
image by image.  xt_next never aliases xt here: the sampler ping-pongs two buffers (svd_ddnm._reverse_loop, `bufs[k & 1]`)
and the kernels declare both __restrict__, so no in-place use is relied on anywhere.

Not bit for bit: finalize_psnr's `sse` (a double accumulated by atomicAdd over 64 workgroups in no fixed order; held to
step_model.sse_bar against the float64 sum of the fp32 squares) and the values of randn_philox (logf / cosf / sinf of the
device library; held to oracle.philox within the 3e-5 of test_gpu_fuse.py, and bit for bit to the B = 1 and keyed draws).

Second trip: GRID_1D caps the grid at 8192 workgroups; one launch per kernel shape class with 8192 * 256 + a few work items
(step_model.SECOND_TRIP, sizes asserted by the host test) makes `i += gridDim.x * 256` and the image index after it run,
on integer-valued data with power-of-two scalars so that a few exact torch device ops give the expected tensor.

Measured on the MI355X (test_zz_record prints these):
  cases     135 (32 fused-step, each with up to 12 launches; 90 operator; 9 finalize_psnr; 4 randn_philox) and 11
            second-trip launches: 175 tests, every bit comparison equal; finalize_psnr's sse at most 0.001 of its bar.
  run time  3.3 s for the file (1.2 s in the tests themselves; the largest, step_x0's second trip, 0.4 s).
  worst |err| / bar of the (bit-equal) result against the float64 twin, per kernel, for information:
            step_x0 0.624, step_combine 0.381, step_sr4 0.611, step_color 0.701, step_inpaint 0.571, step_inpaint_pi 0.653,
            step_denoise 0.722, avgpool 0.232, color_A 0.736, color_pinv 0.971, axpby 0.957, axpby_strided 0.654,
            mask_mix 0.967, mul_planes 0.934, gather_scale 0.974, site_matmul 0.583, site_spectral 0.406, spectral_mix 0.482,
            renoise 0.816, finalize_psnr (img) 0.500; 0 for the pure copies (upsample, inpaint_A/pinv, patchify, fill).
  With `fp contract(off)` taken out of ddnm_step.hip (a scratch build, never committed) 67 of the 175 tests fail, each
  naming the elements, e.g. step_x0_chw4 x0 (et contiguous): "1 of 4 elements differ (0 NaN): {'image': 0, 'channel': 0,
  'y': 1, 'x': 1}: got -1.340490460395813, expected -1.3404903411865234"."""
import ctypes
import functools
import time
import zlib

import numpy as np
import pytest
import torch

from tests import step_model as SM

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 4096

STEP_CASES = [c.name for c in SM.CASES if c.kernel.startswith("step_")]
OP_CASES = [c.name for c in SM.CASES if not c.kernel.startswith("step_") and c.kernel not in ("finalize_psnr", "randn_philox")]
PSNR_CASES = [c.name for c in SM.CASES if c.kernel == "finalize_psnr"]
RANDN_CASES = [c.name for c in SM.CASES if c.kernel == "randn_philox"]

WORST = {}          # kernel -> worst |err| / bar against the float64 twin (printed for the record, never asserted)


_KEEP = []           # operands of the current test: alive until its launches have been taken
_CLOCK = {}


@pytest.fixture(autouse=True)
def _operands_stay_alive():
    _CLOCK.setdefault("t0", time.time())
    yield
    _KEEP.clear()


# ----------------------------------------------------------------------------- buffers
def _p(t):
    return None if t is None else t.data_ptr()


def _out(n, dtype=torch.float32):
    """(buffer, view of n elements between two guards), all NaN."""
    buf = torch.full((int(n) + 2 * GUARD,), NAN, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + int(n)]


def _taken(buf, n, what):
    """The n output elements on the CPU, after both guards were found untouched."""
    torch.cuda.synchronize()
    got = buf.cpu()
    assert bool(torch.isnan(got[:GUARD]).all()), f"{what}: store in front of the output"
    assert bool(torch.isnan(got[GUARD + n:]).all()), f"{what}: store behind the output"
    return got[GUARD:GUARD + n]


def _ro(a, tail=None):
    """Read-only operand on the device followed by 4096 NaN (float) or `tail` (index tables); None stays None."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.reshape(-1))
    fill = NAN if t.dtype.is_floating_point else tail
    buf = torch.full((t.numel() + GUARD,), fill, dtype=t.dtype)
    buf[:t.numel()] = t
    dev = buf.cuda()
    _KEEP.append(dev)
    return dev[:t.numel()].view(a.shape)


def _assert_bits(got, want, what, names):
    """Equality of bits (NaN where and only where the model has NaN) with a report: how many differ, the first indices."""
    got, want = (got.reshape(want.shape) if got.numel() == want.numel() else got).contiguous(), want.contiguous()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    same = (got.view(torch.int32) == want.view(torch.int32)) | (torch.isnan(got) & torch.isnan(want))
    if bool(same.all()):
        return
    idx = (~same).nonzero()
    first = "; ".join(f"{dict(zip(names, i.tolist()))}: got {float(got[tuple(i)])!r}, expected {float(want[tuple(i)])!r}" for i in idx[:6])
    raise AssertionError(f"{what}: {idx.shape[0]} of {got.numel()} elements differ ({int(torch.isnan(got).sum())} NaN): {first}")


def _record(case, got, ref):
    """worst |err| / bar of this output against the float64 twin, kept per kernel."""
    g = got.numpy().astype(np.float64).reshape(ref.v.shape)
    ok = ~np.isnan(ref.v)
    bar = ref.bar()[ok]
    err = np.abs(g[ok] - ref.v[ok])
    ratio = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    WORST[case.kernel] = max(WORST.get(case.kernel, 0.0), ratio)
    return ratio


# ----------------------------------------------------------------------------- fused steps
def _scalars(sc):
    from ddnm_amd._lib import StepScalars
    s = StepScalars()
    s.sqrt_1m_at, s.sqrt_at, s.sqrt_at_next, s.c1, s.c2, s.lam = (float(v) for v in (sc.s1, sc.s2, sc.a, sc.c1, sc.c2, sc.lam))
    return s


def _seed(case):
    lo, hi, it, base = SM.noise_key(case)
    return (hi << 32) | lo, it, base


def _keyed(rows):
    """KeyedPhiloxNoise of [(seed, image counter)] whose device table is followed by rows of another key."""
    from ddnm_amd import ops
    kn = ops.KeyedPhiloxNoise([s for s, _ in rows], [c for _, c in rows])
    B = len(rows)
    big = torch.full((B + 64, 4), 0x5EED5EE, dtype=torch.int32)
    big[:B] = kn._host
    dev = big.cuda()
    _KEEP.append(dev)
    kn._dev[("cuda", torch.cuda.current_device())] = dev[:B]
    return kn


def _draw(seed, it, base, B, chw):
    """[B][chw] of ddnm_randn_philox_f32 into a guarded buffer."""
    from ddnm_amd import ops
    from ddnm_amd._lib import check, lib
    buf, out = _out(B * chw)
    check(lib().ddnm_randn_philox_f32(_p(out), B, chw, seed & 0xFFFFFFFF, seed >> 32, it, base, ops._stream()), "ddnm_randn_philox_f32")
    return _taken(buf, B * chw, "randn_philox").reshape(B, chw)


@functools.lru_cache(maxsize=None)
def _step_host(name):
    """(case, inputs with the device's draw as `nz`, model, twin): once per case, shared, never modified."""
    case = SM.BY_NAME[name]
    t = dict(SM.make_inputs(case))
    if "nz" in t:
        seed, it, base = _seed(case)
        t["nz"] = _draw(seed, it, base, case.p["B"], t["xt"][0].size).numpy().reshape(t["xt"].shape)
    return case, t, SM.model(case, t), SM.twin(case, t)


def _run_step(case, t, noise, six, want_x0, imgs=None):
    """One launch of a fused-step case (of its images `imgs`, a slice) -> {"x0": .., "xn": ..} on the CPU.
    noise: ("tensor", array) | ("in_kernel", (seed, it, base)) | ("keyed", (it, [(seed, counter), ...]))."""
    from ddnm_amd import ops
    k, p = case.kernel, case.p
    sl = slice(None) if imgs is None else imgs
    xt_h = t["xt"][sl]
    B, C, H, W = xt_h.shape
    chw, HW = C * H * W, H * W
    s = _scalars(t["s"])
    xt = _ro(xt_h)
    et = _ro(t["et6"][sl])[:, :C] if six else _ro(SM.et_of(t)[sl])
    kind, arg = noise
    if k == "step_x0":
        nz = None
    elif kind == "tensor":
        nz = _ro(arg[sl])
    elif kind == "in_kernel":
        seed, it, base = arg
        nz = ops.PhiloxNoise(seed, base).kernel_arg(s, it)
    else:
        it, rows = arg
        nz = _keyed(rows).kernel_arg(s, it)
    bufs = {}
    if k == "step_x0":
        bufs["x0"] = _out(B * chw)
        ops.step_x0(xt, et, s, out=bufs["x0"][1].view(B, C, H, W))
    elif k == "step_combine":
        bufs["xn"] = _out(B * chw)
        ops.step_combine(_ro(t["x0"][sl]), _ro(t["proj"][sl]), _ro(None if t["apy"] is None else t["apy"][sl]), nz, et, s,
                         out=bufs["xn"][1].view(B, C, H, W))
    else:
        bufs["xn"] = _out(B * chw)
        x0p = None
        if want_x0:
            bufs["x0"] = _out(B * chw)
            x0p = _p(bufs["x0"][1])
        xnp = _p(bufs["xn"][1])
        if k == "step_sr4":
            ops.step_call("ddnm_step_sr_avgpool_f32", xt, et, nz, _ro(t["y"][sl]), x0p, xnp, B, H, W, 4, s)
        elif k == "step_color":
            w3 = None if p["w3"] is None else (ctypes.c_float * 3)(*p["w3"])
            ops.step_call("ddnm_step_color_f32", xt, et, nz, _ro(t["y"][sl]), x0p, xnp, B, HW, w3, s)
        elif k == "step_denoise":
            ops.step_call("ddnm_step_denoise_f32", xt, et, nz, _ro(t["y"][sl]), x0p, xnp, B, chw, s)
        elif k == "step_inpaint":
            n_kept = int(t["mask"].sum())
            ops.step_call("ddnm_step_inpaint_f32", xt, et, nz, _ro(t["y"][sl]), _p(_ro(t["rank"], tail=n_kept + 64)), n_kept,
                          x0p, xnp, B, HW, s)
        else:
            n_max = int(t["mask"][sl].sum(axis=1).max())
            ops.step_call("ddnm_step_inpaint_pi_f32", xt, et, nz, _ro(t["y"][sl]), p["y_stride"],
                          _p(_ro(t["rank"][sl], tail=p["y_stride"] // 3 + 64)), n_max, x0p, xnp, B, HW, s)
    return {key: _taken(buf, B * chw, f"{case.name} {key}").reshape(B, C, H, W) for key, (buf, _) in bufs.items()}


NAMES4 = ("image", "channel", "y", "x")


@pytest.mark.parametrize("name", STEP_CASES)
def test_fused_step_bits(hip, name):
    """x0 and x_t' of every noise source x et stride x x0 option equal the fp32 model bit for bit."""
    case, t, want, ref = _step_host(name)
    k = case.kernel
    seed, it, base = _seed(case)
    B = case.p["B"]
    sources = {"tensor": ("tensor", t.get("nz")), "in_kernel": ("in_kernel", (seed, it, base)),
               "keyed": ("keyed", (it, [(seed, base + b) for b in range(B)]))}
    n = 0
    for src, stride, x0_opt in SM.variants(k):
        six, want_x0 = stride == "six_channel", x0_opt != "x0_null"
        got = _run_step(case, t, sources[src or "tensor"], six, want_x0)
        assert set(got) == (set(want) if want_x0 else set(want) - {"x0"})
        for key, g in got.items():
            _assert_bits(g, torch.from_numpy(want[key]), f"{name} {key} [noise {src}, et {stride}, {x0_opt}]", NAMES4)
        n += 1
    ratios = {key: _record(case, torch.from_numpy(want[key]), ref[key]) for key in want}
    print(f"{name}: {n} launches, bits equal; worst |err| / bar against float64 " + ", ".join(f"{a} {b:.3f}" for a, b in ratios.items()))


@pytest.mark.parametrize("name", [n for n in STEP_CASES if SM.BY_NAME[n].kernel in SM.NOISY])
def test_keyed_rows_equal_single_image_launches(hip, name):
    """Different key rows {seed_b, counter_b} in one keyed launch = B launches of one image with (seed_b, image_base =
    counter_b) drawn in-kernel, image by image and bit for bit (x0 too)."""
    case, t, _, _ = _step_host(name)
    B = case.p["B"]
    _, it, _ = _seed(case)
    rows = [(0x1234567 + 0x9E3779B97F4A7C15 * b & 0xFFFFFFFFFFFFFFFF, 3 + 11 * b) for b in range(B)]
    fused = _run_step(case, t, ("keyed", (it, rows)), True, True)
    for b in range(B):
        one = _run_step(case, t, ("in_kernel", (rows[b][0], it, rows[b][1])), False, True, imgs=slice(b, b + 1))
        for key in one:
            _assert_bits(fused[key][b:b + 1], one[key], f"{name} {key}: image {b} of the keyed launch against its own launch", NAMES4)
    if B > 1:       # and the rows matter: images 0 and 1 with image 0's row would draw the same noise
        assert rows[0] != rows[1]


# ----------------------------------------------------------------------------- operators
def _run_op(hip, case, t):
    """One launch (patchify: three) -> {output name: CPU tensor}, guards checked."""
    from ddnm_amd import ops
    from ddnm_amd._lib import check
    k, p = case.kernel, case.p
    st = ops._stream()
    res = {}

    def launch(fn, *args):
        check(getattr(hip, fn)(*args, st), fn)

    def done(key, buf, n):
        res[key] = _taken(buf, n, f"{case.name} {key}")

    if k in ("avgpool", "upsample"):
        BC, H, W, r = p["BC"], p["H"], p["W"], p["r"]
        n = BC * (H // r) * (W // r) if k == "avgpool" else BC * H * W
        buf, out = _out(n)
        launch(f"ddnm_op_{k}_f32", _p(_ro(t["x"])), _p(out), BC, H, W, r)
        done("y" if k == "avgpool" else "x", buf, n)
    elif k in ("color_A", "color_pinv"):
        B, HW = p["B"], p["HW"]
        w3 = None if p["w3"] is None else (ctypes.c_float * 3)(*p["w3"])
        n = B * HW if k == "color_A" else 3 * B * HW
        buf, out = _out(n)
        launch(f"ddnm_op_{k}_f32", _p(_ro(t["x" if k == "color_A" else "y"])), _p(out), B, HW, w3)
        done("y" if k == "color_A" else "x", buf, n)
    elif k in ("inpaint_A", "inpaint_pinv", "inpaint_A_pi", "inpaint_pinv_pi"):
        B, HW = p["B"], p["HW"]
        ylen, _ = SM._y_dims(case, t)
        n_kept = int(np.atleast_2d(t["mask"]).sum(axis=1).max())
        rank = _ro(t["rank"], tail=ylen // 3 + 64)
        if k == "inpaint_A":
            buf, out = _out(B * ylen)
            launch("ddnm_op_inpaint_A_f32", _p(_ro(t["x"])), _p(rank), n_kept, _p(out), B, HW)
            done("y", buf, B * ylen)
        elif k == "inpaint_A_pi":
            buf, out = _out(B * ylen)
            launch("ddnm_op_inpaint_A_pi_f32", _p(_ro(t["x"])), _p(rank), n_kept, _p(out), ylen, B, HW)
            done("y", buf, B * ylen)
        elif k == "inpaint_pinv":
            buf, out = _out(3 * B * HW)
            launch("ddnm_op_inpaint_pinv_f32", _p(_ro(t["y"])), _p(rank), n_kept, _p(out), B, HW)
            done("x", buf, 3 * B * HW)
        else:
            buf, out = _out(3 * B * HW)
            launch("ddnm_op_inpaint_pinv_pi_f32", _p(_ro(t["y"])), ylen, _p(rank), n_kept, _p(out), B, HW)
            done("x", buf, 3 * B * HW)
    elif k == "patchify":
        n = t["src"].size
        src = _ro(t["src"])
        b1, fwd = _out(n)
        launch("ddnm_patchify_f32", _p(src), _p(fwd), p["planes"], p["D"], p["ps"], 0)
        b2, inv = _out(n)
        launch("ddnm_patchify_f32", _p(src), _p(inv), p["planes"], p["D"], p["ps"], 1)
        b3, back = _out(n)
        launch("ddnm_patchify_f32", _p(fwd), _p(back), p["planes"], p["D"], p["ps"], 1)
        done("forward", b1, n), done("inverse", b2, n), done("round_trip", b3, n)
    elif k == "gather_scale":
        B, n_in, n_out = p["B"], p["n_in"], p["n_out"]
        buf, out = _out(B * n_out)
        launch("ddnm_gather_scale_f32", _p(_ro(t["in"])), _p(_ro(t["idx"], tail=B * n_in + 64)), _p(_ro(t["scale"])), _p(out), B, n_in, n_out)
        done("out", buf, B * n_out)
    elif k == "site_matmul":
        _, (sb, ss, sj) = SM.site_offsets(p)
        n = t["in"].size
        buf, out = _out(n)
        launch("ddnm_site_matmul_f32", _p(_ro(t["in"])), _p(_ro(t["M"])), _p(out), p["B"], p["sites"], p["n"], sb, ss, sj, p["trans"])
        done("out", buf, n)
    elif k == "site_spectral":
        n = t["x"].size
        buf, out = _out(n)
        launch("ddnm_site_spectral_f32", _p(_ro(t["x"])), _p(_ro(t["y"])), _p(_ro(t["V"])), p["n"], p["mode"], p["r"], p["B"], 3, p["H"],
               p["W"], _p(out), p["op"], *(float(v) for v in t["c"]))
        done("out", buf, n)
    elif k == "mask_mix":
        n = t["x"].size
        buf, out = _out(n)
        launch("ddnm_mask_mix_f32", _p(_ro(t["x"])), _p(_ro(t["y"])), _p(_ro(t["mask"])), p["planes_mask"], p["plane_elems"], _p(out), n,
               *(float(v) for v in t["c"]))
        done("out", buf, n)
    elif k == "mul_planes":
        n = t["x"].size
        buf, out = _out(n)
        launch("ddnm_mul_planes_f32", _p(_ro(t["x"])), _p(_ro(t["table"])), p["planes_table"], p["plane_elems"], _p(out), n)
        done("out", buf, n)
    elif k == "axpby":
        n = p["n"]
        buf, out = _out(n)
        launch("ddnm_axpby_f32", _p(_ro(t["x"])), _p(_ro(t["y"])), _p(out), n, float(t["a"]), float(t["b"]))
        done("out", buf, n)
    elif k == "axpby_strided":
        B, chw = p["B"], p["chw"]
        buf, out = _out(B * chw)
        launch("ddnm_axpby_strided_f32", _p(_ro(t["x2"])), 2 * chw, _p(_ro(t["y"])), _p(out), B, chw, float(t["a"]), float(t["b"]))
        done("out", buf, B * chw)
    elif k == "spectral_mix":
        n = t["x"].size
        buf, out = _out(n)
        launch("ddnm_spectral_mix_f32", _p(_ro(t["x"])), _p(_ro(t["y"])) if p["mode"] == 1 else None, _p(_ro(t["stab"])), p["plane_elems"],
               _p(out), n, float(t["a"]), float(t["sy"]), float(t["st"]), float(t["eta"]), p["mode"])
        done("out", buf, n)
    elif k == "renoise":
        n = p["n"]
        buf, out = _out(n)
        ops.renoise(_ro(t["x0"]), _ro(t["noise"]), float(t["a"]), float(t["b"]), out=out)
        done("xn", buf, n)
    elif k == "fill":
        n = p["n"]
        buf, out = _out(n)
        ops.fill_(out, float(t["value"]))
        done("out", buf, n)
    else:
        raise KeyError(k)
    return res


OUT_NAMES = {"avgpool": ("plane", "y", "x"), "upsample": ("plane", "y", "x"), "color_A": ("image", "pixel"),
             "color_pinv": ("image", "channel", "pixel"), "inpaint_A": ("row", "entry"), "inpaint_A_pi": ("row", "entry"),
             "inpaint_pinv": ("image", "channel", "pixel"), "inpaint_pinv_pi": ("image", "channel", "pixel"),
             "gather_scale": ("row", "entry"), "site_spectral": NAMES4, "mask_mix": ("plane", "entry"), "mul_planes": ("plane", "entry"),
             "spectral_mix": ("plane", "entry"), "axpby_strided": ("row", "entry")}


@pytest.mark.parametrize("name", OP_CASES)
def test_operator_bits(hip, name):
    case = SM.BY_NAME[name]
    t = SM.make_inputs(case)
    want, ref = SM.model(case, t), SM.twin(case, t)
    got = _run_op(hip, case, t)
    assert set(got) == set(want)
    for key in want:
        w = torch.from_numpy(want[key])
        _assert_bits(got[key], w, f"{name} {key}", OUT_NAMES.get(case.kernel, ("entry",)))
    ratios = {key: _record(case, torch.from_numpy(want[key]), ref[key]) for key in want}
    print(f"{name}: bits equal; worst |err| / bar against float64 " + ", ".join(f"{a} {b:.3f}" for a, b in ratios.items()))


@pytest.mark.parametrize("name", PSNR_CASES)
def test_finalize_psnr(hip, name):
    """img bit for bit; sse within (chw + 64) 2^-53 sum(dd^2) of the float64 sum of the fp32 squares.  Called through the
    library (ops.finalize_psnr allocates its own outputs, which cannot be guarded)."""
    from ddnm_amd import ops
    from ddnm_amd._lib import check
    case = SM.BY_NAME[name]
    p, t = case.p, SM.make_inputs(case)
    B, chw = p["B"], p["chw"]
    want = SM.model(case, t)
    ibuf, img = _out(B * chw) if p["img"] else (None, None)
    sbuf, sse = _out(B, torch.float64) if p["x_orig"] else (None, None)
    check(hip.ddnm_finalize_psnr_f32(_p(_ro(t["x"])), _p(_ro(t["xo"])), _p(img), _p(sse), B, chw, ops._stream()), "ddnm_finalize_psnr_f32")
    torch.cuda.synchronize()
    if img is not None:
        got = _taken(ibuf, B * chw, f"{name} img").reshape(B, chw)
        _assert_bits(got, torch.from_numpy(want["img"]), f"{name} img", ("image", "entry"))
        assert float(got.min()) == 0.0 and float(got.max()) == 1.0
        WORST["finalize_psnr"] = max(WORST.get("finalize_psnr", 0.0), _record(case, got, SM.twin(case, t)["img"]))
    if sse is not None:
        got = _taken(sbuf, B, f"{name} sse").numpy()
        ref = want["dd2"].astype(np.float64).sum(axis=1)
        bar = SM.sse_bar(chw, want["dd2"])
        print(f"{name}: sse |err| / bar " + ", ".join(f"{abs(g - r) / b if b else 0.0:.3f}" for g, r, b in zip(got, ref, bar)))
        assert (np.abs(got - ref) <= bar).all(), (got, ref, bar)


@pytest.mark.parametrize("name", RANDN_CASES)
def test_randn_philox(hip, name):
    """The B = 3 draw equals, bit for bit, three B = 1 draws of image_base + b and the keyed draw of the same rows; its
    values (logf / cosf / sinf of the device library) are oracle.philox's within 3e-5."""
    from ddnm_amd import ops
    case = SM.BY_NAME[name]
    B, chw = case.p["B"], case.p["chw"]
    seed, it, base = _seed(case)
    got = _draw(seed, it, base, B, chw)
    for b in range(B):
        _assert_bits(got[b:b + 1], _draw(seed, it, base + b, 1, chw), f"{name}: image {b} against its own draw", ("image", "entry"))
    like = torch.empty(B, chw, device="cuda")
    keyed = _keyed([(seed, base + b) for b in range(B)]).tensor(it, like)
    torch.cuda.synchronize()
    _assert_bits(keyed.cpu(), got, f"{name}: keyed draw", ("image", "entry"))
    ref = torch.from_numpy(SM.model(case, {})["out"])
    assert float((got - ref).abs().max()) <= 3e-5


# ----------------------------------------------------------------------------- second trip of the grid-stride loops
def _ints(gen, *shape, lo=-8, hi=9):
    return torch.randint(lo, hi, shape, generator=gen, device="cuda", dtype=torch.int8).float()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _same_on_device(got, want, what, per_image):
    torch.cuda.synchronize()
    bad = (got != want) | torch.isnan(got)
    n_bad = int(bad.sum())
    if n_bad:
        first = bad.reshape(-1).nonzero()[:6].reshape(-1).tolist()
        raise AssertionError(f"{what}: {n_bad} of {got.numel()} elements differ, first (image, offset in image) "
                             f"{[(i // per_image, i % per_image) for i in first]}")


def _pow2_scalars(lam=0.5, c1=0.25, c2=0.125):
    from ddnm_amd._lib import StepScalars
    s = StepScalars()
    s.sqrt_1m_at, s.sqrt_at, s.sqrt_at_next, s.c1, s.c2, s.lam = 0.25, 0.5, 0.5, c1, c2, lam
    return s


def _x0_exact(xt, et):
    return (xt - et * 0.25) / 0.5


def _update_exact(x0h, nz, et):
    return x0h * 0.5 + nz * 0.25 + et * 0.125


def _flat_step_second_trip(kernel):
    from ddnm_amd import ops
    p = SM.SECOND_TRIP[kernel]
    B, chw = p["B"], p["chw"]
    g = _gen(zlib_seed(kernel))
    shape = (B, 3, chw // 3 // 8, 8)
    assert shape[1] * shape[2] * shape[3] == chw
    return ops, g, shape, B, chw


def zlib_seed(name):
    return zlib.crc32(name.encode())


def test_second_trip_step_x0(hip):
    ops, g, shape, B, chw = _flat_step_second_trip("step_x0")
    xt, et = _ints(g, *shape), _ints(g, *shape)
    out = torch.full(shape, NAN, device="cuda")
    ops.step_x0(xt, et, _pow2_scalars(), out=out)
    _same_on_device(out, _x0_exact(xt, et), "step_x0 second trip", chw)


def test_second_trip_step_combine(hip):
    ops, g, shape, B, chw = _flat_step_second_trip("step_combine")
    x0, proj, apy, nz, et = (_ints(g, *shape) for _ in range(5))
    out = torch.full(shape, NAN, device="cuda")
    ops.step_combine(x0, proj, apy, nz, et, _pow2_scalars(), out=out)
    _same_on_device(out, _update_exact(x0 - (proj - apy) * 0.5, nz, et), "step_combine second trip", chw)


def test_second_trip_step_denoise(hip):
    ops, g, shape, B, chw = _flat_step_second_trip("step_denoise")
    xt, et, nz, y = (_ints(g, *shape) for _ in range(4))
    x0o, out = torch.full(shape, NAN, device="cuda"), torch.full(shape, NAN, device="cuda")
    ops.step_call("ddnm_step_denoise_f32", xt, et, nz, y, _p(x0o), _p(out), B, chw, _pow2_scalars())
    x0 = _x0_exact(xt, et)
    _same_on_device(x0o, x0, "step_denoise x0 second trip", chw)
    _same_on_device(out, _update_exact(x0 - (x0 - y) * 0.5, nz, et), "step_denoise second trip", chw)


def test_second_trip_randn_philox_tensor_equals_in_kernel_draw(hip):
    """The tensor draw of ddnm_randn_philox_f32 and the in-kernel draw of a step kernel (step_denoise over zeros with
    c1 = 1: x_t' = (0 * a + n * 1) + 0 * c2 = n) agree in both trips, image 1 included."""
    ops, g, shape, B, chw = _flat_step_second_trip("randn_philox")
    seed, it, base = 0x0123456789ABCDEF, 41, 6
    zeros = torch.zeros(shape, device="cuda")
    drawn = ops.PhiloxNoise(seed, base).tensor(it, zeros)
    s = _pow2_scalars(lam=1.0, c1=1.0, c2=0.0)
    out = torch.full(shape, NAN, device="cuda")
    ops.step_call("ddnm_step_denoise_f32", zeros, zeros, ops.PhiloxNoise(seed, base).kernel_arg(s, it), zeros, None, _p(out), B, chw, s)
    _same_on_device(out, drawn, "in-kernel draw against the tensor draw, second trip", chw)
    keyed = _keyed([(seed, base), (seed, base + 1)])
    out2 = torch.full(shape, NAN, device="cuda")
    ops.step_call("ddnm_step_denoise_f32", zeros, zeros, keyed.kernel_arg(s, it), zeros, None, _p(out2), B, chw, s)
    _same_on_device(out2, drawn, "keyed draw against the tensor draw, second trip", chw)
    assert float(drawn.std()) > 0.99 and not torch.equal(drawn[0], drawn[1])


def test_second_trip_step_color(hip):
    """w3_host = (0.5, 0.5, 0): |w|^2 = 0.5, w / |w|^2 = (1, 1, 0), all exact."""
    from ddnm_amd import ops
    p = SM.SECOND_TRIP["step_color"]
    B, HW = p["B"], p["HW"]
    g = _gen(zlib_seed("step_color"))
    shape = (B, 3, HW // 8, 8)
    xt, et, nz = (_ints(g, *shape) for _ in range(3))
    y = _ints(g, B, HW // 8, 8)
    x0o, out = torch.full(shape, NAN, device="cuda"), torch.full(shape, NAN, device="cuda")
    ops.step_call("ddnm_step_color_f32", xt, et, nz, y, _p(x0o), _p(out), B, HW, (ctypes.c_float * 3)(0.5, 0.5, 0.0), _pow2_scalars())
    x0 = _x0_exact(xt, et)
    resid = ((x0[:, 0] * 0.5 + x0[:, 1] * 0.5) - y) * 0.5
    x0h = torch.stack([x0[:, 0] - resid, x0[:, 1] - resid, x0[:, 2]], dim=1)
    _same_on_device(x0o, x0, "step_color x0 second trip", 3 * HW)
    _same_on_device(out, _update_exact(x0h, nz, et), "step_color second trip", 3 * HW)


def test_second_trip_step_inpaint(hip):
    from ddnm_amd import ops
    p = SM.SECOND_TRIP["step_inpaint"]
    B, HW = p["B"], p["HW"]
    g = _gen(zlib_seed("step_inpaint"))
    shape = (B, 3, HW // 8, 8)
    xt, et, nz = (_ints(g, *shape) for _ in range(3))
    kept = torch.rand(HW, generator=g, device="cuda") < 0.4
    rank = torch.where(kept, torch.cumsum(kept.int(), 0, dtype=torch.int32) - 1, torch.full((HW,), -1, dtype=torch.int32, device="cuda"))
    n_kept = int(kept.sum())
    y = _ints(g, B, n_kept, 3)
    x0o, out = torch.full(shape, NAN, device="cuda"), torch.full(shape, NAN, device="cuda")
    ops.step_call("ddnm_step_inpaint_f32", xt, et, nz, y, _p(rank), n_kept, _p(x0o), _p(out), B, HW, _pow2_scalars())
    x0 = _x0_exact(xt, et)
    x0f = x0.reshape(B, 3, HW)
    yi = torch.zeros(B, 3, HW, device="cuda")
    yi[:, :, kept] = y.permute(0, 2, 1)
    x0h = torch.where(kept[None, None, :], x0f - (x0f - yi) * 0.5, x0f).reshape(shape)
    _same_on_device(x0o, x0, "step_inpaint x0 second trip", 3 * HW)
    _same_on_device(out, _update_exact(x0h, nz, et), "step_inpaint second trip", 3 * HW)


def test_second_trip_step_sr4(hip):
    """B = 1, H = W = 3348: 3 * 837^2 = 2101707 patches; the sums of sixteen multiples of 1/2 are exact in any order."""
    from ddnm_amd import ops
    p = SM.SECOND_TRIP["step_sr4"]
    B, H, W = p["B"], p["H"], p["W"]
    g = _gen(zlib_seed("step_sr4"))
    xt, et, nz = (_ints(g, B, 3, H, W) for _ in range(3))
    y = _ints(g, B, 3, H // 4, W // 4)
    x0o, out = torch.full((B, 3, H, W), NAN, device="cuda"), torch.full((B, 3, H, W), NAN, device="cuda")
    ops.step_call("ddnm_step_sr_avgpool_f32", xt, et, nz, y, _p(x0o), _p(out), B, H, W, 4, _pow2_scalars())
    x0 = _x0_exact(xt, et)
    pooled = x0.reshape(B, 3, H // 4, 4, W // 4, 4).sum(dim=(3, 5)) / 16.0
    corr = ((pooled - y) * 0.5).repeat_interleave(4, dim=2).repeat_interleave(4, dim=3)
    _same_on_device(x0o, x0, "step_sr4 x0 second trip", 3 * H * W)
    del pooled
    want = _update_exact(x0 - corr, nz, et)
    del corr, x0
    _same_on_device(out, want, "step_sr4 second trip", 3 * H * W)


def test_second_trip_renoise(hip):
    from ddnm_amd import ops
    n = SM.SECOND_TRIP["renoise"]["n"]
    g = _gen(zlib_seed("renoise"))
    x0, nz = _ints(g, n), _ints(g, n)
    out = torch.full((n,), NAN, device="cuda")
    ops.renoise(x0, nz, 0.5, 0.25, out=out)
    _same_on_device(out, x0 * 0.5 + nz * 0.25, "renoise second trip", n)


def test_second_trip_patchify(hip):
    from ddnm_amd import ops
    from ddnm_amd._lib import check
    p = SM.SECOND_TRIP["patchify"]
    P, D, ps = p["planes"], p["D"], p["ps"]
    n = D // ps
    g = _gen(zlib_seed("patchify"))
    src = _ints(g, P, D, D)
    out = torch.full((P * D * D,), NAN, device="cuda")
    check(hip.ddnm_patchify_f32(_p(src), _p(out), P, D, ps, 0, ops._stream()), "ddnm_patchify_f32")
    want = src.reshape(P, n, ps, n, ps).permute(0, 1, 3, 2, 4).reshape(-1)
    _same_on_device(out, want, "patchify second trip", D * D)


def test_second_trip_upsample(hip):
    from ddnm_amd import ops
    from ddnm_amd._lib import check
    p = SM.SECOND_TRIP["upsample"]
    BC, H, W, r = p["BC"], p["H"], p["W"], p["r"]
    g = _gen(zlib_seed("upsample"))
    y = _ints(g, BC, H // r, W // r)
    out = torch.full((BC, H, W), NAN, device="cuda")
    check(hip.ddnm_op_upsample_f32(_p(y), _p(out), BC, H, W, r, ops._stream()), "ddnm_op_upsample_f32")
    _same_on_device(out, y.repeat_interleave(r, dim=1).repeat_interleave(r, dim=2), "upsample second trip", H * W)


def test_second_trip_gather_scale(hip):
    from ddnm_amd import ops
    from ddnm_amd._lib import check
    p = SM.SECOND_TRIP["gather_scale"]
    B, n_in, n_out = p["B"], p["n_in"], p["n_out"]
    g = _gen(zlib_seed("gather_scale"))
    src = _ints(g, B, n_in)
    idx = torch.randint(-n_in // 2, n_in, (n_out,), generator=g, device="cuda", dtype=torch.int32).clamp(min=-1)
    scale = torch.tensor([0.25, 0.5, 1.0, -2.0], device="cuda")[torch.randint(0, 4, (n_out,), generator=g, device="cuda")]
    out = torch.full((B, n_out), NAN, device="cuda")
    check(hip.ddnm_gather_scale_f32(_p(src), _p(idx), _p(scale), _p(out), B, n_in, n_out, ops._stream()), "ddnm_gather_scale_f32")
    want = torch.where(idx[None, :] >= 0, src[:, idx.clamp(min=0).long()], torch.zeros((), device="cuda")) * scale[None, :]
    _same_on_device(out, want, "gather_scale second trip", n_out)


def test_zz_record(hip):
    """Prints what the docstring records: cases, worst |err| / bar per kernel, run time of the file so far."""
    print(f"cases: {len(SM.CASES)} ({len(STEP_CASES)} fused-step, {len(OP_CASES)} operator, {len(PSNR_CASES)} finalize_psnr, "
          f"{len(RANDN_CASES)} randn_philox) + {len(SM.SECOND_TRIP)} second-trip launches")
    print("worst |err| / bar against float64: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    print(f"run time of the file: {time.time() - _CLOCK['t0']:.1f} s")
