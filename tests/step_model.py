"""CPU model of the first-generation sampler-step and operator kernels of csrc/ddnm_step.hip: the fused steps (step_x0,
step_combine, step_sr4, step_color, step_inpaint shared / per image, step_denoise) and the stand-alone operators and DDNM+
building blocks (avgpool, upsample, color_A/pinv, inpaint_A/pinv shared / per image, axpby, axpby_strided, mask_mix,
mul_planes, gather_scale, site_matmul, site_spectral, spectral_mix, patchify, renoise, fill, finalize_psnr, randn_philox).
No GPU import; tests/test_step_model_host.py checks this file on the CPU, tests/test_gpu_step_edges.py holds the kernels
to it.

Three things per kernel:

  model(case, t)   the kernel restated in numpy float32, one rounding per * + - /, in the order the kernel's source takes
                   (read from ddnm_step.hip; contraction into FMA is off there).  The kernels must equal it BIT FOR BIT.
                   `fault=` plants one of FAULTS in it (host test: every case notices the faults it is meant to catch).
  twin(case, t)    the same formula in plain float64, written with whole-array expressions, in the `T` arithmetic below
                   that carries next to each value v the sum m of the magnitudes of the terms it was made of and the
                   number k of fp32 roundings on its longest chain: an fp32 evaluation in ANY order of the same chain lies
                   within   bar = k 2^-24 m   of it (the running error bound gamma_k m, Higham, "Accuracy and Stability
                   of Numerical Algorithms", section 3.1; a product of two rounded factors chains k_1 + k_2 + 1 roundings,
                   a sum max(k_1, k_2) + 1).  The GPU test prints |err| / bar for the record; only finalize_psnr's
                   atomically accumulated double is asserted against a bar.
  CASES / BY_NAME  the smallest shapes that reach every branch; `why` says what each is there for.

The noise of a fused step is an input `nz` of the model: on the CPU oracle.philox.randn of the case's (seed, iteration,
image base), on the GPU what ddnm_randn_philox_f32 draws for them, so that the tensor, the in-kernel and the keyed source
can be compared with each other bit for bit (the Box-Muller values themselves are pinned by test_philox.py /
test_gpu_fuse.py)."""
import zlib
from typing import NamedTuple

import numpy as np

F = np.float32
EPS = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)
BLOCK, GRID_CAP = 256, 8192              # GRID_1D of ddnm_step.hip: at most 8192 workgroups of 256
NAN = F("nan")

ETAS, LAMBDAS, BATCHES = (0.85, 1.0, 0.0), (1.0, 0.3), (1, 3)
W_CUSTOM = (0.299, 0.587, 0.114)
W_DEFAULT = (0.3333, 0.3334, 0.3333)
NOISE_SOURCES = ("tensor", "in_kernel", "keyed")
ET_STRIDES = ("contiguous", "six_channel")
X0_OPTIONS = ("x0_out", "x0_null")

FAULTS = ("fma", "colmajor", "swap_hw", "shift", "et_stride", "key_row", "lambda_operand", "swap_kept", "tie_lt", "tie_gt")


class Case(NamedTuple):
    name: str
    kernel: str
    why: str
    p: dict


# ----------------------------------------------------------------------------- float64 twin arithmetic
class T:
    """(v, m, k): float64 value, sum of the magnitudes of its terms, fp32 roundings on its longest chain."""
    __slots__ = ("v", "m", "k")

    def __init__(self, v, m=None, k=0):
        self.v = np.asarray(v, dtype=np.float64)
        self.m = np.abs(self.v) if m is None else np.asarray(m, dtype=np.float64)
        self.k = int(k)

    @staticmethod
    def of(o):
        return o if isinstance(o, T) else T(o)

    def __add__(self, o):
        o = T.of(o)
        return T(self.v + o.v, self.m + o.m, max(self.k, o.k) + 1)

    def __sub__(self, o):
        o = T.of(o)
        return T(self.v - o.v, self.m + o.m, max(self.k, o.k) + 1)

    def __mul__(self, o):
        o = T.of(o)
        return T(self.v * o.v, self.m * o.m, self.k + o.k + 1)

    def __truediv__(self, o):
        o = T.of(o)
        assert o.k == 0, "the divisors of these kernels are inputs"
        return T(self.v / o.v, self.m / np.abs(o.v), self.k + 1)

    __radd__ = __add__
    __rmul__ = __mul__

    def __getitem__(self, i):
        return T(self.v[i], self.m[i], self.k)

    def reshape(self, *shape):
        return T(self.v.reshape(*shape), self.m.reshape(*shape), self.k)

    def transpose(self, *axes):
        return T(self.v.transpose(*axes), self.m.transpose(*axes), self.k)

    def sum(self, axis):
        """An n-term sum started from 0.f: n roundings in whatever order."""
        n = int(np.prod([self.v.shape[a] for a in (axis if isinstance(axis, tuple) else (axis,))]))
        return T(self.v.sum(axis=axis), self.m.sum(axis=axis), self.k + n)

    def sqrt(self):
        """|sqrt(x + e) - sqrt(x)| <= |e| / sqrt(x), plus the root's own rounding."""
        r = np.sqrt(np.maximum(self.v, 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.where(r > 0, self.m / np.where(r > 0, r, 1.0) + r, 0.0)
        return T(r, m, self.k + 1)

    def bar(self):
        return self.k * EPS * self.m / (1.0 - self.k * EPS)


def t_where(mask, a, b):
    a, b = T.of(a), T.of(b)
    return T(np.where(mask, a.v, b.v), np.where(mask, a.m, b.m), max(a.k, b.k))


def t_stack(ts, axis):
    return T(np.stack([t.v for t in ts], axis), np.stack([t.m for t in ts], axis), max(t.k for t in ts))


# ----------------------------------------------------------------------------- scalars
class Sc(NamedTuple):
    s1: np.float32        # sqrt(1 - abar_t)
    s2: np.float32        # sqrt(abar_t)
    a: np.float32         # sqrt(abar_next)
    c1: np.float32
    c2: np.float32
    lam: np.float32


AT, AT_NEXT = 0.37, 0.52


def scalars(eta, lam):
    """The StepScalars of ops.step_scalars (fp32, the reference's host expressions) for fixed alpha-bars."""
    try:
        import torch
        from ddnm_amd import ops
        s = ops.step_scalars(torch.tensor(AT), torch.tensor(AT_NEXT), eta, lam)
        return Sc(*(F(v) for v in (s.sqrt_1m_at, s.sqrt_at, s.sqrt_at_next, s.c1, s.c2, s.lam)))
    except ImportError:       # restated: fp32 tensor expressions with the Python scalars rounded to fp32
        at, nx = F(AT), F(AT_NEXT)
        sg = np.sqrt(F(1) - nx)
        return Sc(np.sqrt(F(1) - at), np.sqrt(at), np.sqrt(nx), sg * F(eta), sg * F((1 - eta ** 2) ** 0.5), F(lam))


def color_weights(w3):
    """color_weights of ddnm_step.hip, evaluated on the host in fp32: w, and wp = w / ((w0 w0 + w1 w1) + w2 w2)."""
    w = [F(v) for v in (W_DEFAULT if w3 is None else w3)]
    n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    return w, [v / n2 for v in w]


# ----------------------------------------------------------------------------- grid
def grid_of(items):
    return min((items + BLOCK - 1) // BLOCK, GRID_CAP)


def second_trip_start(items):
    """First work item a thread reaches on its second trip of the grid-stride loop (None: one trip)."""
    return GRID_CAP * BLOCK if items > GRID_CAP * BLOCK else None


def work_items(kernel, p):
    """(work items of one launch, work items per image or None): what the kernel's loop counts, from its launcher."""
    B = p.get("B", 1)
    if kernel in ("step_x0", "step_combine", "step_denoise", "randn_philox"):
        return B * p["chw"] // 4, p["chw"] // 4
    if kernel == "step_sr4":
        per = 3 * (p["H"] // 4) * (p["W"] // 4)
        return B * per, per
    if kernel in ("step_color", "step_inpaint", "step_inpaint_pi"):
        return B * p["HW"] // 4, p["HW"] // 4
    if kernel == "renoise":
        return p["n"] // 4, None
    if kernel == "patchify":
        return p["planes"] * p["D"] * p["D"] // 4, None
    if kernel == "upsample":
        return p["BC"] * p["H"] * p["W"], p["H"] * p["W"]
    if kernel == "gather_scale":
        return B * p["n_out"], p["n_out"]
    raise KeyError(kernel)


# ----------------------------------------------------------------------------- inputs
def _rng(name, salt=0):
    return np.random.default_rng(zlib.crc32(name.encode()) + salt)


def _n(r, *shape):
    return r.standard_normal(shape).astype(F)


def noise_key(case):
    """(seed_lo, seed_hi, iteration, image base) of a fused-step or randn case."""
    h = zlib.crc32(("key:" + case.name).encode())
    return h, (h * 2654435761) & 0xFFFFFFFF, 7 + h % 5, case.p.get("image_base", 5)


def host_noise(case, B, chw):
    from oracle import philox
    lo, hi, it, base = noise_key(case)
    return philox.randn((hi << 32) | lo, B, chw, it, base).astype(F)


def rank_of(mask):
    """[.., HW] bool -> the rank table of the inpainting kernels: kept pixels count up in pixel order, others -1."""
    m = np.asarray(mask, dtype=bool)
    return np.where(m, np.cumsum(m, axis=-1) - 1, -1).astype(np.int32)


def _masks(p, r):
    """Kept-pixel masks named by p['mask'] (shared: [HW]) or p['masks'] (per image: [B][HW])."""
    HW = p["HW"]

    def one(kind):
        if kind == "one":
            m = np.zeros(HW, dtype=bool)
            m[int(r.integers(HW))] = True
        elif kind == "all":
            m = np.ones(HW, dtype=bool)
        else:
            m = r.random(HW) < 0.4
            m[:2] = (True, False)
        return m
    if "masks" in p:
        return np.stack([one(k) for k in p["masks"]])
    return one(p["mask"])


def _measurements(p, r, mask):
    """y of the inpainting cases: shared [B][3 n_kept]; per image [B][y_stride] with NaN beyond 3 n_kept[b]."""
    B = p["B"]
    if mask.ndim == 1:
        return _n(r, B, 3 * int(mask.sum()))
    y = np.full((B, p["y_stride"]), NAN, dtype=F)
    for b in range(B):
        nk = 3 * int(mask[b].sum())
        y[b, :nk] = _n(r, nk)
    return y


def step_shape(case):
    """[C, H, W] of one image of a fused-step case."""
    p, k = case.p, case.kernel
    if k == "step_sr4":
        return 3, p["H"], p["W"]
    if k in ("step_color", "step_inpaint", "step_inpaint_pi"):
        return (3,) + p["hw"]
    return p["shape"]


# Cases of a few elements whose first draw could not tell a planted contraction from the separate roundings (the two agree
# on about half of all elements) draw again with these salts (host test: every case notices its faults).
SALT = {"step_x0_chw4": 1, "step_combine_chw4": 1, "site_spectral_m1_hw1_op1_y": 2, "axpby_n1_y": 1, "renoise_n4": 1}


def make_inputs(case):
    """dict of numpy arrays (never modified afterwards)."""
    p, k, r = case.p, case.kernel, _rng(case.name, SALT.get(case.name, 0))
    t = {}
    if k.startswith("step_"):
        B = p["B"]
        C, H, W = step_shape(case)
        chw = C * H * W
        t["s"] = scalars(p.get("eta", 0.85), p.get("lam", 1.0))
        t["xt"] = _n(r, B, C, H, W)
        t["et6"] = _n(r, B, 2 * C, H, W)            # et = et6[:, :C]: batch stride 2 chw; contiguous: its copy
        if k != "step_x0":
            t["nz"] = host_noise(case, B, chw).reshape(B, C, H, W)
        if k == "step_combine":
            t["x0"], t["proj"] = _n(r, B, C, H, W), _n(r, B, C, H, W)
            t["apy"] = _n(r, B, C, H, W) if p["apy"] else None
        elif k == "step_sr4":
            t["y"] = _n(r, B, 3, H // 4, W // 4)
        elif k == "step_color":
            t["y"] = _n(r, B, H * W)
        elif k == "step_denoise":
            t["y"] = _n(r, B, C, H, W)
        elif k in ("step_inpaint", "step_inpaint_pi"):
            t["mask"] = _masks(p, r)
            t["rank"] = rank_of(t["mask"])
            t["y"] = _measurements(p, r, t["mask"])
    elif k in ("avgpool", "upsample"):
        BC, H, W, rr = p["BC"], p["H"], p["W"], p["r"]
        t["x"] = _n(r, BC, H, W) if k == "avgpool" else _n(r, BC, H // rr, W // rr)
    elif k == "color_A":
        t["x"] = _n(r, p["B"], 3, p["HW"])
    elif k == "color_pinv":
        t["y"] = _n(r, p["B"], p["HW"])
    elif k in ("inpaint_A", "inpaint_A_pi", "inpaint_pinv", "inpaint_pinv_pi"):
        t["mask"] = _masks(p, r)
        t["rank"] = rank_of(t["mask"])
        if "pinv" in k:
            t["y"] = _measurements(p, r, t["mask"])
        else:
            t["x"] = _n(r, p["B"], 3, p["HW"])
    elif k == "patchify":
        n = p["planes"] * p["D"] * p["D"]
        t["src"] = _n(r, n)
    elif k == "gather_scale":
        B, n_in, n_out = p["B"], p["n_in"], p["n_out"]
        t["in"] = _n(r, B, n_in)
        t["idx"] = None
        if p["idx"]:
            idx = r.permutation(max(n_in, n_out))[:n_out].astype(np.int32)
            idx = np.where(idx < n_in, idx, -1)
            idx[r.random(n_out) < 1.0 / 3.0] = -1
            idx[idx == n_in - 1] = -1
            idx[0], idx[1] = -1, n_in - 1
            t["idx"] = idx.astype(np.int32)
        t["scale"] = _n(r, n_out) if p["scale"] else None
    elif k == "site_matmul":
        B, n, sites = p["B"], p["n"], p["sites"]
        t["in"] = _n(r, B * sites * n)              # both layouts cover exactly B * sites * n floats
        t["M"] = _n(r, n, n)
    elif k == "site_spectral":
        B, C, H, W, n = p["B"], 3, p["H"], p["W"], p["n"]
        t["x"] = _n(r, B, C, H, W)
        t["y"] = _n(r, B, C, H, W) if p["y"] else None
        q, _ = np.linalg.qr(r.standard_normal((n, n)))
        t["V"] = q.astype(F)
        t["c"] = [F(v) for v in (0.37, 0.81, -0.59, 0.23)]
    elif k == "mask_mix":
        planes, pe = p["planes"], p["plane_elems"]
        t["x"] = _n(r, planes, pe)
        t["y"] = _n(r, planes, pe) if p["y"] else None
        t["mask"] = None
        if p["planes_mask"]:
            m = np.where(r.random((p["planes_mask"], pe)) < 0.5, F(0), _n(r, p["planes_mask"], pe)).astype(F)
            m[0, :4] = (F(0.0), F(-0.0), F(1.0), F(-2.5))       # exact zeros of both signs: both unmeasured
            t["mask"] = m
        t["c"] = [F(v) for v in (0.71, 1.0, -0.43, 0.29)]       # cx_m, cx_n, cy_m, cy_n
    elif k == "mul_planes":
        t["x"] = _n(r, p["planes"], p["plane_elems"])
        t["table"] = _n(r, p["planes_table"], p["plane_elems"])
    elif k == "axpby":
        t["x"] = _n(r, p["n"])
        t["y"] = _n(r, p["n"]) if p["y"] else None
        t["a"], t["b"] = F(0.83), F(-0.41)
    elif k == "axpby_strided":
        t["x2"] = _n(r, p["B"], 2 * p["chw"])       # x = x2[:, :chw]: batch stride 2 chw
        t["y"] = _n(r, p["B"], p["chw"])
        t["a"], t["b"] = F(0.83), F(-0.41)
    elif k == "spectral_mix":
        planes, pe = p["planes"], p["plane_elems"]
        t["x"], t["y"] = _n(r, planes, pe), _n(r, planes, pe)
        a, sy, eta = F(p["a"]), F(p["sigma_y"]), F(0.85)
        stab = np.abs(_n(r, pe)) + F(0.05)
        s_tie = F(0.7318)
        thr = (a * sy) * (F(1) / s_tie)
        st = thr if (a != 0 and sy != 0) else F(0.31)
        # entry 0: the tie sigma_t == thr; 1, 2: zeros; 3, 4: well on either side; the rest random, none within 1e-3 of it
        stab[:5] = (s_tie, F(0), F(0), s_tie * F(2), s_tie * F(0.5))
        near = np.abs(stab[5:] - s_tie) < 1e-3
        stab[5:][near] += F(0.01)
        t["stab"], t["a"], t["sy"], t["st"], t["eta"] = stab.astype(F), a, sy, F(st), eta
        t["eta_c"] = F(np.sqrt(1.0 - float(eta) * float(eta)))
    elif k == "renoise":
        t["x0"], t["noise"] = _n(r, p["n"]), _n(r, p["n"])
        t["a"], t["b"] = F(0.72), F(0.69)
    elif k == "fill":
        t["value"] = F(-1.37)
    elif k == "finalize_psnr":
        B, chw = p["B"], p["chw"]
        t["x"] = (F(0.8) * _n(r, B, chw)).astype(F)              # |x| > 1 for about a fifth: both clamps
        t["xo"] = (F(0.8) * _n(r, B, chw)).astype(F) if p["x_orig"] else None
        t["x"][:, 0] = (F(1.5), F(-1.25), F(0.3))                # above, below and inside the clamps (chw = 1 too)
        if chw > 1:
            t["x"][:, 1] = (F(-1.25), F(0.3), F(1.5))
    elif k == "randn_philox":
        pass
    else:
        raise KeyError(k)
    return t


def et_of(t, fault=None):
    """et as the kernels read it: image b at b * et_bstride of the six-channel buffer -- or, planted, at b * chw."""
    et6 = t["et6"]
    B, C2 = et6.shape[:2]
    if fault == "et_stride":
        chw = et6[0].size // 2
        flat = et6.reshape(-1)
        return np.stack([flat[b * chw:(b + 1) * chw] for b in range(B)]).reshape((B, C2 // 2) + et6.shape[2:])
    return et6[:, :C2 // 2]


# ----------------------------------------------------------------------------- fp32 restatements
def _fma(x, a, z):
    """x * a + z rounded once (the planted contraction)."""
    return (np.asarray(x, np.float64) * np.asarray(a, np.float64) + np.asarray(z, np.float64)).astype(F)


def x0_of(xt, et, s):
    return (xt - et * s.s1) / s.s2


def update_of(x0h, nz, et, s, fault=None):
    if fault == "fma":
        return _fma(et, s.c2, _fma(x0h, s.a, nz * s.c1))
    return (x0h * s.a + nz * s.c1) + et * s.c2


def _noise(t, fault):
    nz = t["nz"]
    if fault == "key_row":
        nz = nz.copy()
        nz[1] = nz[0]
    return nz


def _swap_hw(a):
    return a.reshape(a.shape[:-2] + (a.shape[-1], a.shape[-2]))


def m_step_x0(case, t, fault=None):
    s, xt, et = t["s"], t["xt"], et_of(t, fault)
    if fault == "fma":
        return {"x0": (_fma(et, -s.s1, xt) / s.s2).astype(F)}
    return {"x0": x0_of(xt, et, s)}


def m_step_combine(case, t, fault=None):
    s, et = t["s"], et_of(t, fault)
    p = t["proj"]
    if t["apy"] is not None:
        p = p - t["apy"]
    if fault == "lambda_operand":
        x0h = t["x0"] * s.lam - p
    else:
        x0h = t["x0"] - p * s.lam
    return {"xn": update_of(x0h, _noise(t, fault), et, s, fault)}


def m_step_denoise(case, t, fault=None):
    s, et = t["s"], et_of(t, fault)
    x0 = x0_of(t["xt"], et, s)
    y = np.roll(t["y"].reshape(-1), -1).reshape(t["y"].shape) if fault == "shift" else t["y"]
    if fault == "lambda_operand":
        x0h = x0 - (x0 * s.lam - y)
    else:
        x0h = x0 - (x0 - y) * s.lam
    return {"x0": x0, "xn": update_of(x0h, _noise(t, fault), et, s, fault)}


def m_step_sr4(case, t, fault=None):
    s, et, xt, nz, y = t["s"], et_of(t, fault), t["xt"], _noise(t, fault), t["y"]
    if fault == "swap_hw":
        xt, et, nz, y = _swap_hw(xt), _swap_hw(et), _swap_hw(nz), _swap_hw(y)
    B, _, H, W = xt.shape
    Hy, Wy = H // 4, W // 4
    x0 = x0_of(xt, et, s)
    win = x0.reshape(B, 3, Hy, 4, Wy, 4)
    acc = np.zeros((B, 3, Hy, Wy), dtype=F)
    order = [(j, k) for k in range(4) for j in range(4)] if fault == "colmajor" else [(j, k) for j in range(4) for k in range(4)]
    for j, k in order:
        acc = acc + win[:, :, :, j, :, k]
    if fault == "shift":
        y = np.roll(y.reshape(-1), -1).reshape(y.shape)
    if fault == "lambda_operand":
        corr = (acc / F(16)) * s.lam - y
    else:
        corr = (acc / F(16) - y) * s.lam
    x0h = x0 - np.repeat(np.repeat(corr, 4, axis=2), 4, axis=3)
    xn = update_of(x0h, nz, et, s, fault)
    if fault == "swap_hw":
        x0, xn = _swap_hw(x0), _swap_hw(xn)
    return {"x0": x0, "xn": xn}


def m_step_color(case, t, fault=None):
    s, et = t["s"], et_of(t, fault)
    w, wp = color_weights(case.p["w3"])
    x0 = x0_of(t["xt"], et, s)
    B, _, H, W = x0.shape
    y = t["y"].reshape(B, H, W)
    if fault == "shift":
        y = np.roll(y.reshape(-1), -1).reshape(y.shape)
    if fault == "fma":
        gray = _fma(x0[:, 2], w[2], _fma(x0[:, 1], w[1], x0[:, 0] * w[0]))
    else:
        gray = (x0[:, 0] * w[0] + x0[:, 1] * w[1]) + x0[:, 2] * w[2]
    resid = (gray * s.lam - y) if fault == "lambda_operand" else (gray - y) * s.lam
    x0h = np.stack([x0[:, c] - resid * wp[c] for c in range(3)], axis=1)
    return {"x0": x0, "xn": update_of(x0h, _noise(t, fault), et, s, fault)}


def _swap_kept(rank):
    """One kept and one unkept pixel of (every row of) a rank table exchanged."""
    rk = np.array(rank, copy=True).reshape(-1, rank.shape[-1])
    for row in rk:
        kept, unkept = np.nonzero(row >= 0)[0], np.nonzero(row < 0)[0]
        if len(kept) and len(unkept):
            i, j = kept[0], unkept[0]
            row[i], row[j] = row[j], row[i]
    return rk.reshape(rank.shape)


def m_step_inpaint(case, t, fault=None):
    s, et = t["s"], et_of(t, fault)
    x0 = x0_of(t["xt"], et, s)
    B, _, H, W = x0.shape
    HW = H * W
    rank = _swap_kept(t["rank"]) if fault == "swap_kept" else t["rank"]
    rank = np.broadcast_to(rank, (B, HW))                        # rank_bstride 0 (shared) or HW (per image)
    y = t["y"]
    x0f = x0.reshape(B, 3, HW)
    x0h = x0f.copy()
    for b in range(B):
        kept = np.nonzero(rank[b] >= 0)[0]
        for c in range(3):
            src = rank[b, kept].astype(np.int64) * 3 + c
            if fault == "shift":
                src = (src + 3) % (3 * len(kept))
            yv = y[b, src]
            v = x0f[b, c, kept]
            x0h[b, c, kept] = v - (v * s.lam - yv) if fault == "lambda_operand" else v - (v - yv) * s.lam
    return {"x0": x0, "xn": update_of(x0h.reshape(x0.shape), _noise(t, fault), et, s, fault)}


m_step_inpaint_pi = m_step_inpaint


def m_avgpool(case, t, fault=None):
    p, x = case.p, t["x"]
    r = p["r"]
    if fault == "swap_hw":
        x = _swap_hw(x)
    BC, H, W = x.shape
    win = x.reshape(BC, H // r, r, W // r, r)
    acc = np.zeros((BC, H // r, W // r), dtype=F)
    order = [(j, k) for k in range(r) for j in range(r)] if fault == "colmajor" else [(j, k) for j in range(r) for k in range(r)]
    for j, k in order:
        acc = acc + win[:, :, j, :, k]
    y = acc / F(r * r)
    return {"y": _swap_hw(y) if fault == "swap_hw" else y}


def m_upsample(case, t, fault=None):
    p, y = case.p, t["x"]
    r = p["r"]
    if fault == "swap_hw":
        y = _swap_hw(y)
    if fault == "shift":
        y = np.roll(y.reshape(-1), -1).reshape(y.shape)
    x = np.repeat(np.repeat(y, r, axis=1), r, axis=2)
    return {"x": _swap_hw(x) if fault == "swap_hw" else x}


def m_color_A(case, t, fault=None):
    w, _ = color_weights(case.p["w3"])
    x = t["x"]
    if fault == "fma":
        return {"y": _fma(x[:, 2], w[2], _fma(x[:, 1], w[1], x[:, 0] * w[0]))}
    if fault == "shift":
        return {"y": (x[:, 1] * w[0] + x[:, 2] * w[1]) + x[:, 0] * w[2]}
    return {"y": (x[:, 0] * w[0] + x[:, 1] * w[1]) + x[:, 2] * w[2]}


def m_color_pinv(case, t, fault=None):
    _, wp = color_weights(case.p["w3"])
    if fault == "shift":
        wp = wp[1:] + wp[:1]
    return {"x": np.stack([t["y"] * wp[c] for c in range(3)], axis=1)}


def _y_dims(case, t):
    """(row length, entries used per image) of the measurement rows."""
    B = case.p["B"]
    m = t["mask"]
    if m.ndim == 1:
        return 3 * int(m.sum()), [3 * int(m.sum())] * B
    return case.p["y_stride"], [3 * int(m[b].sum()) for b in range(B)]


def m_inpaint_A(case, t, fault=None):
    B, HW = case.p["B"], case.p["HW"]
    rank = np.broadcast_to(_swap_kept(t["rank"]) if fault == "swap_kept" else t["rank"], (B, HW))
    ylen, _ = _y_dims(case, t)
    y = np.full((B, ylen), NAN, dtype=F)                         # the kernel writes kept entries only
    for b in range(B):
        kept = np.nonzero(rank[b] >= 0)[0]
        for c in range(3):
            src = (c + 1) % 3 if fault == "shift" else c
            y[b, rank[b, kept].astype(np.int64) * 3 + c] = t["x"][b, src, kept]
    return {"y": y}


def m_inpaint_pinv(case, t, fault=None):
    B, HW = case.p["B"], case.p["HW"]
    rank = np.broadcast_to(_swap_kept(t["rank"]) if fault == "swap_kept" else t["rank"], (B, HW))
    x = np.zeros((B, 3, HW), dtype=F)
    for b in range(B):
        kept = np.nonzero(rank[b] >= 0)[0]
        for c in range(3):
            src = (c + 1) % 3 if fault == "shift" else c
            x[b, c, kept] = t["y"][b, rank[b, kept].astype(np.int64) * 3 + src]
    return {"x": x}


m_inpaint_A_pi, m_inpaint_pinv_pi = m_inpaint_A, m_inpaint_pinv


def patch_index(planes, D, ps, fault=None):
    """Image-side float offset of every float of the patch matrix [planes (D/ps)^2][ps ps], in patchify_kernel's order."""
    npd = D // ps
    plane, py, px, r, q = np.meshgrid(np.arange(planes), np.arange(npd), np.arange(npd), np.arange(ps), np.arange(ps),
                                      indexing="ij")
    if fault == "shift":
        px = (px + 1) % npd
    if fault == "swap_hw":
        return ((plane * D + px * ps + r) * D + py * ps + q).reshape(-1)
    return ((plane * D + py * ps + r) * D + px * ps + q).reshape(-1)


def m_patchify(case, t, fault=None):
    p = case.p
    img = patch_index(p["planes"], p["D"], p["ps"], fault)
    src = t["src"]
    fwd = src[img]
    inv = np.empty_like(src)
    inv[img] = src
    back = np.empty_like(src)
    back[patch_index(p["planes"], p["D"], p["ps"])] = fwd
    return {"forward": fwd, "inverse": inv, "round_trip": back}


def m_gather_scale(case, t, fault=None):
    p = case.p
    B, n_in, n_out = p["B"], p["n_in"], p["n_out"]
    idx = t["idx"]
    j = np.where(np.arange(n_out) < n_in, np.arange(n_out), -1) if idx is None else idx.astype(np.int64)
    if fault == "shift":
        j = np.where(j >= 0, (j + 1) % n_in, -1)
    v = np.where(j >= 0, t["in"][:, np.maximum(j, 0)], F(0)).astype(F)
    if t["scale"] is not None:
        v = v * t["scale"]
    return {"out": v}


def site_offsets(p):
    """(offset of (b, site, 0), element stride) of site_matmul's two layouts."""
    B, n, sites = p["B"], p["n"], p["sites"]
    if p["layout"] == "plane":
        sb, ss, sj = n * sites, 1, sites
    else:
        sb, ss, sj = sites * n, n, 1
    base = (np.arange(B)[:, None] * sb + np.arange(sites)[None, :] * ss).reshape(-1)
    return base, (sb, ss, sj)


def m_site_matmul(case, t, fault=None):
    p = case.p
    n = p["n"]
    base, (_, _, sj) = site_offsets(p)
    M = t["M"].T if p["trans"] else t["M"]
    if fault == "swap_hw":
        M = M.T
    v = [t["in"][base + j * sj] for j in range(n)]
    out = np.full_like(t["in"], NAN)
    for i in range(n):
        acc = np.zeros(len(base), dtype=F)
        for j in range(n):
            acc = acc + M[i, j] * v[(j + 1) % n if fault == "shift" else j]
        out[base + i * sj] = acc
    return {"out": out}


def _sites(case, x, fault=None):
    """x [B][3][H][W] -> [sites][n]: mode 0 r x r patches of a plane (entry k at row k / r, column k % r), mode 1 the three
    channels of a pixel; and the inverse."""
    p = case.p
    B, C, H, W = x.shape
    if p["mode"] == 0:
        r = p["r"]
        if fault == "swap_hw":
            x = _swap_hw(x)
            H, W = W, H
        s = x.reshape(B, C, H // r, r, W // r, r).transpose(0, 1, 2, 4, 3, 5).reshape(-1, r * r)

        def back(o):
            o = o.reshape(B, C, H // r, W // r, r, r).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, H, W)
            return _swap_hw(o) if fault == "swap_hw" else o
        return s, back
    s = x.reshape(B, 3, H * W).transpose(0, 2, 1).reshape(-1, 3)
    return s, lambda o: o.reshape(B, H * W, 3).transpose(0, 2, 1).reshape(B, 3, H, W)


def m_site_spectral(case, t, fault=None):
    p, V = case.p, t["V"]
    n = p["n"]
    c0, c1, c2, c3 = t["c"]
    xs, back = _sites(case, t["x"], fault)
    if fault == "shift":
        xs = np.roll(xs, -1, axis=0)
    if p["op"] == 0:
        dot = np.zeros(xs.shape[0], dtype=F)
        for k in range(n):
            dot = dot + V[k, 0] * xs[:, k]
        g = c0 - F(1)
        out = np.stack([xs[:, i] + (g * V[i, 0]) * dot for i in range(n)], axis=1)
        return {"out": back(out)}
    ys = None if t["y"] is None else _sites(case, t["y"], fault)[0]
    acc = np.zeros(xs.shape, dtype=F)
    for k in range(n):
        z = xs[:, k] * (c0 if k == 0 else c1)
        if ys is not None:
            z = _fma(ys[:, k], c2 if k == 0 else c3, z) if fault == "fma" else z + ys[:, k] * (c2 if k == 0 else c3)
        for i in range(n):
            acc[:, i] = acc[:, i] + V[i, k] * z
    return {"out": back(acc)}


def m_mask_mix(case, t, fault=None):
    p = case.p
    cx_m, cx_n, cy_m, cy_n = t["c"]
    x = t["x"]
    if t["mask"] is None:
        m = np.ones(x.shape, dtype=bool)
    else:
        planes = (np.arange(p["planes"]) + (1 if fault == "shift" else 0)) % p["planes_mask"]
        m = t["mask"][planes] != 0
    v = x * np.where(m, cx_m, cx_n)
    if t["y"] is not None:
        cy = np.where(m, cy_m, cy_n)
        v = _fma(t["y"], cy, v) if fault == "fma" else v + t["y"] * cy
    return {"out": v.astype(F)}


def m_mul_planes(case, t, fault=None):
    p = case.p
    planes = (np.arange(p["planes"]) + (1 if fault == "shift" else 0)) % p["planes_table"]
    return {"out": t["x"] * t["table"][planes]}


def m_axpby(case, t, fault=None):
    if t["y"] is None:
        return {"out": t["x"] * t["a"]}
    if fault == "fma":
        return {"out": _fma(t["x"], t["a"], t["y"] * t["b"])}
    return {"out": t["x"] * t["a"] + t["y"] * t["b"]}


def m_axpby_strided(case, t, fault=None):
    chw = case.p["chw"]
    x = t["x2"][:, :chw]
    if fault == "et_stride":
        x = t["x2"].reshape(-1)[:x.size].reshape(x.shape)
    if fault == "fma":
        return {"out": _fma(x, t["a"], t["y"] * t["b"])}
    return {"out": x * t["a"] + t["y"] * t["b"]}


def spectral_coef(s, a, sy, st, eta, eta_c, tie=None):
    """spectral_coef of ddnm_step.hip statement by statement, over a table s; returns (lam, d1, d2, regime) with regime
    -1 / 0 / +1 for sigma_t below / at / above thr (0 also where inactive or s == 0).  `tie` = -1 / +1 plants the tie's
    neighbouring regime."""
    s = np.asarray(s, dtype=F)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(s == 0, F(0), F(1) / s).astype(F)
        lam = np.ones_like(s)
        d1 = np.full_like(s, st * eta)
        d2 = np.full_like(s, st * eta_c)
        regime = np.zeros(s.shape, dtype=np.int8)
        if a != 0 and sy != 0:
            thr = (a * sy) * inv
            lt, gt = st < thr, st > thr
            if tie is not None:
                eq = (st == thr) & (s != 0)
                lt, gt = (lt | eq, gt) if tie < 0 else (lt, gt | eq)
            lam = np.where(lt, (((s * st) * eta_c) / a) / sy, lam)
            d2 = np.where(lt, F(0), d2)
            root = np.sqrt(st * st - ((a * a) * (sy * sy)) * (inv * inv))
            d1 = np.where(gt, root, d1)
            d2 = np.where(gt, F(0), d2)
            z = s == 0
            d1 = np.where(z, st * eta, d1)
            d2 = np.where(z, st * eta_c, d2)
            regime = np.where(z, 0, np.where(lt, -1, np.where(gt, 1, 0))).astype(np.int8)
    return lam.astype(F), d1.astype(F), d2.astype(F), regime


def m_spectral_mix(case, t, fault=None):
    tie = {"tie_lt": -1, "tie_gt": 1}.get(fault)
    lam, d1, d2, _ = spectral_coef(t["stab"], t["a"], t["sy"], t["st"], t["eta"], t["eta_c"], tie)
    if fault == "shift":
        lam, d1, d2 = (np.roll(v, 1) for v in (lam, d1, d2))
    if case.p["mode"] == 0:
        return {"out": t["x"] * lam}
    if fault == "fma":
        return {"out": _fma(t["x"], d1, t["y"] * d2)}
    return {"out": t["x"] * d1 + t["y"] * d2}


def m_renoise(case, t, fault=None):
    if fault == "fma":
        return {"xn": _fma(t["x0"], t["a"], t["noise"] * t["b"])}
    return {"xn": t["x0"] * t["a"] + t["noise"] * t["b"]}


def m_fill(case, t, fault=None):
    return {"out": np.full(case.p["n"], t["value"], dtype=F)}


def _clamp01(x):
    return np.minimum(np.maximum((x + F(1)) / F(2), F(0)), F(1))


def m_finalize_psnr(case, t, fault=None):
    """img bit for bit; `dd2` the fp32 squares the kernel accumulates in double (their float64 sum is the sse)."""
    out = {"img": _clamp01(t["x"])}
    if t["xo"] is not None:
        dd = out["img"] - _clamp01(t["xo"])
        out["dd2"] = dd * dd
    return out


def m_randn_philox(case, t, fault=None):
    p = case.p
    return {"out": host_noise(case, p["B"], p["chw"])}


def model(case, t, fault=None):
    out = globals()["m_" + case.kernel](case, t, fault)
    assert all(v.dtype == np.float32 for v in out.values()), case.name
    return out


# ----------------------------------------------------------------------------- float64 twins
def tw_x0(t):
    s = t["s"]
    return (T(t["xt"]) - T(et_of(t)) * T(s.s1)) / T(s.s2)


def tw_update(x0h, t):
    s = t["s"]
    return (x0h * T(s.a) + T(t["nz"]) * T(s.c1)) + T(et_of(t)) * T(s.c2)


def t_step_x0(case, t):
    return {"x0": tw_x0(t)}


def t_step_combine(case, t):
    p = T(t["proj"]) - T(t["apy"]) if t["apy"] is not None else T(t["proj"])
    return {"xn": tw_update(T(t["x0"]) - p * T(t["s"].lam), t)}


def t_step_denoise(case, t):
    x0 = tw_x0(t)
    return {"x0": x0, "xn": tw_update(x0 - (x0 - T(t["y"])) * T(t["s"].lam), t)}


def _t_up(v, r):
    return T(np.kron(v.v, np.ones((r, r))), np.kron(v.m, np.ones((r, r))), v.k)


def t_step_sr4(case, t):
    x0 = tw_x0(t)
    B, _, H, W = x0.v.shape
    pooled = x0.reshape(B, 3, H // 4, 4, W // 4, 4).sum((3, 5)) / T(16.0)
    corr = (pooled - T(t["y"])) * T(t["s"].lam)
    return {"x0": x0, "xn": tw_update(x0 - _t_up(corr, 4), t)}


def t_step_color(case, t):
    w, wp = color_weights(case.p["w3"])
    x0 = tw_x0(t)
    B, _, H, W = x0.v.shape
    gray = (x0[:, 0] * T(w[0]) + x0[:, 1] * T(w[1])) + x0[:, 2] * T(w[2])
    resid = (gray - T(t["y"].reshape(B, H, W))) * T(t["s"].lam)
    x0h = t_stack([x0[:, c] - resid * T(wp[c]) for c in range(3)], 1)
    return {"x0": x0, "xn": tw_update(x0h, t)}


def _y_at_pixels(case, t):
    """y scattered to image order [B][3][HW] (0 where unkept) and the kept mask [B][HW]."""
    B, HW = case.p["B"], case.p["HW"]
    mask = np.broadcast_to(t["mask"], (B, HW))
    yi = np.zeros((B, 3, HW))
    for b in range(B):
        nk = int(mask[b].sum())
        yi[b][:, mask[b]] = t["y"][b, :3 * nk].astype(np.float64).reshape(nk, 3).T
    return yi, mask


def t_step_inpaint(case, t):
    x0 = tw_x0(t)
    yi, mask = _y_at_pixels(case, t)
    shape = x0.v.shape
    m3 = np.broadcast_to(mask[:, None, :], yi.shape).reshape(shape)
    x0h = t_where(m3, x0 - (x0 - T(yi.reshape(shape))) * T(t["s"].lam), x0)
    return {"x0": x0, "xn": tw_update(x0h, t)}


t_step_inpaint_pi = t_step_inpaint


def t_avgpool(case, t):
    r = case.p["r"]
    BC, H, W = t["x"].shape
    return {"y": T(t["x"]).reshape(BC, H // r, r, W // r, r).sum((2, 4)) / T(float(r * r))}


def t_upsample(case, t):
    return {"x": _t_up(T(t["x"]), case.p["r"])}


def t_color_A(case, t):
    w, _ = color_weights(case.p["w3"])
    x = T(t["x"])
    return {"y": (x[:, 0] * T(w[0]) + x[:, 1] * T(w[1])) + x[:, 2] * T(w[2])}


def t_color_pinv(case, t):
    _, wp = color_weights(case.p["w3"])
    return {"x": T(t["y"])[:, None, :] * T(np.array(wp, dtype=np.float64)[None, :, None])}


def t_inpaint_A(case, t):
    B, HW = case.p["B"], case.p["HW"]
    mask = np.broadcast_to(t["mask"], (B, HW))
    ylen, _ = _y_dims(case, t)
    y = np.full((B, ylen), np.nan)
    for b in range(B):
        nk = int(mask[b].sum())
        y[b, :3 * nk] = t["x"][b][:, mask[b]].T.reshape(-1)
    return {"y": T(y)}


def t_inpaint_pinv(case, t):
    return {"x": T(_y_at_pixels(case, t)[0])}


t_inpaint_A_pi, t_inpaint_pinv_pi = t_inpaint_A, t_inpaint_pinv


def t_patchify(case, t):
    p = case.p
    P, D, ps = p["planes"], p["D"], p["ps"]
    n = D // ps
    src = t["src"].astype(np.float64)
    fwd = src.reshape(P, n, ps, n, ps).transpose(0, 1, 3, 2, 4).reshape(-1)
    inv = src.reshape(P, n, n, ps, ps).transpose(0, 1, 3, 2, 4).reshape(-1)
    return {"forward": T(fwd), "inverse": T(inv), "round_trip": T(src)}


def t_gather_scale(case, t):
    p = case.p
    B, n_in, n_out = p["B"], p["n_in"], p["n_out"]
    pad = np.concatenate([t["in"].astype(np.float64), np.zeros((B, max(n_out, 1)))], axis=1)
    v = T(pad[:, :n_out] if t["idx"] is None else pad[:, np.where(t["idx"] >= 0, t["idx"], n_in)])
    return {"out": v * T(t["scale"]) if t["scale"] is not None else v}


def t_site_matmul(case, t):
    p = case.p
    n = p["n"]
    base, (_, _, sj) = site_offsets(p)
    M = t["M"].T if p["trans"] else t["M"]
    idx = base[:, None] + np.arange(n)[None, :] * sj
    prod = T(M[None, :, :]) * T(t["in"][idx][:, None, :])       # [site][i][j]
    o = prod.sum(2)
    v, m = np.full(t["in"].shape, np.nan), np.zeros(t["in"].shape)
    v[idx], m[idx] = o.v, o.m
    return {"out": T(v, m, o.k)}


def t_site_spectral(case, t):
    p, V = case.p, t["V"]
    c0, c1, c2, c3 = (T(v) for v in t["c"])
    xs, back = _sites(case, t["x"].astype(np.float64))
    xs = T(xs)
    v0 = T(V[:, 0][None, :])
    if p["op"] == 0:
        dot = (v0 * xs).sum(1)
        o = xs + ((c0 - T(1.0)) * v0) * dot[:, None]
    else:
        n = p["n"]
        cx = T(np.array([c0.v] + [c1.v] * (n - 1))[None, :])
        z = xs * cx
        if t["y"] is not None:
            cy = T(np.array([c2.v] + [c3.v] * (n - 1))[None, :])
            z = z + T(_sites(case, t["y"].astype(np.float64))[0]) * cy
        o = (T(V[None, :, :]) * z[:, None, :]).sum(2)
    return {"out": T(back(o.v), back(o.m), o.k)}


def t_mask_mix(case, t):
    p = case.p
    cx_m, cx_n, cy_m, cy_n = (float(v) for v in t["c"])
    m = np.ones(t["x"].shape, dtype=bool) if t["mask"] is None else np.tile(t["mask"], (p["planes"] // p["planes_mask"], 1)) != 0
    v = T(t["x"]) * T(np.where(m, cx_m, cx_n))
    if t["y"] is not None:
        v = v + T(t["y"]) * T(np.where(m, cy_m, cy_n))
    return {"out": v}


def t_mul_planes(case, t):
    p = case.p
    return {"out": T(t["x"]) * T(np.tile(t["table"], (p["planes"] // p["planes_table"], 1)))}


def t_axpby(case, t):
    v = T(t["x"]) * T(t["a"])
    return {"out": v + T(t["y"]) * T(t["b"]) if t["y"] is not None else v}


def t_axpby_strided(case, t):
    return {"out": T(t["x2"][:, :case.p["chw"]]) * T(t["a"]) + T(t["y"]) * T(t["b"])}


def t_spectral_mix(case, t):
    """The rule in the words of the kernel's header, per regime; the regime itself is the fp32 comparison (a discontinuity
    is not a rounding)."""
    a, sy, st, eta, eta_c = (T(t[k]) for k in ("a", "sy", "st", "eta", "eta_c"))
    regime = spectral_coef(t["stab"], t["a"], t["sy"], t["st"], t["eta"], t["eta_c"])[3]
    s = t["stab"].astype(np.float64)
    safe = np.where(s == 0, 1.0, s)
    inv = T(1.0) / T(safe)
    lam = t_where(regime < 0, T(safe) * st * eta_c / a / sy if float(t["a"]) != 0 and float(t["sy"]) != 0 else T(1.0), T(1.0))
    arg = st * st - a * a * (sy * sy) * (inv * inv)
    root = T(np.where(regime > 0, arg.v, 1.0), np.where(regime > 0, arg.m, 1.0), arg.k).sqrt()
    d1 = t_where(regime > 0, root, st * eta)
    d2 = t_where(regime != 0, T(0.0), st * eta_c)
    x = T(t["x"])
    if case.p["mode"] == 0:
        return {"out": x * lam[None, :]}
    return {"out": x * d1[None, :] + T(t["y"]) * d2[None, :]}


def t_renoise(case, t):
    return {"xn": T(t["x0"]) * T(t["a"]) + T(t["noise"]) * T(t["b"])}


def t_fill(case, t):
    return {"out": T(np.full(case.p["n"], float(t["value"])))}


def _t_clamp01(x):
    h = (T(x) + T(1.0)) / T(2.0)
    return T(np.clip(h.v, 0.0, 1.0), np.clip(h.m, 0.0, None), h.k)


def t_finalize_psnr(case, t):
    out = {"img": _t_clamp01(t["x"])}
    if t["xo"] is not None:
        dd = out["img"] - _t_clamp01(t["xo"])
        out["dd2"] = dd * dd
    return out


def t_randn_philox(case, t):
    return {"out": T(host_noise(case, case.p["B"], case.p["chw"]))}


def twin(case, t):
    return globals()["t_" + case.kernel](case, t)


def sse_bar(chw, dd2):
    """finalize_psnr's sse against the float64 sum of the fp32 squares `dd2` [B][chw]: the squares enter exactly, the
    double additions -- chw per-thread terms, the wave and block reductions and 64 atomics in no fixed order -- are at most
    chw + 64 roundings of 2^-53 each."""
    return (chw + 64) * 2.0 ** -53 * dd2.astype(np.float64).sum(axis=1)


# ----------------------------------------------------------------------------- case table
def _fused(kernel, tag, why, B, lam, eta, **p):
    return Case(f"{kernel}_{tag}", kernel, f"{why}; B = {B}, lambda = {lam}, eta = {eta}", dict(B=B, lam=lam, eta=eta, **p))


PI_STRIDE = 188          # 3 * 60 = 180 entries of the all-kept image, padded by 8 (NaN)


def _cases():
    c = []
    # ---- fused steps: every case runs with every noise source, et stride and x0 option (test_gpu_step_edges.py)
    for tag, shape, B, lam, eta in (("chw4", (1, 2, 2), 1, 1.0, 0.85), ("chw12", (3, 2, 2), 3, 0.3, 1.0),
                                    ("chw480", (3, 20, 8), 3, 1.0, 0.0)):
        chw = shape[0] * shape[1] * shape[2]
        c.append(_fused("step_x0", tag, f"chw = {chw}: one float4 per image / three / 120 (no multiple of a wave)", B, lam, eta,
                        shape=shape, chw=chw))
        c.append(_fused("step_denoise", tag, f"chw = {chw}", B, lam, eta, shape=shape, chw=chw))
        c.append(_fused("step_combine", tag, f"chw = {chw}, apy NULL", B, lam, eta, shape=shape, chw=chw, apy=False))
    c.append(_fused("step_combine", "chw12_apy", "chw = 12, apy given (proj - apy first)", 3, 1.0, 0.85, shape=(3, 2, 2), chw=12,
                    apy=True))
    c.append(_fused("step_combine", "chw480_apy", "chw = 480, apy given, lambda != 1", 3, 0.3, 0.85, shape=(3, 20, 8), chw=480,
                    apy=True))
    c.append(_fused("step_combine", "chw4_b1_lam", "chw = 4, one image, lambda != 1, eta = 1 (c2 == 0)", 1, 0.3, 1.0,
                    shape=(1, 2, 2), chw=4, apy=False))
    c.append(_fused("step_x0", "chw12_b1", "chw = 12, one image", 1, 1.0, 0.85, shape=(3, 2, 2), chw=12))
    c.append(_fused("step_denoise", "chw480_b1", "chw = 480, one image, lambda != 1, eta = 0 (c1 == 0)", 1, 0.3, 0.0,
                    shape=(3, 20, 8), chw=480))
    for (H, W), B, lam, eta, why in (((4, 4), 1, 1.0, 0.85, "one patch per plane"),
                                     ((4, 12), 3, 0.3, 1.0, "one patch row, W > H: row stride W, not H"),
                                     ((12, 4), 3, 1.0, 0.0, "one patch column, H > W"),
                                     ((8, 20), 3, 0.3, 0.85, "2 x 5 patches, H != W, 30 patches per image")):
        c.append(_fused("step_sr4", f"{H}x{W}", f"(H, W) = ({H}, {W}): {why}", B, lam, eta, H=H, W=W))
    c.append(_fused("step_sr4", "8x20_b1", "(H, W) = (8, 20), one image, eta = 1", 1, 1.0, 1.0, H=8, W=20))
    for tag, hw, B, lam, eta, w3 in (("hw4", (2, 2), 1, 1.0, 0.85, None), ("hw12_w", (3, 4), 3, 0.3, 1.0, W_CUSTOM),
                                     ("hw160", (20, 8), 3, 1.0, 0.0, None), ("hw160_w", (20, 8), 3, 0.3, 0.85, W_CUSTOM),
                                     ("hw12_b1", (3, 4), 1, 0.3, 0.0, None), ("hw4_w", (2, 2), 3, 1.0, 1.0, W_CUSTOM)):
        c.append(_fused("step_color", tag, f"HW = {hw[0] * hw[1]}, {'custom w3_host' if w3 else 'default weights'}", B, lam, eta,
                        hw=hw, HW=hw[0] * hw[1], w3=w3))
    for tag, hw, mask, B, lam, eta in (("hw4_one", (2, 2), "one", 1, 1.0, 0.85), ("hw60_all", (6, 10), "all", 3, 0.3, 1.0),
                                       ("hw60_part", (6, 10), "part", 3, 1.0, 0.0), ("hw60_part_lam", (6, 10), "part", 1, 0.3, 0.85)):
        c.append(_fused("step_inpaint", tag, f"shared mask, HW = {hw[0] * hw[1]}, kept: {mask}", B, lam, eta, hw=hw,
                        HW=hw[0] * hw[1], mask=mask))
    for tag, B, masks, lam, eta in (("b3", 3, ("one", "all", "part"), 0.3, 0.85), ("b3_eta1", 3, ("part", "one", "all"), 1.0, 1.0),
                                    ("b1_eta0", 1, ("part",), 0.3, 0.0)):
        c.append(_fused("step_inpaint_pi", tag, f"one mask per image, HW = 60, kept: {', '.join(masks)}; y rows of {PI_STRIDE} "
                        "with NaN padding", B, lam, eta, hw=(6, 10), HW=60, masks=masks, y_stride=PI_STRIDE))
    # ---- operators
    for H, W, r, why in ((6, 9, 3, "odd r, H != W"), (4, 12, 4, "one output row"), (5, 7, 1, "r = 1: the identity"),
                         (16, 32, 16, "256-term window"), (8, 4, 2, "H > W")):
        for k in ("avgpool", "upsample"):
            c.append(Case(f"{k}_{H}x{W}_r{r}", k, f"(H, W, r) = ({H}, {W}, {r}): {why}; BC = 5", dict(BC=5, H=H, W=W, r=r)))
    for HW in (1, 7, 160):
        for w3, wt in ((None, "dflt"), (W_CUSTOM, "w")):
            for k in ("color_A", "color_pinv"):
                c.append(Case(f"{k}_hw{HW}_{wt}", k, f"HW = {HW}, {'custom' if w3 else 'default'} weights, B = 3",
                              dict(B=3, HW=HW, w3=w3)))
    for k in ("inpaint_A", "inpaint_pinv"):
        for tag, HW, mask in (("hw4_one", 4, "one"), ("hw60_all", 60, "all"), ("hw60_part", 60, "part")):
            c.append(Case(f"{k}_{tag}", k, f"shared mask, HW = {HW}, kept: {mask}, B = 3", dict(B=3, HW=HW, mask=mask)))
        c.append(Case(f"{k}_pi", k + "_pi", f"one mask per image (one / all / part kept), HW = 60, rows of {PI_STRIDE} with NaN "
                      "padding that stays NaN", dict(B=3, HW=60, masks=("one", "all", "part"), y_stride=PI_STRIDE)))
    for D, ps in ((4, 4), (12, 4), (24, 8), (64, 32)):
        c.append(Case(f"patchify_d{D}_ps{ps}", "patchify", f"(D, ps) = ({D}, {ps}), 5 planes: forward, inverse, round trip",
                      dict(planes=5, D=D, ps=ps)))
    for idx in (False, True):
        for scale in (False, True):
            for n_in, n_out, rel in ((35, 50, "above"), (35, 20, "below"), (35, 35, "equal")):
                if idx and rel != "above":
                    continue
                tag = f"{'idx' if idx else 'noidx'}_{rel}{'_scale' if scale else ''}"
                c.append(Case(f"gather_scale_{tag}", "gather_scale",
                              f"idx {'a permutation with a third -1' if idx else 'NULL'}, n_out {rel} n_in, "
                              f"{'with' if scale else 'without'} scale, B = 3", dict(B=3, n_in=n_in, n_out=n_out, idx=idx, scale=scale)))
    for n in (1, 3, 4, 16):
        for trans in (0, 1):
            c.append(Case(f"site_matmul_n{n}_t{trans}", "site_matmul", f"site-major layout, n = {n}, trans = {trans}, 2 x 150 sites "
                          "(no multiple of 256, two workgroups)", dict(B=2, n=n, sites=150, layout="site", trans=trans)))
    for trans in (0, 1):
        c.append(Case(f"site_matmul_plane_t{trans}", "site_matmul", f"plane layout (ss = 1, sj = H W, sb = 3 H W), n = 3, "
                      f"trans = {trans}, H W = 150", dict(B=2, n=3, sites=150, layout="plane", trans=trans)))
    for H, W, r in ((4, 6, 2), (8, 4, 4), (6, 9, 3)):
        for op, y in ((0, False), (1, False), (1, True)):
            c.append(Case(f"site_spectral_m0_{H}x{W}_r{r}_op{op}{'_y' if y else ''}", "site_spectral",
                          f"mode 0, (H, W, r) = ({H}, {W}, {r}), op {op}, y {'given' if y else 'NULL'}, B = 2",
                          dict(B=2, H=H, W=W, r=r, n=r * r, mode=0, op=op, y=y)))
    for H, W in ((1, 1), (5, 7)):
        for op, y in ((0, False), (1, False), (1, True)):
            c.append(Case(f"site_spectral_m1_hw{H * W}_op{op}{'_y' if y else ''}", "site_spectral",
                          f"mode 1, H W = {H * W}, op {op}, y {'given' if y else 'NULL'}, B = 2",
                          dict(B=2, H=H, W=W, r=1, n=3, mode=1, op=op, y=y)))
    for pm in (0, 1, 3):
        for y in (False, True):
            c.append(Case(f"mask_mix_pm{pm}{'_y' if y else ''}", "mask_mix",
                          f"{'mask NULL' if pm == 0 else f'planes_mask = {pm} (zeros of both signs)'} over 6 planes of 35, "
                          f"y {'given' if y else 'NULL'}", dict(planes=6, plane_elems=35, planes_mask=pm, y=y)))
    for pt in (1, 3):
        c.append(Case(f"mul_planes_pt{pt}", "mul_planes", f"planes_table = {pt} over 6 planes of 35",
                      dict(planes=6, plane_elems=35, planes_table=pt)))
    for n in (1, 257):
        for y in (False, True):
            c.append(Case(f"axpby_n{n}{'_y' if y else ''}", "axpby", f"n = {n}, y {'given' if y else 'NULL'}", dict(n=n, y=y)))
        c.append(Case(f"fill_n{n}", "fill", f"n = {n}", dict(n=n)))
    c.append(Case("axpby_strided", "axpby_strided", "x_bstride = 2 chw, chw = 35, B = 3", dict(B=3, chw=35)))
    for mode in (0, 1):
        c.append(Case(f"spectral_mix_m{mode}", "spectral_mix", f"mode {mode}: table with zeros, the exact tie sigma_t == thr and "
                      "entries on both sides; 3 planes of 35", dict(planes=3, plane_elems=35, mode=mode, a=0.7211, sigma_y=0.1)))
        c.append(Case(f"spectral_mix_m{mode}_a0", "spectral_mix", f"mode {mode}, a == 0: no regime change",
                      dict(planes=3, plane_elems=35, mode=mode, a=0.0, sigma_y=0.1)))
        c.append(Case(f"spectral_mix_m{mode}_sy0", "spectral_mix", f"mode {mode}, sigma_y == 0: no regime change",
                      dict(planes=3, plane_elems=35, mode=mode, a=0.7211, sigma_y=0.0)))
    for n in (4, 1028):
        c.append(Case(f"renoise_n{n}", "renoise", f"n = {n}: one float4 / 257 (two workgroups)", dict(n=n)))
    for chw in (1, 3 * 32 * 32, 16384 + 5):
        for tag, img, xo in (("both", True, True), ("noimg", False, True), ("noorig", True, False)):
            c.append(Case(f"finalize_psnr_chw{chw}_{tag}", "finalize_psnr",
                          f"chw = {chw} ({'fewer elements than threads' if chw == 1 else 'under one trip' if chw < 16384 else 'five elements into the second trip of the 64 x 256 threads of an image'}), "
                          f"img {'given' if img else 'NULL'}, x_orig {'given' if xo else 'NULL'}, B = 3, both clamps",
                          dict(B=3, chw=chw, img=img, x_orig=xo)))
    for chw in (4, 12):
        for base in (0, 5):
            c.append(Case(f"randn_philox_chw{chw}_base{base}", "randn_philox", f"chw = {chw}, B = 3, image_base = {base}",
                          dict(B=3, chw=chw, image_base=base)))
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FUSED = ("step_sr4", "step_color", "step_inpaint", "step_inpaint_pi", "step_denoise")       # x0 optional, three noise sources
NOISY = FUSED + ("step_combine",)


def variants(kernel):
    """The (noise source, et stride, x0 option) launches the GPU test makes of EVERY case of a fused-step kernel: step_x0
    takes no noise and step_combine writes no x0 (None there)."""
    noise = NOISE_SOURCES if kernel in NOISY else (None,)
    x0 = X0_OPTIONS if kernel in FUSED else (None,)
    return [(n, e, x) for n in noise for e in ET_STRIDES for x in x0]


def faults_of(case):
    """The planted faults this case is meant to catch (host test: each changes at least one output bit)."""
    k, p = case.kernel, case.p
    f = []
    if k.startswith("step_"):
        f += ["fma"]
        if p["B"] > 1 and not (k == "step_combine" and p["eta"] == 1.0):      # combine reads et through c2 only
            f += ["et_stride"]
        if k in NOISY and p["B"] > 1 and p["eta"] != 0.0:
            f += ["key_row"]
        if k != "step_x0" and p["lam"] != 1.0:
            f += ["lambda_operand"]
        if k == "step_sr4":
            f += ["colmajor"] + (["swap_hw"] if p["H"] != p["W"] else []) + ["shift"]
        if k in ("step_color", "step_denoise"):
            f += ["shift"]
        if k in ("step_inpaint", "step_inpaint_pi"):
            kinds = p["masks"] if "masks" in p else (p["mask"],)
            f += ["swap_kept"] if any(m != "all" for m in kinds) else []
            f += ["shift"] if any(m != "one" for m in kinds) else []
    elif k == "avgpool":
        f += (["colmajor"] if p["r"] > 1 else []) + (["swap_hw"] if p["r"] > 1 else [])
    elif k == "upsample":
        f += ["shift"] + (["swap_hw"] if p["r"] > 1 else [])
    elif k == "color_A":
        f += ["fma", "shift"]
    elif k == "color_pinv":
        f += ["shift"]
    elif k in ("inpaint_A", "inpaint_pinv", "inpaint_A_pi", "inpaint_pinv_pi"):
        kinds = p["masks"] if "masks" in p else (p["mask"],)
        f += ["shift"] + (["swap_kept"] if any(m != "all" for m in kinds) else [])
    elif k == "patchify":
        f += ["shift", "swap_hw"] if p["D"] > p["ps"] else []
    elif k == "gather_scale":
        f += ["shift"]
    elif k == "site_matmul":
        f += ["shift", "swap_hw"] if p["n"] > 1 else []
    elif k == "site_spectral":
        f += ["shift"] if p["B"] * 3 * p["H"] * p["W"] > p["n"] else []
        f += ["swap_hw"] if p["mode"] == 0 else []
        f += ["fma"] if p["op"] == 1 and p["y"] else []
    elif k == "mask_mix":
        f += (["fma"] if p["y"] else []) + (["shift"] if p["planes_mask"] == 3 else [])
    elif k == "mul_planes":
        f += ["shift"] if p["planes_table"] == 3 else []
    elif k == "axpby":
        f += ["fma"] if p["y"] else []
    elif k == "axpby_strided":
        f += ["fma", "et_stride"]
    elif k == "spectral_mix":
        active = p["a"] != 0.0 and p["sigma_y"] != 0.0
        f += (["tie_lt", "shift"] + (["tie_gt"] if p["mode"] == 1 else []) if active else []) + (["fma"] if p["mode"] == 1 and not active else [])
    elif k == "renoise":
        f += ["fma"]
    return f


# ----------------------------------------------------------------------------- second-trip launches (GPU test)
# One launch per kernel shape class with GRID_CAP * BLOCK < work items <= 1.01 GRID_CAP * BLOCK: the threads of the first
# workgroups run the loop body a second time.  B = 2 for the kernels indexed per image: the second trip starts in image 1.
_ST4 = 1048584 * 4           # chw: 2 * 1048584 = 2097168 float4 items = 8192 * 256 + 16
SECOND_TRIP = {
    "step_x0": dict(B=2, chw=_ST4),
    "step_combine": dict(B=2, chw=_ST4),
    "step_denoise": dict(B=2, chw=_ST4),
    "randn_philox": dict(B=2, chw=_ST4),
    "step_color": dict(B=2, HW=_ST4),
    "step_inpaint": dict(B=2, HW=_ST4),
    "renoise": dict(n=_ST4 * 2),
    "patchify": dict(planes=2049, D=64, ps=16),
    "step_sr4": dict(B=1, H=3348, W=3348),
    "upsample": dict(BC=2, H=1026, W=1024, r=2),
    "gather_scale": dict(B=2, n_in=1000000, n_out=1048600, idx=True, scale=True),
}
