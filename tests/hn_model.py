"""CPU model of the two per-entry-noise DDNM+ step kernels of csrc/ddnm_step.hip (step_plus_mosaic_hn_kernel,
step_plus_denoise_hn_kernel; entry points ddnm_step_plus_mosaic_hn_f32 / ddnm_step_plus_denoise_hn_f32), in the manner of
tests/step_model.py, whose float32 / `T` arithmetic it shares.  No GPU import; tests/test_hn_host.py checks this file on
the CPU, tests/test_gpu_hn.py holds the kernels to it.

  model(case, t)   the kernel -- and the host's part of its arguments: the map's doubling, the double-evaluated sigma_t^2,
                   c1, c2 -- restated in numpy float32, one rounding per * + - / sqrt, in the order of the source
                   (contraction into FMA is off there).  The kernels must equal it BIT FOR BIT.  `fault=` plants one of
                   FAULTS; every fault is noticed by at least one case.
  twin(case, t)    the same formula in float64 with step_model's `T` error bars; each entry's branch is taken from the
                   model's fp32 comparison, so a rounding-level tie cannot flip a branch between the two.
  coef64(...)      the per-entry table in float64: (a lambda, d1, d2) of measured entries with sigma_j, from the branch
                   codes of `branches32` (the identity test, the loop test's oracle operator).
  CASES            the union of shapes, strides, sigma sources, eta and alpha-bar values the issue asks for.

Per measured entry, a = sqrt_at_next, thr = a sigma_j (sigma_j on the engine's [-1, 1] scale):
  sigma_j == 0 or a == 0 : (a lambda, d1, d2) = (a, c1, c2)            BR_PASS
  sigma_t < thr          : (a (c2 / thr), c1, 0)                       BR_BELOW
  sigma_t > thr          : (a, sqrt(max(sigma_t2 - thr thr, 0)), 0)    BR_ABOVE
  sigma_t == thr         : (a, c1, c2)                                 BR_PASS
  x_{t-1} = ((a x0 - a lambda (x0 - y)) + d1 n) + d2 eps;   unmeasured entries (the mosaic's other two planes): (0, c1, c2)."""
from typing import NamedTuple

import numpy as np

from tests.step_model import EPS, F, T, _fma, et_of, t_where

FAULTS = ("fma", "tie_lt", "tie_gt", "sigma_not_doubled", "shot_unclamped", "map_per_image", "et_stride")
BR_PASS, BR_BELOW, BR_ABOVE = 0, 1, 2
AT = 0.45                                   # alpha-bar of t in every case (only x0 depends on it)
SIGMA_SOURCES = ("map", "shot")
NOISE_SOURCES = ("tensor", "in_kernel", "keyed")


class Case(NamedTuple):
    name: str
    kernel: str          # "mosaic" | "denoise"
    why: str
    p: dict              # B, d, pattern (mosaic), sigma ("map" | "shot"), eta, at_next, six, s / g (shot, [0, 1] scale)


class Sc(NamedTuple):
    s1: np.float32       # sqrt(1 - abar_t)
    s2: np.float32       # sqrt(abar_t)
    a: np.float32        # sqrt(abar_next)
    st: np.float32       # sigma_t = sqrt(1 - abar_next)
    st2: np.float32      # sigma_t^2, c1 = sigma_t eta, c2 = sigma_t sqrt(1 - eta^2): evaluated in double on the host from
    c1: np.float32       # the fp32 sigma_t and rounded once (svd_operators._PerEntryNoisePlus.ddnm_plus_step_hn)
    c2: np.float32


def scalars(at_next, eta, at=AT):
    """The scalars of one step: fp32 tensor arithmetic for the square roots (ops.step_scalars, the loop's sigma_t), Python
    doubles rounded once for what the hook derives from sigma_t."""
    at, nx = F(at), F(at_next)
    st = np.sqrt(F(1) - nx)
    sd = float(st)
    return Sc(np.sqrt(F(1) - at), np.sqrt(at), np.sqrt(nx), st, F(sd ** 2), F(sd * eta), F(sd * (1 - eta ** 2) ** 0.5))


# ----------------------------------------------------------------------------- cases and inputs
def _cases():
    c = []

    def add(name, kernel, why, **p):
        p.setdefault("B", 3)
        c.append(Case(name, kernel, why, p))

    add("mosaic_xtrans16_map_tie", "mosaic", "period 6 does not divide 16; a = 0.5 exactly: sigma_j = 0, below, above and "
        "an exact tie in one launch; six-channel et", d=16, pattern="xtrans", sigma="map", eta=0.85, at_next=0.25, six=True)
    add("mosaic_rggb32_shot", "mosaic", "more than one workgroup; shot + read with y outside [-1, 1] (clamp), both branches; "
        "eta = 1 (c2 == 0)", d=32, pattern="rggb", sigma="shot", eta=1.0, at_next=0.99, six=False, s=0.02, g=0.01)
    add("mosaic_rggb32_map", "mosaic", "map at a small sigma_t, eta = 0 (c1 == 0)", d=32, pattern="rggb", sigma="map", eta=0.0,
        at_next=0.99, six=False)
    add("mosaic_xtrans16_shot", "mosaic", "shot + read at a = 0.5, both branches, six-channel et", d=16, pattern="xtrans",
        sigma="shot", eta=0.85, at_next=0.25, six=True, s=0.5, g=3.0)
    add("denoise16_map_tie", "denoise", "all entries measured; sigma_j = 0, below, above and an exact tie; eta = 0", d=16,
        sigma="map", eta=0.0, at_next=0.25, six=False)
    add("denoise16_shot", "denoise", "shot + read with the clamp taken, six-channel et", d=16, sigma="shot", eta=0.85,
        at_next=0.99, six=True, s=0.02, g=0.01)
    add("denoise16_map", "denoise", "map at a small sigma_t, eta = 1, six-channel et", d=16, sigma="map", eta=1.0, at_next=0.99,
        six=True)
    add("denoise16_shot_a05", "denoise", "shot + read at a = 0.5, eta = 1", d=16, sigma="shot", eta=1.0, at_next=0.25, six=False,
        s=0.5, g=3.0)
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def cfa_codes(name, d):
    """[d*d] channel code of every pixel (0 = R, 1 = G, 2 = B)."""
    from tests.test_mosaic_host import numpy_cfa
    pat = numpy_cfa(name)
    r, c = np.divmod(np.arange(d * d), d)
    return pat[r % pat.shape[0], c % pat.shape[1]]


def measurement_size(case):
    d = case.p["d"]
    return d * d if case.kernel == "mosaic" else 3 * d * d


def host_noise(case):
    from oracle import philox
    lo, hi, it, base = noise_key(case)
    B, d = case.p["B"], case.p["d"]
    return philox.randn((hi << 32) | lo, B, 3 * d * d, it, base).astype(F).reshape(B, 3, d, d)


def noise_key(case):
    """(seed_lo, seed_hi, iteration, image base) of a case's Philox draw."""
    import zlib
    h = zlib.crc32(("hn:" + case.name).encode())
    return h, (h * 2654435761) & 0xFFFFFFFF, 3 + h % 5, 5


def make_inputs(case, nz=None):
    """Seeded inputs of a case (never written to): xt, et6 [B][6][d][d] (the kernels read [:, :3]: contiguous cases copy it),
    y [B][n], the [0, 1]-scale map row [n] or (s, g), the step's scalars and its noise `nz` (given: the device's draw)."""
    import zlib
    p = case.p
    B, d, n = p["B"], p["d"], measurement_size(case)
    r = np.random.default_rng(zlib.crc32(case.name.encode()))
    sc = scalars(p["at_next"], p["eta"])
    t = {"s": sc, "xt": r.standard_normal((B, 3, d, d)).astype(F), "et6": r.standard_normal((B, 6, d, d)).astype(F)}
    if p["sigma"] == "shot":
        t["y"] = r.uniform(-1.3, 1.3, (B, n)).astype(F)          # below -1 and above +1: the clamp is taken
        assert (t["y"] < -1).any() and (t["y"] > 1).any()
        t["shot"] = (float(p["s"]), float(p["g"]))
    else:
        t["y"] = r.uniform(-1.0, 1.0, (B, n)).astype(F)
        # the row: a quarter each of 0, sigma_j far below / far above the threshold sigma_t / a, and the threshold itself
        # -- at a = 0.5 (at_next = 0.25) the engine's 2 * row is sigma_t / a exactly, so thr == sigma_t in fp32: an exact tie
        st01 = float(sc.st) / float(sc.a) / 2
        kind = r.integers(0, 4, n)
        row = np.select([kind == 0, kind == 1, kind == 2], [0.0, st01 * r.uniform(0.05, 0.9, n), st01 * r.uniform(1.1, 4.0, n)],
                        st01).astype(F)
        if p["at_next"] == 0.25:
            assert sc.a == F(0.5) and (sc.a * (row[kind == 3] * F(2)) == sc.st).all()
        t["row"], t["kind"] = row, kind
    t["nz"] = host_noise(case) if nz is None else np.asarray(nz, dtype=F).reshape(B, 3, d, d)
    return t


# ----------------------------------------------------------------------------- fp32 restatement
def sigma32(kind, y, row=None, shot=None, fault=None):
    """sigma_j [B][n] fp32 on the engine's scale, as the kernel has it in registers: `kind` "map" with the [0, 1]-scale
    `row` [n], or "shot" with `shot` = (s, g) and the measurement `y` [B][n] itself."""
    B, n = y.shape
    two = F(1) if fault == "sigma_not_doubled" else F(2)
    if kind == "map":
        row = np.asarray(row, dtype=F) * two                    # NoiseModel.device_row: doubled on the host, exact
        if fault == "map_per_image":                            # image b reading past the shared row: another row
            return np.stack([np.roll(row, 4 * b) for b in range(B)])
        return np.broadcast_to(row, (B, n)).copy()
    s, g = shot
    s2, g = F(s ** 2), F(g)                                      # doubles of the host, rounded once by the call
    u = (np.asarray(y, dtype=F) + F(1)) * F(0.5)
    if fault != "shot_unclamped":
        u = np.where(u < F(0), F(0), np.where(u > F(1), F(1), u))
    with np.errstate(invalid="ignore"):
        v = _fma(u, g, s2) if fault == "fma" else s2 + g * u
        return two * np.sqrt(v)


def sigma_of(case, t, fault=None):
    return sigma32(case.p["sigma"], t["y"], t.get("row"), t.get("shot"), fault)


def branches32(a, sig, st, fault=None):
    """Branch code per entry from the kernel's fp32 comparison of thr = a * sigma_j with sigma_t."""
    thr = F(a) * sig
    with np.errstate(invalid="ignore"):
        below, above = F(st) < thr, F(st) > thr
        if fault == "tie_lt":
            below = F(st) <= thr
        if fault == "tie_gt":
            above = (F(st) >= thr) & ~below
    br = np.where(below, BR_BELOW, np.where(above, BR_ABOVE, BR_PASS))
    return np.where((sig == 0) | (F(a) == 0), BR_PASS, br), thr


def coef32(sc, sig, fault=None):
    """(a lambda, d1, d2, branch) of measured entries: hn_coef4 of the source."""
    br, thr = branches32(sc.a, sig, sc.st, fault)
    with np.errstate(divide="ignore", invalid="ignore"):
        al_below = sc.a * (sc.c2 / thr)
        v = (_fma(-thr, thr, sc.st2) if fault == "fma" else sc.st2 - thr * thr)
        d1_above = np.sqrt(np.where(v > 0, v, F(0)))
    al = np.where(br == BR_BELOW, al_below, sc.a).astype(F)
    d1 = np.where(br == BR_ABOVE, d1_above, sc.c1).astype(F)
    d2 = np.where(br == BR_PASS, sc.c2, F(0)).astype(F)
    return al, d1, d2, br


def expand(kernel, pattern, d, v, fill):
    """Per-measurement values [B][n] -> per image entry [B][3][d][d]: `fill` on the planes a mosaic pixel does not sample."""
    B = v.shape[0]
    if kernel == "denoise":
        return v.reshape(B, 3, d, d)
    m = (np.arange(3)[:, None] == cfa_codes(pattern, d)[None, :]).reshape(1, 3, d, d)
    return np.where(m, v.reshape(B, 1, d, d), fill)


def _expand(case, v, fill):
    return expand(case.kernel, case.p.get("pattern"), case.p["d"], v, fill)


def measured_mask(case):
    B, d = case.p["B"], case.p["d"]
    return _expand(case, np.ones((B, measurement_size(case)), dtype=bool), False)


def model(case, t, fault=None):
    sc = t["s"]
    et = et_of(t, fault)
    x0 = (t["xt"] - et * sc.s1) / sc.s2
    if fault == "fma":
        x0 = (_fma(et, -sc.s1, t["xt"]) / sc.s2).astype(F)
    al, d1, d2, br = coef32(sc, sigma_of(case, t, fault), fault)
    al, d1, d2 = _expand(case, al, F(0)), _expand(case, d1, sc.c1), _expand(case, d2, sc.c2)
    y = _expand(case, t["y"], F(0)) if case.kernel == "denoise" else np.broadcast_to(
        t["y"].reshape(case.p["B"], 1, case.p["d"], case.p["d"]), x0.shape)
    if fault == "fma":
        xn = _fma(et, d2, _fma(t["nz"], d1, _fma(x0, sc.a, -((x0 - y) * al))))
    else:
        xn = ((x0 * sc.a - (x0 - y) * al) + t["nz"] * d1) + et * d2
    out = {"x0": x0.astype(F), "xn": xn.astype(F), "branch": _expand(case, br, -1)}
    assert out["x0"].dtype == out["xn"].dtype == np.float32
    return out


# ----------------------------------------------------------------------------- float64 table and twin
def coef64(a, sig, st, eta, br):
    """(a lambda, d1, d2) in float64 for measured entries with sigma_j = `sig`, branch codes `br` given."""
    a, sig, st = np.float64(a), np.asarray(sig, np.float64), np.float64(st)
    c1, c2 = st * eta, st * (1 - eta ** 2) ** 0.5
    with np.errstate(divide="ignore", invalid="ignore"):
        al = np.where(br == BR_BELOW, c2 / sig, a)               # a * (c2 / (a sigma_j))
        d1 = np.where(br == BR_ABOVE, np.sqrt(np.maximum(st * st - (a * sig) ** 2, 0.0)), c1)
    d2 = np.where(br == BR_PASS, c2, 0.0)
    return al, d1, d2


def t_div(n, d):
    """n / d of two rounded quantities: the divisor's relative error k_d eps m_d / |d| carries over."""
    ad = np.abs(d.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        return T(n.v / d.v, n.m / ad * (d.m / ad), n.k + d.k + 1)


def twin(case, t):
    sc = t["s"]
    B, n = t["y"].shape
    if case.p["sigma"] == "map":
        sig = T(np.broadcast_to(t["row"].astype(np.float64) * 2, (B, n)))
    else:
        s, g = t["shot"]
        u = (T(t["y"]) + T(1.0)) * T(0.5)
        u = t_where(u.v < 0, T(np.zeros_like(u.v)), t_where(u.v > 1, T(np.ones_like(u.v)), u))
        sig = T(2.0) * (T(np.float64(F(s ** 2))) + T(np.float64(F(g))) * u).sqrt()
    br = branches32(sc.a, sigma_of(case, t), sc.st)[0]
    thr = T(sc.a) * sig
    al = t_where(br == BR_BELOW, T(sc.a) * t_div(T(sc.c2), thr), T(np.float64(sc.a)))
    d1 = t_where(br == BR_ABOVE, t_where((T(sc.st2) - thr * thr).v > 0, T(sc.st2) - thr * thr, T(0.0)).sqrt(), T(np.float64(sc.c1)))
    d2 = T(np.where(br == BR_PASS, np.float64(sc.c2), 0.0))

    def ex(v, fill):
        return T(_expand(case, v.v, fill), _expand(case, v.m, abs(fill)), v.k)

    al, d1, d2 = ex(al, 0.0), ex(d1, float(sc.c1)), ex(d2, float(sc.c2))
    d = case.p["d"]
    y = T(t["y"].reshape(B, 3, d, d)) if case.kernel == "denoise" else T(np.broadcast_to(t["y"].reshape(B, 1, d, d), (B, 3, d, d)))
    e = T(et_of(t))
    x0 = (T(t["xt"]) - e * T(sc.s1)) / T(sc.s2)
    xn = ((x0 * T(sc.a) - (x0 - y) * al) + T(t["nz"]) * d1) + e * d2
    return {"x0": x0, "xn": xn}


def faults_of(case):
    """The planted faults `case` is meant to notice."""
    f = ["fma", "et_stride", "sigma_not_doubled"]
    if case.p["sigma"] == "shot":
        f.append("shot_unclamped")
    else:
        f.append("map_per_image")
        if case.p["at_next"] == 0.25:
            f += ["tie_lt", "tie_gt"]
    return f


__all__ = ["CASES", "BY_NAME", "FAULTS", "EPS", "model", "twin", "coef64", "branches32", "make_inputs", "faults_of"]
