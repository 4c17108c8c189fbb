"""The degradation operators at the `--deg_scale` values that switch a kernel, each against a float64 model built here
from the operator's definition:

  SuperResolution x2  generic ddnm_step chain (x0 / A / A^+ / combine), ddnm_site_matmul_f32 with n = 4
  SuperResolution x8  V / Vt as ONE ddnm_bgemm_f32 over all sites: d = 32, B = 2 gives 96 rows (scalar fallback),
                      d = 64, B = 2 gives 384 rows (64x64 MFMA tile)
  WalshHadamardCS     d = 32 (fwht_cols_kernel) and d = 128 (fwht_cols_reg_kernel<128>); ratio 3 leaves n_keep % 3 == 1
  CS 0.1              cs = 102: N of A and K of A^+ are no multiples of 64 / 32 (scalar fallback)
  CS 0.5              cs = 512 on the MFMA tiles (d = 256: 192 patch rows)

Tolerances.  The engine operators have no host path: every method launches HIP kernels on the pointers it is given, so an
operator built with device="cpu" cannot be run as the fp32 reference.  As the plan for this file provides for that case,
every comparison asserts the DERIVED bound instead: a length-K dot product in fp32, in any order, is within
(K + 4) 2^-24 |M| |x| of the exact one (tests/models64.py::gemm_bound; the FWHT: (2 log2 d + 2) 2^-24, fwht_bound), and
`Tr` carries that bound through a chain of stages -- each stage adds its own rounding on top of |M| times the error it
is handed.  The float64 value and the bound are computed from the model alone, never from the engine's output.  For the
record every comparison also prints the relative L2 error of the engine and of the SAME model evaluated by torch in
float32 on the CPU (the reference arithmetic), both against float64: lines `scale-table | ...`.
Measured on the MI355X: worst |err| / bound 0.63 (the three-rounding x0 kernel against its 4 u bound), 0.43 elsewhere;
worst rel-L2, engine / CPU fp32: SR x2 2.2e-7 / 7.4e-8, SR x8 4.6e-7 / 2.0e-7, WH d = 32 1.2e-7 / 2.2e-7, WH d = 128
1.4e-7 / 4.1e-7, CS 0.1 5.6e-7 / 2.7e-7, CS 0.5 6.0e-7 / 3.0e-7 (its DDNM+ step 1.3e-6 against CSPlus64, whose
re-orthonormalised V differs from the engine's by that much)."""
import math

import numpy as np
import pytest
import torch

from tests import models64 as M64
from tests.helpers import rel

pytestmark = pytest.mark.gpu

U = M64.U32
ETA = 0.85


def gen(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------ tracked evaluation
class Tr:
    """A float64 value with an elementwise bound on the error of its fp32 evaluation."""

    def __init__(self, val, err=None):
        self.val = val.double()
        self.err = torch.zeros_like(self.val) if err is None else err

    def reshape(self, *shape):
        return Tr(self.val.reshape(*shape), self.err.reshape(*shape))


def lin(f, fabs, c, t):
    """One fp32 linear stage y = f(x) with entrywise-absolute form fabs and rounding constant c (K + 4 for dot products
    of length K): |fl(f(x^)) - f(x)| <= c u fabs(|x^|) + fabs(|x^ - x|), |x^| <= |x| + err."""
    return Tr(f(t.val), c * U * fabs(t.val.abs() + t.err) + fabs(t.err))


def mix(*terms):
    """Pointwise sum_i c_i x_i with fp32 coefficients c_i: every term is rounded by its product and by at most
    len(terms) - 1 additions; counted as 2 len(terms) + 2 roundings of the sum of magnitudes (room for a division)."""
    val = sum(c * t.val for c, t in terms)
    mag = sum(abs(c) * (t.val.abs() + t.err) for c, t in terms)
    return Tr(val, sum(abs(c) * t.err for c, t in terms) + (2 * len(terms) + 2) * U * mag)


def check(tag, got, t, cpu32=None):
    got = got.detach().double().cpu().reshape(t.val.shape)
    err = (got - t.val).abs()
    ratio = float((err / t.err.clamp_min(1e-300)).max())
    host = "-" if cpu32 is None else f"{rel(cpu32.reshape(t.val.shape), t.val):.2e}"
    line = f"scale-table | {tag} | GPU rel-L2 {rel(got, t.val):.2e} | CPU-fp32 rel-L2 {host} | worst |err|/bound {ratio:.4f}"
    print(line)
    assert bool(torch.isfinite(got).all()), tag
    assert bool((err <= t.err).all()), f"{tag}: worst |err| / bound = {ratio:.3f}"


# ------------------------------------------------------------------------------------------------ float64 models
class SRModel:
    """Average pooling from its definition: y = (P (x) P) x per channel, P = kron(I_yd, 1_r^T / r); A^+ replicates."""

    def __init__(self, d, r):
        self.d, self.r, self.yd = d, r, d // r
        self.P = torch.kron(torch.eye(self.yd, dtype=torch.float64), torch.full((1, r), 1.0 / r, dtype=torch.float64))
        self.R = (self.P * r).T.contiguous()                                # [d, yd] of ones: A^+ = R Y R^T
        self.cA, self.cAp = r * r + 4, 1 + 4

    def A(self, x):
        P = self.P.to(x.dtype)
        return (P @ x.reshape(x.shape[0], 3, self.d, self.d) @ P.T).reshape(x.shape[0], -1)

    def Ap(self, y):
        R = self.R.to(y.dtype)
        return (R @ y.reshape(y.shape[0], 3, self.yd, self.yd) @ R.T).reshape(y.shape[0], -1)

    A_abs, Ap_abs = A, Ap                                                   # non-negative matrices

    def patches(self, v):                                                   # [B, 3*d*d] -> [B, 3, sites, r*r]
        b, r = v.shape[0], self.r
        p = v.reshape(b, 3, self.yd, r, self.yd, r).permute(0, 1, 2, 4, 3, 5)
        return p.reshape(b, 3, self.yd ** 2, r * r)

    def unpatch(self, p):
        b, r = p.shape[0], self.r
        return p.reshape(b, 3, self.yd, self.yd, r, r).permute(0, 1, 2, 4, 3, 5).reshape(b, -1)


class WHModel:
    """H = hadamard64(d): coefficients H X H / d per channel, permuted by `perm`, (k, c)-interleaved, first n_keep kept."""

    def __init__(self, d, ratio, perm):
        self.d, self.N, self.perm = d, d * d, perm.long()
        self.n_keep = 3 * self.N // ratio
        self.H = M64.hadamard64(d)
        self.ones = torch.ones(d, d, dtype=torch.float64)
        k = torch.arange(self.N)
        self.mask = torch.zeros(3, self.N, dtype=torch.bool)
        for c in range(3):
            self.mask[c, self.perm] = (k * 3 + c) < self.n_keep               # the keep rule
        self.c = 2 * math.log2(d) + 2

    def fwht(self, x):
        H = self.H.to(x.dtype)
        return (H @ x.reshape(x.shape[0], 3, self.d, self.d) @ H / self.d).reshape(x.shape[0], -1)

    def fwht_abs(self, x):
        o = self.ones.to(x.dtype)
        return (o @ x.reshape(x.shape[0], 3, self.d, self.d) @ o / self.d).reshape(x.shape[0], -1)

    def gather(self, coef, n_keep=None):
        b = coef.shape[0]
        z = coef.reshape(b, 3, self.N)[:, :, self.perm].permute(0, 2, 1).reshape(b, -1)
        return z[:, :self.n_keep if n_keep is None else n_keep].contiguous()

    def scatter(self, y):
        b = y.shape[0]
        full = torch.zeros(b, 3 * self.N, dtype=y.dtype)
        full[:, :y.shape[1]] = y
        planes = torch.zeros(b, 3, self.N, dtype=y.dtype)
        planes[:, :, self.perm] = full.reshape(b, self.N, 3).permute(0, 2, 1)
        return planes.reshape(b, -1)

    def A(self, x):
        return self.gather(self.fwht(x))

    def A_abs(self, x):
        return self.gather(self.fwht_abs(x))

    def Ap(self, y):
        return self.fwht(self.scatter(y))

    def Ap_abs(self, y):
        return self.fwht_abs(self.scatter(y))

    @property
    def cA(self):
        return self.c

    cAp = cA

    def masked(self, x):                                                    # mask .* x on [B, 3*N]
        return x * self.mask.reshape(1, -1).to(x.dtype)


class CSModel:
    """`op.M.double()` ([cs, 1024], the engine's own measurement rows) applied to the 32 x 32 patches."""

    def __init__(self, d, Mrows):
        self.d, self.n, self.M = d, d // 32, Mrows.double().cpu()
        self.cs = self.M.shape[0]
        self.cA, self.cAp = 1024 + 4, self.cs + 4

    def patches(self, x):
        b, n = x.shape[0], self.n
        return x.reshape(b, 3, n, 32, n, 32).permute(0, 1, 2, 4, 3, 5).reshape(b * 3 * n * n, 1024)

    def unpatch(self, p, b):
        n = self.n
        return p.reshape(b, 3, n, n, 32, 32).permute(0, 1, 2, 4, 3, 5).reshape(b, -1)

    def _A(self, x, Mm):
        return (self.patches(x) @ Mm.to(x.dtype).T).reshape(x.shape[0], -1)

    def _Ap(self, y, Mm):
        return self.unpatch(y.reshape(-1, self.cs) @ Mm.to(y.dtype), y.shape[0])

    def A(self, x):
        return self._A(x, self.M)

    def A_abs(self, x):
        return self._A(x, self.M.abs())

    def Ap(self, y):
        return self._Ap(y, self.M)

    def Ap_abs(self, y):
        return self._Ap(y, self.M.abs())


# ------------------------------------------------------------------------------------------------ shared checks
def _scalars():
    from ddnm_amd import ops
    from oracle import cases, schedule
    betas = cases.betas()
    return ops.step_scalars(schedule.alpha_bar(betas, 500), schedule.alpha_bar(betas, 490), ETA)


def _x0(xt, et, s):
    """x0 = (xt - et sqrt(1 - abar)) / sqrt(abar) with the fp32 scalars the kernel receives: product, difference, quotient."""
    val = (xt.double() - et.double() * s.sqrt_1m_at) / s.sqrt_at
    return Tr(val, 4 * U * (xt.double().abs() + et.double().abs() * s.sqrt_1m_at) / s.sqrt_at)


def _step_formula(mdl, xt, et, nz, y, s):
    """The float64 formula of tests/test_gpu_kernels.py::test_ddnm_step on plain tensors of one dtype (float64: must be the
    tracked value; float32: the CPU-fp32 column of the table)."""
    B = xt.shape[0]
    x0 = ((xt - et * s.sqrt_1m_at) / s.sqrt_at).reshape(B, -1)
    x0h = x0 - mdl.Ap(mdl.A(x0) - y)
    return s.sqrt_at_next * x0h + s.c1 * nz.reshape(B, -1) + s.c2 * et.reshape(B, -1)


def _check_A_pinv_step(tag, op, mdl, d, B, project=None):
    """A, A^+, A A^+ y = y and one ddnm_step (3-channel and 6-channel-view eps) of engine operator `op` against `mdl`.
    project(x0: Tr, y: Tr) -> Tr is the tracked A^+(A x0 - y) in the operator's own launch order (default: the generic
    chain A, difference, A^+)."""
    x = gen(B, 3, d, d, seed=d + 1)
    xf = Tr(x.reshape(B, -1))
    tA = lin(mdl.A, mdl.A_abs, mdl.cA, xf)
    y_e = op.A(x.cuda())
    check(f"{tag} | A", y_e, tA, mdl.A(x.reshape(B, -1)))
    y = gen(*tA.val.shape, seed=d + 2)                                      # any measurement vector, exact input
    tP = lin(mdl.Ap, mdl.Ap_abs, mdl.cAp, Tr(y))
    p_e = op.A_pinv(y.cuda())
    check(f"{tag} | A_pinv", p_e, tP, mdl.Ap(y))
    assert y_e.shape == tA.val.shape and p_e.shape == tP.val.shape and y_e.is_contiguous() and p_e.is_contiguous()
    tAP = lin(mdl.A, mdl.A_abs, mdl.cA, tP)
    yy = op.A(p_e)
    check(f"{tag} | A A_pinv y", yy, tAP, mdl.A(mdl.Ap(y)))
    assert rel(yy, y) < 1e-5                                                # the Moore-Penrose bar of test_operator_A_and_pinv
    # one step
    s = _scalars()
    xt, et6, nz = gen(B, 3, d, d, seed=d + 3), gen(B, 6, d, d, seed=d + 4), gen(B, 3, d, d, seed=d + 5)
    et = et6[:, :3].contiguous()
    ym = mdl.A(gen(B, 3, d, d, seed=d + 6).reshape(B, -1).double()).float()
    t0 = _x0(xt, et, s).reshape(B, -1)
    ty = Tr(ym)
    if project is None:
        resid = mix((1.0, lin(mdl.A, mdl.A_abs, mdl.cA, t0)), (-1.0, ty))
        proj = lin(mdl.Ap, mdl.Ap_abs, mdl.cAp, resid)
    else:
        proj = project(t0, ty)
    tn = mix((s.sqrt_at_next, t0), (-s.sqrt_at_next, proj), (s.c1, Tr(nz.reshape(B, -1))), (s.c2, Tr(et.reshape(B, -1))))
    want = _step_formula(mdl, xt.double(), et.double(), nz.double(), ym.double(), s)
    assert rel(tn.val, want) < 1e-12, "the tracked chain is not the formula of test_ddnm_step"
    host = _step_formula(mdl, xt, et, nz, ym, s)
    for six in (False, True):
        et_dev = et6.cuda()[:, :3] if six else et.cuda()
        x0_e, out = torch.full((B, 3, d, d), float("nan"), device="cuda"), torch.full((B, 3, d, d), float("nan"), device="cuda")
        y_dev = ym.cuda()
        op.ddnm_step(xt.cuda(), et_dev, nz.cuda(), y_dev, s, x0_e, out)
        torch.cuda.synchronize()
        check(f"{tag} | ddnm_step x0 six={int(six)}", x0_e, t0, ((xt - et * s.sqrt_1m_at) / s.sqrt_at))
        check(f"{tag} | ddnm_step x_next six={int(six)}", out, tn, host)


REGIMES = {"early": (0.2, 0.97), "late": (0.98, 0.15)}                      # (a, sigma_t) at sigma_y = 0.4, as at ratio 16
SIGMA_Y = 0.4


# ------------------------------------------------------------------------------------------------ SuperResolution
@pytest.mark.parametrize("d,r,B", [(32, 2, 2), (32, 8, 2), (64, 8, 2)])
def test_superresolution_scales(hip, d, r, B):
    from ddnm_amd.functions import svd_operators as E
    op, mdl = E.SuperResolution(3, d, r, "cuda"), SRModel(d, r)
    _check_A_pinv_step(f"sr_averagepooling d={d} x{r} B={B}", op, mdl, d, B)


@pytest.mark.parametrize("d,r,B", [(32, 2, 2), (32, 8, 2), (64, 8, 2)])
def test_superresolution_svd_surface(hip, d, r, B):
    """The algebraic half of test_operator_svd_surface (same bars) at the ratios that leave the register-resident site
    kernel's n = 16, and Lambda / Lambda_noise against float64 with the engine's own V (op._svd(): LAPACK's basis is
    part of the contract).  Lambda = V diag(lambda, 1, ..) V^T per r x r site, Lambda_noise = V (d1 .* v~ + d2 .* e~) on
    the RAW site entries; bounds: two chained products of length n (Lambda; the orthogonality defect of a LAPACK fp32 V is
    itself a rounding error of that size), one of length n on a two-term mix (Lambda_noise)."""
    from ddnm_amd.functions import svd_operators as E
    op, mdl = E.SuperResolution(3, d, r, "cuda"), SRModel(d, r)
    n = r * r
    x = gen(B, 3, d, d, seed=50 + d + r).cuda()
    xf = x.reshape(B, -1)
    assert rel(op.V(op.Vt(x)), xf) < 2e-6 and rel(op.Vt(op.V(xf)), xf) < 2e-6
    y = op.A(x)
    assert rel(op.U(op.Ut(y)), y) < 2e-6
    s = op.singulars().float()
    ns = s.numel()
    assert ns == 3 * (d // r) ** 2 and bool((s == 1.0 / r).all())
    assert rel(op.U(s * op.Vt(x)[:, :ns]), y) < 2e-5                         # A = U S V^T[:n]
    z = op.add_zeros(y)
    assert z.shape == (B, 3 * d * d) and torch.equal(z[:, :ns], y) and not bool(z[:, ns:].any())
    w = gen(B, ns, seed=5).cuda()
    lhs, rhs = (y.double() * w.double()).sum(), (xf.double() * op.At(w).double()).sum()
    assert abs(lhs - rhs) / abs(lhs) < 1e-4                                  # <A x, w> = <x, At w>
    assert rel(op.A_pinv_eta(w, 0.0), op.A_pinv(w)) < 2e-5
    # Vt / V against the float64 site products in the reference's spectral order (component 0 of every site first)
    sv, V = op._svd()
    V64 = V.double().cpu()
    S = 3 * (d // r) ** 2

    def spec(p):                                                             # [B, 3, sites, n] -> spectral order
        p = p.reshape(B, S, n)
        return torch.cat([p[:, :, 0], p[:, :, 1:].reshape(B, -1)], 1)

    def unspec(zz):
        return torch.cat([zz[:, :S, None], zz[:, S:].reshape(B, S, n - 1)], 2).reshape(B, 3, S // 3, n)

    xc = xf.cpu()
    tag = f"sr_averagepooling d={d} x{r} B={B}"
    Va = V64.abs()
    check(f"{tag} | Vt", op.Vt(x), lin(lambda t: spec(mdl.patches(t) @ V64), lambda t: spec(mdl.patches(t) @ Va), n + 4, Tr(xc)),
          spec(mdl.patches(xc) @ V64.float()))
    check(f"{tag} | V", op.V(xf), lin(lambda t: mdl.unpatch(unspec(t) @ V64.T), lambda t: mdl.unpatch(unspec(t) @ Va.T), n + 4,
                                      Tr(xc)), mdl.unpatch(unspec(xc) @ V64.float().T))
    e = gen(B, 3 * d * d, seed=6)
    for name, (a, st) in REGIMES.items():
        lam, d1m, d2m = (f32(c) for c in E.spectral_coefficients(sv, a, SIGMA_Y, st, ETA))
        _, d1n, d2n = (f32(c) for c in E.spectral_coefficients(0.0, a, SIGMA_Y, st, ETA))
        lamv = torch.ones(n, dtype=torch.float64)
        lamv[0] = lam
        t1 = lin(lambda t: mdl.patches(t) @ V64 * lamv, lambda t: mdl.patches(t) @ Va * lamv.abs(), n + 5, Tr(xc))
        tL = lin(lambda t: mdl.unpatch(t @ V64.T), lambda t: mdl.unpatch(t @ Va.T), n + 4, t1)
        check(f"{tag} | Lambda {name}", op.Lambda(xf, a, SIGMA_Y, st, ETA), tL,
              mdl.unpatch((mdl.patches(xc) @ V64.float() * lamv.float()) @ V64.float().T))
        d1 = torch.full((n,), d1n, dtype=torch.float64)
        d2 = torch.full((n,), d2n, dtype=torch.float64)
        d1[0], d2[0] = d1m, d2m
        pv, pe = mdl.patches(xc.double()), mdl.patches(e.double())
        zt = Tr(pv * d1 + pe * d2, 3 * U * (pv.abs() * d1.abs() + pe.abs() * d2.abs()))
        tN = lin(lambda t: mdl.unpatch(t @ V64.T), lambda t: mdl.unpatch(t @ Va.T), n + 4, zt)
        check(f"{tag} | Lambda_noise {name}", op.Lambda_noise(xf, a, SIGMA_Y, st, ETA, e.cuda()), tN,
              mdl.unpatch((mdl.patches(xc) * d1.float() + mdl.patches(e) * d2.float()) @ V64.float().T))


# ------------------------------------------------------------------------------------------------ WalshHadamardCS
@pytest.mark.parametrize("d,ratio", [(32, 4), (32, 3), (128, 2), (128, 3)])
def test_walsh_hadamard_scales(hip, d, ratio):
    from ddnm_amd.functions import svd_operators as E
    from oracle import cases
    B = 2
    perm = cases.wh_perm(d)
    op, mdl = E.WalshHadamardCS(3, d, ratio, perm, "cuda"), WHModel(d, ratio, perm)
    assert op.n_keep == mdl.n_keep and (ratio != 3 or mdl.n_keep % 3 == 1)
    assert torch.equal(op.mask.cpu().bool(), mdl.mask)
    tag = f"cs_walshhadamard d={d} ratio={ratio} B={B}"

    def project(t0, ty):
        """The engine's order: P = H (W .* (H x0)) in one masked launch (two transforms, the 0 / 1 mask exact), A^+ y
        once per run, and their difference inside the combine kernel."""
        spec_ = lin(lambda t: mdl.masked(mdl.fwht(t)), lambda t: mdl.masked(mdl.fwht_abs(t)), mdl.c, t0)
        return mix((1.0, lin(mdl.fwht, mdl.fwht_abs, mdl.c, spec_)), (-1.0, lin(mdl.Ap, mdl.Ap_abs, mdl.c, ty)))

    _check_A_pinv_step(tag, op, mdl, d, B, project)
    # Vt / V / Lambda / Lambda_noise
    x = gen(B, 3 * d * d, seed=60 + d)
    e = gen(B, 3 * d * d, seed=61 + d)
    full = 3 * mdl.N
    check(f"{tag} | Vt", op.Vt(x.cuda()), lin(lambda t: mdl.gather(mdl.fwht(t), full), lambda t: mdl.gather(mdl.fwht_abs(t), full),
                                              mdl.c, Tr(x)), mdl.gather(mdl.fwht(x), full))
    check(f"{tag} | V", op.V(x.cuda()), lin(mdl.Ap, mdl.Ap_abs, mdl.c, Tr(x)), mdl.Ap(x))
    m = mdl.mask.reshape(1, -1)
    for name, (a, st) in REGIMES.items():
        lam, d1m, d2m = (f32(c) for c in E.spectral_coefficients(1.0, a, SIGMA_Y, st, ETA))
        _, d1n, d2n = (f32(c) for c in E.spectral_coefficients(0.0, a, SIGMA_Y, st, ETA))
        lamv = torch.where(m, torch.tensor(lam, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64))
        t1 = lin(lambda t: mdl.fwht(t) * lamv, lambda t: mdl.fwht_abs(t) * lamv.abs(), mdl.c + 1, Tr(x))
        check(f"{tag} | Lambda {name}", op.Lambda(x.cuda(), a, SIGMA_Y, st, ETA), lin(mdl.fwht, mdl.fwht_abs, mdl.c, t1),
              mdl.fwht(mdl.fwht(x) * lamv.float()))
        d1 = torch.where(m, torch.tensor(d1m, dtype=torch.float64), torch.tensor(d1n, dtype=torch.float64))
        d2 = torch.where(m, torch.tensor(d2m, dtype=torch.float64), torch.tensor(d2n, dtype=torch.float64))
        zt = Tr(x.double() * d1 + e.double() * d2, 3 * U * (x.double().abs() * d1.abs() + e.double().abs() * d2.abs()))
        check(f"{tag} | Lambda_noise {name}", op.Lambda_noise(x.cuda(), a, SIGMA_Y, st, ETA, e.cuda()),
              lin(mdl.fwht, mdl.fwht_abs, mdl.c, zt), mdl.fwht(x * d1.float() + e * d2.float()))


# ------------------------------------------------------------------------------------------------ block-based CS
_CS = {}


def _cs_case(d, ratio):
    """Engine operator and models of one (d, ratio), built once per module (two 1024 x 1024 SVDs each)."""
    if (d, ratio) not in _CS:
        from ddnm_amd.functions import svd_operators as E
        from oracle import cases
        from oracle import operators as O
        from tests.test_plus_cs_host import CSPlus64
        gauss = O.gauss_matrix(cases.SEED + 21)
        op = E.CS(3, d, ratio, "cuda", gauss=gauss)
        _CS[(d, ratio)] = (op, CSModel(d, op.M), CSPlus64(3, d, ratio, gauss))
    return _CS[(d, ratio)]


CS_CASES = [(32, 0.1, 2), (256, 0.1, 1), (256, 0.5, 1)]


@pytest.mark.parametrize("d,ratio,B", CS_CASES)
def test_cs_blockbased_scales(hip, d, ratio, B):
    op, mdl, _ = _cs_case(d, ratio)
    assert op.cs_size == int(1024 * ratio) == mdl.cs
    _check_A_pinv_step(f"cs_blockbased d={d} ratio={ratio} B={B}", op, mdl, d, B)


@pytest.mark.parametrize("d,ratio,B", CS_CASES)
@pytest.mark.parametrize("regime", range(4))
def test_cs_blockbased_plus_step(hip, d, ratio, B, regime):
    """begin_plus_run + ddnm_plus_step against CSPlus64 (tests/test_plus_cs_host.py) at the ratios off the tested 0.25: the
    tracked chain below is CSPlus64.fused_step term by term (asserted), with the fp32 scalars the kernels receive:
    w = -a lambda x0 + dd1 n + dd2 eps; T = w M^T (K = 1024); P = T M (K = cs); x_next = a x0 + d1n n + d2n eps +
    a lambda A^+ y + P, A^+ y a product of length cs.  CSPlus64's M64 is the engine's M re-orthonormalised in float64
    (they differ by 1.3e-6, rel-L2): far inside the (K + 4) 2^-24 = 6e-5 of the K = 1024 stage, relative to the same envelope."""
    from ddnm_amd.functions.svd_operators import cs_plus_coefficients
    from tests.test_gpu_plus_spectral import ABAR_T, _scalars as plus_scalars
    from tests.test_plus_cs_host import CS_REGIMES
    op, _, p64 = _cs_case(d, ratio)
    a, sigma_y, sigma_t = (f32(v) for v in CS_REGIMES[regime])
    eta = f32(ETA)
    g = torch.Generator().manual_seed(70 + d + regime)
    xt, et6, nz = (torch.randn(B, c, d, d, generator=g) for c in (3, 6, 3))
    et = et6[:, :3].contiguous()
    y = p64.A((torch.rand(B, 3, d, d, generator=g) * 2 - 1).double()).float() + 0.4 * torch.randn(B, p64.n_meas, generator=g)
    s = plus_scalars(a, eta)
    al, d1n, d2n, dd1, dd2 = (f32(c) for c in cs_plus_coefficients(s.sqrt_at_next, sigma_y, sigma_t, eta))
    Mm, Ma, cs = p64.M64, p64.M64.abs(), p64.cs

    def flat(t):
        return Tr(t.reshape(B, -1))

    def unp(p):
        return p64._unpatch(p.reshape(B, 3, -1, 1024)).reshape(B, -1)

    def pat(v):
        return p64._patches(v.reshape(B, 3, d, d)).reshape(-1, 1024)

    t0 = _x0(xt, et, s).reshape(B, -1)
    w = mix((-al, t0), (dd1, flat(nz)), (dd2, flat(et)))
    T = lin(lambda t: pat(t) @ Mm.T, lambda t: pat(t) @ Ma.T, 1024 + 4, w)
    P = lin(lambda t: unp(t @ Mm), lambda t: unp(t @ Ma), cs + 4, T)
    aty = lin(lambda t: unp(t.reshape(-1, cs) @ Mm), lambda t: unp(t.reshape(-1, cs) @ Ma), cs + 4, Tr(y))
    tn = mix((s.sqrt_at_next, t0), (d1n, flat(nz)), (d2n, flat(et)), (al, aty), (1.0, P))
    m0, mn = p64.fused_step(xt, et, nz, y, ABAR_T, a, sigma_y, sigma_t, eta)
    assert rel(t0.val, m0.reshape(B, -1)) < 1e-6 and rel(tn.val, mn.reshape(B, -1)) < 1e-6, \
        "the tracked chain is not CSPlus64.fused_step"
    tag = f"cs_blockbased d={d} ratio={ratio} B={B} | ddnm_plus_step regime {regime}"
    for six in (False, True):
        et_dev = et6.cuda()[:, :3] if six else et.cuda()
        x0_e, out = torch.full((B, 3, d, d), float("nan"), device="cuda"), torch.full((B, 3, d, d), float("nan"), device="cuda")
        op.begin_plus_run(y.cuda())
        op.ddnm_plus_step(xt.cuda(), et_dev, nz.cuda(), s, sigma_y, sigma_t, eta, x0_e, out)
        torch.cuda.synchronize()
        check(f"{tag} x0 six={int(six)}", x0_e, t0)
        check(f"{tag} x_next six={int(six)}", out, tn)
