"""DDNM+ for block-based compressed sensing (cs_blockbased), host side: the C ABI carries the three new entry points under
version 7 and they validate before any launch, `CS` exposes the `ddnm_plus_step` hook while `CS.Lambda` still raises,
`cs_plus_coefficients` is the `spectral_coefficients` composition, and the float64 model the GPU tests compare against
(tests/test_gpu_plus_cs.py imports it from here) agrees with itself: the step fused per patch equals the unfused
Lambda / Lambda_noise composition."""
import ctypes
import os
import re

import pytest
import torch

from oracle import cases
from oracle import operators as O
from tests.test_plus_spectral_host import ETA, REGIMES, step_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ddnm_step_plus_cs_pre_f32", "ddnm_step_plus_cs_pre_keyed_f32", "ddnm_step_plus_cs_post_f32")
# (a, sigma_y, sigma_t): sigma_t above a*sigma_y, below it, the last step (a = 1, sigma_t = 0), and no measurement noise
CS_REGIMES = [REGIMES[0], REGIMES[2], (1.0, 0.4, 0.0), (0.5, 0.0, 0.9)]
ABAR_T = 0.37


class CSPlus64(O.CS):
    """float64 model of DDNM+ for block-based CS with the FULL 1024 x 1024 V_small and the reference's coefficient order
    (svd_operators.py:131-145: the first `cs` coefficients of every (channel, patch), then the remaining ones):
    `Lambda(v) = V(lambda .* V^T v)`, `Lambda_noise(v, e) = V(d1 .* V^T v + d2 .* V^T e)` with lambda / d1 / d2 from
    `spectral_coefficients` of singular value 1 on the first block and of the null space on the second.

    V_small is the factor of torch.svd of the fp32 Gaussian matrix -- the decomposition the engine and the oracle run --
    re-orthonormalised in float64 by a QR with positive diagonal.  LAPACK's fp32 factor is orthogonal only to 5e-6
    (spectral norm of V^T V - I for the matrix of the tests), which is what the fused and the unfused form would differ
    by, since only the fused one assumes V V^T = I; after the QR they agree to rounding.  The QR leaves the span of the
    first k columns unchanged for every k, so the measured subspace is exactly the engine's, and moves V by 1.3e-6 (rel-L2).
    Results are returned in the dtype of the argument (the network of a whole-loop run is fp32)."""

    def __init__(self, channels, img_dim, ratio, gauss):
        O.CS.__init__(self, channels, img_dim, ratio, gauss)
        _, _, V = torch.svd(gauss.float(), some=False)
        Q, R = torch.linalg.qr(V.double())
        self.V64 = Q * torch.sign(torch.diagonal(R))[None, :]
        self.M64 = self.V64.T[:self.cs].contiguous()                      # [cs, 1024]: Vt_small[:cs]
        self.n_meas = channels * self.n ** 2 * self.cs

    # ---- V / Vt in the reference's order
    def _patches(self, x):
        b, c, n = x.shape[0], self.channels, self.n
        return x.double().reshape(b, c, n, 32, n, 32).permute(0, 1, 2, 4, 3, 5).reshape(b, c, n * n, 1024)

    def _unpatch(self, p):
        b, c, n = p.shape[0], self.channels, self.n
        return p.reshape(b, c, n, n, 32, 32).permute(0, 1, 2, 4, 3, 5).reshape(b, c, 32 * n, 32 * n)

    def Vt(self, x):
        co = self._patches(x) @ self.V64                                  # row p -> Vt_small p
        b = x.shape[0]
        return torch.cat([co[..., :self.cs].reshape(b, -1), co[..., self.cs:].reshape(b, -1)], 1)

    def V(self, z):
        b, c, n = z.shape[0], self.channels, self.n
        co = torch.cat([z[:, :self.n_meas].reshape(b, c, n * n, self.cs),
                        z[:, self.n_meas:].reshape(b, c, n * n, 1024 - self.cs)], 3)
        return self._unpatch(co @ self.V64.T).reshape(b, -1)

    def A(self, x):
        return self.Vt(x)[:, :self.n_meas].to(x.dtype)

    def A_pinv(self, y):
        z = torch.zeros(y.shape[0], self.channels * self.img_dim ** 2, dtype=torch.float64)
        z[:, :self.n_meas] = y.double().reshape(y.shape[0], -1)
        return self.V(z).to(y.dtype)

    def coefficients(self, a, sigma_y, sigma_t, eta):
        from ddnm_amd.functions.svd_operators import spectral_coefficients
        meas = spectral_coefficients(1.0, a, sigma_y, sigma_t, eta)
        null = spectral_coefficients(0.0, a, sigma_y, sigma_t, eta)
        N = self.channels * self.img_dim ** 2
        out = []
        for k in range(3):
            v = torch.full((N,), null[k], dtype=torch.float64)
            v[:self.n_meas] = meas[k]
            out.append(v)
        return tuple(out)                                                  # lambda, d1, d2 over the spectral vector

    def Lambda(self, vec, a, sigma_y, sigma_t, eta):
        lam = self.coefficients(a, sigma_y, sigma_t, eta)[0]
        return self.V(self.Vt(vec) * lam).to(vec.dtype)

    def Lambda_noise(self, vec, a, sigma_y, sigma_t, eta, epsilon):
        _, d1, d2 = self.coefficients(a, sigma_y, sigma_t, eta)
        return self.V(self.Vt(vec) * d1 + self.Vt(epsilon) * d2).to(vec.dtype)

    def x0(self, xt, et, abar_t):
        return (xt.double() - et.double() * (1 - abar_t) ** 0.5) / abar_t ** 0.5

    def unfused_step(self, xt, et, n, y, abar_t, a, sigma_y, sigma_t, eta):
        """The loop body of functions/svd_ddnm.py:118-131 spelled out: (x0|t, x_{t-1})."""
        B = xt.shape[0]
        x0 = self.x0(xt, et, abar_t)
        corr = self.A_pinv(self.A(x0.reshape(B, -1)) - y.double().reshape(B, -1))
        x0_hat = x0 - self.Lambda(corr, a, sigma_y, sigma_t, eta).reshape(x0.shape)
        nz = self.Lambda_noise(n.double().reshape(B, -1), a, sigma_y, sigma_t, eta, et.double().reshape(B, -1))
        return x0, a * x0_hat + nz.reshape(x0.shape)

    def fused_step(self, xt, et, n, y, abar_t, a, sigma_y, sigma_t, eta):
        """The same step collapsed per patch (what the engine's two kernels and two GEMMs evaluate)."""
        from ddnm_amd.functions.svd_operators import cs_plus_coefficients
        al, d1n, d2n, dd1, dd2 = cs_plus_coefficients(a, sigma_y, sigma_t, eta)
        x0 = self.x0(xt, et, abar_t)
        e, nn = et.double(), n.double()
        w = self._patches(-al * x0 + dd1 * nn + dd2 * e)
        proj = self._unpatch((w @ self.M64.T) @ self.M64)
        aty = self.A_pinv(y.double()).reshape(x0.shape)
        return x0, a * x0 + d1n * nn + d2n * e + al * aty + proj


def model_operator(d, ratio=0.25):
    """The float64 model of `--deg cs_blockbased`, from the Gaussian matrix of oracle.cases.make_operator."""
    return CSPlus64(3, d, ratio, O.gauss_matrix(cases.SEED + 21))


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def lib():
    from ddnm_amd import _lib, build
    build.build()
    return _lib.lib()


def _header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddnm_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/ddnm_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype_of(decl):
    from ddnm_amd._lib import StepScalars
    if "ddnm_step_scalars" in decl:
        return ctypes.POINTER(StepScalars)
    if "*" in decl:
        return ctypes.c_void_p
    return {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[decl.split()[0]]


def test_library_exports_the_plus_cs_entry_points(lib):
    from ddnm_amd import _lib
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is ctypes.c_int32
        assert list(argtypes) == [_ctype_of(a) for a in _header_args(name)], name
    assert lib.ddnm_version() == 7


def test_plus_cs_argument_validation_without_gpu(lib):
    """Bad arguments are refused before any launch: null pointers, non-positive sizes, a missing noise source and
    aliased outputs are DDNM_E_BADARG; D % ps, ps % 4 or et_bstride % 4 are DDNM_E_SHAPE."""
    from ddnm_amd._lib import StepScalars
    s = StepScalars()
    p = [4096 * (i + 1) for i in range(8)]                     # distinct non-null dummies, never dereferenced
    ok = dict(xt=p[0], et=p[1], es=3 * 64 * 64, nz=p[2], aty=p[3], x0=p[4], xn=p[5], w=p[6], B=2, C=3, D=64, ps=32)

    def pre(fn=lib.ddnm_step_plus_cs_pre_f32, **kw):
        a = dict(ok, **kw)
        return fn(a["xt"], a["et"], a["es"], a["nz"], a["aty"], a["x0"], a["xn"], a["w"], a["B"], a["C"], a["D"], a["ps"],
                  0.1, 0.2, 0.3, 0.4, 0.5, ctypes.byref(s), None)

    for fn in (lib.ddnm_step_plus_cs_pre_f32, lib.ddnm_step_plus_cs_pre_keyed_f32):
        for key in ("xt", "et", "aty", "x0", "xn", "w"):
            assert pre(fn, **{key: None}) == -1, key
        for key in ("B", "C", "D", "ps"):
            assert pre(fn, **{key: 0}) == -1 and pre(fn, **{key: -1}) == -1, key
        assert pre(fn, nz=None) == -1                          # rng_on == 0 and no tensor / no key table
        assert pre(fn, D=48) == -2                             # D % ps
        assert pre(fn, D=60, ps=6) == -2                       # ps % 4
        assert pre(fn, es=3 * 64 * 64 + 2) == -2               # et_bstride % 4
        for other in ("xt", "et", "x0"):                       # the sampler's rotating buffers never alias
            assert pre(fn, xn=ok[other]) == -1, other
        assert pre(fn, w=ok["xn"]) == -1
    assert pre(lib.ddnm_step_plus_cs_pre_keyed_f32, nz=4104) == -1          # key table not 16-byte aligned
    assert lib.ddnm_step_plus_cs_pre_f32(ok["xt"], ok["et"], ok["es"], ok["nz"], ok["aty"], ok["x0"], ok["xn"], ok["w"],
                                         2, 3, 64, 32, 0.1, 0.2, 0.3, 0.4, 0.5, None, None) == -1

    def post(P=p[6], xn=p[5], planes=6, D=64, ps=32):
        return lib.ddnm_step_plus_cs_post_f32(P, xn, planes, D, ps, None)

    assert post(P=None) == -1 and post(xn=None) == -1
    assert post(planes=0) == -1 and post(D=0) == -1 and post(ps=0) == -1
    assert post(D=48) == -2 and post(D=60, ps=6) == -2
    assert post(P=p[5]) == -1                                  # in place: the scatter would read what it overwrites


# ------------------------------------------------------------------------------------------------ operator
def _host_cs(d=32, ratio=0.25):
    from ddnm_amd.functions import svd_operators as E
    try:
        return E.CS(3, d, ratio, "cpu", gauss=O.gauss_matrix(cases.SEED + 21))
    except Exception as e:                                     # noqa: BLE001
        pytest.skip(f"CS cannot be constructed without a device: {e}")


def test_cs_exposes_the_hook():
    from ddnm_amd.functions import svd_operators as E
    assert callable(E.CS.ddnm_plus_step) and callable(E.CS.begin_plus_run)
    assert E.CS.Lambda is E.A_functions.Lambda and E.CS.Lambda_noise is E.A_functions.Lambda_noise


def test_cs_lambda_still_raises_and_the_hook_needs_begin_plus_run():
    op = _host_cs()
    v = torch.zeros(1, 3 * 32 * 32)
    with pytest.raises(NotImplementedError):                   # reference behaviour kept (svd_operators.py:93-97)
        op.Lambda(v, 0.9, 0.2, 0.3, ETA)
    with pytest.raises(NotImplementedError):
        op.Lambda_noise(v, 0.9, 0.2, 0.3, ETA, v)
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(RuntimeError, match="begin_plus_run"):
        op.ddnm_plus_step(x, x, x, None, 0.2, 0.3, ETA, x, x)
    assert op.M.shape == (256, 1024) and op.cs_size == 256


@pytest.mark.parametrize("regime", CS_REGIMES)
def test_cs_plus_coefficients_are_the_spectral_composition(regime):
    from ddnm_amd.functions.svd_operators import cs_plus_coefficients, spectral_coefficients
    a, sigma_y, sigma_t = regime
    lam, d1r, d2r = spectral_coefficients(1, a, sigma_y, sigma_t, ETA)
    one, d1n, d2n = spectral_coefficients(0, a, sigma_y, sigma_t, ETA)
    assert one == 1.0
    got = cs_plus_coefficients(a, sigma_y, sigma_t, ETA)
    assert got == (a * lam, d1n, d2n, d1r - d1n, d2r - d2n)
    assert all(isinstance(v, float) for v in got)
    if sigma_y == 0:
        assert got[0] == a and got[3] == 0.0 and got[4] == 0.0
    elif sigma_t > a * sigma_y:                                # lambda = 1, measured noise sqrt(sigma_t^2 - a^2 sigma_y^2)
        assert got[0] == a and got[4] == -d2n
        assert got[3] + d1n == pytest.approx((sigma_t ** 2 - a ** 2 * sigma_y ** 2) ** 0.5, rel=1e-14)
    else:                                                      # lambda < 1, measured noise sigma_t * eta: d1r = d1n
        assert got[0] == pytest.approx(sigma_t * (1 - ETA ** 2) ** 0.5 / sigma_y, rel=1e-14)
        assert got[3] == 0.0 and got[4] == -d2n


# ------------------------------------------------------------------------------------------------ the float64 model
_MODELS = {}


def _model(d):
    if d not in _MODELS:
        _MODELS[d] = model_operator(d)
    return _MODELS[d]


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("regime", CS_REGIMES)
def test_model_fused_equals_unfused_in_float64(d, regime):
    """a x0 + d1n n + d2n eps + a lambda A^+y + unpatch((w M^T) M) equals
    a (x0 - V lambda V^T A^+ (A x0 - y)) + V (d1 .* V^T n + d2 .* V^T eps) to 1e-10 (float64 rounding of 1024-term
    products is 1e-15 ... 1e-14; a wrong coefficient, sign or patch index shows at 1e-2 or more)."""
    B = 2
    a, sigma_y, sigma_t = regime
    op = _model(d)
    x_orig, xt, et, n = step_inputs("cs_blockbased", d, B)
    y = op.A(x_orig.double())
    y = y + sigma_y * torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    x0_f, xn_f = op.fused_step(xt, et, n, y, ABAR_T, a, sigma_y, sigma_t, ETA)
    x0_u, xn_u = op.unfused_step(xt, et, n, y, ABAR_T, a, sigma_y, sigma_t, ETA)
    assert torch.equal(x0_f, x0_u)
    err = ((xn_f - xn_u).norm() / xn_u.norm()).item()
    print(f"cs_blockbased d={d} {regime}: fused vs unfused rel-L2 {err:.3e}")
    assert err < 1e-10


def test_model_reduces_to_the_oracle_operator():
    """A / A_pinv of the float64 model are the oracle's CS (fp32) up to the re-orthonormalisation of V (1.3e-6) and fp32
    rounding; V and Vt are inverse to each other and keep the reference's coefficient order."""
    d, B = 64, 2
    mdl, orc = _model(d), cases.make_operator("cs_blockbased", d)
    x = step_inputs("cs_blockbased", d, B)[0]
    y = orc.A(x)
    assert ((mdl.A(x.double()) - y).norm() / y.norm()).item() < 1e-5
    xr = orc.A_pinv(y)
    assert ((mdl.A_pinv(y.double()) - xr).norm() / xr.norm()).item() < 1e-5
    z = mdl.Vt(x)
    assert ((mdl.V(z) - x.double().reshape(B, -1)).norm() / x.double().norm()).item() < 1e-12
    assert torch.equal(z[:, :mdl.n_meas], mdl.A(x.double()))
