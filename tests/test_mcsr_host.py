"""Old-photo restoration (svd_operators.MaskColorSR: mask, grey, average pool) on the host: the dense float64 model of
the operator that the GPU tests compare against (tests/test_gpu_mcsr.py imports it from here) checked against itself
and against the closed forms the kernels evaluate, the `--deg mask_color_sr` / `sr_color` names of build_operator, the
measurement's shape, and the argument validation of the `*_mcsr_*` entry points through the built library.  No GPU.

    y_j = sum_c sum_{p in j} w_c m_p x[c][p] / r^2,   s_j = sqrt(k_j) |w| / r^2,   q_j[c][p] = w_c m_p / (sqrt(k_j) |w|),
    (A^+ y)[c][p] = m_p w_c r^2 y_j / (k_j |w|^2)     (site j = an r x r block with k_j kept pixels; k_j = 0: null space)
"""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

ETA = 0.85
W_THIRDS = (1 / 3, 1 / 3, 1 / 3)
W_LUMA = (0.299, 0.587, 0.114)
# (abar', sigma_y) of the one-step DDNM+ checks, sigma_t = sqrt(1 - abar'), a = sqrt(abar'); a site is damped (lambda < 1)
# where sigma_t < a sigma_y / s_j and full (lambda = 1) where sigma_t > a sigma_y / s_j.
#   mixed:  with w = 1/3 and r = 4, a sigma_y / s_j = 1.96 (k = 1), 0.876 (k = 5), 0.566 (k = 12) around sigma_t = 0.707
#   damped: the largest s_j there is, |w| = 0.577 (r = 1), still has a sigma_y / s_j = 0.69 > sigma_t = 0.1
#   full:   the smallest, |w| / 64 (r = 8, k = 1), has a sigma_y / s_j = 0.078 < sigma_t = 0.707
PLUS_SETTINGS = {"mixed": (0.5, 0.1), "damped": (0.99, 0.4), "full": (0.5, 0.001)}
DENSE_V_LIMIT = 768      # a full V (3 d^2 square) is formed up to d = 16


def check_mask():
    """The 8 x 8 mask of the r = 4 self-checks: sites (row-major) with 0, 1, 5 and 12 kept pixels of 16; the one kept pixel
    of site 1 lies in the site's last row and column."""
    m = np.zeros((8, 8), np.int64)
    m[3, 7] = 1                                             # site 1: k = 1
    m[4, 0:4] = 1
    m[5, 0] = 1                                             # site 2: k = 5
    m[4:7, 4:8] = 1                                         # site 3: k = 12
    return m


def site_counts(mask, r, d):
    m = np.ones((d, d)) if mask is None else np.asarray(mask, dtype=np.float64)
    return m.reshape(d // r, r, d // r, r).sum(axis=(1, 3)).reshape(-1)


def _coef(s, a, sigma_y, sigma_t, eta):
    from ddnm_amd.functions.svd_operators import spectral_coefficients
    return spectral_coefficients(float(s), float(a), float(sigma_y), float(sigma_t), eta)


class DenseModel:
    """float64 model of MaskColorSR from the matrix itself: A [(d/r)^2, 3 d^2] is built entry by entry, A^+ is
    numpy.linalg.pinv, and the DDNM+ step is V (a (x^0 - mu (x^0 - y^)) + d1 V^T n + d2 V^T eps) with the SVD's V, x^ = V^T x,
    y^ = S^+ U^T y and (lambda, d1, d2) = spectral_coefficients per singular value (mu = lambda where s > 0, else 0).
    Up to 3 d^2 = DENSE_V_LIMIT the full V is formed and the formula is applied as written; beyond, only the rows of V^T
    that span the row space are (`full_matrices=False`) and V f(S) V^T v = f(0) v + V_r (f(s) - f(0)) V_r^T v, the same
    product since the columns left out all carry f(0) -- `test_thin_and_full_v_agree` holds the two forms together.
    `A`, `A_pinv`, `Lambda`, `Lambda_noise` take and return [n, .] tensors in the argument's dtype (oracle.sampler)."""

    def __init__(self, mask, r, w, d, full=None):
        self.r, self.d, self.w = r, d, np.asarray(w, dtype=np.float64)
        self.m = np.ones((d, d)) if mask is None else np.asarray(mask, dtype=np.float64)
        n = d // r
        A = np.zeros((n * n, 3 * d * d))
        for c in range(3):
            for py in range(d):
                for px in range(d):
                    A[(py // r) * n + px // r, c * d * d + py * d + px] = self.w[c] * self.m[py, px] / r ** 2
        self.Amat, self.pinv = A, np.linalg.pinv(A.T).T              # (A^T)^+ = (A^+)^T; LAPACK is quicker on the tall matrix
        self.full = 3 * d * d <= DENSE_V_LIMIT if full is None else full
        U, S, Vh = np.linalg.svd(A, full_matrices=self.full)
        S = np.where(S > 1e-12, S, 0.0)
        self.U, self.S, self.Vh = U, S, Vh
        self.Sfull = np.concatenate([S, np.zeros(Vh.shape[0] - S.size)])        # one value per row of Vh

    # ---- linear algebra in numpy float64 on [n, .] arrays
    def _spread(self, f_of_s, f0, v):
        """V diag(f) V^T v, f = f_of_s on the rows of Vh and f0 on the columns of V left out (none when `full`)."""
        vh = v @ self.Vh.T
        if self.full:
            return (vh * f_of_s) @ self.Vh
        return f0 * v + (vh * (f_of_s - f0)) @ self.Vh

    def coefficients(self, a, sigma_y, sigma_t, eta):
        tab = np.array([_coef(s, a, sigma_y, sigma_t, eta) for s in self.Sfull])
        return tab[:, 0], tab[:, 1], tab[:, 2], _coef(0.0, a, sigma_y, sigma_t, eta)

    def step(self, xt, et, n, y, abar_t, abar_next, sigma_y, eta, lam=None):
        """(x0|t, x_{t-1}) of one reverse step on [B, 3 d^2] / [B, (d/r)^2] float64 arrays: DDNM with `lam` given
        (x0 - lam A^+(A x0 - y), then the DDIM update), DDNM+ otherwise (the formula of the class docstring)."""
        a, sigma_t = abar_next ** 0.5, (1 - abar_next) ** 0.5
        x0 = (xt - et * (1 - abar_t) ** 0.5) / abar_t ** 0.5
        if lam is not None:
            x0h = x0 - lam * ((x0 @ self.Amat.T - y) @ self.pinv.T)
            return x0, a * x0h + sigma_t * eta * n + sigma_t * (1 - eta ** 2) ** 0.5 * et
        lmb, d1, d2, (_, d1n, d2n) = self.coefficients(a, sigma_y, sigma_t, eta)
        mu = np.where(self.Sfull > 0, lmb, 0.0)
        Sinv = np.where(self.S > 0, 1.0 / np.where(self.S > 0, self.S, 1.0), 0.0)
        y_hat = np.zeros((y.shape[0], self.Vh.shape[0]))
        y_hat[:, :self.S.size] = (y @ self.U) * Sinv
        x0_hat, n_hat, e_hat = x0 @ self.Vh.T, n @ self.Vh.T, et @ self.Vh.T
        z = a * (x0_hat - mu * (x0_hat - y_hat)) + d1 * n_hat + d2 * e_hat
        if self.full:
            return x0, z @ self.Vh
        rest = a * x0 + d1n * n + d2n * et                      # the columns of V left out: mu = 0, (d1n, d2n)
        return x0, rest + (z - (a * x0_hat + d1n * n_hat + d2n * e_hat)) @ self.Vh

    # ---- the operator protocol of oracle.sampler (torch in, torch out, the argument's dtype)
    @staticmethod
    def _np(v):
        return v.detach().double().cpu().reshape(v.shape[0], -1).numpy()

    @staticmethod
    def _like(out, v):
        return torch.from_numpy(np.ascontiguousarray(out)).to(v.dtype)

    def A(self, x):
        return self._like(self._np(x) @ self.Amat.T, x)

    def A_pinv(self, y):
        return self._like(self._np(y) @ self.pinv.T, y)

    def Lambda(self, vec, a, sigma_y, sigma_t, eta):
        lmb = self.coefficients(a, sigma_y, sigma_t, eta)[0]
        return self._like(self._spread(lmb, 1.0, self._np(vec)), vec)

    def Lambda_noise(self, vec, a, sigma_y, sigma_t, eta, epsilon):
        _, d1, d2, (_, d1n, d2n) = self.coefficients(a, sigma_y, sigma_t, eta)
        return self._like(self._spread(d1, d1n, self._np(vec)) + self._spread(d2, d2n, self._np(epsilon)), vec)


def model_operator(mask, r, w, d):
    """The dense float64 model of MaskColorSR(3, d, mask, r, weights=w), with the weights as given (`kernel_weights(w)`:
    as the kernels get them)."""
    return DenseModel(mask, r, w, d)


def kernel_weights(w):
    """The grey weights rounded to fp32, as the entry points receive them."""
    return tuple(float(np.float32(v)) for v in w)


# ---- the closed forms (what the kernels evaluate), float64
def closed_singulars(mask, r, w, d):
    w = np.asarray(w, dtype=np.float64)
    return np.sqrt(site_counts(mask, r, d)) * np.sqrt((w ** 2).sum()) / r ** 2


def _site_of_pixel(r, d):
    py, px = np.divmod(np.arange(d * d), d)
    return (py // r) * (d // r) + px // r


def closed_pinv(mask, r, w, d, y):
    """[B, (d/r)^2] -> [B, 3 d^2]: m_p w_c r^2 y_j / (k_j |w|^2), 0 on empty sites."""
    w = np.asarray(w, dtype=np.float64)
    m = (np.ones((d, d)) if mask is None else np.asarray(mask, dtype=np.float64)).reshape(-1)
    k = site_counts(mask, r, d)
    g = np.where(k > 0, y * r ** 2 / np.where(k > 0, k, 1.0), 0.0)[:, _site_of_pixel(r, d)] * m          # [B, d^2]
    return np.concatenate([g * (w[c] / (w ** 2).sum()) for c in range(3)], axis=1)


def closed_plus_step(mask, r, w, d, xt, et, n, y, abar_t, abar_next, sigma_y, eta):
    """The DDNM+ step as three dot products per site:
    x_{t-1} = a x0 + d1n n + d2n eps + q_j [-a lambda_j (q_j.x0 - y_j / s_j) + (d1_j - d1n) q_j.n + (d2_j - d2n) q_j.eps]."""
    w = np.asarray(w, dtype=np.float64)
    m = (np.ones((d, d)) if mask is None else np.asarray(mask, dtype=np.float64)).reshape(-1)
    k, s = site_counts(mask, r, d), closed_singulars(mask, r, w, d)
    a, sigma_t = abar_next ** 0.5, (1 - abar_next) ** 0.5
    x0 = (xt - et * (1 - abar_t) ** 0.5) / abar_t ** 0.5
    _, d1n, d2n = _coef(0.0, a, sigma_y, sigma_t, eta)
    out = a * x0 + d1n * n + d2n * et
    site = _site_of_pixel(r, d)
    wn = np.sqrt((w ** 2).sum())
    for j in np.nonzero(k)[0]:
        q = np.concatenate([w[c] * m * (site == j) for c in range(3)]) / (np.sqrt(k[j]) * wn)
        lam, d1, d2 = _coef(s[j], a, sigma_y, sigma_t, eta)
        amp = -a * lam * (x0 @ q - y[:, j] / s[j]) + (d1 - d1n) * (n @ q) + (d2 - d2n) * (et @ q)
        out = out + amp[:, None] * q[None, :]
    return x0, out


def step_inputs(d, r, B, seed=31):
    """Seeded (x_orig in [-1, 1], x_t, eps (6 channels), n) of a one-step case; never written to."""
    g = torch.Generator().manual_seed(seed + 100 * d + r)
    return (torch.rand(B, 3, d, d, generator=g) * 2 - 1, torch.randn(B, 3, d, d, generator=g),
            torch.randn(B, 6, d, d, generator=g), torch.randn(B, 3, d, d, generator=g))


def _flat64(t):
    return t.double().reshape(t.shape[0], -1).numpy()


def _config(d):
    return argparse.Namespace(data=argparse.Namespace(channels=3, image_size=d))


# ---------------------------------------------------------------------------------------------- 1. model self-checks
@pytest.fixture(scope="module")
def check_model():
    return model_operator(check_mask(), 4, W_THIRDS, 8)


def test_check_mask_has_the_sites_it_names():
    assert site_counts(check_mask(), 4, 8).tolist() == [0, 1, 5, 12]
    assert check_mask()[3, 7] == 1                          # last row and column of site 1


def test_closed_form_singulars_and_pinv_equal_the_dense_ones(check_model):
    M = check_model
    s = closed_singulars(check_mask(), 4, W_THIRDS, 8)
    assert M.full and np.abs(np.sort(s)[::-1] - M.S).max() < 1e-12
    assert np.count_nonzero(M.S) == 3                       # the empty site is null space
    y = np.random.default_rng(3).standard_normal((2, 4))
    assert np.abs(closed_pinv(check_mask(), 4, W_THIRDS, 8, y) - y @ M.pinv.T).max() < 1e-12
    # rows with disjoint supports: A A^T is diagonal with the s_j^2 on it
    assert np.abs(M.Amat @ M.Amat.T - np.diag(s ** 2)).max() < 1e-15


@pytest.mark.parametrize("setting", sorted(PLUS_SETTINGS))
def test_closed_form_step_equals_the_dense_step(check_model, setting):
    abar_next, sigma_y = PLUS_SETTINGS[setting]
    x, xt, et6, n = step_inputs(8, 4, 2)
    y = _flat64(x) @ check_model.Amat.T
    args = (_flat64(xt), _flat64(et6[:, :3]), _flat64(n), y, 0.45, abar_next, sigma_y, ETA)
    x0_d, out_d = check_model.step(*args)
    x0_c, out_c = closed_plus_step(check_mask(), 4, W_THIRDS, 8, *args)
    assert np.abs(x0_d - x0_c).max() == 0 and np.abs(out_d - out_c).max() < 1e-12
    # ... and the dense step is the loop body of oracle.sampler.ddnm_plus_diffusion spelled with Lambda / Lambda_noise
    a, sigma_t = abar_next ** 0.5, (1 - abar_next) ** 0.5
    t = lambda v: torch.from_numpy(v)      # noqa: E731
    corr = check_model.A_pinv(check_model.A(t(x0_d)) - t(y))
    ref = a * (t(x0_d) - check_model.Lambda(corr, a, sigma_y, sigma_t, ETA)) \
        + check_model.Lambda_noise(t(args[2]), a, sigma_y, sigma_t, ETA, t(args[1]))
    assert (ref - t(out_d)).abs().max() < 1e-12


def test_regimes_of_the_mixed_setting():
    """abar' = 0.5, sigma_y = 0.1, eta = 0.85: the sites with k = 1 and 5 are damped, the site with k = 12 is full."""
    abar_next, sigma_y = PLUS_SETTINGS["mixed"]
    a, sigma_t = abar_next ** 0.5, (1 - abar_next) ** 0.5
    s = closed_singulars(check_mask(), 4, W_THIRDS, 8)
    assert s[0] == 0
    assert [sigma_t < a * sigma_y / v for v in s[1:]] == [True, True, False]
    assert [_coef(v, a, sigma_y, sigma_t, ETA)[0] < 1 for v in s[1:]] == [True, True, False]
    for name, (ab, sy) in PLUS_SETTINGS.items():            # the other two settings, at the extreme singular values
        lo, hi = np.sqrt(1 / 3) / 64, np.sqrt(1 / 3)
        damped = [(1 - ab) ** 0.5 < ab ** 0.5 * sy / v for v in (lo, hi)]
        assert damped == {"mixed": [True, False], "damped": [True, True], "full": [False, False]}[name], name


@pytest.mark.parametrize("r", [1, 2, 4, 8])
def test_thin_and_full_v_agree(r):
    """The two forms of DenseModel (full V up to d = 16, row-space rows beyond) are the same operator: step, Lambda and
    Lambda_noise at d = 8 with both, every pool factor, a random mask with an empty site."""
    rng = np.random.default_rng(r)
    mask = (rng.random((8, 8)) < 0.6).astype(np.int64)
    mask[:r, :r] = 0
    full, thin = DenseModel(mask, r, W_LUMA, 8, full=True), DenseModel(mask, r, W_LUMA, 8, full=False)
    x, xt, et6, n = step_inputs(8, r, 2)
    y = _flat64(x) @ full.Amat.T
    for abar_next, sigma_y in PLUS_SETTINGS.values():
        args = (_flat64(xt), _flat64(et6[:, :3]), _flat64(n), y, 0.45, abar_next, sigma_y, ETA)
        assert np.abs(full.step(*args)[1] - thin.step(*args)[1]).max() < 1e-12
        assert np.abs(full.step(*args)[1] - closed_plus_step(mask, r, W_LUMA, 8, *args)[1]).max() < 1e-12
        a, sigma_t = abar_next ** 0.5, (1 - abar_next) ** 0.5
        v, e = torch.from_numpy(args[2]), torch.from_numpy(args[1])
        assert (full.Lambda(v, a, sigma_y, sigma_t, ETA) - thin.Lambda(v, a, sigma_y, sigma_t, ETA)).abs().max() < 1e-12
        assert (full.Lambda_noise(v, a, sigma_y, sigma_t, ETA, e)
                - thin.Lambda_noise(v, a, sigma_y, sigma_t, ETA, e)).abs().max() < 1e-12


def test_the_chained_inverse_of_the_simplified_path_is_no_pseudo_inverse(check_model):
    """oracle.operators.mask_color_sr: its A is the model's; its Ap = mask . colour . upsample equals A^+ on a site-aligned
    mask and is A^+ scaled by k_j / r^2 on a site the mask cuts, so A Ap has 1/16, 5/16 and 12/16 on its diagonal there."""
    from oracle import operators as O
    x = step_inputs(8, 4, 2)[0].double()
    cut = torch.from_numpy(check_mask()).double()
    A, Ap = O.mask_color_sr(cut, 4, 8)
    assert (A(x)[:, 0].reshape(2, -1) - check_model.A(x)).abs().max() < 1e-12
    y = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 4)))
    chain = Ap(y.reshape(2, 1, 2, 2).repeat(1, 3, 1, 1)).reshape(2, 3, 2, 4, 2, 4)      # [B, c, site row, ., site col, .]
    exact = check_model.A_pinv(y).reshape(2, 3, 2, 4, 2, 4)
    k = site_counts(check_mask(), 4, 8).reshape(2, 2)
    for sy in range(2):
        for sx in range(2):
            scale = 16 / k[sy, sx] if k[sy, sx] else 1.0
            assert (chain[:, :, sy, :, sx] * scale - exact[:, :, sy, :, sx]).abs().max() < 1e-12, (sy, sx)
    diag = np.diag(check_model.Amat @ _flat64(Ap(torch.eye(4).double().reshape(4, 1, 2, 2).repeat(1, 3, 1, 1))).T)
    assert np.abs(diag - k.reshape(-1) / 16).max() < 1e-12
    # a site-aligned mask (whole sites kept or missing): the chain IS the pseudo-inverse
    aligned = np.kron(np.array([[1, 0], [1, 1]]), np.ones((4, 4), np.int64))
    M = model_operator(aligned, 4, W_THIRDS, 8)
    _, Ap2 = O.mask_color_sr(torch.from_numpy(aligned).double(), 4, 8)
    assert (Ap2(y.reshape(2, 1, 2, 2).repeat(1, 3, 1, 1)).reshape(2, -1) - M.A_pinv(y)).abs().max() < 1e-12


# ---------------------------------------------------------------------------------------------- 2. operator and names
def test_operator_tables():
    from ddnm_amd.functions import svd_operators as E
    op = E.MaskColorSR(3, 8, check_mask(), 4, "cpu")
    assert op.measurement_size() == 4 and op.measurement_image_shape() == (1, 2, 2)
    assert op.kept.tolist() == [0, 1, 5, 12] and op.mask.shape == (64,) and op.mask.dtype == torch.float32
    s = closed_singulars(check_mask(), 4, W_THIRDS, 8)
    assert op.singulars().shape == (4,) and np.abs(op.singulars().double().numpy() - s).max() < 1e-7
    none = E.MaskColorSR(3, 16, None, 8, "cpu", weights=W_LUMA)
    assert none.mask is None and none.kept.tolist() == [64] * 4 and none.measurement_image_shape() == (1, 2, 2)
    assert [float(v) for v in none._w] == [float(np.float32(v)) for v in W_LUMA]
    assert torch.equal(E.MaskColorSR(3, 8, torch.from_numpy(check_mask()), 4, "cpu").mask, op.mask)      # a tensor mask too
    for name in ("Lambda", "V", "Vt", "U", "Ut"):
        with pytest.raises(NotImplementedError):
            getattr(op, name)(torch.zeros(1, 4), *([0.5, 0.1, 0.5, ETA] if name == "Lambda" else []))
    with pytest.raises(NotImplementedError):
        op.Lambda_noise(torch.zeros(1, 192), 0.5, 0.1, 0.5, ETA, torch.zeros(1, 192))


def test_constructor_refusals():
    from ddnm_amd.functions import svd_operators as E
    ok = np.ones((16, 16), np.int64)
    with pytest.raises(ValueError, match="channels"):
        E.MaskColorSR(1, 16, ok, 4, "cpu")
    with pytest.raises(ValueError, match="ratio"):
        E.MaskColorSR(3, 16, ok, 3, "cpu")
    with pytest.raises(ValueError, match="ratio"):
        E.MaskColorSR(3, 16, ok, 16, "cpu")
    with pytest.raises(ValueError, match="multiple of the pool ratio"):
        E.MaskColorSR(3, 12, np.ones((12, 12)), 8, "cpu")
    with pytest.raises(ValueError, match="multiple of 4"):
        E.MaskColorSR(3, 6, np.ones((6, 6)), 2, "cpu")
    with pytest.raises(ValueError, match="shape"):
        E.MaskColorSR(3, 16, np.ones((16, 8)), 4, "cpu")
    with pytest.raises(ValueError, match="shape"):
        E.MaskColorSR(3, 16, np.ones((2, 16, 16)), 4, "cpu")
    with pytest.raises(ValueError, match="0 .* 1"):
        E.MaskColorSR(3, 16, ok * 0.5, 4, "cpu")
    with pytest.raises(ValueError, match="weights"):
        E.MaskColorSR(3, 16, ok, 4, "cpu", weights=(0, 0, 0))
    with pytest.raises(ValueError, match="weights"):
        E.MaskColorSR(3, 16, ok, 4, "cpu", weights=(1, 1))


def test_build_operator_maps_both_names(tmp_path):
    """`--deg mask_color_sr` reads the 2-D mask and takes r from round(deg_scale); `--deg sr_color` has no mask; a bank of
    masks is refused with the reason.  (Both names ended in `degradation type not supported` before.)"""
    from ddnm_amd.functions import svd_operators as E
    path = str(tmp_path / "mask.npy")
    rng = np.random.default_rng(2)
    mask = (rng.random((16, 16)) < 0.6).astype(np.float32)
    np.save(path, mask)
    for scale, r in ((4, 4), (4.0, 4), (1, 1), (2.2, 2), (8, 8)):
        op = E.build_operator("mask_color_sr", scale, _config(16), "cpu", mask_path=path)
        assert isinstance(op, E.MaskColorSR) and op.ratio == r and isinstance(op.ratio, int)
        assert np.array_equal(op.mask.numpy().reshape(16, 16), mask) and op.weights == W_THIRDS
        assert op.kept.tolist() == site_counts(mask, r, 16).tolist()
    op = E.build_operator("sr_color", 4, _config(16), "cpu", mask_path=str(tmp_path / "absent.npy"))      # no file is read
    assert isinstance(op, E.MaskColorSR) and op.mask is None and op.ratio == 4 and op.measurement_size() == 16
    np.save(path, np.ones((3, 16, 16), np.float32))
    with pytest.raises(ValueError, match="inpainting feature"):
        E.build_operator("mask_color_sr", 4, _config(16), "cpu", mask_path=path)
    np.save(path, mask)
    with pytest.raises(ValueError, match="ratio"):
        E.build_operator("mask_color_sr", 3, _config(16), "cpu", mask_path=path)
    with pytest.raises(ValueError, match="ratio"):
        E.build_operator("sr_color", 0.0, _config(16), "cpu")
    # the simplified path keeps the Composition and the reference's chain
    comp = E.mask_color_sr(3, 16, torch.from_numpy(mask), 4, "cpu")
    assert isinstance(comp, E.Composition) and [type(p).__name__ for p in comp.parts] == ["PixelMask", "Colorization",
                                                                                        "SuperResolution"]


def test_a_small_grey_picture_is_a_measurement(tmp_path):
    """A scan is a grey (d/r) x (d/r) picture: it loads to data_transform of its pixels exactly; an RGB picture or one of
    the full size is refused when the folder is bound."""
    from PIL import Image
    from ddnm_amd.functions import svd_operators as E
    from ddnm_amd.guided_diffusion import diffusion as D
    cfg = argparse.Namespace(data=argparse.Namespace(channels=3, image_size=16, rescaled=True))
    op = E.MaskColorSR(3, 16, None, 4, "cpu")
    rng = np.random.default_rng(8)
    grey = rng.integers(0, 256, (4, 4), dtype=np.uint8)
    good = tmp_path / "good"
    good.mkdir()
    Image.fromarray(grey).save(good / "scan_0.png")
    np.save(good / "scan_1.npy", np.zeros(16, np.float32))
    ds = D.MeasurementFolder(str(good)).bind(op, cfg)
    x, picture = ds[0]
    assert picture and x.shape == (1, 4, 4)
    assert torch.equal(x, D.data_transform(cfg, torch.from_numpy(grey.copy()).float().div(255.0))[None])
    assert ds[1][0].shape == (16,) and not ds[1][1]
    for name, arr in (("rgb", rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)),
                      ("full", rng.integers(0, 256, (16, 16), dtype=np.uint8))):
        folder = tmp_path / name
        folder.mkdir()
        Image.fromarray(arr).save(folder / "scan_0.png")
        with pytest.raises(ValueError, match="scan_0.png"):
            D.MeasurementFolder(str(folder)).bind(op, cfg)
    short = tmp_path / "short"
    short.mkdir()
    np.save(short / "scan_0.npy", np.zeros(15, np.float32))
    with pytest.raises(ValueError, match="15"):
        D.MeasurementFolder(str(short)).bind(op, cfg)


# ---------------------------------------------------------------------------------------------- 3. argument validation
def check_mcsr_validation(lib, ptr):
    """Every refusal of the six `*_mcsr_*` entry points, with distinct addresses from `ptr` on standing for the tensors
    (never dereferenced: all of it happens before a launch).  DDNM_E_BADARG = -1 comes before DDNM_E_SHAPE = -2."""
    from ddnm_amd._lib import StepScalars
    s = StepScalars()
    s.rng_on = 1
    sp = ctypes.byref(s)
    w = (ctypes.c_float * 3)(1 / 3, 1 / 3, 1 / 3)
    zero = (ctypes.c_float * 3)(0, 0, 0)
    P = [ptr + 64 * i for i in range(8)]                    # xt, et, y, mask, x0, xt_next, keys / noise, spare

    def op(fn, a=P[0], mask=P[3], b=P[2], B=2, H=16, W=16, r=4, wt=w):
        return fn(a, mask, b, B, H, W, r, wt, None)

    def step(fn, xt=P[0], et=P[1], es=768, nz=None, y=P[2], mask=P[3], x0=P[4], xn=P[5], B=2, H=16, W=16, r=4, wt=w, sc=sp):
        extra = (0.1, 0.5, ETA) if "plus" in fn.__name__ else ()
        return fn(xt, et, es, nz, y, mask, x0, xn, B, H, W, r, wt, *extra, sc, None)

    ops_ = (lib.ddnm_op_mcsr_A_f32, lib.ddnm_op_mcsr_pinv_f32)
    steps = (lib.ddnm_step_mcsr_f32, lib.ddnm_step_plus_mcsr_f32)
    keyed = (lib.ddnm_step_mcsr_keyed_f32, lib.ddnm_step_plus_mcsr_keyed_f32)
    for fn in ops_:
        assert op(fn, a=None) == -1 and op(fn, b=None) == -1 and op(fn, wt=None) == -1, fn.__name__
        assert op(fn, B=0) == -1 and op(fn, B=-2) == -1 and op(fn, wt=zero) == -1, fn.__name__
        assert op(fn, a=None, r=3) == -1 and op(fn, wt=zero, W=6) == -1, fn.__name__          # ... wins over a bad shape
        for r in (0, 3, 5, 16, -4):
            assert op(fn, r=r) == -2, (fn.__name__, r)
        assert op(fn, H=18) == -2 and op(fn, W=18) == -2 and op(fn, W=6, r=2) == -2 and op(fn, H=0) == -2, fn.__name__
        assert op(fn, H=12, r=8) == -2 and op(fn, W=12, r=8) == -2, fn.__name__
    for fn in steps + keyed:
        nz = P[6] if fn in keyed else None                  # (a multiple of 16: a valid key table address)
        for arg in ("xt", "et", "y", "xn", "wt", "sc"):
            assert step(fn, nz=nz, **{arg: None}) == -1, (fn.__name__, arg)
        assert step(fn, nz=nz, B=0) == -1 and step(fn, nz=nz, wt=zero) == -1, fn.__name__
        assert step(fn, nz=nz, y=None, W=6) == -1 and step(fn, nz=nz, B=0, r=3) == -1, fn.__name__
        # two passes over a strip: an output that is xt, et or the other output is refused
        assert step(fn, nz=nz, xn=P[0]) == -1 and step(fn, nz=nz, xn=P[1]) == -1 and step(fn, nz=nz, xn=P[4]) == -1
        assert step(fn, nz=nz, x0=P[0]) == -1 and step(fn, nz=nz, x0=P[1]) == -1, fn.__name__
        for r in (0, 3, 16):
            assert step(fn, nz=nz, r=r) == -2, (fn.__name__, r)
        assert step(fn, nz=nz, H=18) == -2 and step(fn, nz=nz, W=18) == -2 and step(fn, nz=nz, W=6, r=2) == -2, fn.__name__
        assert step(fn, nz=nz, H=12, r=8) == -2 and step(fn, nz=nz, es=770) == -2 and step(fn, nz=nz, es=6) == -2, fn.__name__
    for fn in keyed:
        assert step(fn, nz=None) == -1 and step(fn, nz=P[6] + 4) == -1, fn.__name__          # null / misaligned key table
    off = StepScalars()                                      # rng_on = 0 and no noise tensor: no source
    for fn in steps:
        assert step(fn, sc=ctypes.byref(off)) == -1, fn.__name__
    # x0 is optional in the noise-free step only (with everything else valid that call would launch: checked on the GPU)
    assert step(lib.ddnm_step_plus_mcsr_f32, x0=None) == -1 and step(lib.ddnm_step_plus_mcsr_keyed_f32, nz=P[6], x0=None) == -1


def test_argument_validation_without_gpu():
    """The pattern of tests/test_cabi.py::test_argument_validation_without_gpu: the entry points refuse bad arguments
    before touching the device, so the built library answers on a host without one."""
    from ddnm_amd import _lib, build
    build.build()
    lib = _lib.lib()
    assert lib.ddnm_version() == 7
    check_mcsr_validation(lib, 4096)


def test_hooks_marshal_their_arguments():
    """Host-only dry run (tools/dry_run.py): A, A_pinv, ddnm_step and the DDNM+ hook reach their entry points with arguments
    of the declared types, with and without a mask, for a tensor, an in-kernel and a keyed noise source."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import dry_run
    finally:
        sys.path.pop(0)
    from ddnm_amd import _lib, ops
    from ddnm_amd.functions import svd_operators as E
    saved = (_lib._lib, ops._stream, ops._f32c, ops._f16c)
    try:
        dry = dry_run.install()
        d, B = 16, 2
        for mask in (None, np.ones((d, d))):
            op = E.MaskColorSR(3, d, mask, 8, "cpu")
            x = torch.zeros(B, 3, d, d)
            y = op.A(x)
            assert y.shape == (B, 4) and op.A_pinv(y).shape == (B, 3 * d * d)
            et6 = torch.zeros(B, 6, d, d)
            s = ops.step_scalars(torch.tensor(0.5), torch.tensor(0.6), ETA)
            out = torch.zeros_like(x), torch.zeros_like(x)
            op.ddnm_step(x, et6[:, :3], torch.zeros_like(x), y, s, *out)
            op.ddnm_step(x, et6[:, :3], None, y, ops.PhiloxNoise(5).stamp(s, 1), None, out[1])
            with pytest.raises(RuntimeError, match="begin_plus_run"):
                op.ddnm_plus_step(x, et6[:, :3], None, s, 0.2, 0.5, ETA, *out)
            op.begin_plus_run(y)
            op.ddnm_plus_step(x, et6[:, :3], torch.zeros_like(x), s, 0.2, 0.5, ETA, *out)
            with pytest.raises(ValueError):
                op.ddnm_step(x, et6[:, :3], None, y[:, :-1], s, *out)
            with pytest.raises(ValueError):
                op.A_pinv(y[:, :-1])
        assert dry.calls == {"ddnm_op_mcsr_A_f32": 2, "ddnm_op_mcsr_pinv_f32": 2, "ddnm_step_mcsr_f32": 4,
                             "ddnm_step_plus_mcsr_f32": 2}
    finally:
        _lib._lib, ops._stream, ops._f32c, ops._f16c = saved
