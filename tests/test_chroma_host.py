"""Chroma-subsampled restoration (svd_operators.ChromaSubsample: full-resolution luma, chroma averaged per rw x rh site)
on the host: the dense float64 model of the operator that the GPU tests compare against (tests/test_gpu_chroma.py imports
it from here) checked against itself and against the closed forms the kernels evaluate, `ddnm_chroma_constants` against
numpy, the `--deg chroma_*` names of build_operator, the measurement's shape, and the argument validation of the
`*_chroma_*` entry points through the built library.  No GPU.

    Y[p] = w_Y . x[:, p],  Cb[site] = mean_{p in site} w_Cb . x[:, p],  Cr likewise;  y row = [ Y | Cb | Cr ]
    (A^+ y)[:, p] = w+ (Y_p - Ybar) + M^-1 (Ybar, Cb, Cr)^T,  w+ = w_Y / |w_Y|^2,  Ybar the site mean of Y
    singular values: |w_Y| (n - 1 per site) and those of D = diag(1, 1/sqrt n, 1/sqrt n) M (one each per site)
"""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

ETA = 0.85
BT601 = ((0.299, 0.587, 0.114), (-0.168736, -0.331264, 0.5), (0.5, -0.418688, -0.081312))


def ycbcr_matrix(kr, kb):
    """Full-range Y'CbCr from the luma coefficients: Cb = (B - Y) / (2 (1 - Kb)), Cr = (R - Y) / (2 (1 - Kr))."""
    kg = 1.0 - kr - kb
    return ((kr, kg, kb), (-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), 0.5), (0.5, -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr))))


BT709 = ycbcr_matrix(0.2126, 0.0722)
MATRICES = {"bt601": BT601, "bt709": BT709}
SITES = [(2, 1), (4, 1), (2, 2), (4, 4), (8, 8)]                      # (rw, rh): columns x rows
# (abar', sigma_y) of the one-step DDNM+ checks, sigma_t = sqrt(1 - abar'), a = sqrt(abar'); a singular value s is damped
# (lambda < 1) where s < tau = a sigma_y / sigma_t and full (lambda = 1) where s > tau.
#   damped: tau = 3.98, above every singular value (the largest is 0.75, |w_Y| of BT.709)
#   full:   tau = 0.001, below every singular value (the smallest is 0.068, Cr at 8 x 8)
#   mixed:  tau = 0.54, between the chroma values (at most 0.4545, BT.601 Cb at n = 2) and the luma ones (at least 0.66856):
#           luma full, chroma damped, at every site and with both matrices (test_regimes_are_what_their_names_say)
PLUS_SETTINGS = {"mixed": (0.9, 0.18), "damped": (0.99, 0.4), "full": (0.5, 0.001)}
DENSE_LIMIT = 768         # the whole-image matrix (3 d^2 columns) is formed up to d = 16


def kernel_matrix(M):
    """The colour matrix rounded to fp32, as the entry points receive it (float64 array of fp32 values)."""
    return np.asarray(M, dtype=np.float32).astype(np.float64)


def _coef(s, a, sigma_y, sigma_t, eta):
    from ddnm_amd.functions.svd_operators import spectral_coefficients
    return spectral_coefficients(float(s), float(a), float(sigma_y), float(sigma_t), eta)


def dense_matrix(rw, rh, M, H, W):
    """A [H W + 2 H W / n, 3 H W] of an H x W image, entry by entry (float64)."""
    M = np.asarray(M, dtype=np.float64)
    n, sw, sites = rw * rh, W // rw, (H // rh) * (W // rw)
    A = np.zeros((H * W + 2 * sites, 3 * H * W))
    for c in range(3):
        for i in range(H):
            for j in range(W):
                col, site = c * H * W + i * W + j, (i // rh) * sw + j // rw
                A[i * W + j, col] = M[0, c]
                A[H * W + site, col] = M[1, c] / n
                A[H * W + sites + site, col] = M[2, c] / n
    return A


class _Dense:
    """float64 linear algebra of one explicit matrix A [rows, cols]: A^+ is numpy.linalg.pinv, and the DDNM+ step is
    V (a (x^0 - mu (x^0 - y^)) + d1 V^T n + d2 V^T eps) with the full SVD's V, x^ = V^T x, y^ = S^+ U^T y and
    (lambda, d1, d2) = spectral_coefficients per singular value (mu = lambda where s > 0, else 0)."""

    def __init__(self, A):
        self.Amat, self.pinv = A, np.linalg.pinv(A)
        U, S, Vh = np.linalg.svd(A, full_matrices=True)
        S = np.where(S > 1e-12, S, 0.0)
        self.U, self.S, self.Vh = U, S, Vh
        self.Sfull = np.concatenate([S, np.zeros(Vh.shape[0] - S.size)])        # one value per row of Vh

    def coefficients(self, a, sigma_y, sigma_t, eta):
        memo = {}
        tab = np.array([memo.setdefault(s, _coef(s, a, sigma_y, sigma_t, eta)) for s in self.Sfull])
        return tab[:, 0], tab[:, 1], tab[:, 2]

    def spread(self, f, v):
        """V diag(f) V^T v"""
        return ((v @ self.Vh.T) * f) @ self.Vh

    def plus(self, x0, et, n, y, a, sigma_y, sigma_t, eta):
        lmb, d1, d2 = self.coefficients(a, sigma_y, sigma_t, eta)
        mu = np.where(self.Sfull > 0, lmb, 0.0)
        Sinv = np.where(self.S > 0, 1.0 / np.where(self.S > 0, self.S, 1.0), 0.0)
        y_hat = np.zeros((y.shape[0], self.Vh.shape[0]))
        y_hat[:, :self.S.size] = (y @ self.U)[:, :self.S.size] * Sinv
        x0_hat, n_hat, e_hat = x0 @ self.Vh.T, n @ self.Vh.T, et @ self.Vh.T
        return (a * (x0_hat - mu * (x0_hat - y_hat)) + d1 * n_hat + d2 * e_hat) @ self.Vh


class DenseModel:
    """float64 model of ChromaSubsample(3, d, rw, rh, matrix=M) from the matrix itself.  Up to 3 d^2 = DENSE_LIMIT columns
    (`whole`) the image's A [d^2 + 2 d^2 / n, 3 d^2] is built entry by entry and everything is `_Dense` of it.  Beyond, the
    same is done per site: A is block diagonal over the sites (a pixel enters its own luma and its own site's chroma), so
    the site's A_s [n + 2, 3 n] is built entry by entry and applied to every site; the spectral coefficients depend on the
    singular value alone, so V f(S) V^T of the image is V_s f(S_s) V_s^T per site.  `test_site_model_is_the_whole_model`
    holds the two forms together.  `A`, `A_pinv`, `Lambda`, `Lambda_noise` take and return [n, .] tensors in the argument's
    dtype (oracle.sampler)."""

    def __init__(self, rw, rh, M, d, whole=None):
        self.rw, self.rh, self.d, self.M = rw, rh, d, np.asarray(M, dtype=np.float64)
        self.n, self.sites = rw * rh, (d // rw) * (d // rh)
        self.whole = 3 * d * d <= DENSE_LIMIT if whole is None else whole
        n, M = self.n, self.M
        if self.whole:
            A = dense_matrix(rw, rh, M, d, d)
        else:
            A = np.zeros((n + 2, 3 * n))                     # site coordinates: x (c, p), y (Y_0 .. Y_{n-1}, Cb, Cr)
            for c in range(3):
                for p in range(n):
                    A[p, c * n + p] = M[0, c]
                    A[n, c * n + p] = M[1, c] / n
                    A[n + 1, c * n + p] = M[2, c] / n
        self.core = _Dense(A)
        self.Amat = A
        self.S = np.sort(np.tile(self.core.S, 1 if self.whole else self.sites))[::-1]

    # ---- image order <-> the order of `core` ([B, 3 d^2] / [B, d^2 + 2 sites] float64 arrays on the image side)
    def _x_in(self, x):
        if self.whole:
            return x
        d, rw, rh = self.d, self.rw, self.rh
        v = x.reshape(-1, 3, d // rh, rh, d // rw, rw).transpose(0, 2, 4, 1, 3, 5)
        return v.reshape(-1, 3 * self.n)

    def _x_out(self, v):
        if self.whole:
            return v
        d, rw, rh = self.d, self.rw, self.rh
        x = v.reshape(-1, d // rh, d // rw, 3, rh, rw).transpose(0, 3, 1, 4, 2, 5)
        return x.reshape(-1, 3 * d * d)

    def _y_in(self, y):
        if self.whole:
            return y
        d, rw, rh, ns = self.d, self.rw, self.rh, self.sites
        Y = y[:, :d * d].reshape(-1, d // rh, rh, d // rw, rw).transpose(0, 1, 3, 2, 4).reshape(-1, ns, self.n)
        return np.concatenate([Y, y[:, d * d:d * d + ns, None], y[:, d * d + ns:, None]], axis=2).reshape(-1, self.n + 2)

    def _y_out(self, v):
        if self.whole:
            return v
        d, rw, rh, ns = self.d, self.rw, self.rh, self.sites
        v = v.reshape(-1, ns, self.n + 2)
        Y = v[:, :, :self.n].reshape(-1, d // rh, d // rw, rh, rw).transpose(0, 1, 3, 2, 4).reshape(-1, d * d)
        return np.concatenate([Y, v[:, :, self.n], v[:, :, self.n + 1]], axis=1)

    # ---- numpy float64
    def apply_A(self, x):
        return self._y_out(self._x_in(x) @ self.core.Amat.T)

    def apply_pinv(self, y):
        return self._x_out(self._y_in(y) @ self.core.pinv.T)

    def step(self, xt, et, n, y, abar_t, abar_next, sigma_y, eta, lam=None):
        """(x0|t, x_{t-1}) of one reverse step on [B, 3 d^2] / [B, d^2 + 2 sites] float64 arrays: DDNM with `lam` given
        (x0 - lam A^+(A x0 - y), then the DDIM update), DDNM+ otherwise (the formula of `_Dense`)."""
        a, sigma_t = abar_next ** 0.5, (1 - abar_next) ** 0.5
        x0 = (xt - et * (1 - abar_t) ** 0.5) / abar_t ** 0.5
        if lam is not None:
            x0h = x0 - lam * self.apply_pinv(self.apply_A(x0) - y)
            return x0, a * x0h + sigma_t * eta * n + sigma_t * (1 - eta ** 2) ** 0.5 * et
        return x0, self._x_out(self.core.plus(self._x_in(x0), self._x_in(et), self._x_in(n), self._y_in(y), a, sigma_y,
                                              sigma_t, eta))

    # ---- the operator protocol of oracle.sampler (torch in, torch out, the argument's dtype)
    @staticmethod
    def _np(v):
        return v.detach().double().cpu().reshape(v.shape[0], -1).numpy()

    @staticmethod
    def _like(out, v):
        return torch.from_numpy(np.ascontiguousarray(out)).to(v.dtype)

    def A(self, x):
        return self._like(self.apply_A(self._np(x)), x)

    def A_pinv(self, y):
        return self._like(self.apply_pinv(self._np(y)), y)

    def Lambda(self, vec, a, sigma_y, sigma_t, eta):
        lmb = self.core.coefficients(a, sigma_y, sigma_t, eta)[0]
        return self._like(self._x_out(self.core.spread(lmb, self._x_in(self._np(vec)))), vec)

    def Lambda_noise(self, vec, a, sigma_y, sigma_t, eta, epsilon):
        _, d1, d2 = self.core.coefficients(a, sigma_y, sigma_t, eta)
        out = self.core.spread(d1, self._x_in(self._np(vec))) + self.core.spread(d2, self._x_in(self._np(epsilon)))
        return self._like(self._x_out(out), vec)


def model_operator(rw, rh, M, d):
    """The dense float64 model of ChromaSubsample(3, d, rw, rh, matrix=M), with the matrix as given (`kernel_matrix(M)`:
    as the kernels get it)."""
    return DenseModel(rw, rh, M, d)


# ---- the closed forms (what the kernels evaluate); `dtype` float32 gives the fp32 figure a GPU bar may be derived from
def dc_svd(M, n):
    """U_D, S_D, V_D of D = diag(1, 1/sqrt n, 1/sqrt n) M (columns are the singular vectors)."""
    U, S, Vh = np.linalg.svd(np.diag([1.0, n ** -0.5, n ** -0.5]) @ np.asarray(M, dtype=np.float64))
    return U, S, Vh.T


def closed_singulars(rw, rh, M, d):
    M = np.asarray(M, dtype=np.float64)
    n, sites = rw * rh, d * d // (rw * rh)
    parts = [np.full(sites * (n - 1), np.sqrt((M[0] ** 2).sum()))] + [np.full(sites, s) for s in dc_svd(M, n)[1]]
    return np.sort(np.concatenate(parts))[::-1]


def _site_mean(v, rw, rh, d):
    """[.., d, d] -> the same shape, every pixel replaced by the mean of its site"""
    s = v.reshape(*v.shape[:-2], d // rh, rh, d // rw, rw)
    m = s.sum(axis=(-3, -1), keepdims=True, dtype=v.dtype) / v.dtype.type(rw * rh)
    return np.broadcast_to(m, s.shape).reshape(v.shape)


def _up(v, rw, rh):
    return np.repeat(np.repeat(v, rh, axis=-2), rw, axis=-1)


def closed_pinv(rw, rh, M, d, y, dtype=np.float64):
    """[B, d^2 + 2 sites] -> [B, 3 d^2]: w+ (Y_p - Ybar) + M^-1 (Ybar, Cb, Cr)"""
    M64 = np.asarray(M, dtype=np.float64)
    mi, wp = np.linalg.inv(M64).astype(dtype), (M64[0] / (M64[0] ** 2).sum()).astype(dtype)
    y = y.astype(dtype)
    B, ns = y.shape[0], d * d // (rw * rh)
    Y = y[:, :d * d].reshape(B, d, d)
    Yb = _site_mean(Y, rw, rh, d)
    Cb = _up(y[:, d * d:d * d + ns].reshape(B, d // rh, d // rw), rw, rh)
    Cr = _up(y[:, d * d + ns:].reshape(B, d // rh, d // rw), rw, rh)
    out = [(Y - Yb) * wp[c] + ((Yb * mi[c, 0] + Cb * mi[c, 1]) + Cr * mi[c, 2]) for c in range(3)]
    return np.stack(out, axis=1).reshape(B, -1)


def closed_A(rw, rh, M, d, x, dtype=np.float64):
    M = np.asarray(M, dtype=dtype)
    x = x.astype(dtype).reshape(-1, 3, d, d)
    planes = [(x[:, 0] * M[k, 0] + x[:, 1] * M[k, 1]) + x[:, 2] * M[k, 2] for k in range(3)]
    chroma = [_site_mean(p, rw, rh, d)[:, ::rh, ::rw].reshape(x.shape[0], -1) for p in planes[1:]]
    return np.concatenate([planes[0].reshape(x.shape[0], -1)] + chroma, axis=1)


def closed_plus_step(rw, rh, M, d, xt, et, n, y, abar_t, abar_next, sigma_y, eta):
    """The DDNM+ step per site: the pixel term along w^ and the site term through the 3 x 3 SVD of D, as the kernel's
    header states it."""
    M = np.asarray(M, dtype=np.float64)
    nn, B, ns = rw * rh, xt.shape[0], d * d // (rw * rh)
    a, sigma_t = abar_next ** 0.5, (1 - abar_next) ** 0.5
    x0 = (xt - et * (1 - abar_t) ** 0.5) / abar_t ** 0.5
    wn = np.sqrt((M[0] ** 2).sum())
    wh = M[0] / wn
    U, S, V = dc_svd(M, nn)
    la, d1a, d2a = _coef(wn, a, sigma_y, sigma_t, eta)
    _, d1n, d2n = _coef(0.0, a, sigma_y, sigma_t, eta)
    cd = np.array([_coef(s, a, sigma_y, sigma_t, eta) for s in S])
    img = lambda v: v.reshape(B, 3, d, d)      # noqa: E731
    t = lambda v: np.einsum("c,bcij->bij", wh, img(v))      # noqa: E731
    mu = lambda v: _site_mean(img(v), rw, rh, d)      # noqa: E731
    Y = y[:, :d * d].reshape(B, d, d)
    Yb = _site_mean(Y, rw, rh, d)
    Cb = _up(y[:, d * d:d * d + ns].reshape(B, d // rh, d // rw), rw, rh)
    Cr = _up(y[:, d * d + ns:].reshape(B, d // rh, d // rw), rw, rh)
    dev = lambda v: t(v) - _site_mean(t(v), rw, rh, d)      # noqa: E731
    ac = -a * la * (dev(x0) - (Y - Yb) / wn) + (d1a - d1n) * dev(n) + (d2a - d2n) * dev(et)
    z = np.stack([Yb, Cb / nn ** 0.5, Cr / nn ** 0.5], axis=1)                              # [B, 3, d, d]
    vt = lambda v: np.einsum("ck,bcij->bkij", V, v)      # noqa: E731
    k3 = lambda c: c[None, :, None, None]      # noqa: E731
    dc = -a * k3(cd[:, 0]) * (vt(mu(x0)) - np.einsum("ck,bcij->bkij", U, z) / k3(S)) \
        + k3(cd[:, 1] - d1n) * vt(mu(n)) + k3(cd[:, 2] - d2n) * vt(mu(et))
    out = a * img(x0) + d1n * img(n) + d2n * img(et) + wh[None, :, None, None] * ac[:, None] \
        + np.einsum("ck,bkij->bcij", V, dc)
    return x0, out.reshape(B, -1)


def step_inputs(d, B, seed=31):
    """Seeded (x_orig in [-1, 1], x_t, eps (6 channels), n) of a one-step case; never written to."""
    g = torch.Generator().manual_seed(seed + 100 * d)
    return (torch.rand(B, 3, d, d, generator=g) * 2 - 1, torch.randn(B, 3, d, d, generator=g),
            torch.randn(B, 6, d, d, generator=g), torch.randn(B, 3, d, d, generator=g))


def _flat64(t):
    return t.double().reshape(t.shape[0], -1).numpy()


def _config(d):
    return argparse.Namespace(data=argparse.Namespace(channels=3, image_size=d))


CASES = [(name, rw, rh) for name in sorted(MATRICES) for rw, rh in SITES]


# ---------------------------------------------------------------------------------------------- 1. model self-checks
@pytest.mark.parametrize("name,rw,rh", CASES)
def test_closed_form_spectrum_and_pinv_equal_the_dense_ones(name, rw, rh):
    M = MATRICES[name]
    D = DenseModel(rw, rh, M, 8)
    assert D.whole and D.Amat.shape == (64 + 2 * 64 // (rw * rh), 192)
    assert np.count_nonzero(D.core.S) == D.Amat.shape[0]                   # full row rank
    assert np.abs(closed_singulars(rw, rh, M, 8) - D.core.S).max() < 1e-12
    assert len(np.unique(np.round(D.core.S, 9))) == 4                       # four singular values per launch
    assert np.abs(D.Amat @ D.core.pinv - np.eye(D.Amat.shape[0])).max() < 1e-12      # A A^+ = I
    rng = np.random.default_rng(3)
    y, x = rng.standard_normal((2, D.Amat.shape[0])), rng.standard_normal((2, 192))
    assert np.abs(closed_pinv(rw, rh, M, 8, y) - y @ D.core.pinv.T).max() < 1e-12
    assert np.abs(closed_A(rw, rh, M, 8, x) - x @ D.Amat.T).max() < 1e-12


def test_singular_values_of_bt601():
    """The table of DESIGN.md 1.11."""
    want = {2: (0.72159, 0.45450, 0.36022), 4: (0.69131, 0.32192, 0.26543), 16: (0.67361, 0.16115, 0.13604),
            64: (0.66978, 0.08060, 0.06839)}
    for n, s in want.items():
        assert np.abs(dc_svd(BT601, n)[1] - s).max() < 6e-6
    assert abs(np.sqrt((np.asarray(BT601[0]) ** 2).sum()) - 0.66856) < 6e-6


@pytest.mark.parametrize("name,rw,rh", CASES)
@pytest.mark.parametrize("setting", sorted(PLUS_SETTINGS))
def test_closed_form_step_equals_the_dense_step(name, rw, rh, setting):
    M = MATRICES[name]
    D = DenseModel(rw, rh, M, 8)
    abar_next, sigma_y = PLUS_SETTINGS[setting]
    x, xt, et6, n = step_inputs(8, 2)
    y = _flat64(x) @ D.Amat.T
    args = (_flat64(xt), _flat64(et6[:, :3]), _flat64(n), y, 0.45, abar_next, sigma_y, ETA)
    x0_d, out_d = D.step(*args)
    x0_c, out_c = closed_plus_step(rw, rh, M, 8, *args)
    assert np.abs(x0_d - x0_c).max() == 0 and np.abs(out_d - out_c).max() < 1e-12
    # ... and the dense step is the loop body of oracle.sampler.ddnm_plus_diffusion spelled with Lambda / Lambda_noise
    a, sigma_t = abar_next ** 0.5, (1 - abar_next) ** 0.5
    t = lambda v: torch.from_numpy(v)      # noqa: E731
    corr = D.A_pinv(D.A(t(x0_d)) - t(y))
    ref = a * (t(x0_d) - D.Lambda(corr, a, sigma_y, sigma_t, ETA)) + D.Lambda_noise(t(args[2]), a, sigma_y, sigma_t, ETA, t(args[1]))
    assert (ref - t(out_d)).abs().max() < 1e-12
    # the noise-free step with the closed-form A and A^+
    for lam in (1.0, 0.3):
        want = D.step(*args[:6], 0.0, ETA, lam=lam)[1]
        x0h = x0_c - lam * closed_pinv(rw, rh, M, 8, closed_A(rw, rh, M, 8, x0_c) - y)
        got = a * x0h + sigma_t * ETA * args[2] + sigma_t * (1 - ETA ** 2) ** 0.5 * args[1]
        assert np.abs(got - want).max() < 1e-12


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_regimes_are_what_their_names_say(name):
    """damped: every singular value damped; full: none; mixed: luma (|w_Y| and the largest of S_D) full, the two chroma
    values of S_D damped -- at every site.  (0.9, 0.15) mixes at n = 4 and not at n = 2, where BT.601's Cb value 0.4545
    lies above tau = 0.45."""
    M = np.asarray(MATRICES[name])
    wn = np.sqrt((M[0] ** 2).sum())

    def damped(s, abar_next, sigma_y):
        a, sigma_t = abar_next ** 0.5, (1 - abar_next) ** 0.5
        lam = _coef(s, a, sigma_y, sigma_t, ETA)[0]
        assert (lam < 1) == (sigma_t < a * sigma_y / s)
        return lam < 1

    for rw, rh in SITES:
        S = dc_svd(M, rw * rh)[1]
        for setting, (ab, sy) in PLUS_SETTINGS.items():
            got = [damped(s, ab, sy) for s in (wn, *S)]
            assert got == {"damped": [True] * 4, "full": [False] * 4, "mixed": [False, False, True, True]}[setting], \
                (name, rw, rh, setting)
    if name == "bt601":
        assert [damped(s, 0.9, 0.15) for s in (wn, *dc_svd(M, 4)[1])] == [False, False, True, True]
        assert [damped(s, 0.9, 0.15) for s in (wn, *dc_svd(M, 2)[1])] == [False, False, False, True]
        lam = [round(_coef(s, 0.5 ** 0.5, 0.1, 0.5 ** 0.5, ETA)[0], 2) for s in dc_svd(M, 64)[1][1:]]
        assert lam == [0.42, 0.36]                            # (0.5, 0.1) at 8 x 8: luma full, chroma damped


@pytest.mark.parametrize("rw,rh,d", [(rw, rh, 8) for rw, rh in SITES] + [(8, 8, 16)])
def test_site_model_is_the_whole_model(rw, rh, d):
    """The two forms of DenseModel (the image's matrix up to d = 16, the site's matrix beyond) are the same operator: A,
    A^+, both steps, Lambda and Lambda_noise."""
    M = kernel_matrix(BT601)
    whole, site = DenseModel(rw, rh, M, d, whole=True), DenseModel(rw, rh, M, d, whole=False)
    assert np.abs(whole.S - site.S).max() < 1e-12
    x, xt, et6, n = step_inputs(d, 2)
    y = whole.apply_A(_flat64(x))
    assert np.abs(y - site.apply_A(_flat64(x))).max() < 1e-12
    assert np.abs(whole.apply_pinv(y) - site.apply_pinv(y)).max() < 1e-12
    for abar_next, sigma_y in PLUS_SETTINGS.values():
        args = (_flat64(xt), _flat64(et6[:, :3]), _flat64(n), y, 0.45, abar_next, sigma_y, ETA)
        assert np.abs(whole.step(*args)[1] - site.step(*args)[1]).max() < 1e-12
        assert np.abs(whole.step(*args, lam=0.3)[1] - site.step(*args, lam=0.3)[1]).max() < 1e-12
        a, sigma_t = abar_next ** 0.5, (1 - abar_next) ** 0.5
        v, e = torch.from_numpy(args[2]), torch.from_numpy(args[1])
        assert (whole.Lambda(v, a, sigma_y, sigma_t, ETA) - site.Lambda(v, a, sigma_y, sigma_t, ETA)).abs().max() < 1e-12
        assert (whole.Lambda_noise(v, a, sigma_y, sigma_t, ETA, e)
                - site.Lambda_noise(v, a, sigma_y, sigma_t, ETA, e)).abs().max() < 1e-12


# ---------------------------------------------------------------------------------------------- 2. the library's constants
def chroma_constants(lib, M, rw, rh):
    """ddnm_chroma_constants as a dict of float64 arrays (None: refused, with the code)."""
    m = (ctypes.c_float * 9)(*[float(v) for v in np.asarray(M, dtype=np.float32).reshape(-1)])
    out = (ctypes.c_double * 37)()
    rc = lib.ddnm_chroma_constants(m, rw, rh, out)
    if rc:
        return rc
    v = np.array(out[:])
    return {"mi": v[0:9].reshape(3, 3), "wp": v[9:12], "wh": v[12:15], "wn": v[15], "U": v[16:25].reshape(3, 3),
            "S": v[25:28], "V": v[28:37].reshape(3, 3)}


@pytest.fixture(scope="module")
def lib():
    from ddnm_amd import _lib, build
    build.build()
    return _lib.lib()


@pytest.mark.parametrize("name,rw,rh", CASES)
def test_library_constants_agree_with_numpy(lib, name, rw, rh):
    """M^-1, w+, w^, |w_Y| directly; the SVD through what does not depend on signs: S_D, V f(S) V^T and U f(S) U^T for a
    non-constant f, U S V^T = D, and the orthogonality of U and V.  All at 1e-12."""
    M = kernel_matrix(MATRICES[name])
    k = chroma_constants(lib, M, rw, rh)
    n2 = (M[0] ** 2).sum()
    assert np.abs(k["mi"] - np.linalg.inv(M)).max() < 1e-12
    assert np.abs(k["wp"] - M[0] / n2).max() < 1e-12 and np.abs(k["wh"] - M[0] / n2 ** 0.5).max() < 1e-12
    assert abs(k["wn"] - n2 ** 0.5) < 1e-12
    U, S, V = dc_svd(M, rw * rh)
    assert np.abs(k["S"] - S).max() < 1e-12 and (np.diff(k["S"]) < 0).all()
    f = np.array([1.0, -2.0, 0.5]) + S ** 2
    assert np.abs(k["V"] * f @ k["V"].T - V * f @ V.T).max() < 1e-12
    assert np.abs(k["U"] * f @ k["U"].T - U * f @ U.T).max() < 1e-12
    D = np.diag([1.0, (rw * rh) ** -0.5, (rw * rh) ** -0.5]) @ M
    assert np.abs(k["U"] * k["S"] @ k["V"].T - D).max() < 1e-12
    assert np.abs(k["V"].T @ k["V"] - np.eye(3)).max() < 1e-12 and np.abs(k["U"].T @ k["U"] - np.eye(3)).max() < 1e-12


def test_library_constants_refusals(lib):
    """A singular matrix is |det| < 1e-6 |M|_F^3 in double: DDNM_E_BADARG (-1), before an unsupported site (-2)."""
    rank2 = np.array([BT601[0], BT601[1], np.add(BT601[0], BT601[1])])
    assert chroma_constants(lib, rank2, 2, 2) == -1 and chroma_constants(lib, np.zeros((3, 3)), 2, 2) == -1
    assert chroma_constants(lib, rank2, 3, 3) == -1
    for site in ((1, 1), (1, 2), (3, 3), (2, 4), (8, 4), (16, 16), (0, 0), (2, -1)):
        assert chroma_constants(lib, BT601, *site) == -2, site
    # around the bound: diag(1, 1, e) has |det| = e and |M|_F^3 = (2 + e^2)^1.5 ~ 2.83
    assert chroma_constants(lib, np.diag([1.0, 1.0, 2e-6]), 2, 2) == -1
    assert isinstance(chroma_constants(lib, np.diag([1.0, 1.0, 4e-6]), 2, 2), dict)
    out = (ctypes.c_double * 37)()
    m = (ctypes.c_float * 9)(*np.asarray(BT601, dtype=np.float32).reshape(-1))
    assert lib.ddnm_chroma_constants(None, 2, 2, out) == -1 and lib.ddnm_chroma_constants(m, 2, 2, None) == -1


# ---------------------------------------------------------------------------------------------- 3. operator and names
def test_operator_tables():
    from ddnm_amd.functions import svd_operators as E
    op = E.ChromaSubsample(3, 8, 2, 2, "cpu")
    assert op.measurement_size() == 64 + 2 * 16 and op.measurement_image_shape() is None
    assert (op.rw, op.rh) == (2, 2) and [float(v) for v in op._m] == [float(np.float32(v)) for r in BT601 for v in r]
    s = closed_singulars(2, 2, kernel_matrix(BT601), 8)
    assert op.singulars().shape == (96,) and np.abs(op.singulars().double().numpy() - s).max() < 1e-7
    assert bool((op.singulars()[:-1] >= op.singulars()[1:]).all())
    wide = E.ChromaSubsample(3, 16, 4, 1, "cpu", matrix=BT709)
    assert wide.measurement_size() == 256 + 2 * 64
    assert np.abs(wide.singulars().double().numpy() - closed_singulars(4, 1, kernel_matrix(BT709), 16)).max() < 1e-7
    for name in ("Lambda", "V", "Vt", "U", "Ut"):
        with pytest.raises(NotImplementedError):
            getattr(op, name)(torch.zeros(1, 96), *([0.5, 0.1, 0.5, ETA] if name == "Lambda" else []))
    with pytest.raises(NotImplementedError):
        op.Lambda_noise(torch.zeros(1, 192), 0.5, 0.1, 0.5, ETA, torch.zeros(1, 192))


def test_constructor_refusals():
    from ddnm_amd.functions import svd_operators as E
    with pytest.raises(ValueError, match="channels"):
        E.ChromaSubsample(1, 16, 2, 2, "cpu")
    for site in ((1, 1), (1, 2), (3, 3), (8, 4), (16, 16)):
        with pytest.raises(ValueError, match="sites"):
            E.ChromaSubsample(3, 16, *site, "cpu")
    with pytest.raises(ValueError, match="multiple of the site"):
        E.ChromaSubsample(3, 12, 8, 8, "cpu")
    with pytest.raises(ValueError, match="multiple of 4"):
        E.ChromaSubsample(3, 6, 2, 2, "cpu")
    with pytest.raises(ValueError, match="3 x 3"):
        E.ChromaSubsample(3, 16, 2, 2, "cpu", matrix=BT601[:2])
    with pytest.raises(ValueError, match="invertible"):
        E.ChromaSubsample(3, 16, 2, 2, "cpu", matrix=[BT601[0], BT601[1], np.add(BT601[0], BT601[1])])
    with pytest.raises(ValueError, match="invertible"):
        E.ChromaSubsample(3, 16, 2, 2, "cpu", matrix=np.zeros((3, 3)))


def test_build_operator_maps_the_names():
    """chroma_420 / chroma_422 / chroma_411 fix the site and do not read --deg_scale; chroma_sub takes square sites of
    --deg_scale 2 | 4 | 8 and refuses anything else with the choices.  (Every name ended in `degradation type not
    supported` before.)"""
    from ddnm_amd.functions import svd_operators as E
    for name, site in (("chroma_420", (2, 2)), ("chroma_422", (2, 1)), ("chroma_411", (4, 1))):
        for scale in (1.0, 4, 0.25, 3, None):
            op = E.build_operator(name, scale, _config(16), "cpu")
            assert isinstance(op, E.ChromaSubsample) and (op.rw, op.rh) == site and op.img_dim == 16
            assert np.array_equal(op.matrix, kernel_matrix(BT601))
    for scale, r in ((2, 2), (4.0, 4), (8, 8)):
        op = E.build_operator("chroma_sub", scale, _config(16), "cpu")
        assert isinstance(op, E.ChromaSubsample) and (op.rw, op.rh) == (r, r) and isinstance(op.rw, int)
    for scale in (1, 3, 16, 0.25, 2.2, 0.0):
        with pytest.raises(ValueError, match=r"2 \| 4 \| 8"):
            E.build_operator("chroma_sub", scale, _config(16), "cpu")
    with pytest.raises(ValueError, match="degradation type not supported"):
        E.build_operator("chroma_444", 1, _config(16), "cpu")


def test_a_picture_is_no_measurement(tmp_path):
    """A measurement is three planes of two sizes: .npy rows of d^2 + 2 d^2 / n values bind, a picture is refused with the
    reason when the folder is bound, and so is a row of another length."""
    from PIL import Image
    from ddnm_amd.functions import svd_operators as E
    from ddnm_amd.guided_diffusion import diffusion as D
    cfg = argparse.Namespace(data=argparse.Namespace(channels=3, image_size=16, rescaled=True))
    op = E.ChromaSubsample(3, 16, 2, 2, "cpu")
    good = tmp_path / "good"
    good.mkdir()
    np.save(good / "y_0.npy", np.arange(384, dtype=np.float32))
    ds = D.MeasurementFolder(str(good)).bind(op, cfg)
    row, picture = ds[0]
    assert not picture and row.shape == (384,) and torch.equal(row, torch.arange(384, dtype=torch.float32))
    pic = tmp_path / "pic"
    pic.mkdir()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(pic / "y_0.png")
    with pytest.raises(ValueError, match=r"y_0\.png is a picture, but a measurement of this operator is no picture.*384"):
        D.MeasurementFolder(str(pic)).bind(op, cfg)
    short = tmp_path / "short"
    short.mkdir()
    np.save(short / "y_0.npy", np.zeros(256, np.float32))
    with pytest.raises(ValueError, match="256"):
        D.MeasurementFolder(str(short)).bind(op, cfg)


# ---------------------------------------------------------------------------------------------- 4. argument validation
def check_chroma_validation(lib, ptr):
    """Every refusal of the six launching `*_chroma_*` entry points, with distinct addresses from `ptr` on standing for the
    tensors (never dereferenced: all of it happens before a launch).  DDNM_E_BADARG = -1 comes before DDNM_E_SHAPE = -2."""
    from ddnm_amd._lib import StepScalars
    s = StepScalars()
    s.rng_on = 1
    sp = ctypes.byref(s)
    m = (ctypes.c_float * 9)(*np.asarray(BT601, dtype=np.float32).reshape(-1))
    sing = (ctypes.c_float * 9)(*np.asarray([BT601[0], BT601[1], BT601[1]], dtype=np.float32).reshape(-1))
    zero = (ctypes.c_float * 9)()
    P = [ptr + 64 * i for i in range(8)]                    # xt, et, y, -, x0, xt_next, keys / noise, spare
    bad_sites = ((1, 1), (1, 2), (3, 3), (2, 4), (8, 4), (16, 16), (0, 0), (-2, 1))

    def op(fn, a=P[0], b=P[2], B=2, H=16, W=16, rw=4, rh=4, mt=m):
        return fn(a, b, B, H, W, rw, rh, mt, None)

    def step(fn, xt=P[0], et=P[1], es=768, nz=None, y=P[2], x0=P[4], xn=P[5], B=2, H=16, W=16, rw=4, rh=4, mt=m, sc=sp):
        extra = (0.1, 0.5, ETA) if "plus" in fn.__name__ else ()
        return fn(xt, et, es, nz, y, x0, xn, B, H, W, rw, rh, mt, *extra, sc, None)

    ops_ = (lib.ddnm_op_chroma_A_f32, lib.ddnm_op_chroma_pinv_f32)
    steps = (lib.ddnm_step_chroma_f32, lib.ddnm_step_plus_chroma_f32)
    keyed = (lib.ddnm_step_chroma_keyed_f32, lib.ddnm_step_plus_chroma_keyed_f32)
    for fn in ops_:
        assert op(fn, a=None) == -1 and op(fn, b=None) == -1 and op(fn, mt=None) == -1, fn.__name__
        assert op(fn, B=0) == -1 and op(fn, B=-2) == -1 and op(fn, mt=sing) == -1 and op(fn, mt=zero) == -1, fn.__name__
        assert op(fn, a=None, rw=3) == -1 and op(fn, mt=sing, W=6) == -1 and op(fn, mt=sing, rw=3, rh=3) == -1, fn.__name__
        for rw, rh in bad_sites:
            assert op(fn, rw=rw, rh=rh) == -2, (fn.__name__, rw, rh)
        assert op(fn, H=18) == -2 and op(fn, W=18) == -2 and op(fn, W=6, rw=2, rh=2) == -2 and op(fn, H=0) == -2, fn.__name__
        assert op(fn, H=12, rw=8, rh=8) == -2 and op(fn, W=12, rw=8, rh=8) == -2 and op(fn, H=15, rw=2, rh=2) == -2, fn.__name__
        assert op(fn, W=10, rw=2, rh=1) == -2 and op(fn, W=0) == -2, fn.__name__
    for fn in steps + keyed:
        nz = P[6] if fn in keyed else None                  # (a multiple of 16: a valid key table address)
        for arg in ("xt", "et", "y", "xn", "mt", "sc"):
            assert step(fn, nz=nz, **{arg: None}) == -1, (fn.__name__, arg)
        assert step(fn, nz=nz, B=0) == -1 and step(fn, nz=nz, mt=sing) == -1 and step(fn, nz=nz, mt=zero) == -1, fn.__name__
        assert step(fn, nz=nz, y=None, W=6) == -1 and step(fn, nz=nz, B=0, rw=3) == -1, fn.__name__
        assert step(fn, nz=nz, mt=sing, rw=3, rh=3) == -1 and step(fn, nz=nz, mt=sing, es=770) == -1, fn.__name__
        # two passes over a strip: an output that is xt, et or the other output is refused
        assert step(fn, nz=nz, xn=P[0]) == -1 and step(fn, nz=nz, xn=P[1]) == -1 and step(fn, nz=nz, xn=P[4]) == -1
        assert step(fn, nz=nz, x0=P[0]) == -1 and step(fn, nz=nz, x0=P[1]) == -1, fn.__name__
        for rw, rh in bad_sites:
            assert step(fn, nz=nz, rw=rw, rh=rh) == -2, (fn.__name__, rw, rh)
        assert step(fn, nz=nz, H=18) == -2 and step(fn, nz=nz, W=18) == -2 and step(fn, nz=nz, W=6, rw=2, rh=2) == -2, fn.__name__
        assert step(fn, nz=nz, H=12, rw=8, rh=8) == -2 and step(fn, nz=nz, es=770) == -2 and step(fn, nz=nz, es=6) == -2, fn.__name__
    for fn in keyed:
        assert step(fn, nz=None) == -1 and step(fn, nz=P[6] + 4) == -1, fn.__name__          # null / misaligned key table
    off = StepScalars()                                      # rng_on = 0 and no noise tensor: no source
    for fn in steps:
        assert step(fn, sc=ctypes.byref(off)) == -1, fn.__name__
    # x0 is optional in the noise-free step only (with everything else valid that call would launch: checked on the GPU)
    assert step(lib.ddnm_step_plus_chroma_f32, x0=None) == -1 and step(lib.ddnm_step_plus_chroma_keyed_f32, nz=P[6], x0=None) == -1


def test_argument_validation_without_gpu(lib):
    """The pattern of tests/test_cabi.py::test_argument_validation_without_gpu: the entry points refuse bad arguments
    before touching the device, so the built library answers on a host without one."""
    assert lib.ddnm_version() == 7
    check_chroma_validation(lib, 4096)


def test_hooks_marshal_their_arguments():
    """Host-only dry run (tools/dry_run.py): A, A_pinv, ddnm_step and the DDNM+ hook reach their entry points with arguments
    of the declared types, for a tensor, an in-kernel and a keyed noise source."""
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
        for rw, rh in ((2, 1), (8, 8)):
            op = E.ChromaSubsample(3, d, rw, rh, "cpu")
            x = torch.zeros(B, 3, d, d)
            y = op.A(x)
            assert y.shape == (B, d * d + 2 * d * d // (rw * rh)) and op.A_pinv(y).shape == (B, 3 * d * d)
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
        assert dry.calls == {"ddnm_op_chroma_A_f32": 2, "ddnm_op_chroma_pinv_f32": 2, "ddnm_step_chroma_f32": 4,
                             "ddnm_step_plus_chroma_f32": 2}
    finally:
        _lib._lib, ops._stream, ops._f32c, ops._f16c = saved
