"""Degradation operators of DDNM on MI355X, behind the reference's `A_functions` API.

Drop-in for `functions/svd_operators.py` on the hot path: the classes keep the
reference's names and constructor signatures and expose `A(vec)`, `A_pinv(vec)`
(`[B, ...] -> [B, D]` contiguous fp32) plus `singulars()`.  The reference applies
each operator through its SVD factors (U, Sigma, V^T; svd_operators.py:52-80) with
~60 tiny ATen launches per call; here each A / A^+ is the operator's direct form
as one (or a few) hand-written HIP kernels:

  SuperResolution  -> r x r mean / replicate                    (svd_operators.py:479-533)
  SRConv           -> Ae X Ae^T / Pe Y Pe^T on MFMA f32          (svd_operators.py:851-931)
  Colorization     -> w . rgb / w |w|^-2                         (svd_operators.py:627-667)
  Inpainting       -> gather / scatter through a rank table      (svd_operators.py:324-359)
  InpaintingBank / PerImageInpainting -> the same with one mask (rank table) per image of the batch; the reference
                      holds one mask per run, so each image is checked against its single-mask operator
  Mosaic           -> demosaicing: that Inpainting over single entries, one colour sample per pixel behind a periodic
                      colour filter array; no table, y is a dense one-channel picture; `ddnm_plus_step` is ONE kernel
  MaskColorSR      -> old photo: mask, grey, r x r mean in one operator with its exact A^+ (the simplified path's
                      Composition has the same A but a chained inverse that is no pseudo-inverse where the mask cuts a
                      site); one singular value per site, evaluated in the kernels; `ddnm_plus_step` is ONE kernel
  ChromaSubsample  -> Y'CbCr 4:2:0 / 4:2:2 / 4:1:1: full-resolution luma, chroma averaged per rw x rh site, with the exact
                      A^+ = w+ (Y - Ybar) + M^-1 (Ybar, Cb, Cr); four singular values per launch (|w_Y| and the 3 x 3 SVD of
                      the site means), evaluated on the host; `ddnm_plus_step` is ONE kernel
  JPEG             -> a baseline JPEG file: the 8 x 8 block-DCT coefficients of those planes (4:4:4 / 4:2:2 / 4:2:0), each
                      known up to its quantisation cell; `ddnm_step` projects T x0 into the cell in ONE kernel; noise-free only
  WalshHadamardCS -> separable FWHT (shuffle + LDS) + permuted mask (svd_operators.py:211-251)
  Denoising        -> identity                                   (svd_operators.py:442-462)

Every class also implements `ddnm_step(...)`, the fused x0 / projection / DDIM
update of one sampler step (functions/svd_ddnm.py:57-65) that `ddnm_diffusion`
uses when it is handed one of these objects.  Its `noise` is a tensor, None (the
kernel draws in-kernel from ddnm_step_scalars::rng_*) or an `ops.KeyedPhiloxNoise`
(per-image keys: the `*_keyed_f32` entry points, ops.step_noise_args).

`Lambda` / `Lambda_noise` (the sigma_y > 0 path of `ddnm_plus_diffusion`) follow the reference's
per-class definitions, including its quirk of feeding the RAW patch / needle / permuted entries of
the noise and of eps to `V` in `Lambda_noise`.  `SRConv` and `Deblurring2D` define none, like the reference
(`Lambda` raises NotImplementedError); their DDNM+ runs through the engine hook `ddnm_plus_step` instead
(`_SpectralPlus`: the whole step fused in the operator's spectral planes, thresholded singular values, eps
entering as V^T eps).  `Deblurring` opts out of the hook and keeps its `Lambda` / `Lambda_noise`.  `CS` (cs_blockbased)
has the hook too and no `Lambda` either: all its singular values are 1, so its step collapses per 32x32 patch to one
image-order pass, the two GEMMs of `A` / `A_pinv` and one scatter-add (`CS.ddnm_plus_step`, `cs_plus_coefficients`).
"""
import ctypes

import numpy as np
import torch

from .. import _lib, ops
from ..ops import _p


def _img(vec, c, d):
    v = vec.reshape(vec.shape[0], c, d, d)
    if v.dtype != torch.float32 or not v.is_contiguous():
        v = v.float().contiguous()
    return v


def spectral_coefficients(s, a, sigma_y, sigma_t, eta):
    """(lambda, d1, d2) of one singular value `s` (0 = null space) -- the per-entry rules that every
    `Lambda` / `Lambda_noise` of the reference spells out with change_index masks (e.g. svd_operators.py:548-605):
      lambda = s*sigma_t*sqrt(1-eta^2)/(a*sigma_y) where sigma_t < a*sigma_y/s, else 1;
      (d1, d2) = (sigma_t*eta, 0) below that threshold, (sqrt(sigma_t^2 - a^2 sigma_y^2/s^2), 0) above it,
      (sigma_t*eta, sigma_t*sqrt(1-eta^2)) for s = 0."""
    a, sigma_y, sigma_t = float(a), float(sigma_y), float(sigma_t)
    c1, c2 = sigma_t * eta, sigma_t * (1 - eta ** 2) ** 0.5
    if s == 0 or a == 0 or sigma_y == 0:
        return 1.0, c1, c2
    thr = a * sigma_y / s
    if sigma_t < thr:
        return s * sigma_t * (1 - eta ** 2) ** 0.5 / a / sigma_y, c1, 0.0
    if sigma_t > thr:
        return 1.0, (sigma_t ** 2 - a ** 2 * sigma_y ** 2 / s ** 2) ** 0.5, 0.0
    return 1.0, c1, c2


def noise_coefficients(s, a, sigma_y, sigma_t, eta):
    """(d1m, d1n, d2m, d2n) of a `Lambda_noise`: the noise factors (d1) and the eps factors (d2) on the entries measured with
    singular value `s` (m) and on the null space (n)."""
    _, d1m, d2m = spectral_coefficients(s, a, sigma_y, sigma_t, eta)
    _, d1n, d2n = spectral_coefficients(0.0, a, sigma_y, sigma_t, eta)
    return d1m, d1n, d2m, d2n


def cs_plus_coefficients(a, sigma_y, sigma_t, eta):
    """The five scalars of the fused DDNM+ step of `CS` (every singular value is 1, svd_operators.py:110):
    (a*lambda, d1n, d2n, d1r - d1n, d2r - d2n) with (lambda, d1r, d2r) = spectral_coefficients(1, ...) on the measured
    subspace and (1, d1n, d2n) = spectral_coefficients(0, ...) on the null space; evaluated in double on the host."""
    lam, d1r, d2r = spectral_coefficients(1.0, a, sigma_y, sigma_t, eta)
    _, d1n, d2n = spectral_coefficients(0.0, a, sigma_y, sigma_t, eta)
    return float(a) * lam, d1n, d2n, d1r - d1n, d2r - d2n


HN_OPERATORS = "Mosaic (--deg demosaic_*) and Denoising (--deg denoising)"


def noise_map_row(arr, n, image_shape=None, name="the noise map"):
    """A per-entry noise map -> its validated float32 row [n] (the [0, 1] scale it was stated on).  `arr` holds one
    standard deviation per measurement entry, as [n], [1, n] or the operator's `measurement_image_shape()`; the entries
    are finite and non-negative (zeros are allowed: an entry measured exactly).  `name` is the file the errors speak of."""
    a = np.asarray(arr)
    if a.dtype.kind not in "fiu":
        raise ValueError(f"{name}: a noise map is a float array of {n} standard deviations, got dtype {a.dtype}")
    shapes = [(n,), (1, n)] + ([tuple(image_shape)] if image_shape is not None else [])
    if tuple(a.shape) not in shapes:
        raise ValueError(f"{name}: a noise map holds one row of {n} entries, shaped "
                         f"{' or '.join(str(list(s)) for s in shapes)} (one row for every image of the run); got shape "
                         f"{list(a.shape)} with {a.size} entries")
    row = np.ascontiguousarray(a.reshape(-1), dtype=np.float32)
    if not np.isfinite(row).all():
        bad = int((~np.isfinite(row)).sum())
        raise ValueError(f"{name}: the {n} entries of a noise map are finite, got {bad} that are inf or nan "
                         f"(the first at entry {int(np.flatnonzero(~np.isfinite(row))[0])})")
    if (row < 0).any():
        raise ValueError(f"{name}: the {n} entries of a noise map are standard deviations >= 0, got {int((row < 0).sum())} "
                         f"negative ones (minimum {float(row.min())!r})")
    return row


class NoiseModel:
    """The noise of a measurement, where `ddnm_plus_diffusion` takes the scalar `sigma_y`; every figure is stated on the
    [0, 1] scale of `--sigma_y` (the engine works on [-1, 1] and doubles it).  Three forms:

      NoiseModel.scalar(s)        every entry has the standard deviation s: exactly `--sigma_y s`, today's launches
      NoiseModel.shot(s, g)       shot + read noise: Var_j = s^2 + g u_j with u_j = clamp((y_j + 1) / 2, 0, 1) the measured
                                  intensity (the plug-in estimate), so sigma_j = 2 sqrt(s^2 + g u_j) on the engine's scale;
                                  g = 0 is the scalar form
      NoiseModel.map(row)         one standard deviation per measurement entry (`noise_map_row`), shared by every image

    The per-entry forms are exact for operators whose U is the identity and whose measured entries have singular value 1
    -- a diagonal covariance is diagonal in their spectral basis --, which here are Mosaic and Denoising (`ddnm_plus_step_hn`)."""

    def __init__(self, kind, sigma=0.0, gain=0.0, row=None):
        self.kind, self.sigma, self.gain, self.row = kind, float(sigma), float(gain), row
        self._dev = {}

    @classmethod
    def scalar(cls, sigma):
        sigma = float(sigma)
        if not np.isfinite(sigma) or sigma < 0:
            raise ValueError(f"sigma_y is a finite standard deviation >= 0, got {sigma!r}")
        return cls("scalar", sigma)

    @classmethod
    def shot(cls, sigma, gain):
        sigma, gain = float(sigma), float(gain)
        if not np.isfinite(gain) or gain < 0:
            raise ValueError(f"sigma_y_shot is a finite shot-noise gain >= 0 (Var = sigma_y^2 + gain * intensity), got {gain!r}")
        base = cls.scalar(sigma)
        return base if gain == 0 else cls("shot", sigma, gain)

    @classmethod
    def map(cls, row, n=None, image_shape=None, name="the noise map"):
        row = noise_map_row(row, np.asarray(row).size if n is None else n, image_shape, name)
        return cls("map", row=row)

    @classmethod
    def from_options(cls, sigma_y, sigma_y_shot=0.0, sigma_y_map=None, op=None):
        """The model of the command line: `--sigma_y s [--sigma_y_shot g]` or `--sigma_y_map FILE.npy` (with --sigma_y 0
        or unset, and no --sigma_y_shot); `op` is the operator whose measurement the map describes."""
        if sigma_y_map is None:
            return cls.shot(sigma_y, sigma_y_shot or 0.0)
        if float(sigma_y or 0.0) != 0.0 or float(sigma_y_shot or 0.0) != 0.0:
            raise ValueError(f"--sigma_y_map {sigma_y_map} states the noise of every entry: --sigma_y and --sigma_y_shot must "
                             f"be 0 or unset with it, got --sigma_y {sigma_y} --sigma_y_shot {sigma_y_shot or 0.0}")
        if op is None or not hasattr(op, "ddnm_plus_step_hn"):
            raise ValueError(f"--sigma_y_map: per-entry measurement noise is supported by {HN_OPERATORS}, not by "
                             f"{type(op).__name__}")
        try:
            arr = np.load(sigma_y_map, allow_pickle=False)
        except (OSError, ValueError) as e:
            raise ValueError(f"--sigma_y_map {sigma_y_map}: not a readable .npy array ({e})") from None
        return cls.map(arr, op.measurement_size(), op.measurement_image_shape(), str(sigma_y_map))

    @property
    def is_scalar(self):
        return self.kind == "scalar"

    def sigma_engine(self):
        """The scalar form's sigma_y on the engine's [-1, 1] scale: what `ddnm_plus_diffusion` takes as a float."""
        if not self.is_scalar:
            raise ValueError(f"a {self.kind} noise model has no single sigma_y")
        return 2 * self.sigma

    def device_row(self, device):
        """The map's row on the engine's scale (2 x, exact in fp32) on `device`; one copy per device."""
        key = str(torch.device(device))
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = torch.from_numpy(self.row * np.float32(2)).to(device).contiguous()
        return t

    def std(self, y_clean):
        """sigma_j on the engine's scale for the clean measurement rows `y_clean` [b, n] (the simulation of --add_noise:
        shot noise takes the clean intensity): a tensor that broadcasts against [b, n]."""
        if self.kind == "scalar":
            return torch.full((1, 1), 2 * self.sigma, dtype=torch.float32, device=y_clean.device)
        if self.kind == "map":
            if y_clean.shape[-1] != self.row.size:
                raise ValueError(f"the noise map has {self.row.size} entries, the measurement rows have {y_clean.shape[-1]}")
            return self.device_row(y_clean.device).reshape(1, -1)
        u = ((y_clean.float() + 1) * 0.5).clamp(0, 1)
        return 2 * (self.sigma ** 2 + self.gain * u).sqrt()

    def settings(self):
        """What a saved measurement records of the model next to `sigma_y`: the shot gain, and a map's SHA-256 (of its
        float32 little-endian row on the [0, 1] scale) and length."""
        import hashlib
        out = {"sigma_y_shot": self.gain, "sigma_y_map_sha256": None, "sigma_y_map_len": None}
        if self.kind == "map":
            out["sigma_y_map_sha256"] = hashlib.sha256(self.row.astype("<f4").tobytes()).hexdigest()
            out["sigma_y_map_len"] = int(self.row.size)
        return out

    def kernel_args(self, device, n):
        """(sigma_map, sigma_mode, s2, g) of the `*_hn_*` entry points (include/ddnm_hip.h) for rows of n entries."""
        if self.kind == "map":
            if self.row.size != n:
                raise ValueError(f"the noise map has {self.row.size} entries, the operator's measurement has {n}")
            return _p(self.device_row(device)), 0, 0.0, 0.0
        if self.kind == "shot":
            return None, 1, self.sigma ** 2, self.gain
        raise ValueError("the scalar noise model runs the scalar DDNM+ step (pass sigma_engine())")


class _PerEntryNoisePlus:
    """DDNM+ with a per-entry `NoiseModel` (shot + read, or a map) in ONE launch: the hook `ddnm_plus_diffusion` calls
    when it is handed a non-scalar model.  `begin_plus_run(y, noise_model)` keeps y -- and moves the map's row to the
    device -- for the run; the class names its entry point and geometry in `_hn_launch`."""

    def begin_plus_run(self, y, noise_model=None):
        y = _flat(y)
        B, n = y.shape[0], self.measurement_size()
        if y.shape[1] != n:
            raise ValueError(f"y must be [{B}, {n}], got {tuple(y.shape)}")
        self._plus_run = (B, ops._f32c(y, "y"))
        self._plus_hn = None
        if noise_model is not None:
            self._plus_hn = noise_model.kernel_args(y.device, n) + (noise_model,)      # (the model keeps the row alive)

    def ddnm_plus_step_hn(self, xt, et, noise, s, sigma_t, eta, x0_out, xt_next):
        """One DDNM+ reverse step under the run's per-entry noise model in one launch: x0|t into `x0_out` (uncorrected),
        x_{t-1} into `xt_next`; `et` may be the [:, :3] view of a 6-channel network output."""
        B = xt.shape[0]
        y, = _plus_state(self, B)
        if getattr(self, "_plus_hn", None) is None:
            raise RuntimeError("ddnm_plus_step_hn needs begin_plus_run(y, noise_model) for this batch first")
        n_x = B * self.channels * self.img_dim ** 2
        for name, t in (("xt", xt), ("x0_out", x0_out), ("xt_next", xt_next)):
            if ops._f32c(t, name).numel() != n_x:
                raise ValueError(f"ddnm_plus_step_hn: {name} has {t.numel()} entries, expected {n_x}")
        sigma_t, eta = float(sigma_t), float(eta)
        fn, geometry = self._hn_launch(B)
        ops.step_call(fn, xt, et, noise, y, _p(x0_out), _p(xt_next), *geometry, *self._plus_hn[:4], sigma_t, sigma_t ** 2,
                      sigma_t * eta, sigma_t * (1 - eta ** 2) ** 0.5, s)


def _flat(vec):
    v = vec.reshape(vec.shape[0], -1)
    if v.dtype != torch.float32 or not v.is_contiguous():
        v = v.float().contiguous()
    return v


def _axpby(x, y, a, b):
    out = torch.empty_like(x)
    ops.call("ddnm_axpby_f32", _p(x), _p(y), _p(out), x.numel(), a, b)
    return out


def _mask_mix(x, y, mask, planes_mask, plane_elems, cx_m, cx_n, cy_m=0.0, cy_n=0.0):
    out = torch.empty_like(x)
    ops.call("ddnm_mask_mix_f32", _p(x), _p(y), _p(mask), planes_mask, plane_elems, _p(out), x.numel(), cx_m, cx_n, cy_m, cy_n)
    return out


def _mul_planes(x, gain, planes_gain, plane_elems):
    """x *= gain in place, `gain` holding `planes_gain` planes of `plane_elems` entries that repeat over the planes of x."""
    ops.call("ddnm_mul_planes_f32", _p(x), _p(gain), planes_gain, plane_elems, _p(x), x.numel())
    return x


def _mask_lambda(vec, epsilon, mask, planes_mask, plane_elems, a, sigma_y, sigma_t, eta):
    """`Lambda` (epsilon None) / `Lambda_noise` of the mask-type operators: singular value 1 where `mask` is 1, null space
    where it is 0 (svd_operators.py:361-439)."""
    if epsilon is None:
        lam = spectral_coefficients(1.0, a, sigma_y, sigma_t, eta)[0]
        return _mask_mix(_flat(vec), None, mask, planes_mask, plane_elems, lam, 1.0)
    coef = noise_coefficients(1.0, a, sigma_y, sigma_t, eta)
    return _mask_mix(_flat(vec), _flat(epsilon), mask, planes_mask, plane_elems, *coef)


def _site_spectral(x, y, V, n, mode, r, B, C, H, W, op, c0, c1=0.0, c2=0.0, c3=0.0):
    out = torch.empty_like(x)
    ops.call("ddnm_site_spectral_f32", _p(x), _p(y), _p(V), n, mode, r, B, C, H, W, _p(out), op, c0, c1, c2, c3)
    return out


def _row_svd(row, device):
    """sigma, V and U[0, 0] (= +-1) of a 1 x n measurement row via torch.svd on the host, like the reference's constructors
    (svd_operators.py:487,633); the null-space columns of V are LAPACK's choice and are part of the contract."""
    U, S, V = torch.svd(torch.tensor([row], dtype=torch.float32), some=False)
    return float(S[0]), V.contiguous().to(device), float(U[0, 0])


def _gather(vec, idx, n_out, scale=None):
    """out[b][i] = vec[b][idx[i]] (idx -1 -> 0; idx None: identity, zero padded) * scale[i] -- ddnm_gather_scale_f32."""
    v = _flat(vec)
    B, n_in = v.shape
    out = torch.empty(B, n_out, dtype=torch.float32, device=v.device)
    ops.call("ddnm_gather_scale_f32", _p(v), _p(idx), _p(scale), _p(out), B, n_in, n_out)
    return out


def _site_matmul(vec, M, sites, n, sb, ss, sj, trans):
    v = _flat(vec)
    out = torch.empty_like(v)
    if n > 16:
        # ddnm_site_matmul_f32 keeps one n x n site matrix in registers (n <= 16: ratio <= 4, colour = 3).  Larger sites
        # (sr_averagepooling with deg_scale 8 / 16 / 32, evaluation.sh:18: n = ratio^2 entries per patch) lie contiguously
        # in the site-major layout, so all sites of all images are the rows of ONE matrix and V_small / Vt_small act as a
        # single MFMA GEMM: out[B*sites][n] = in[B*sites][n] . Mop^T  (svd_operators.py:490-517)
        if sj != 1 or ss != n or sb != sites * n:
            raise NotImplementedError(f"site matrix with {n} entries per site needs the contiguous site-major layout")
        rows = v.shape[0] * sites
        # Mop = M (trans 0): out = in . M^T -> B operand stored [N = i][K = j] = M itself; Mop = M^T: stored [K = j][N = i]
        ops.bgemm(v, M, out, rows, n, n, lda=n, ldb=n, ldc=n, transb=not trans)
        return out
    ops.call("ddnm_site_matmul_f32", _p(v), _p(M), _p(out), v.shape[0], sites, n, sb, ss, sj, int(trans))
    return out


def _left(L, x, rows, inner, planes, out=None, images=None):
    """out[p] = L . X[p] for the `planes` planes X [inner x inner] of `x`; L is [rows x inner].  `images` = (C, batch stride):
    `x` is [B][C] planes read through its batch stride (et as the [:, :3] view of a 6-channel output)."""
    if out is None:
        out = torch.empty(planes, rows, inner, dtype=torch.float32, device=x.device)
    C, sb = images or (1, 0)
    return ops.bgemm(L, x, out, rows, inner, inner, lda=inner, ldb=inner, ldc=inner, transb=False, batch=planes, inner=C,
                     sB=(sb, inner * inner) if images else (inner * inner, 0),
                     sC=(C * rows * inner, rows * inner) if images else (rows * inner, 0))


def _right(t, Rt, rows, inner, cols, planes, out=None, ldc=None, D=None, beta=None):
    """out[p] = T[p] . R for the `planes` planes T [rows x inner] of `t`; R is given transposed, Rt [cols x inner] row-major
    (the [N][K] operand layout of the GEMM).  `out` with its own leading dimension `ldc`: the product lands in the top-left
    rows x cols of wider planes.  `beta`: the epilogue out += beta * D[p], D [rows x cols] per plane (D may be None)."""
    if out is None:
        out = torch.empty(planes, rows, cols, dtype=torch.float32, device=t.device)
    ldd, sD = (0, 0) if beta is None else (cols, rows * cols)
    return ops.bgemm(t, Rt, out, rows, cols, inner, lda=inner, ldb=inner, ldc=ldc or cols, transb=True, batch=planes,
                     sA=(rows * inner, 0), sC=(out.numel() // planes, 0), D=D, ldd=ldd, sD=(sD, 0), beta=beta or 0.0)


def _two_sided(L, x, Rt, rows, inner, cols, **right):
    """L . X . R for every (image, channel) plane X [inner x inner] of `x`, as [planes, rows, cols] (see _left / _right)."""
    planes = x.numel() // (inner * inner)
    return _right(_left(L, x, rows, inner, planes), Rt, rows, inner, cols, planes, **right)


def _plus_state(op, B):
    """What begin_plus_run(y) left for a batch of B images (`op._plus_run` behind its batch size)."""
    run = getattr(op, "_plus_run", None)
    if run is None or run[0] != B:
        raise RuntimeError("ddnm_plus_step needs begin_plus_run(y) for this batch first")
    return run[1:]


def _pad_scale(f, n):
    """Per-entry factors over the big (V) dimension: `f` on the first len(f) entries, ONES beyond (those entries of the
    gathered vector are zero already, so their factor is never seen)."""
    out = torch.ones(n, dtype=torch.float32, device=f.device)
    out[: f.numel()] = f
    return out.contiguous()


def _inverse_perm(idx):
    inv = torch.empty_like(idx)
    inv[idx.long()] = torch.arange(idx.numel(), dtype=idx.dtype)
    return inv


class A_functions:
    """Abstract base, same surface as svd_operators.py:9-97 (matrix-free SVD operator)."""

    channels = 3
    img_dim = 256

    def A(self, vec):
        raise NotImplementedError()

    def A_pinv(self, vec):
        raise NotImplementedError()

    def singulars(self):
        raise NotImplementedError()

    # ---- what a measurement looks like (host only, nothing is launched): the runner writes y with DDNM_SAVE_Y=1 and
    # reads it back with --path_y measurements:DIR
    def measurement_size(self):
        """Number of valid entries of a row of A(x)."""
        raise NotImplementedError()

    def measurement_image_shape(self):
        """(c, h, w) when a row of A(x) is a picture in CHW order that an image file can hold, else None."""
        return None

    # ---- the matrix-free SVD surface (svd_operators.py:16-50).  The sampling path never calls these -- A / A_pinv /
    # Lambda* above are evaluated in their direct forms -- but a drop-in offers them: the BASELINE operators implement
    # V / Vt / U / Ut / add_zeros with the reference's spectral orderings, and At / A_pinv_eta follow from them exactly
    # as the reference base class derives them (:60-66,82-91).
    def V(self, vec):
        raise NotImplementedError()

    def Vt(self, vec):
        raise NotImplementedError()

    def U(self, vec):
        raise NotImplementedError()

    def Ut(self, vec):
        raise NotImplementedError()

    def add_zeros(self, vec):
        raise NotImplementedError()

    def _spectral_dim(self):
        return self.channels * self.img_dim ** 2

    def At(self, vec):                                              # :60-66
        s = self.singulars().float().contiguous()
        temp = self.Ut(vec)
        return self.V(_gather(temp, None, self._spectral_dim(), scale=_pad_scale(s, self._spectral_dim())))

    def A_pinv_eta(self, vec, eta):                                 # :82-91
        s = self.singulars().float()
        temp = self.Ut(vec)
        return self.V(_gather(temp, None, self._spectral_dim(), scale=_pad_scale(s / (s * s + eta), self._spectral_dim())))

    def Lambda(self, vec, a, sigma_y, sigma_t, eta):
        raise NotImplementedError()

    def Lambda_noise(self, vec, a, sigma_y, sigma_t, eta, epsilon):
        raise NotImplementedError()

    # ---- engine hook -----------------------------------------------------------------
    def ddnm_step(self, xt, et, noise, y, s, x0_out, xt_next):
        """Generic step: x0, proj = A^+(A x0 - y), combine.  Subclasses fuse it."""
        ops.step_x0(xt, et, s, out=x0_out)
        resid = _axpby(self.A(x0_out), _flat(y), 1.0, -1.0)
        proj = self.A_pinv(resid).reshape(xt.shape)
        ops.step_combine(x0_out, proj, None, noise, et, s, out=xt_next)


class Denoising(_PerEntryNoisePlus, A_functions):
    def __init__(self, channels, img_dim, device):
        self.channels, self.img_dim, self.device = channels, img_dim, device

    def A(self, vec):
        return vec.reshape(vec.shape[0], -1).clone()

    def A_pinv(self, vec):
        return vec.reshape(vec.shape[0], -1).clone()

    def measurement_size(self):
        return self.channels * self.img_dim ** 2

    def measurement_image_shape(self):
        return (self.channels, self.img_dim, self.img_dim)

    def singulars(self):
        return torch.ones(self.channels * self.img_dim ** 2, device=self.device)

    def V(self, vec):                                                      # svd_operators.py:447-462: all identities
        return _flat(vec).clone()

    Vt = U = Ut = add_zeros = V

    def Lambda(self, vec, a, sigma_y, sigma_t, eta):                       # svd_operators.py:464-469
        if float(sigma_t) < float(a) * sigma_y:
            return _axpby(_flat(vec), None, float(sigma_t) * (1 - eta ** 2) ** 0.5 / float(a) / sigma_y, 0.0)
        return _flat(vec)

    def Lambda_noise(self, vec, a, sigma_y, sigma_t, eta, epsilon):        # :471-476 (epsilon is ignored there)
        a, sigma_t = float(a), float(sigma_t)
        f = (sigma_t ** 2 - a ** 2 * sigma_y ** 2) ** 0.5 if sigma_t >= a * sigma_y else sigma_t * eta
        return _axpby(_flat(vec), None, f, 0.0)

    def ddnm_step(self, xt, et, noise, y, s, x0_out, xt_next):
        B = xt.shape[0]
        ops.step_call("ddnm_step_denoise_f32", xt, et, noise, y, _p(x0_out), _p(xt_next), B, xt.numel() // B, s)

    # A per-entry NoiseModel runs the DDNM+ step in ONE launch (`begin_plus_run(y, noise_model)`, `ddnm_plus_step_hn` of
    # _PerEntryNoisePlus); the scalar sigma_y keeps the reference's Lambda / Lambda_noise chain above (no `ddnm_plus_step`).
    def _hn_launch(self, B):
        return "ddnm_step_plus_denoise_hn_f32", (B, self.channels * self.img_dim ** 2)


class _RowOperator(A_functions):
    """What SuperResolution and Colorization share: every site (r x r patch / pixel) is measured by the same 1 x n row
    `_row()`, decomposed once on the host; `_site(v)` = (n, mode, r, B, C, H, W) of ddnm_site_spectral_f32."""

    def _svd(self):
        if not hasattr(self, "_V"):
            self._s, self._V, self._u = _row_svd(self._row(), self.device)
        return self._s, self._V

    def U(self, vec):                                                      # svd_operators.py:519-523,658-662 (U is 1 x 1)
        self._svd()
        return _axpby(_flat(vec), None, self._u, 0.0)

    Ut = U

    def add_zeros(self, vec):                                              # :528-533,667-671
        return _gather(vec, None, self._spectral_dim())

    def Lambda(self, vec, a, sigma_y, sigma_t, eta):                       # svd_operators.py:535-571,669-695
        s, V = self._svd()
        v = _flat(vec)
        return _site_spectral(v, None, V, *self._site(v), 0, spectral_coefficients(s, a, sigma_y, sigma_t, eta)[0])

    def Lambda_noise(self, vec, a, sigma_y, sigma_t, eta, epsilon):        # :573-623,697-736
        s, V = self._svd()
        v = _flat(vec)
        return _site_spectral(v, _flat(epsilon), V, *self._site(v), 1, *noise_coefficients(s, a, sigma_y, sigma_t, eta))


class SuperResolution(_RowOperator):
    def __init__(self, channels, img_dim, ratio, device):
        assert img_dim % ratio == 0
        self.channels, self.img_dim, self.ratio, self.device = channels, img_dim, ratio, device
        self.y_dim = img_dim // ratio

    def measurement_size(self):
        return self.channels * self.y_dim ** 2

    def measurement_image_shape(self):
        return (self.channels, self.y_dim, self.y_dim)

    def A(self, vec):
        x = _img(vec, self.channels, self.img_dim)
        B = x.shape[0]
        y = torch.empty(B, self.channels * self.y_dim ** 2, dtype=torch.float32, device=x.device)
        ops.call("ddnm_op_avgpool_f32", _p(x), _p(y), B * self.channels, self.img_dim, self.img_dim, self.ratio)
        return y

    def A_pinv(self, vec):
        B = vec.shape[0]
        y = vec.reshape(B, -1).float().contiguous()
        x = torch.empty(B, self.channels * self.img_dim ** 2, dtype=torch.float32, device=y.device)
        ops.call("ddnm_op_upsample_f32", _p(y), _p(x), B * self.channels, self.img_dim, self.img_dim, self.ratio)
        return x

    def singulars(self):
        return torch.full((self.channels * self.y_dim ** 2,), 1.0 / self.ratio, device=self.device)

    def _row(self):
        return [1 / self.ratio ** 2] * self.ratio ** 2

    def _site(self, v):
        return self.ratio ** 2, 0, self.ratio, v.shape[0], self.channels, self.img_dim, self.img_dim

    def _tables(self):
        """Index tables of V / Vt (svd_operators.py:490-517): image (CHW) <-> site-major patches [C*y*y][r*r]
        (`unfold(2,r,r).unfold(3,r,r)`) <-> spectral order (component 0 of every site first, then the other r*r-1
        components interleaved per site: `recon[:, (S+idx)::(n-1)]`)."""
        if not hasattr(self, "_t_img2site"):
            C, d, r, yd = self.channels, self.img_dim, self.ratio, self.y_dim
            n, S = r * r, C * yd * yd
            c, py, px, dy, dx = torch.meshgrid(torch.arange(C), torch.arange(yd), torch.arange(yd), torch.arange(r),
                                               torch.arange(r), indexing="ij")
            img2site = (c * d * d + (py * r + dy) * d + (px * r + dx)).reshape(-1).to(torch.int32)     # [(s, j)] -> image index
            sidx, k = torch.meshgrid(torch.arange(S), torch.arange(n), indexing="ij")
            site2spec = torch.where(k == 0, sidx, S + sidx * (n - 1) + (k - 1)).reshape(-1).to(torch.int32)
            dev = self.device
            self._t_img2site, self._t_site2img = img2site.to(dev), _inverse_perm(img2site).to(dev)
            self._t_site2spec, self._t_spec2site = site2spec.to(dev), _inverse_perm(site2spec).to(dev)
        return self._t_img2site, self._t_site2img, self._t_site2spec, self._t_spec2site

    def Vt(self, vec):                                                     # svd_operators.py:505-517
        img2site, _, _, spec2site = self._tables()
        n, N = self.ratio ** 2, self._spectral_dim()
        t = _gather(vec, img2site, N)
        t = _site_matmul(t, self._svd()[1], N // n, n, N, n, 1, trans=True)
        return _gather(t, spec2site, N)

    def V(self, vec):                                                      # :490-503
        _, site2img, site2spec, _ = self._tables()
        n, N = self.ratio ** 2, self._spectral_dim()
        t = _gather(vec, site2spec, N)
        t = _site_matmul(t, self._svd()[1], N // n, n, N, n, 1, trans=False)
        return _gather(t, site2img, N)

    def ddnm_step(self, xt, et, noise, y, s, x0_out, xt_next):
        if self.ratio != 4 or self.channels != 3:
            return super().ddnm_step(xt, et, noise, y, s, x0_out, xt_next)
        ops.step_call("ddnm_step_sr_avgpool_f32", xt, et, noise, y, _p(x0_out), _p(xt_next), xt.shape[0], self.img_dim,
                      self.img_dim, self.ratio, s)


class Colorization(_RowOperator):
    THIRDS = (0.3333, 0.3334, 0.3333)       # the default measurement row (svd_operators.py:632)

    def __init__(self, img_dim, device, weights=None):
        """`weights`: per-pixel measurement row; None = (0.3333, 0.3334, 0.3333) (svd_operators.py:632).
        The simplified path passes (1/3, 1/3, 1/3) (guided_diffusion/diffusion.py:33-42)."""
        self.channels, self.img_dim, self.device = 3, img_dim, device
        self._w = None if weights is None else (ctypes.c_float * 3)(*[float(v) for v in weights])

    def measurement_size(self):
        return self.img_dim ** 2

    def measurement_image_shape(self):
        return (1, self.img_dim, self.img_dim)

    def A(self, vec):
        x = _img(vec, 3, self.img_dim)
        B, HW = x.shape[0], self.img_dim ** 2
        y = torch.empty(B, HW, dtype=torch.float32, device=x.device)
        ops.call("ddnm_op_color_A_f32", _p(x), _p(y), B, HW, self._w)
        return y

    def A_pinv(self, vec):
        B, HW = vec.shape[0], self.img_dim ** 2
        y = vec.reshape(B, -1).float().contiguous()
        x = torch.empty(B, 3 * HW, dtype=torch.float32, device=y.device)
        ops.call("ddnm_op_color_pinv_f32", _p(y), _p(x), B, HW, self._w)
        return x

    def singulars(self):
        w = torch.tensor(self._row())
        return torch.full((self.img_dim ** 2,), float((w * w).sum().sqrt()), device=self.device)

    def _row(self):
        return list(self.THIRDS) if self._w is None else [float(v) for v in self._w]

    def _site(self, v):
        return 3, 1, 1, v.shape[0], 3, self.img_dim, self.img_dim

    def Vt(self, vec):                                                     # svd_operators.py:647-656
        hw = self.img_dim ** 2                  # needles of the CHW planes; the spectral order is component-major too
        return _site_matmul(vec, self._svd()[1], hw, 3, 3 * hw, 1, hw, trans=True)

    def V(self, vec):                                                      # :636-645
        hw = self.img_dim ** 2
        return _site_matmul(vec, self._svd()[1], hw, 3, 3 * hw, 1, hw, trans=False)

    def ddnm_step(self, xt, et, noise, y, s, x0_out, xt_next):
        ops.step_call("ddnm_step_color_f32", xt, et, noise, y, _p(x0_out), _p(xt_next), xt.shape[0], self.img_dim ** 2,
                      self._w, s)


def _rank_table(keep):
    """bool [HW] (pixel kept) -> int32 [HW]: index of the pixel among the kept ones in ascending order, -1 = missing."""
    rank = torch.cumsum(keep.int(), 0) - 1
    rank[~keep] = -1
    return rank.to(torch.int32)


class _MissingEntries(A_functions):
    """The spectral surface of the reference's Inpainting (svd_operators.py:324-359) for ANY set of missing entries of the
    HWC-interleaved image: whole pixels (Inpainting) or the two colour entries a filter array does not sample (Mosaic).
    A subclass sets `missing_indices`, `img_dim` and `device`."""

    def _tables(self):
        """Vt = the permutation [kept (ascending HWC-interleaved index), missing (in `missing_indices` order)] of the
        HWC-interleaved image (svd_operators.py:339-344); V its inverse."""
        if not hasattr(self, "_t_vt"):
            hw = self.img_dim ** 2
            miss = self.missing_indices.detach().cpu().long()
            keep = torch.ones(3 * hw, dtype=torch.bool)
            keep[miss] = False
            order = torch.cat([torch.nonzero(keep).reshape(-1), miss])          # spectral position -> HWC index
            img = ((order % 3) * hw + order // 3).to(torch.int32)               # HWC index p*3 + c -> CHW index c*HW + p
            self._t_vt, self._t_v = img.to(self.device), _inverse_perm(img).to(self.device)
        return self._t_vt, self._t_v

    def Vt(self, vec):
        return _gather(vec, self._tables()[0], self._spectral_dim())

    def V(self, vec):                                                      # :332-337
        return _gather(vec, self._tables()[1], self._spectral_dim())

    def U(self, vec):                                                      # :346-350
        return _flat(vec).clone()

    Ut = U

    def add_zeros(self, vec):                                              # :355-359
        return _gather(vec, None, self._spectral_dim())


class Inpainting(_MissingEntries):
    def __init__(self, channels, img_dim, missing_indices, device):
        if channels != 3:
            raise NotImplementedError("Inpainting kernels assume 3 channels")
        self.channels, self.img_dim, self.device = channels, img_dim, device
        hw = img_dim ** 2
        # `missing_indices` index the HWC-interleaved image (guided_diffusion/diffusion.py:465-470);
        # a pixel is missing iff its 3 interleaved entries are.
        miss = torch.zeros(3 * hw, dtype=torch.bool)
        miss[missing_indices.detach().cpu().long()] = True
        miss = miss.reshape(hw, 3)
        if not bool((miss.all(1) == miss.any(1)).all()):
            raise NotImplementedError("per-channel masks are not supported (reference masks whole pixels)")
        keep = ~miss[:, 0]
        self.n_kept = int(keep.sum())
        self.rank = _rank_table(keep).to(device).contiguous()
        self.kept_mask = keep.float().to(device).contiguous()            # [HW], shared by the 3 channel planes
        self.missing_indices = missing_indices

    def measurement_size(self):
        return 3 * self.n_kept

    def measurement_image_shape(self):
        """A full-size picture: the measurement is read from it by applying A (the hole's pixels are ignored)."""
        return (3, self.img_dim, self.img_dim)

    def A(self, vec):
        x = _img(vec, 3, self.img_dim)
        B = x.shape[0]
        y = torch.empty(B, 3 * self.n_kept, dtype=torch.float32, device=x.device)
        ops.call("ddnm_op_inpaint_A_f32", _p(x), _p(self.rank), self.n_kept, _p(y), B, self.img_dim ** 2)
        return y

    def A_pinv(self, vec):
        B = vec.shape[0]
        y = vec.reshape(B, -1).float().contiguous()
        x = torch.empty(B, 3 * self.img_dim ** 2, dtype=torch.float32, device=y.device)
        ops.call("ddnm_op_inpaint_pinv_f32", _p(y), _p(self.rank), self.n_kept, _p(x), B, self.img_dim ** 2)
        return x

    def singulars(self):
        return torch.ones(3 * self.n_kept, device=self.device)

    def Lambda(self, vec, a, sigma_y, sigma_t, eta):                       # svd_operators.py:361-387
        return _mask_lambda(vec, None, self.kept_mask, 1, self.img_dim ** 2, a, sigma_y, sigma_t, eta)

    def Lambda_noise(self, vec, a, sigma_y, sigma_t, eta, epsilon):        # :389-439
        return _mask_lambda(vec, epsilon, self.kept_mask, 1, self.img_dim ** 2, a, sigma_y, sigma_t, eta)

    def ddnm_step(self, xt, et, noise, y, s, x0_out, xt_next):
        ops.step_call("ddnm_step_inpaint_f32", xt, et, noise, y, _p(self.rank), self.n_kept, _p(x0_out), _p(xt_next),
                      xt.shape[0], self.img_dim ** 2, s)


class InpaintingBank:
    """N inpainting masks for a run whose images each have their own hole: `masks` is [N, S, S] or [N, S*S], nonzero =
    kept (the reference's `mask == 0 -> missing`, guided_diffusion/diffusion.py:465-470).  All N rank tables are built
    once, like Inpainting's; `for_images(indices)` gives the operator of a batch, image i using mask i % N.  `y_dim`, the
    row length of every measurement, is 3 * max(n_kept) rounded up to a multiple of 4 and constant for the bank, so
    measurements of different loader batches concatenate."""

    def __init__(self, channels, img_dim, masks, device):
        if channels != 3:
            raise ValueError(f"inpainting masks whole RGB pixels: channels must be 3, got {channels}")
        masks = torch.as_tensor(np.asarray(masks))
        hw = img_dim ** 2
        if masks.dim() not in (2, 3) or masks.shape[0] < 1 or masks.numel() != masks.shape[0] * hw or \
                (masks.dim() == 3 and tuple(masks.shape[1:]) != (img_dim, img_dim)):
            raise ValueError(f"mask bank must be [N, {img_dim}, {img_dim}] or [N, {hw}], got {tuple(masks.shape)}")
        keep = masks.reshape(masks.shape[0], hw) != 0
        self.n_kept = [int(k) for k in keep.sum(1)]
        if min(self.n_kept) < 1:
            raise ValueError(f"mask {self.n_kept.index(min(self.n_kept))} of the bank keeps no pixel")
        self.channels, self.img_dim, self.device = channels, img_dim, device
        self.y_dim = 4 * ((3 * max(self.n_kept) + 3) // 4)
        self.rank = torch.stack([_rank_table(k) for k in keep]).to(device).contiguous()      # [N][HW]
        self.kept_mask = keep.float().to(device).contiguous()                                # [N][HW]

    def __len__(self):
        return len(self.n_kept)

    def measurement_size(self, i):
        """Valid entries of the measurement row of the image with global index `i` (mask i % N); the row is `y_dim` long."""
        return 3 * self.n_kept[int(i) % len(self)]

    def measurement_image_shape(self):
        return (3, self.img_dim, self.img_dim)

    def for_images(self, indices):
        """The operator of the images with these global indices, in this order (one index-to-row gather on the device)."""
        rows = [int(i) % len(self) for i in indices]
        if not rows:
            raise ValueError("for_images needs at least one image index")
        idx = torch.tensor(rows, dtype=torch.long).to(self.device)
        hw = self.img_dim ** 2
        kept3 = self.kept_mask.index_select(0, idx)[:, None, :].expand(len(rows), 3, hw).contiguous()
        return PerImageInpainting(self.img_dim, self.rank.index_select(0, idx), kept3, [self.n_kept[r] for r in rows],
                                  self.y_dim, rows)


class PerImageInpainting(A_functions):
    """Inpainting whose mask differs per image: image b of the batch has the rank table `rank[b]` and the measurement row
    y[b] = its 3 * n_kept[b] kept entries in the reference's HWC order (svd_operators.py:324-359), zero padded to
    `y_dim`.  Built by InpaintingBank.for_images; `narrow` / `concat` re-batch built operators without a host round trip.
    The operator is tied to its batch: every method raises ValueError for another batch size."""

    def __init__(self, img_dim, rank, kept3, n_kept, y_dim, rows):
        self.channels, self.img_dim, self.device = 3, img_dim, rank.device
        self.rank, self.kept3 = rank, kept3               # int32 [B][HW]; fp32 [B][3][HW] kept-mask of the CHW planes
        self.n_kept, self.y_dim, self.rows = list(n_kept), y_dim, list(rows)

    def __len__(self):
        return len(self.n_kept)

    def measurement_size(self):
        """One number per image of the batch: the rest of each `y_dim`-long row is padding."""
        return [3 * n for n in self.n_kept]

    def measurement_image_shape(self):
        return (3, self.img_dim, self.img_dim)

    def _check_batch(self, B):
        if B != len(self):
            raise ValueError(f"PerImageInpainting holds the masks of {len(self)} images, the batch has {B} images")

    def narrow(self, lo, hi):
        """The operator of images [lo, hi) of this batch (views of its device rows)."""
        if not 0 <= lo < hi <= len(self):
            raise ValueError(f"narrow({lo}, {hi}) of a batch of {len(self)} images")
        return PerImageInpainting(self.img_dim, self.rank[lo:hi], self.kept3[lo:hi], self.n_kept[lo:hi], self.y_dim,
                                  self.rows[lo:hi])

    @classmethod
    def concat(cls, parts):
        """One operator for the images of several batches of the same bank, in order."""
        parts = list(parts)
        if len({(p.img_dim, p.y_dim) for p in parts}) != 1:
            raise ValueError("concat needs operators of one bank")
        if len(parts) == 1:
            return parts[0]
        return cls(parts[0].img_dim, torch.cat([p.rank for p in parts], 0), torch.cat([p.kept3 for p in parts], 0),
                   [n for p in parts for n in p.n_kept], parts[0].y_dim, [r for p in parts for r in p.rows])

    def A(self, vec):
        x = _img(vec, 3, self.img_dim)
        B = x.shape[0]
        self._check_batch(B)
        y = ops.fill_(torch.empty(B, self.y_dim, dtype=torch.float32, device=x.device))      # padding is exactly 0
        ops.call("ddnm_op_inpaint_A_pi_f32", _p(x), _p(self.rank), max(self.n_kept), _p(y), self.y_dim, B, self.img_dim ** 2)
        return y

    def A_pinv(self, vec):
        B = vec.shape[0]
        self._check_batch(B)
        y = vec.reshape(B, -1).float().contiguous()
        if y.shape[1] != self.y_dim:
            raise ValueError(f"measurement rows have {y.shape[1]} entries, the bank's y_dim is {self.y_dim}")
        x = torch.empty(B, 3 * self.img_dim ** 2, dtype=torch.float32, device=y.device)
        ops.call("ddnm_op_inpaint_pinv_pi_f32", _p(y), self.y_dim, _p(self.rank), max(self.n_kept), _p(x), B, self.img_dim ** 2)
        return x

    def _ragged(self, *args, **kwargs):
        raise NotImplementedError("the spectral dimension is ragged (3 * n_kept differs per image): PerImageInpainting "
                                  "has A, A_pinv, Lambda, Lambda_noise and ddnm_step only")

    singulars = V = Vt = U = Ut = add_zeros = At = A_pinv_eta = _ragged

    def Lambda(self, vec, a, sigma_y, sigma_t, eta):                       # Inpainting.Lambda with image b's mask
        self._check_batch(vec.shape[0])
        return _mask_lambda(vec, None, self.kept3, 3 * len(self), self.img_dim ** 2, a, sigma_y, sigma_t, eta)

    def Lambda_noise(self, vec, a, sigma_y, sigma_t, eta, epsilon):
        self._check_batch(vec.shape[0])
        return _mask_lambda(vec, epsilon, self.kept3, 3 * len(self), self.img_dim ** 2, a, sigma_y, sigma_t, eta)

    def ddnm_step(self, xt, et, noise, y, s, x0_out, xt_next):
        B = xt.shape[0]
        self._check_batch(B)
        if y.shape[0] != B or y.numel() != B * self.y_dim:
            raise ValueError(f"y must be [{B}, {self.y_dim}], got {tuple(y.shape)}")
        ops.step_call("ddnm_step_inpaint_pi_f32", xt, et, noise, y, self.y_dim, _p(self.rank), max(self.n_kept), _p(x0_out),
                      _p(xt_next), B, self.img_dim ** 2, s)


# Colour filter arrays by name: [ph, pw] channel codes (0 = R, 1 = G, 2 = B), pixel (r, c) samples pattern[r % ph][c % pw].
# `xtrans` (20 G, 8 R and 8 B per 6 x 6 period) is this project's definition of the name.
_G, _R, _B = 1, 0, 2
CFA_PATTERNS = {
    "rggb": [[0, 1], [1, 2]],
    "bggr": [[2, 1], [1, 0]],
    "grbg": [[1, 0], [2, 1]],
    "gbrg": [[1, 2], [0, 1]],
    "xtrans": [[_G, _B, _G, _G, _R, _G],
               [_R, _G, _R, _B, _G, _B],
               [_G, _B, _G, _G, _R, _G],
               [_G, _R, _G, _G, _B, _G],
               [_B, _G, _B, _R, _G, _R],
               [_G, _R, _G, _G, _B, _G]],
}
CFA_MAX_PERIOD = 8


def cfa_pattern(pattern):
    """A name of CFA_PATTERNS or a 2-D integer array -> the validated uint8 array [ph, pw] of channel codes."""
    if isinstance(pattern, str):
        if pattern not in CFA_PATTERNS:
            raise ValueError(f"unknown colour filter array {pattern!r}: the named ones are {', '.join(CFA_PATTERNS)}")
        pattern = CFA_PATTERNS[pattern]
    p = np.asarray(pattern)
    if p.ndim != 2 or p.dtype.kind not in "iu" or p.size == 0:
        raise ValueError(f"a colour filter array is a 2-D integer array of channel codes, got shape {p.shape} of {p.dtype}")
    if max(p.shape) > CFA_MAX_PERIOD:
        raise ValueError(f"the period of a colour filter array is 1 to {CFA_MAX_PERIOD} pixels each way, got {p.shape[0]} x "
                         f"{p.shape[1]}")
    if p.min() < 0 or p.max() > 2:
        raise ValueError("the channel codes of a colour filter array are 0 (R), 1 (G) and 2 (B), got "
                         f"{sorted(set(int(v) for v in p.reshape(-1)))}")
    return np.ascontiguousarray(p, dtype=np.uint8)


class Mosaic(_PerEntryNoisePlus, _MissingEntries):
    """Demosaicing: a raw sensor frame keeps ONE colour sample per pixel, behind the periodic colour filter array
    `pattern` (a name of CFA_PATTERNS or a [ph, pw] array of channel codes).  It is the reference's Inpainting
    (svd_operators.py:324-439) over the HWC-interleaved entries with the two channels a pixel does not sample missing:
    `missing_indices` holds those entries 3p + c in ascending order, y[b][p] = x[b][cfa(p)][p] in pixel order, A^+ the
    scatter back, every singular value 1.  The sampling set is periodic, so the kernels derive it from the pattern in
    their arguments (no rank table) and read y as a dense one-channel picture; the whole DDNM+ step is diagonal in the
    image and runs as ONE kernel (`ddnm_plus_step`).  A pattern that never samples a channel leaves it in the null space."""

    def __init__(self, channels, img_dim, pattern, device):
        if channels != 3:
            raise ValueError(f"a colour filter array samples RGB images: channels must be 3, got {channels}")
        if img_dim % 4:
            raise ValueError(f"Mosaic kernels handle four pixels of a row at once: img_dim must be a multiple of 4, got {img_dim}")
        self.channels, self.img_dim, self.device = channels, img_dim, device
        self.pattern = cfa_pattern(pattern)
        ph, pw = self.pattern.shape
        self._cfa = ((ctypes.c_uint8 * (ph * pw))(*[int(v) for v in self.pattern.reshape(-1)]), ph, pw)
        r, c = np.divmod(np.arange(img_dim ** 2), img_dim)
        code = torch.from_numpy(self.pattern[r % ph, c % pw].astype(np.int64))              # [HW]: the channel pixel p samples
        sampled = torch.arange(3)[:, None] == code[None, :]                                   # [3][HW]
        self.sampled_mask = sampled.float().to(device).contiguous()
        self.missing_indices = torch.nonzero(~sampled.t().reshape(-1)).reshape(-1)            # HWC entries 3p + c, ascending

    def measurement_size(self):
        return self.img_dim ** 2

    def measurement_image_shape(self):
        return (1, self.img_dim, self.img_dim)

    def A(self, vec):
        x = _img(vec, 3, self.img_dim)
        B, d = x.shape[0], self.img_dim
        y = torch.empty(B, d * d, dtype=torch.float32, device=x.device)
        ops.call("ddnm_op_mosaic_A_f32", _p(x), _p(y), B, d, d, *self._cfa)
        return y

    def A_pinv(self, vec):
        y = _flat(vec)
        B, d = y.shape[0], self.img_dim
        if y.shape[1] != d * d:
            raise ValueError(f"measurement rows have {y.shape[1]} entries, a {d} x {d} mosaic has {d * d}")
        x = torch.empty(B, 3 * d * d, dtype=torch.float32, device=y.device)
        ops.call("ddnm_op_mosaic_pinv_f32", _p(y), _p(x), B, d, d, *self._cfa)
        return x

    def singulars(self):
        return torch.ones(self.img_dim ** 2, device=self.device)

    def Lambda(self, vec, a, sigma_y, sigma_t, eta):                       # svd_operators.py:361-387
        return _mask_lambda(vec, None, self.sampled_mask, 3, self.img_dim ** 2, a, sigma_y, sigma_t, eta)

    def Lambda_noise(self, vec, a, sigma_y, sigma_t, eta, epsilon):        # :389-439
        return _mask_lambda(vec, epsilon, self.sampled_mask, 3, self.img_dim ** 2, a, sigma_y, sigma_t, eta)

    def _check_y(self, y, B):
        if y.shape[0] != B or y.numel() != B * self.img_dim ** 2:
            raise ValueError(f"y must be [{B}, {self.img_dim ** 2}], got {tuple(y.shape)}")
        return ops._f32c(y, "y")

    def ddnm_step(self, xt, et, noise, y, s, x0_out, xt_next):
        B, d = xt.shape[0], self.img_dim
        ops.step_call("ddnm_step_mosaic_f32", xt, et, noise, self._check_y(y, B), _p(x0_out), _p(xt_next), B, d, d, *self._cfa, s)

    # ---- DDNM+ (sigma_y > 0): the engine hook of `ddnm_plus_diffusion`.  Lambda / Lambda_noise above stay callable (the
    # reference's object protocol); the loop takes the one fused launch instead of their eight.
    # `begin_plus_run(y, noise_model=None)` and `ddnm_plus_step_hn` (a per-entry NoiseModel) come from _PerEntryNoisePlus.
    def _hn_launch(self, B):
        return "ddnm_step_plus_mosaic_hn_f32", (B, self.img_dim, self.img_dim, *self._cfa)

    def ddnm_plus_step(self, xt, et, noise, s, sigma_y, sigma_t, eta, x0_out, xt_next):
        """One DDNM+ reverse step in one launch: x0|t into `x0_out` (uncorrected, as the loop returns and time-travels
        from it), x_{t-1} into `xt_next`; `et` may be the [:, :3] view of a 6-channel network output."""
        B, d = xt.shape[0], self.img_dim
        y, = _plus_state(self, B)
        for name, t in (("xt", xt), ("x0_out", x0_out), ("xt_next", xt_next)):
            if ops._f32c(t, name).numel() != 3 * B * d * d:
                raise ValueError(f"ddnm_plus_step: {name} has {t.numel()} entries, expected {3 * B * d * d}")
        coef = cs_plus_coefficients(s.sqrt_at_next, sigma_y, sigma_t, eta)
        ops.step_call("ddnm_step_plus_mosaic_f32", xt, et, noise, y, _p(x0_out), _p(xt_next), B, d, d, *self._cfa,
                      *(float(v) for v in coef), s)


class WalshHadamardCS(A_functions):
    def __init__(self, channels, img_dim, ratio, perm, device):
        self.channels, self.img_dim, self.ratio, self.device = channels, img_dim, ratio, device
        self.N = img_dim ** 2
        self.n_keep = channels * self.N // ratio
        self.perm = perm.to(device=device, dtype=torch.int32).contiguous()
        # spectral mask W[c][q] = 1 iff the (k, c)-interleaved index of q = perm[k] is measured
        k = torch.arange(self.N)
        mask = torch.zeros(channels, self.N)
        pc = perm.detach().cpu().long()
        for c in range(channels):
            mask[c, pc] = ((k * channels + c) < self.n_keep).float()
        self.mask = mask.to(device).contiguous()
        self._scratch = None
        self._apy = None
        self._apy_key = None

    def _buf(self, B):
        if self._scratch is None or self._scratch.shape[0] < B:
            self._scratch = torch.empty(B, self.channels, self.N, dtype=torch.float32, device=self.device)
        return self._scratch

    def measurement_size(self):
        return self.n_keep

    def _fwht(self, planes):
        out = torch.empty_like(planes)
        B = planes.numel() // (self.channels * self.N)
        ops.call("ddnm_fwht2d_f32", _p(planes), _p(out), B * self.channels, self.img_dim)
        return out

    def _permuted(self, vec, n):
        """The first `n` entries of the permuted, (k, c)-interleaved order of the coefficient planes of `vec`, as [B, n]."""
        x = _img(vec, self.channels, self.img_dim)
        coef = self._fwht(x)                    # held in a local across the launch that reads it
        out = torch.empty(x.shape[0], n, dtype=torch.float32, device=x.device)
        ops.call("ddnm_wh_gather_f32", _p(coef), _p(self.perm), _p(out), x.shape[0], self.channels, self.N, n)
        return out

    def _unpermuted(self, vec, n):
        """Inverse of `_permuted`: [B, n] (entries beyond n are zero) -> the image, as [B, C * N]."""
        z = _flat(vec)
        B = z.shape[0]
        planes = torch.empty(B, self.channels, self.N, dtype=torch.float32, device=z.device)
        ops.call("ddnm_wh_scatter_f32", _p(z), _p(self.perm), _p(planes), B, self.channels, self.N, n)
        return self._fwht(planes).reshape(B, -1)

    def A(self, vec):
        return self._permuted(vec, self.n_keep)

    def A_pinv(self, vec):
        return self._unpermuted(vec, self.n_keep)

    def singulars(self):
        return torch.ones(self.n_keep, device=self.device)

    def Vt(self, vec):                                                     # svd_operators.py:236-237: fwht, permute, (k, c) interleave
        return self._permuted(vec, self.channels * self.N)

    def V(self, vec):                                                      # :231-234
        return self._unpermuted(vec, self.channels * self.N)

    def U(self, vec):                                                      # :239-243
        return _flat(vec).clone()

    Ut = U

    def add_zeros(self, vec):                                              # :248-251
        return _gather(vec, None, self._spectral_dim())

    def Lambda(self, vec, a, sigma_y, sigma_t, eta):                       # svd_operators.py:253-279
        coef = self._fwht(_flat(vec))
        return self._fwht(_mask_lambda(coef, None, self.mask, self.channels, self.N, a, sigma_y, sigma_t, eta))

    def Lambda_noise(self, vec, a, sigma_y, sigma_t, eta, epsilon):        # :281-320 (no forward transform there)
        return self._fwht(_mask_lambda(vec, epsilon, self.mask, self.channels, self.N, a, sigma_y, sigma_t, eta))

    def begin_run(self, y):
        """Called by the reverse loop once per run: A^+ y is constant over the run and is evaluated here.  (It used to
        be cached under the key (y.data_ptr(), y._version): the caching allocator hands a freed block back at the same
        address and raw kernels never bump `_version`, so a NEW measurement could hit the stale entry.)"""
        self._apy = self.A_pinv(y)
        self._apy_key = y

    def ddnm_step(self, xt, et, noise, y, s, x0_out, xt_next):
        # A^+(A x0 - y) = H(W .* H x0) - A^+ y ; A^+ y is constant over the run
        B = xt.shape[0]
        if self._apy_key is not y:        # stepped outside a run (tests drive single steps): identity of the tensor
            self.begin_run(y)
        self._apy = self._apy.reshape(xt.shape)
        ops.step_x0(xt, et, s, out=x0_out)
        proj = torch.empty_like(xt)
        ops.call("ddnm_fwht2d_masked_f32", _p(x0_out), _p(self.mask), self.channels, _p(proj), B * self.channels, self.img_dim,
                 _p(self._buf(B)))
        ops.step_combine(x0_out, proj, self._apy, noise, et, s, out=xt_next)


class CS(A_functions):
    """Block-based compressed sensing, svd_operators.py:101-159: every 32x32 patch of every channel is measured by
    the first `32*32*ratio` rows of Vt_small, the right-singular basis of one Gaussian 1024x1024 matrix (:107-108);
    all singular values are 1 (:110), so A^+ = A^T.  Here: one patch-gather pass + ONE MFMA GEMM over all
    B*C*(D/32)^2 patches per A / A^+ (the reference runs 1024x1024 mat-vecs through torch.matmul broadcasting and
    then re-sorts the coefficient vector, :113-146).  `gauss`: the Gaussian matrix (default: torch.randn from the
    global CPU generator exactly like :107); the SVD runs on the host like every other operator constructor."""

    PATCH = 32

    def __init__(self, channels, img_dim, ratio, device, gauss=None):
        ps = self.PATCH
        if img_dim % ps:
            raise ValueError("img_dim must be a multiple of 32")
        self.channels, self.img_dim, self.device = channels, img_dim, device
        self.y_dim, self.ratio = img_dim // ps, ps
        if gauss is None:
            gauss = torch.randn(ps ** 2, ps ** 2)
        _, _, V = torch.svd(gauss.detach().float().cpu(), some=False)
        self.cs_size = int(ps * ps * ratio)
        self.V_small = V.contiguous().to(device)
        self.M = V[:, :self.cs_size].T.contiguous().to(device)             # [cs, 1024] = Vt_small[:cs]

    def _npatch(self, B):
        return B * self.channels * self.y_dim ** 2

    def measurement_size(self):
        return self.channels * self.y_dim ** 2 * self.cs_size

    def _measure(self, P, T):
        """T [patches, cs] = P [patches, 1024] . M^T: the measured coefficients of every patch, (c, patch, k) order (:143)."""
        ps2, cs = self.ratio ** 2, self.cs_size
        return ops.bgemm(P, self.M, T, P.numel() // ps2, cs, ps2, lda=ps2, ldb=ps2, ldc=cs, transb=True)

    def _expand(self, T, P):
        """P [patches, 1024] = T [patches, cs] . M: back from the measured subspace."""
        ps2, cs = self.ratio ** 2, self.cs_size
        return ops.bgemm(T, self.M, P, P.numel() // ps2, ps2, cs, lda=cs, ldb=ps2, ldc=ps2, transb=False)

    def A(self, vec):
        x = _img(vec, self.channels, self.img_dim)
        B = x.shape[0]
        P = torch.empty(self._npatch(B), self.ratio ** 2, dtype=torch.float32, device=x.device)
        ops.call("ddnm_patchify_f32", _p(x), _p(P), B * self.channels, self.img_dim, self.ratio, 0)
        return self._measure(P, torch.empty(B, self.measurement_size(), dtype=torch.float32, device=x.device))

    def A_pinv(self, vec):
        y = _flat(vec)
        B = y.shape[0]
        P = self._expand(y, torch.empty(self._npatch(B), self.ratio ** 2, dtype=torch.float32, device=y.device))
        x = torch.empty(B, self.channels * self.img_dim ** 2, dtype=torch.float32, device=y.device)
        ops.call("ddnm_patchify_f32", _p(P), _p(x), B * self.channels, self.img_dim, self.ratio, 1)
        return x

    def singulars(self):
        return torch.ones(self.cs_size, device=self.device).repeat(self.channels * self.y_dim ** 2)

    # ---- DDNM+ (sigma_y > 0): the engine hook of `ddnm_plus_diffusion`, like _SpectralPlus.  `Lambda` / `Lambda_noise`
    # keep raising as in the reference.  All singular values are 1, so with M = Vt_small[:cs] (M^T M projects a patch onto
    # its measured subspace) the step of functions/svd_ddnm.py:118-131 collapses per patch without the full V_small
    # (csrc/ddnm_step.hip, ddnm_step_plus_cs_pre_f32 / _post_f32; coefficients: cs_plus_coefficients):
    #   w       = -a lambda x0 + (d1r - d1n) n + (d2r - d2n) eps
    #   x_{t-1} = a x0 + d1n n + d2n eps + a lambda A^+ y + unpatch((w M^T) M)
    # eps enters as V^T eps (here: eps, projected) and n ~ N(0, I) is drawn in the image domain (V is orthogonal).
    def begin_plus_run(self, y):
        """Per-run constants: A^+ y as [B, C, D, D] and the scratch of the two GEMMs (w [patches, 1024], T [patches, cs])."""
        y = _flat(y)
        B, cs = y.shape[0], self.cs_size
        if y.shape[1] != self.channels * self.y_dim ** 2 * cs:
            raise ValueError(f"measurement rows have {y.shape[1]} entries, expected {self.channels} x {self.y_dim ** 2} "
                             f"patches x {cs}")
        npatch = self._npatch(B)
        self._plus_run = (B, self.A_pinv(y).reshape(B, self.channels, self.img_dim, self.img_dim),
                          torch.empty(npatch, self.ratio ** 2, dtype=torch.float32, device=y.device),
                          torch.empty(npatch, cs, dtype=torch.float32, device=y.device))

    def ddnm_plus_step(self, xt, et, noise, s, sigma_y, sigma_t, eta, x0_out, xt_next):
        """One DDNM+ reverse step: x0|t into `x0_out` (uncorrected, as the loop returns and time-travels from it), x_{t-1}
        into `xt_next`.  `et` may be the [:, :3] view of a 6-channel network output (read through its strides).  Four
        launches: pre kernel, T = w M^T, P = T M (into w's buffer), post kernel."""
        aty, w, T = _plus_state(self, xt.shape[0])
        coef = cs_plus_coefficients(s.sqrt_at_next, sigma_y, sigma_t, eta)
        ops.step_plus_cs_pre(xt, et, noise, aty, s, coef, x0_out, xt_next, w, self.ratio)
        ops.step_plus_cs_post(self._expand(self._measure(w, T), w), xt_next, self.ratio)


class PixelMask(A_functions):
    """A = A^+ = z * mask of the simplified path (guided_diffusion/diffusion.py:258-259,263-264)."""

    def __init__(self, channels, img_dim, mask, device):
        self.channels, self.img_dim, self.device = channels, img_dim, device
        self.mask = mask.reshape(-1).float().to(device).contiguous()       # [HW], shared by the channel planes

    def A(self, vec):
        return _mask_mix(_flat(vec), None, self.mask, 1, self.img_dim ** 2, 1.0, 0.0)

    A_pinv = A

    def measurement_size(self):
        return self.channels * self.img_dim ** 2


class Composition(A_functions):
    """A = A_n ... A_2 A_1 and the reference's "pseudo-inverse" A_1^+ A_2^+ ... A_n^+ of the simplified path's
    composed degradations (mask_color_sr / diy, guided_diffusion/diffusion.py:260-290)."""

    def __init__(self, parts):
        self.parts = list(parts)
        self.channels, self.img_dim, self.device = parts[0].channels, parts[0].img_dim, parts[0].device

    def A(self, vec):
        for op in self.parts:
            vec = op.A(vec)
        return vec

    def A_pinv(self, vec):
        for op in reversed(self.parts):
            vec = op.A_pinv(vec)
        return vec

    def measurement_size(self):
        return self.parts[-1].measurement_size()


def mask_color_sr(channels, img_dim, mask, scale, device):
    """`--deg mask_color_sr` / `diy` (diffusion.py:260-290): mask, then grey (color2gray :33-36), then average-pool.
    The reference keeps three identical grey channels; one is kept here (same information, same A^+ A)."""
    return Composition([PixelMask(channels, img_dim, mask, device),
                        Colorization(img_dim, device, weights=(1 / 3, 1 / 3, 1 / 3)),
                        SuperResolution(1, img_dim, int(scale), device)])


MCSR_RATIOS = (1, 2, 4, 8)


class MaskColorSR(A_functions):
    """Old-photo restoration as ONE operator: mask, then grey, then `ratio` x `ratio` average pool -- the A of the
    Composition above -- with its exact pseudo-inverse, for the DDNM and DDNM+ loops.  `mask` is a d x d array of 0 / 1
    (1 = kept) or None (nothing masked: hq_demo's `sr_color`); `weights` are the grey weights, (1/3, 1/3, 1/3) by default.

    The measurement rows have disjoint supports (row j: the kept pixels of site j, an r x r block, in the three planes),
    so A A^T is diagonal, U = I, and with k_j kept pixels in site j
        s_j = sqrt(k_j) |w| / r^2,   q_j[c][p] = w_c m_p / (sqrt(k_j) |w|),   (A^+ y)[c][p] = m_p w_c r^2 y_j / (k_j |w|^2);
    a site with k_j = 0 is null space.  The chained inverse of the simplified path, mask . colour . upsample, gives
    A A^+ y = (k_j / r^2) y on a site the mask cuts, so its "consistent" solution is not consistent around a scratch.
    The kernels count k_j from the mask themselves (`*_mcsr_*`, csrc/ddnm_step.hip); `singulars()` is the s_j, one per
    site.  `Lambda`, `Lambda_noise`, `V`, `Vt`, `U`, `Ut` stay NotImplementedError as for `SRConv`: they would need a
    null-space basis and a spectral ordering of one's own invention; DDNM+ runs through the hook `ddnm_plus_step`, one launch
    with the per-site coefficients evaluated in the kernel (singular values differ inside one launch)."""

    def __init__(self, channels, img_dim, mask, ratio, device, weights=None):
        if channels != 3:
            raise ValueError(f"MaskColorSR turns RGB images grey: channels must be 3, got {channels}")
        if ratio not in MCSR_RATIOS:
            raise ValueError(f"MaskColorSR kernels pool by {', '.join(str(r) for r in MCSR_RATIOS)}: got ratio {ratio!r}")
        if img_dim % ratio:
            raise ValueError(f"img_dim must be a multiple of the pool ratio: {img_dim} % {ratio} != 0")
        if img_dim % 4:
            raise ValueError(f"MaskColorSR kernels handle four pixels of a row at once: img_dim must be a multiple of 4, got {img_dim}")
        w = (1 / 3, 1 / 3, 1 / 3) if weights is None else tuple(float(v) for v in weights)
        if len(w) != 3 or not any(np.float32(v) != 0 for v in w):
            raise ValueError(f"MaskColorSR needs three grey weights that are not all zero, got {w}")
        self.channels, self.img_dim, self.ratio, self.device = channels, img_dim, int(ratio), device
        self.weights = w
        self._w = (ctypes.c_float * 3)(*w)
        if mask is None:
            self.mask, m = None, np.ones((img_dim, img_dim), np.float32)
        else:
            m = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
            if m.shape != (img_dim, img_dim):
                raise ValueError(f"the mask of a {img_dim} x {img_dim} image is a 2-D array of that shape, got {m.shape}")
            if not np.isin(m, (0, 1)).all():
                raise ValueError("mask values are 0 (missing) and 1 (kept)")
            m = np.ascontiguousarray(m, dtype=np.float32)
            self.mask = torch.from_numpy(m).reshape(-1).to(device).contiguous()                # [HW], shared by the images
        r, n = self.ratio, img_dim // self.ratio
        self.kept = m.reshape(n, r, n, r).sum(axis=(1, 3)).reshape(-1).astype(np.int64)       # k_j per site, row-major
        wn = float(np.sqrt(np.sum(np.asarray(self._w[:], dtype=np.float64) ** 2)))
        self._singulars = torch.from_numpy((np.sqrt(self.kept) * wn / r ** 2).astype(np.float32)).to(device)

    def measurement_size(self):
        return (self.img_dim // self.ratio) ** 2

    def measurement_image_shape(self):
        return (1, self.img_dim // self.ratio, self.img_dim // self.ratio)

    def singulars(self):
        return self._singulars

    def _geometry(self):
        return self.img_dim, self.img_dim, self.ratio, self._w

    def A(self, vec):
        x = _img(vec, 3, self.img_dim)
        B = x.shape[0]
        y = torch.empty(B, self.measurement_size(), dtype=torch.float32, device=x.device)
        ops.call("ddnm_op_mcsr_A_f32", _p(x), _p(self.mask), _p(y), B, *self._geometry())
        return y

    def A_pinv(self, vec):
        y = _flat(vec)
        B = y.shape[0]
        if y.shape[1] != self.measurement_size():
            raise ValueError(f"measurement rows have {y.shape[1]} entries, this operator has {self.measurement_size()}")
        x = torch.empty(B, 3 * self.img_dim ** 2, dtype=torch.float32, device=y.device)
        ops.call("ddnm_op_mcsr_pinv_f32", _p(y), _p(self.mask), _p(x), B, *self._geometry())
        return x

    def _check_y(self, y, B):
        if y.shape[0] != B or y.numel() != B * self.measurement_size():
            raise ValueError(f"y must be [{B}, {self.measurement_size()}], got {tuple(y.shape)}")
        return ops._f32c(y, "y")

    def ddnm_step(self, xt, et, noise, y, s, x0_out, xt_next):
        """x0_out (may be None) and xt_next must not alias xt or et: the kernel passes over a strip twice."""
        B = xt.shape[0]
        ops.step_call("ddnm_step_mcsr_f32", xt, et, noise, self._check_y(y, B), _p(self.mask), _p(x0_out), _p(xt_next), B,
                      *self._geometry(), s)

    # ---- DDNM+ (sigma_y > 0): the engine hook of `ddnm_plus_diffusion`
    def begin_plus_run(self, y):
        y = _flat(y)
        self._plus_run = (y.shape[0], self._check_y(y, y.shape[0]))

    def ddnm_plus_step(self, xt, et, noise, s, sigma_y, sigma_t, eta, x0_out, xt_next):
        """One DDNM+ reverse step in one launch: x0|t into `x0_out` (uncorrected), x_{t-1} into `xt_next`, neither of them
        xt or et; `et` may be the [:, :3] view of a 6-channel network output."""
        B, d = xt.shape[0], self.img_dim
        y, = _plus_state(self, B)
        for name, t in (("xt", xt), ("x0_out", x0_out), ("xt_next", xt_next)):
            if ops._f32c(t, name).numel() != 3 * B * d * d:
                raise ValueError(f"ddnm_plus_step: {name} has {t.numel()} entries, expected {3 * B * d * d}")
        ops.step_call("ddnm_step_plus_mcsr_f32", xt, et, noise, y, _p(self.mask), _p(x0_out), _p(xt_next), B,
                      *self._geometry(), float(sigma_y), float(sigma_t), float(eta), s)


BT601 = ((0.299, 0.587, 0.114), (-0.168736, -0.331264, 0.5), (0.5, -0.418688, -0.081312))      # full range, rows w_Y, w_Cb, w_Cr
CHROMA_SITES = ((2, 1), (4, 1), (2, 2), (4, 4), (8, 8))                                         # (rw, rh): columns x rows
CHROMA_NAMES = {"chroma_420": (2, 2), "chroma_422": (2, 1), "chroma_411": (4, 1)}
CHROMA_SQUARE = (2, 4, 8)


class ChromaSubsample(A_functions):
    """Chroma subsampling as JPEG and the video codecs store it: luma Y = w_Y . x at every pixel, the chroma planes
    Cb = w_Cb . x and Cr = w_Cr . x averaged over sites of `rw` columns x `rh` rows (n = rw rh).  `matrix` is an invertible
    3 x 3 colour matrix with rows w_Y, w_Cb, w_Cr (no offsets: the data are centred), full-range BT.601 by default.  A
    measurement row is [ Y | Cb | Cr ], each plane row-major: d^2 + 2 d^2 / n entries.

    Per site, with mu(v) the mean colour: the n - 1 zero-mean patterns are seen through w^ = w_Y / |w_Y| alone (singular
    value |w_Y|; the two colour directions orthogonal to w^ are null space) and the mean through the 3 x 3 matrix
    D = diag(1, 1/sqrt n, 1/sqrt n) M = U_D S_D V_D^T.  So there are four singular values, the same at every site, A has
    full row rank, and with Ybar the site mean of Y and w+ = w_Y / |w_Y|^2
        (A^+ y)[:, p] = w+ (Y_p - Ybar) + M^-1 (Ybar, Cb, Cr)^T.
    The entry points (`*_chroma_*`, csrc/ddnm_step.hip) derive all of this from the nine matrix entries on the host
    (`ddnm_chroma_constants`).  `Lambda`, `Lambda_noise`, `V`, `Vt`, `U`, `Ut` stay NotImplementedError as for `MaskColorSR`;
    DDNM+ runs through the hook `ddnm_plus_step`, one launch with the four coefficient triples evaluated per launch."""

    def __init__(self, channels, img_dim, rw, rh, device, matrix=None):
        if channels != 3:
            raise ValueError(f"ChromaSubsample splits RGB images into luma and chroma: channels must be 3, got {channels}")
        if (rw, rh) not in CHROMA_SITES:
            raise ValueError(f"ChromaSubsample kernels have the sites (rw, rh) {', '.join(str(v) for v in CHROMA_SITES)}: "
                             f"got {(rw, rh)!r}")
        if img_dim % rw or img_dim % rh:
            raise ValueError(f"img_dim must be a multiple of the site: {img_dim} % {rw} or {img_dim} % {rh} != 0")
        if img_dim % 4:
            raise ValueError(f"ChromaSubsample kernels handle four pixels of a row at once: img_dim must be a multiple of 4, got {img_dim}")
        m = np.asarray(BT601 if matrix is None else matrix, dtype=np.float32)
        if m.shape != (3, 3):
            raise ValueError(f"the colour matrix is 3 x 3 (rows w_Y, w_Cb, w_Cr), got shape {m.shape}")
        m64 = m.astype(np.float64)                                  # what the entry points see: fp32 entries, algebra in double
        if not np.isfinite(m64).all() or not abs(np.linalg.det(m64)) >= 1e-6 * np.linalg.norm(m64) ** 3 or not m64.any():
            raise ValueError(f"the colour matrix must be invertible (|det| >= 1e-6 |M|_F^3), got det {np.linalg.det(m64):.3e}")
        self.channels, self.img_dim, self.rw, self.rh, self.device = channels, img_dim, int(rw), int(rh), device
        self.matrix = m64
        self._m = (ctypes.c_float * 9)(*[float(v) for v in m.reshape(-1)])
        n, sites = self.rw * self.rh, img_dim ** 2 // (self.rw * self.rh)
        self.wn = float(np.sqrt((m64[0] ** 2).sum()))
        self.dc_singulars = np.linalg.svd(np.diag([1.0, n ** -0.5, n ** -0.5]) @ m64, compute_uv=False)
        spectrum = np.concatenate([np.full(sites * (n - 1), self.wn)] + [np.full(sites, v) for v in self.dc_singulars])
        self._singulars = torch.from_numpy(np.sort(spectrum)[::-1].astype(np.float32)).to(device)

    def measurement_size(self):
        return self.img_dim ** 2 + 2 * (self.img_dim ** 2 // (self.rw * self.rh))

    def measurement_image_shape(self):
        return None                                                  # three planes of two sizes: measurements are .npy rows

    def singulars(self):
        return self._singulars

    def _geometry(self):
        return self.img_dim, self.img_dim, self.rw, self.rh, self._m

    def A(self, vec):
        x = _img(vec, 3, self.img_dim)
        B = x.shape[0]
        y = torch.empty(B, self.measurement_size(), dtype=torch.float32, device=x.device)
        ops.call("ddnm_op_chroma_A_f32", _p(x), _p(y), B, *self._geometry())
        return y

    def A_pinv(self, vec):
        y = _flat(vec)
        B = y.shape[0]
        if y.shape[1] != self.measurement_size():
            raise ValueError(f"measurement rows have {y.shape[1]} entries, this operator has {self.measurement_size()}")
        x = torch.empty(B, 3 * self.img_dim ** 2, dtype=torch.float32, device=y.device)
        ops.call("ddnm_op_chroma_pinv_f32", _p(y), _p(x), B, *self._geometry())
        return x

    def _check_y(self, y, B):
        if y.shape[0] != B or y.numel() != B * self.measurement_size():
            raise ValueError(f"y must be [{B}, {self.measurement_size()}], got {tuple(y.shape)}")
        return ops._f32c(y, "y")

    def ddnm_step(self, xt, et, noise, y, s, x0_out, xt_next):
        """x0_out (may be None) and xt_next must not alias xt or et: the kernel passes over a strip twice."""
        B = xt.shape[0]
        ops.step_call("ddnm_step_chroma_f32", xt, et, noise, self._check_y(y, B), _p(x0_out), _p(xt_next), B,
                      *self._geometry(), s)

    # ---- DDNM+ (sigma_y > 0): the engine hook of `ddnm_plus_diffusion`
    def begin_plus_run(self, y):
        y = _flat(y)
        self._plus_run = (y.shape[0], self._check_y(y, y.shape[0]))

    def ddnm_plus_step(self, xt, et, noise, s, sigma_y, sigma_t, eta, x0_out, xt_next):
        """One DDNM+ reverse step in one launch: x0|t into `x0_out` (uncorrected), x_{t-1} into `xt_next`, neither of them
        xt or et; `et` may be the [:, :3] view of a 6-channel network output."""
        B, d = xt.shape[0], self.img_dim
        y, = _plus_state(self, B)
        for name, t in (("xt", xt), ("x0_out", x0_out), ("xt_next", xt_next)):
            if ops._f32c(t, name).numel() != 3 * B * d * d:
                raise ValueError(f"ddnm_plus_step: {name} has {t.numel()} entries, expected {3 * B * d * d}")
        ops.step_call("ddnm_step_plus_chroma_f32", xt, et, noise, y, _p(x0_out), _p(xt_next), B, *self._geometry(),
                      float(sigma_y), float(sigma_t), float(eta), s)


JPEG_SITES = ((1, 1), (2, 1), (2, 2))                                                           # (rw, rh): 4:4:4, 4:2:2, 4:2:0
JPEG_NAMES = {"jpeg_444": (1, 1), "jpeg_422": (2, 1), "jpeg_420": (2, 2)}
JPEG_DC_SHIFT = -4.0 / 127.5            # an encoder subtracts 128 from 8-bit samples: the luma DC offset on the [-1, 1] scale


def jpeg_quality_tables(quality, dc_shift=True):
    """(q [128] float32 in x units, delta) of libjpeg's tables for `quality` 1..100 (`ddnm_jpeg_quality_tables`, host only):
    luma [64] then chroma [64] in natural order, the 8-bit entry / 127.5."""
    q, delta = (ctypes.c_float * 128)(), ctypes.c_float()
    if int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f"a JPEG quality is an integer in 1..100, got {quality!r}")
    _lib.check(_lib.lib().ddnm_jpeg_quality_tables(int(quality), int(bool(dc_shift)), q, ctypes.byref(delta)),
              "ddnm_jpeg_quality_tables")
    return np.array(q[:], dtype=np.float32), float(delta.value)


class JPEG(A_functions):
    """A baseline JPEG file as a measurement: the 8 x 8 block-DCT coefficients of the planes of `ChromaSubsample`
    (site (rw, rh) = (1,1) 4:4:4, (2,1) 4:2:2, (2,2) 4:2:0), each rounded to a multiple of its quantisation step.

    `A_linear` = T: the planes Y | Cb | Cr, then per plane and 8 x 8 block the orthonormal DCT-II; coefficient (u, v) of
    block (I, J) sits at plane position (8 I + u, 8 J + v), so a row has d^2 (1 + 2 / (rw rh)) entries like the chroma
    operator's.  T has full row rank and `A_pinv` = T^+ = A_chroma^+ . IDCT is its exact pseudo-inverse.  `A` is the
    encoder, y = q rint((T x - delta) / q) + delta (the dequantised cell centre; `levels(y)` are the integers), with the
    steps q of libjpeg's tables for `quality` 1..100 -- or of `qtables`, a [2, 8, 8] integer array (luma, chroma; natural
    order) that overrides it -- in x units (entry / 127.5), and delta = -4 / 127.5 on the luma DC only (`dc_shift`).
    `A_pinv(y)` is what a JPEG decoder shows before clipping.

    The measurement says which CELL a coefficient lay in, so `ddnm_step` pulls T x0 back into the cell, not onto its
    centre:  x0h = x0 - lambda T^+(c - clamp(c, y - h, y + h)),  c = T x0,  h = box q / 2  (one launch, csrc/jpeg.hip).
    `box` = 0 is the plain DDNM step against the centres; with `box` = 0.98 the restoration re-encodes to the measured
    levels (clamped coefficients land on the cell edge; the 2 % margin keeps fp32 rounding out of the re-quantisation).
    Quantisation error is bounded, not Gaussian: there is no `ddnm_plus_step`, and `Lambda` and friends stay
    NotImplementedError.  `singulars()` is the chroma spectrum, which the orthogonal DCT does not change."""

    def __init__(self, channels, img_dim, quality, rw, rh, device, matrix=None, qtables=None, dc_shift=True, box=0.98):
        if channels != 3:
            raise ValueError(f"JPEG splits RGB images into luma and chroma: channels must be 3, got {channels}")
        if (rw, rh) not in JPEG_SITES:
            raise ValueError(f"JPEG kernels have the sites (rw, rh) {', '.join(str(v) for v in JPEG_SITES)}: got {(rw, rh)!r}")
        if img_dim % (8 * rw) or img_dim % (8 * rh):
            raise ValueError(f"img_dim must be a multiple of the MCU ({8 * rw} x {8 * rh} pixels), got {img_dim}")
        if not 0.0 <= float(box) <= 1.0:
            raise ValueError(f"box is the share of the quantisation cell the step projects onto, in [0, 1]: got {box!r}")
        self._chroma = ChromaSubsample(channels, img_dim, 2, 2, "cpu", matrix)     # the matrix checks; the site is set below
        self.channels, self.img_dim, self.rw, self.rh, self.device = channels, img_dim, int(rw), int(rh), device
        self.matrix, self._m = self._chroma.matrix, self._chroma._m
        self.box, self.dc_shift = float(box), bool(dc_shift)
        if qtables is None:
            q, self.delta = jpeg_quality_tables(quality, dc_shift)
            self.quality = int(quality)
        else:
            t = np.asarray(qtables)
            if t.shape != (2, 8, 8) or not np.issubdtype(t.dtype, np.integer) or t.min() < 1 or t.max() > 65535:
                raise ValueError("qtables is a [2, 8, 8] integer array (luma, chroma) of quantisation steps >= 1, got "
                                 f"shape {t.shape}, dtype {t.dtype}")
            q = (t.reshape(128).astype(np.float64) / 127.5).astype(np.float32)
            self.delta = float(np.float32(JPEG_DC_SHIFT)) if dc_shift else 0.0
            self.quality = None
        self.q = q
        self._q = (ctypes.c_float * 128)(*[float(v) for v in q])
        d, n = img_dim, self.rw * self.rh
        # q and delta of every entry of a measurement row (for `levels`): the block tables tiled over the planes
        luma = np.tile(q[:64].reshape(8, 8), (d // 8, d // 8)).reshape(-1)
        chroma = np.tile(q[64:].reshape(8, 8), (d // self.rh // 8, d // self.rw // 8)).reshape(-1)
        dl = np.zeros((d, d))
        dl[::8, ::8] = self.delta
        self._q_row = torch.from_numpy(np.concatenate([luma, chroma, chroma]).astype(np.float64)).to(device)
        self._delta_row = torch.from_numpy(np.concatenate([dl.reshape(-1), np.zeros(2 * d * d // n)])).to(device)
        sites = d * d // n
        if n == 1:                       # every pixel its own site: the three singular values of M
            spectrum = np.concatenate([np.full(sites, v) for v in np.linalg.svd(self.matrix, compute_uv=False)])
        else:
            wn = float(np.sqrt((self.matrix[0] ** 2).sum()))
            dc = np.linalg.svd(np.diag([1.0, n ** -0.5, n ** -0.5]) @ self.matrix, compute_uv=False)
            spectrum = np.concatenate([np.full(sites * (n - 1), wn)] + [np.full(sites, v) for v in dc])
        self._singulars = torch.from_numpy(np.sort(spectrum)[::-1].astype(np.float32)).to(device)

    def mcus_per_workgroup(self):
        """The launch geometry of the `*_jpeg_*` kernels: a workgroup of 256 threads owns 16 / rw consecutive MCUs."""
        return 16 // self.rw

    def workgroups(self, B):
        mcus = B * (self.img_dim // (8 * self.rw)) * (self.img_dim // (8 * self.rh))
        return -(-mcus // self.mcus_per_workgroup())

    def measurement_size(self):
        return self.img_dim ** 2 + 2 * (self.img_dim ** 2 // (self.rw * self.rh))

    def measurement_image_shape(self):
        return None                                                  # coefficient planes of two sizes: measurements are .npy rows

    def singulars(self):
        return self._singulars

    def _geometry(self):
        return self.img_dim, self.img_dim, self.rw, self.rh, self._m

    def _rows_of(self, name, vec, *tail):
        x = _img(vec, 3, self.img_dim)
        B = x.shape[0]
        y = torch.empty(B, self.measurement_size(), dtype=torch.float32, device=x.device)
        ops.call(name, _p(x), _p(y), B, *self._geometry(), *tail)
        return y

    def A(self, vec):
        """The encoder: the dequantised cell centres of T x."""
        return self._rows_of("ddnm_op_jpeg_A_f32", vec, self._q, self.delta)

    def A_linear(self, vec):
        """T x, unquantised."""
        return self._rows_of("ddnm_op_jpeg_T_f32", vec)

    def A_pinv(self, vec):
        y = _flat(vec)
        B = y.shape[0]
        if y.shape[1] != self.measurement_size():
            raise ValueError(f"measurement rows have {y.shape[1]} entries, this operator has {self.measurement_size()}")
        x = torch.empty(B, 3 * self.img_dim ** 2, dtype=torch.float32, device=y.device)
        ops.call("ddnm_op_jpeg_pinv_f32", _p(y), _p(x), B, *self._geometry())
        return x

    def levels(self, y):
        """The integer quantisation levels rint((y - delta) / q) of measurement rows (int64; not on the sampler's path)."""
        y = _flat(y)
        if y.shape[1] != self.measurement_size():
            raise ValueError(f"measurement rows have {y.shape[1]} entries, this operator has {self.measurement_size()}")
        return torch.round((y.double() - self._delta_row.to(y.device)) / self._q_row.to(y.device)).long()

    def _check_y(self, y, B):
        if y.shape[0] != B or y.numel() != B * self.measurement_size():
            raise ValueError(f"y must be [{B}, {self.measurement_size()}], got {tuple(y.shape)}")
        return ops._f32c(y, "y")

    def ddnm_step(self, xt, et, noise, y, s, x0_out, xt_next):
        """One launch, one pass; x0_out (may be None) and xt_next must not be xt or et."""
        B = xt.shape[0]
        ops.step_call("ddnm_step_jpeg_f32", xt, et, noise, self._check_y(y, B), _p(x0_out), _p(xt_next), B,
                      *self._geometry(), self._q, self.box, s)


class GeneralA(A_functions):
    """svd_operators.py:173-208: an explicit dense measurement matrix A [m, d] with a full LAPACK SVD (torch.svd on the
    host, like the reference's constructor; singular values below 1e-3 are zeroed, :184-185).  Used by none of the `--deg`
    choices of guided_diffusion/diffusion.py:451-523 -- a dense operator at 3 x 256 x 256 would be 1.5 TB -- but it is the
    reference's way to plug in ANY small linear degradation, so the drop-in offers it: U / Ut / V / Vt are dense
    products on the MFMA GEMM kernel (ddnm_bgemm_f32), A / A_pinv their compositions (:52-58,68-80), At / A_pinv_eta
    come from the base class.  Like the reference it has no Lambda / Lambda_noise (DDNM+ raises NotImplementedError)."""
    ZERO = 1e-3

    def __init__(self, A):
        A = A.detach().float()
        dev = A.device if A.is_cuda else torch.device("cuda")
        U, S, V = torch.svd(A.cpu(), some=False)
        S = S.clone()
        S[S < self.ZERO] = 0
        self._U, self._V = U.contiguous().to(dev), V.contiguous().to(dev)
        self._Ut, self._Vt = U.t().contiguous().to(dev), V.t().contiguous().to(dev)
        self._singulars = S.to(dev)
        self.device = dev
        self._m, self._d = A.shape
        sinv = torch.where(S > 0, 1.0 / S, torch.zeros_like(S))        # host arithmetic, once
        self._sinv_pad = _pad_scale(sinv.to(dev), self._d)

    def _spectral_dim(self):
        return self._d

    def measurement_size(self):
        return self._m

    @staticmethod
    def _mat_by_vec(M, vec):            # out[b] = M @ vec[b]   (svd_operators.py:174-179)
        v = _flat(vec)
        rows, cols = M.shape
        if v.shape[1] != cols:
            raise ValueError(f"GeneralA: a vector of {v.shape[1]} entries does not fit a {rows} x {cols} factor")
        out = torch.empty(v.shape[0], rows, dtype=torch.float32, device=v.device)
        ops.bgemm(v, M, out, v.shape[0], rows, cols, lda=cols, ldb=cols, ldc=rows, transb=True)
        return out

    def V(self, vec):
        return self._mat_by_vec(self._V, vec)

    def Vt(self, vec):
        return self._mat_by_vec(self._Vt, vec)

    def U(self, vec):
        return self._mat_by_vec(self._U, vec)

    def Ut(self, vec):
        return self._mat_by_vec(self._Ut, vec)

    def singulars(self):
        return self._singulars

    def add_zeros(self, vec):
        return _gather(vec, None, self._d)

    def A(self, vec):                   # U . (S .* (V^T x)[:m])   (:52-58)
        s = self._singulars.contiguous()
        return self.U(_gather(self.Vt(vec), None, s.numel(), scale=s))

    def A_pinv(self, vec):              # V . pad(S^+ .* (U^T y))   (:68-80)
        return self.V(_gather(self.Ut(vec), None, self._d, scale=self._sinv_pad))


class _SpectralPlus:
    """DDNM+ (sigma_y > 0) for operators whose SVD is separable per plane, A X = Ul (g .* (Vl^T X Vr)) Ur^T -- SRConv and
    Deblurring2D.  The reference defines no Lambda / Lambda_noise for them (and neither do these classes: a flattened
    spectral ordering would have to be invented); the whole step of functions/svd_ddnm.py:118-131 collapses in the planes
    x^ = Vl^T X Vr instead (csrc/ddnm_step.hip, ddnm_step_plus_spectral_f32):

      x^_0 = (x^_t - e^ sqrt(1 - abar_t)) / sqrt(abar_t),   z^ = a (x^_0 - mu .* (x^_0 - y^)) + d1 .* n + d2 .* e^,
      X_{t-1} = Vl z^ Vr^T,   y^ = g^+ .* (Ul^T Y Ur)

    with (lambda, d1, d2) = spectral_coefficients(g, ...) per entry of the THRESHOLDED gain table `g` (the values A and
    A_pinv use; g = 0 is null space throughout: mu = 0, (d1, d2) = (sigma_t eta, sigma_t sqrt(1 - eta^2))) and mu = lambda
    where g > 0.  eps enters as V^T eps -- the mathematically meant form, unlike the raw entries the reference's other
    operators feed to V -- and n ~ N(0, I) is drawn directly in the spectral planes (V is orthogonal).
    A subclass provides `_plus_factors()`; `ddnm_plus_diffusion` calls `begin_plus_run(y)` once and `ddnm_plus_step`
    per reverse step."""

    def _plus_factors(self):
        """dict: Vl, Vlt, Vr, Vrt [d, d], Ult, Urt [m, m], m, gains / ginv [Cg][d*d] (Cg = 1 or channels)."""
        raise NotImplementedError()

    def begin_plus_run(self, y):
        """Per-run constants: y^ (the measurement in the spectral planes, zero in the null space) and the scratch planes."""
        f = self._plus_factors()
        C, d, m = self.channels, self.img_dim, f["m"]
        y = _flat(y)
        B = y.shape[0]
        if y.shape[1] != C * m * m:
            raise ValueError(f"measurement rows have {y.shape[1]} entries, expected {C} x {m} x {m}")
        bc = B * C
        t = _left(f["Ult"], y, m, m, bc)
        y_hat = ops.fill_(torch.empty(B, C, d, d, dtype=torch.float32, device=y.device))
        # (Ul^T Y) Ur into the top-left m x m of each zeroed d x d plane (ldc = d), then g^+
        _right(t, f["Urt"], m, m, m, bc, out=y_hat, ldc=d)
        _mul_planes(y_hat, f["ginv"], f["ginv"].shape[0], d * d)
        self._plus_run = (B, y_hat, torch.empty(2, bc, d, d, dtype=torch.float32, device=y.device),
                          torch.empty(2, B, C, d, d, dtype=torch.float32, device=y.device))

    def ddnm_plus_step(self, xt, et, noise, s, sigma_y, sigma_t, eta, x0_out, xt_next):
        """One DDNM+ reverse step: x0|t into `x0_out` (uncorrected, as the loop returns and time-travels from it), x_{t-1}
        into `xt_next`.  `et` may be the [:, :3] view of a 6-channel network output (read through its strides)."""
        B = xt.shape[0]
        y_hat, t1, hat = _plus_state(self, B)
        f = self._plus_factors()
        C, d = self.channels, self.img_dim
        bc = B * C
        ops.step_x0(xt, et, s, out=x0_out)                 # validates et's layout too
        # x^_t = Vl^T X_t Vr and e^ = Vl^T E Vr: left products per tensor, the right product over all 2 B C planes
        _left(f["Vlt"], xt, d, d, bc, out=t1[0])
        _left(f["Vlt"], et, d, d, bc, out=t1[1], images=(C, et.stride(0)))
        _right(t1, f["Vrt"], d, d, d, 2 * bc, out=hat)
        g = f["gains"]
        ops.step_plus_spectral(hat[0], hat[1], y_hat, g, d * d if g.shape[0] > 1 else 0, noise, s, sigma_y, sigma_t, eta,
                               out=hat[0])
        _right(_left(f["Vl"], hat[0], d, d, bc, out=t1[0]), f["Vr"], d, d, d, bc, out=xt_next)


class SRConv(_SpectralPlus, A_functions):
    ZERO = 3e-2     # svd_operators.py:878

    def __init__(self, kernel, channels, img_dim, device, stride=1):
        self.channels, self.img_dim, self.ratio, self.device = channels, img_dim, stride, device
        self.small_dim = small = img_dim // stride
        # 1-D strided blur matrix with reflective padding (svd_operators.py:862-875); host-side setup
        k = kernel.detach().float().cpu()
        A_small = torch.zeros(small, img_dim)
        half = k.shape[0] // 2
        for i in range(stride // 2, img_dim + stride // 2, stride):
            for j in range(i - half, i + half):
                je = j
                if je < 0:
                    je = -je - 1
                if je >= img_dim:
                    je = (img_dim - 1) - (je - img_dim)
                A_small[i // stride, je] += k[j - i + half]
        U, S, V = torch.svd(A_small, some=False)
        S = S.clone()
        S[S < self.ZERO] = 0
        Sp = torch.where(S > 0, 1.0 / S, torch.zeros_like(S))
        self.singulars_small = S.to(device)
        self.Ae = ((U * S[None, :]) @ V[:, :small].T).contiguous().to(device)       # [small, img_dim]
        self.Pe = ((V[:, :small] * Sp[None, :]) @ U.T).contiguous().to(device)      # [img_dim, small]
        self._svd_host = (U.contiguous(), V.contiguous())     # factors of the spectral surface (V / Vt / U / Ut), built lazily

    # ---- matrix-free SVD surface (svd_operators.py:886-931); the sampling path uses the Ae / Pe forms above
    def _spectral(self):
        if not hasattr(self, "_Vs"):
            U, V = self._svd_host
            dev, d, m, C = self.device, self.img_dim, self.small_dim, self.channels
            self._Vs, self._Vts = V.to(dev), V.T.contiguous().to(dev)
            self._Us, self._Uts = U.to(dev), U.T.contiguous().to(dev)
            # P_1 of Appendix D.5 (:881-884): the small x small block first, then the rest of the first `small` rows
            perm = torch.tensor([d * i + j for i in range(m) for j in range(m)] +
                                [d * i + j for i in range(m) for j in range(m, d)], dtype=torch.long)
            src = torch.arange(d * d)
            src[: perm.numel()] = perm                                   # spectral position -> row-major (i, j) entry
            pos, c = torch.meshgrid(torch.arange(d * d), torch.arange(C), indexing="ij")
            vt = (c * d * d + src[pos]).reshape(-1).to(torch.int32)      # [(pos, c)] -> CHW index of V^T X V
            self._t_vt, self._t_v = vt.to(dev), _inverse_perm(vt).to(dev)
            pos, c = torch.meshgrid(torch.arange(m * m), torch.arange(C), indexing="ij")
            ut = (c * m * m + pos).reshape(-1).to(torch.int32)           # [(pos, c)] -> CHW index of the small image
            self._t_ut, self._t_u = ut.to(dev), _inverse_perm(ut).to(dev)
        return self

    def Vt(self, vec):                                                     # :899-907: V^T X V, then P_1 and (pos, c) interleave
        sp, d = self._spectral(), self.img_dim
        t = _two_sided(sp._Vts, _img(vec, self.channels, d), sp._Vts, d, d, d)
        return _gather(t.reshape(vec.shape[0], -1), sp._t_vt, self._spectral_dim())

    def V(self, vec):                                                      # :886-897
        sp, d = self._spectral(), self.img_dim
        t = _gather(vec, sp._t_v, self._spectral_dim())
        return _two_sided(sp._Vs, t, sp._Vs, d, d, d).reshape(vec.shape[0], -1)

    def Ut(self, vec):                                                     # :919-925
        sp, m = self._spectral(), self.small_dim
        y = _flat(vec)
        t = _two_sided(sp._Uts, y, sp._Uts, m, m, m)
        return _gather(t.reshape(y.shape[0], -1), sp._t_ut, self.channels * m * m)

    def U(self, vec):                                                      # :909-917
        sp, m = self._spectral(), self.small_dim
        t = _gather(vec, sp._t_u, self.channels * m * m)
        return _two_sided(sp._Us, t, sp._Us, m, m, m).reshape(vec.shape[0], -1)

    def add_zeros(self, vec):                                              # :930-934
        return _gather(vec, None, self._spectral_dim())

    def _A(self, x, y_sub=None):
        """Y = Ae X Ae^T (- y_sub, fused in the GEMM epilogue) for every (b, c) plane."""
        d, m = self.img_dim, self.small_dim
        return _two_sided(self.Ae, x, self.Ae, m, d, m, D=y_sub, beta=-1.0).reshape(x.shape[0], -1)

    def measurement_size(self):
        return self.channels * self.small_dim ** 2

    def measurement_image_shape(self):
        return (self.channels, self.small_dim, self.small_dim)

    def A(self, vec):
        return self._A(_img(vec, self.channels, self.img_dim))

    def A_pinv(self, vec):
        d, m = self.img_dim, self.small_dim
        return _two_sided(self.Pe, _flat(vec), self.Pe, d, m, d).reshape(vec.shape[0], -1)

    def _plus_factors(self):
        if not hasattr(self, "_plus_f"):
            U, V = self._svd_host
            dev, d, m = self.device, self.img_dim, self.small_dim
            S = self.singulars_small.detach().cpu()
            g = torch.zeros(d, d)
            g[:m, :m] = S[:, None] * S[None, :]                          # thresholded: the values Ae / Pe are built from
            dv = lambda t: t.contiguous().to(dev)                        # noqa: E731
            self._plus_f = dict(Vl=dv(V), Vlt=dv(V.T), Vr=dv(V), Vrt=dv(V.T), Ult=dv(U.T), Urt=dv(U.T), m=m,
                                gains=dv(g.reshape(1, d * d)),
                                ginv=dv(torch.where(g > 0, 1.0 / g, torch.zeros_like(g)).reshape(1, d * d)))
        return self._plus_f

    def singulars(self):
        s = self.singulars_small
        return torch.matmul(s.reshape(-1, 1), s.reshape(1, -1)).reshape(-1).repeat_interleave(3).reshape(-1)

    def ddnm_step(self, xt, et, noise, y, s, x0_out, xt_next):
        B = xt.shape[0]
        ops.step_x0(xt, et, s, out=x0_out)
        resid = self._A(x0_out, y_sub=y.reshape(B, -1))          # A x0 - y fused in the GEMM epilogue
        proj = self.A_pinv(resid).reshape(xt.shape)
        ops.step_combine(x0_out, proj, None, noise, et, s, out=xt_next)


class Deblurring2D(_SpectralPlus, A_functions):
    """Separable blur A = (U1 (x) U2) diag(g) (V1 (x) V2)^T (svd_operators.py:1094-1165), applied as four
    N x N MFMA GEMMs per plane + one gain kernel.  The gain table reproduces the reference's tiling quirk
    (`singulars()` = sorted values repeated 3x against a (position, channel)-interleaved spectral vector):
    entry (k, c) is scaled by s_sorted[(3k + c) mod N^2]; `A_pinv` inverts the same table (:1014-1023)."""

    ZERO = 3e-2

    def __init__(self, kernel1, kernel2, channels, img_dim, device):
        self.channels, self.img_dim, self.device = channels, img_dim, device
        n = img_dim

        def blur_matrix(kernel):
            k = kernel.detach().float().cpu()
            A = torch.zeros(n, n)
            half = k.shape[0] // 2
            for i in range(n):
                for j in range(i - half, i + half):
                    if 0 <= j < n:
                        A[i, j] = k[j - i + half]
            return A
        U1, S1, V1 = torch.svd(blur_matrix(kernel1), some=False)          # host-side setup like the reference ctor
        U2, S2, V2 = torch.svd(blur_matrix(kernel2), some=False)
        # un-thresholded table s1_i * s2_j in spectral-plane order: what `_singulars_orig[_perm]` holds (:959,963)
        self.S_orig = torch.matmul(S1.reshape(n, 1), S2.reshape(1, n)).reshape(n * n).contiguous().to(device)
        S1, S2 = S1.clone(), S2.clone()
        S1[S1 < self.ZERO] = 0
        S2[S2 < self.ZERO] = 0
        big = torch.matmul(S1.reshape(n, 1), S2.reshape(1, n)).reshape(n * n)
        s_sorted, perm = big.sort(descending=True)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(n * n)
        idx = (3 * inv[None, :] + torch.arange(channels)[:, None]) % (n * n)
        G = s_sorted[idx]
        self._singulars = s_sorted.to(device)
        self.G = G.contiguous().to(device)
        self.Ginv = torch.where(G > 0, 1.0 / G, torch.zeros_like(G)).contiguous().to(device)
        dv = lambda m: m.contiguous().to(device)                            # noqa: E731
        self.U1, self.U1t, self.V1, self.V1t = dv(U1), dv(U1.T), dv(V1), dv(V1.T)
        self.U2, self.U2t, self.V2, self.V2t = dv(U2), dv(U2.T), dv(V2), dv(V2.T)

    def _sandwich(self, L, x, Rt_rows, gain, L2, R2_rows):
        """out = L2 . (gain .* (L . X . R)) . R2  for every plane; Rt_rows / R2_rows hold R^T / R2^T row-major
        (= the `[N][K]` operand layout of the GEMM)."""
        n = self.img_dim
        spec = _mul_planes(_two_sided(L, x, Rt_rows, n, n, n), gain, self.channels, n * n)
        return _two_sided(L2, spec, R2_rows, n, n, n).reshape(x.shape[0], -1)

    def measurement_size(self):
        return self.channels * self.img_dim ** 2

    def measurement_image_shape(self):
        return (self.channels, self.img_dim, self.img_dim)

    def A(self, vec):
        x = _img(vec, self.channels, self.img_dim)
        # V1^T X V2 -> gains -> U1 (.) U2^T ;  X . V2 = X . (V2^T)^T, (.) . U2^T uses U2 rows
        return self._sandwich(self.V1t, x, self.V2t, self.G, self.U1, self.U2)

    def A_pinv(self, vec):
        y = _img(vec, self.channels, self.img_dim)
        return self._sandwich(self.U1t, y, self.U2t, self.Ginv, self.V1, self.V2)

    def _plus_factors(self):
        # the per-channel table self.G (thresholded, with the 3x tiling quirk): the values A / A_pinv use
        return dict(Vl=self.V1, Vlt=self.V1t, Vr=self.V2, Vrt=self.V2t, Ult=self.U1t, Urt=self.U2t, m=self.img_dim,
                    gains=self.G, ginv=self.Ginv)

    def singulars(self):
        return self._singulars.repeat(1, 3).reshape(-1)


class Deblurring(Deblurring2D):
    # deblur_uni / deblur_gauss keep the reference's Lambda / Lambda_noise (un-thresholded table, raw eps): no spectral hook
    begin_plus_run = None
    ddnm_plus_step = None

    def __init__(self, kernel, channels, img_dim, device, ZERO=3e-2):
        self.ZERO = ZERO
        super().__init__(kernel, kernel, channels, img_dim, device)

    def _spectral_mix(self, x, y, a, sigma_y, sigma_t, eta, mode):
        out = torch.empty_like(x)
        ops.call("ddnm_spectral_mix_f32", _p(x), _p(y), _p(self.S_orig), self.img_dim ** 2, _p(out), x.numel(), float(a),
                 float(sigma_y), float(sigma_t), float(eta), mode)
        return out

    def Lambda(self, vec, a, sigma_y, sigma_t, eta):                       # svd_operators.py:1016-1040
        """V diag(lambda) V^T vec, lambda from the un-thresholded singular values; the reference's sort and its
        inverse cancel, so the weights are applied directly in the (V1^T X V1) plane."""
        n = self.img_dim
        spec = _two_sided(self.V1t, _img(vec, self.channels, n), self.V1t, n, n, n)
        spec = self._spectral_mix(spec, None, a, sigma_y, sigma_t, eta, 0)
        return _two_sided(self.V1, spec, self.V1, n, n, n).reshape(vec.shape[0], -1)

    def Lambda_noise(self, vec, a, sigma_y, sigma_t, eta, epsilon):        # :1042-1091 (raw entries fed to V)
        n = self.img_dim
        mixed = self._spectral_mix(_flat(vec), _flat(epsilon), a, sigma_y, sigma_t, eta, 1)
        return _two_sided(self.V1, mixed, self.V1, n, n, n).reshape(vec.shape[0], -1)


def gaussian_taps(sigma, radius):
    """diffusion.py:507-520: fp32 exp(-0.5 (x/sigma)^2) for x = -radius..radius."""
    return torch.tensor([float(torch.exp(torch.Tensor([-0.5 * (x / sigma) ** 2]))) for x in range(-radius, radius + 1)])


def missing_indices_of_mask(mask):
    """2-D numpy mask (0 = missing) -> the `missing_indices` of `Inpainting`: the three HWC-interleaved entries of every
    missing pixel (guided_diffusion/diffusion.py:465-470)."""
    r = torch.nonzero(torch.from_numpy(mask).reshape(-1) == 0).long().reshape(-1) * 3
    return torch.cat([r, r + 1, r + 2], dim=0)


DEMOSAIC = "demosaic"


def demosaic_choices():
    return [DEMOSAIC] + [f"{DEMOSAIC}_{name}" for name in CFA_PATTERNS]


def demosaic_pattern(deg, cfa_path="exp/cfa/pattern.npy"):
    """The colour filter array of `--deg demosaic_<name>` (a name of CFA_PATTERNS) or of `--deg demosaic` (the 2-D integer
    array in `cfa_path`); a ValueError that names the valid choices otherwise."""
    valid = f"the demosaicing tasks are {', '.join(demosaic_choices())} ({DEMOSAIC} alone reads {cfa_path})"
    if deg == DEMOSAIC:
        try:
            return cfa_pattern(np.load(cfa_path, allow_pickle=False))
        except (OSError, ValueError) as e:
            raise ValueError(f"--deg {deg}: {cfa_path} does not hold a colour filter array ({e}); {valid}") from e
    name = deg[len(DEMOSAIC) + 1:]
    if not deg.startswith(DEMOSAIC + "_") or name not in CFA_PATTERNS:
        raise ValueError(f"--deg {deg}: unknown colour filter array; {valid}")
    return cfa_pattern(name)


def build_operator(deg, deg_scale, config, device, mask_path="exp/inp_masks/mask.npy", perm=None,
                   cfa_path="exp/cfa/pattern.npy", jpeg_box=None):
    """Operator factory of guided_diffusion/diffusion.py:451-523 for the --deg values on the hot path, and of the
    demosaicing tasks (`demosaic_<cfa name>`, `demosaic`: deg_scale is ignored).  `jpeg_box` (--jpeg_box) is the share of
    the quantisation cell of `--deg jpeg_*`, JPEG_BOX when None."""
    c, d = config.data.channels, config.data.image_size
    if deg.startswith(DEMOSAIC):
        return Mosaic(c, d, demosaic_pattern(deg, cfa_path), device)
    if deg == "cs_walshhadamard":
        compress_by = round(1 / deg_scale)
        if perm is None:
            perm = torch.randperm(d ** 2, device=device)     # global device RNG, diffusion.py:458
        return WalshHadamardCS(c, d, compress_by, perm, device)
    if deg == "inpainting":
        mask = np.load(mask_path)
        if mask.ndim == 3:           # [N, S, S]: one mask per image, image i uses mask i % N
            return InpaintingBank(c, d, mask, device)
        if mask.ndim != 2:
            raise ValueError(f"{mask_path}: a mask file is 2-D (one mask) or 3-D (a bank of masks), got {mask.ndim}-D")
        return Inpainting(c, d, missing_indices_of_mask(mask), device)
    if deg == "denoising":
        return Denoising(c, d, device)
    if deg == "colorization":
        return Colorization(d, device)
    if deg == "sr_averagepooling":
        return SuperResolution(c, d, int(deg_scale), device)
    if deg == "sr_bicubic":
        factor = int(deg_scale)
        return SRConv(bicubic_kernel(factor), c, d, device, stride=factor)
    if deg == "deblur_uni":
        return Deblurring(torch.Tensor([1 / 9] * 9), c, d, device)
    if deg == "deblur_gauss":
        k = gaussian_taps(10, 2)
        return Deblurring(k / k.sum(), c, d, device)
    if deg == "deblur_aniso":
        k2, k1 = gaussian_taps(20, 4), gaussian_taps(1, 4)
        return Deblurring2D(k1 / k1.sum(), k2 / k2.sum(), c, d, device)
    if deg == "cs_blockbased":
        return CS(c, d, deg_scale, device)                   # diffusion.py:459-462
    if deg == "mask_color_sr":                               # old photo: masked, grey, small (deg_scale 1: masked colorization)
        mask = np.load(mask_path)
        if mask.ndim != 2:
            raise ValueError(f"{mask_path}: --deg mask_color_sr takes one 2-D mask, got {mask.ndim}-D (banks of masks, one "
                             "per image, are an inpainting feature)")
        return MaskColorSR(c, d, mask, round(deg_scale), device)
    if deg == "sr_color":                                    # hq_demo's name: grey and small, nothing masked
        return MaskColorSR(c, d, None, round(deg_scale), device)
    if deg in CHROMA_NAMES:                                  # 4:2:0, 4:2:2, 4:1:1; --deg_scale is not read
        return ChromaSubsample(c, d, *CHROMA_NAMES[deg], device)
    if deg == "chroma_sub":                                  # square sites of --deg_scale 2 | 4 | 8
        if deg_scale not in CHROMA_SQUARE:
            raise ValueError(f"--deg chroma_sub takes --deg_scale {' | '.join(str(r) for r in CHROMA_SQUARE)} (square chroma "
                             f"sites), got {deg_scale!r}")
        return ChromaSubsample(c, d, int(deg_scale), int(deg_scale), device)
    if deg in JPEG_NAMES:                                    # 4:4:4, 4:2:2, 4:2:0; --deg_scale is the quality
        return JPEG(c, d, jpeg_quality_of(deg, deg_scale), *JPEG_NAMES[deg], device,
                    box=JPEG_BOX if jpeg_box is None else jpeg_box)
    raise ValueError("degradation type not supported")


JPEG_BOX = 0.98


def jpeg_quality_of(deg, deg_scale):
    """The integer quality of `--deg jpeg_* --deg_scale Q`; a ValueError that names the range otherwise."""
    try:
        ok = deg_scale is not None and float(deg_scale) == int(deg_scale) and 1 <= int(deg_scale) <= 100
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"--deg {deg} takes --deg_scale Q, the JPEG quality, an integer in 1..100: got {deg_scale!r}")
    return int(deg_scale)


def bicubic_kernel(factor):
    """diffusion.py:485-499: cubic (a=-0.5) taps, normalised in float64 then again in fp32."""
    def cubic(x, a=-0.5):
        ax = abs(x)
        if ax <= 1:
            return (a + 2) * ax ** 3 - (a + 3) * ax ** 2 + 1
        if 1 < ax < 2:
            return a * ax ** 3 - 5 * a * ax ** 2 + 8 * a * ax - 4 * a
        return 0
    k = np.zeros(factor * 4)
    for i in range(factor * 4):
        k[i] = cubic((1 / factor) * (i - np.floor(factor * 4 / 2) + 0.5))
    k = torch.from_numpy(k / np.sum(k)).float()
    return k / k.sum()
