"""JPEG-artifact restoration (svd_operators.JPEG, the `*_jpeg_*` entry points of csrc/jpeg.hip) on the host: the dense
float64 model that the GPU tests compare against (tests/test_gpu_jpeg.py imports it from here) checked against itself,
`ddnm_jpeg_quality_tables` against libjpeg's formula and against the tables Pillow writes, the `--deg jpeg_*` names and the
flags of the runner, and the argument validation of the entry points through the built library.  No GPU.

    T = blockdiag(D, D_c, D_c) A_chroma,  D the in-place 8 x 8 block DCT-II of a plane (orthonormal),  T^+ = pinv(T)
    encoder:  levels = rint((T x - delta) / q),  y = q levels + delta
    step:     x0h = x0 - lam T^+(c - clamp(c, y - h, y + h)),  c = T x0,  h = box q / 2
"""
import argparse
import ctypes
import io
import os

import numpy as np
import pytest
import torch

from tests.test_chroma_host import BT601, dense_matrix, kernel_matrix

ETA = 0.85
SITES = [(1, 1), (2, 1), (2, 2)]                       # (rw, rh): 4:4:4, 4:2:2, 4:2:0
QUALITIES = (1, 10, 49, 50, 51, 90, 100)
LUMA_ROW0, CHROMA_ROW0 = [16, 11, 10, 16, 24, 40, 51, 61], [17, 18, 24, 47, 99, 99, 99, 99]
DELTA = -4.0 / 127.5
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
          28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
          47, 55, 62, 63]


# ---------------------------------------------------------------------------------------------- the tables
def pillow_tables(quality):
    """The two 8-bit tables Pillow writes into a file saved at `quality`, as it reports them (lists of 64)."""
    from PIL import Image
    rng = np.random.default_rng(1)
    buf = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)).save(buf, "JPEG", quality=quality)
    buf.seek(0)
    q = Image.open(buf).quantization
    return [int(v) for v in q[0]], [int(v) for v in q[1]]


def base_tables():
    """The Annex K tables in natural order, from Pillow at quality 50 (scale 100 %); a Pillow that reports zig-zag order is
    put back.  [2, 64] int."""
    out = []
    for tab, row0 in zip(pillow_tables(50), (LUMA_ROW0, CHROMA_ROW0)):
        if tab[:8] != row0:
            nat = [0] * 64
            for k, pos in enumerate(ZIGZAG):
                nat[pos] = tab[k]
            tab = nat
        assert tab[:8] == row0
        out.append(tab)
    return np.array(out, dtype=np.int64)


def formula_tables(quality, base):
    """libjpeg: scale = 5000 // Q below 50, else 200 - 2 Q; entry = clamp((base scale + 50) // 100, 1, 255).  [2, 64] int."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * scale + 50) // 100, 1, 255)


def steps_of(quality):
    """(q [128] float64 holding the fp32 values the entry points get, delta likewise) of `quality`, from the formula."""
    q8 = formula_tables(quality, base_tables()).reshape(128)
    return (q8 / 127.5).astype(np.float32).astype(np.float64), float(np.float32(DELTA))


# ---------------------------------------------------------------------------------------------- the dense model
def dct_matrix():
    """C[k][n] = s_k cos((2n + 1) k pi / 16), s_0 = sqrt(1/8), s_k = sqrt(2/8)."""
    C = np.zeros((8, 8))
    for k in range(8):
        for n in range(8):
            C[k, n] = (np.sqrt(1 / 8) if k == 0 else np.sqrt(2 / 8)) * np.cos((2 * n + 1) * k * np.pi / 16)
    return C


def block_dct_matrix(rows, cols):
    """[rows cols, rows cols]: a row-major plane -> its 8 x 8 block DCTs in place, entry by entry."""
    C = dct_matrix()
    D = np.zeros((rows * cols, rows * cols))
    for I in range(rows // 8):
        for J in range(cols // 8):
            for u in range(8):
                for v in range(8):
                    for i in range(8):
                        D[(8 * I + u) * cols + 8 * J + v, (8 * I + i) * cols + 8 * J:(8 * I + i) * cols + 8 * J + 8] = C[u, i] * C[v]
    return D


def dense_T(rw, rh, M, H, W):
    """T [H W + 2 H W / n, 3 H W] of an H x W image: the chroma dense matrix, then the block DCT of each plane."""
    A = dense_matrix(rw, rh, M, H, W)
    hw, hwn = H * W, H * W // (rw * rh)
    T = np.empty_like(A)
    T[:hw] = block_dct_matrix(H, W) @ A[:hw]
    Dc = block_dct_matrix(H // rh, W // rw)
    T[hw:hw + hwn], T[hw + hwn:] = Dc @ A[hw:hw + hwn], Dc @ A[hw + hwn:]
    return T


def step_rows(q, delta, rw, rh, H, W):
    """(q, delta) of every entry of a measurement row [H W + 2 H W / n]: the block tables tiled over the planes."""
    luma = np.tile(q[:64].reshape(8, 8), (H // 8, W // 8)).reshape(-1)
    chroma = np.tile(q[64:].reshape(8, 8), (H // rh // 8, W // rw // 8)).reshape(-1)
    dl = np.zeros((H, W))
    dl[::8, ::8] = delta
    return np.concatenate([luma, chroma, chroma]), np.concatenate([dl.reshape(-1), np.zeros(2 * H * W // (rw * rh))])


class JpegModel:
    """float64 model of JPEG(3, ., quality, rw, rh, matrix=M) on H x W images.  `whole`: T of the image, entry by entry, and
    T^+ = numpy.linalg.pinv(T).  Otherwise the same per MCU (8 rh x 8 rw pixels): T is block diagonal over the MCUs, so the
    MCU's T [64 n + 128, 192 n] is built entry by entry (the same `dense_T`) and applied to every MCU;
    `test_mcu_model_is_the_whole_model` holds the two forms together.  Arrays are [B, 3 H W] / [B, H W + 2 H W / n]."""

    def __init__(self, rw, rh, M, H, W, q, delta, whole=False):
        self.rw, self.rh, self.H, self.W, self.n, self.whole = rw, rh, H, W, rw * rh, whole
        self.T = dense_T(rw, rh, M, H, W) if whole else dense_T(rw, rh, M, 8 * rh, 8 * rw)
        self.pinv = np.linalg.pinv(self.T)
        self.q_row, self.delta_row = step_rows(np.asarray(q, dtype=np.float64), float(delta), rw, rh, H, W)

    # ---- image order <-> MCU order
    def _x_in(self, x):
        if self.whole:
            return x
        H, W, rw, rh = self.H, self.W, self.rw, self.rh
        v = x.reshape(-1, 3, H // (8 * rh), 8 * rh, W // (8 * rw), 8 * rw).transpose(0, 2, 4, 1, 3, 5)
        return v.reshape(-1, 192 * self.n)

    def _x_out(self, v):
        if self.whole:
            return v
        H, W, rw, rh = self.H, self.W, self.rw, self.rh
        x = v.reshape(-1, H // (8 * rh), W // (8 * rw), 3, 8 * rh, 8 * rw).transpose(0, 3, 1, 4, 2, 5)
        return x.reshape(-1, 3 * H * W)

    def _y_in(self, y):
        if self.whole:
            return y
        H, W, rw, rh = self.H, self.W, self.rw, self.rh
        mh, mw, hw, hwn = H // (8 * rh), W // (8 * rw), H * W, H * W // self.n
        Y = y[:, :hw].reshape(-1, mh, 8 * rh, mw, 8 * rw).transpose(0, 1, 3, 2, 4).reshape(-1, 64 * self.n)
        C = [y[:, hw + k * hwn:hw + (k + 1) * hwn].reshape(-1, mh, 8, mw, 8).transpose(0, 1, 3, 2, 4).reshape(-1, 64)
             for k in range(2)]
        return np.concatenate([Y] + C, axis=1)

    def _y_out(self, v):
        if self.whole:
            return v
        H, W, rw, rh, n = self.H, self.W, self.rw, self.rh, self.n
        mh, mw = H // (8 * rh), W // (8 * rw)
        Y = v[:, :64 * n].reshape(-1, mh, mw, 8 * rh, 8 * rw).transpose(0, 1, 3, 2, 4).reshape(-1, H * W)
        C = [v[:, 64 * n + 64 * k:64 * n + 64 * (k + 1)].reshape(-1, mh, mw, 8, 8).transpose(0, 1, 3, 2, 4).reshape(-1, H * W // n)
             for k in range(2)]
        return np.concatenate([Y] + C, axis=1)

    # ---- numpy float64
    def apply_T(self, x):
        return self._y_out(self._x_in(x) @ self.T.T)

    def apply_pinv(self, y):
        return self._x_out(self._y_in(y) @ self.pinv.T)

    def scaled(self, x):
        """(T x - delta) / q: the encoder rounds this to the levels."""
        return (self.apply_T(x) - self.delta_row) / self.q_row

    def levels(self, x):
        return np.rint(self.scaled(x))

    def encode(self, x):
        return self.q_row * self.levels(x) + self.delta_row

    def project(self, c, y, box):
        """c - clamp(c, y - h, y + h), h = box q / 2, and the share of clamped coefficients"""
        h = box * self.q_row / 2
        r = c - np.clip(c, y - h, y + h)
        return r, float((r != 0).mean())

    def step(self, xt, et, n, y, abar_t, abar_next, eta, lam, box):
        """(x0|t, x_{t-1}, clamped share) of one reverse step."""
        a, sigma_t = abar_next ** 0.5, (1 - abar_next) ** 0.5
        x0 = (xt - et * (1 - abar_t) ** 0.5) / abar_t ** 0.5
        r, share = self.project(self.apply_T(x0), y, box)
        x0h = x0 - lam * self.apply_pinv(r)
        return x0, a * x0h + sigma_t * eta * n + sigma_t * (1 - eta ** 2) ** 0.5 * et, share


class CellOperator:
    """The model wrapped for the unchanged oracle.sampler.ddnm_diffusion: A(x) = T x - clamp(T x, y - h, y + h) + y and
    A_pinv = T^+, so that its x0 - A_pinv(A(x0) - y) is exactly the projection.  Torch in, torch out, the argument's dtype."""

    def __init__(self, model, y, box):
        self.m, self.y, self.box = model, np.asarray(y, dtype=np.float64), box

    @staticmethod
    def _np(v):
        return v.detach().double().cpu().reshape(v.shape[0], -1).numpy()

    def A(self, x):
        r, _ = self.m.project(self.m.apply_T(self._np(x)), self.y, self.box)
        return torch.from_numpy(np.ascontiguousarray(r + self.y)).to(x.dtype)

    def A_pinv(self, y):
        return torch.from_numpy(np.ascontiguousarray(self.m.apply_pinv(self._np(y)))).to(y.dtype)


# ---- the closed forms (what the kernels evaluate); `dtype` float32 gives the fp32 figure a GPU bar may be derived from
def _block_transform(p, C):
    """[B, h, w] -> C X C^T of every 8 x 8 block, in place, in the dtype of p"""
    B, h, w = p.shape
    t = p.reshape(B, h // 8, 8, w // 8, 8)
    return np.einsum("ui,bIiJj,vj->bIuJv", C, t, C).astype(p.dtype).reshape(B, h, w)


def _planes(y, rw, rh, d):
    hw, hwn = d * d, d * d // (rw * rh)
    return (y[:, :hw].reshape(-1, d, d), y[:, hw:hw + hwn].reshape(-1, d // rh, d // rw),
            y[:, hw + hwn:].reshape(-1, d // rh, d // rw))


def closed_T(rw, rh, M, d, x, dtype=np.float64):
    """[B, 3 d^2] -> [B, d^2 + 2 d^2 / n]: the chroma planes (closed_A), then the DCT of every block"""
    from tests.test_chroma_host import closed_A
    C = dct_matrix().astype(dtype)
    planes = _planes(closed_A(rw, rh, M, d, x, dtype), rw, rh, d)
    return np.concatenate([_block_transform(p, C).reshape(p.shape[0], -1) for p in planes], axis=1)


def closed_T_pinv(rw, rh, M, d, y, dtype=np.float64):
    """[B, d^2 + 2 d^2 / n] -> [B, 3 d^2]: the inverse DCT of every block, then A_chroma^+ (closed_pinv)"""
    from tests.test_chroma_host import closed_pinv
    Ct = dct_matrix().T.astype(dtype)
    planes = _planes(y.astype(dtype), rw, rh, d)
    back = np.concatenate([_block_transform(p, Ct).reshape(p.shape[0], -1) for p in planes], axis=1)
    return closed_pinv(rw, rh, M, d, back, dtype)


def _config(d):
    return argparse.Namespace(data=argparse.Namespace(channels=3, image_size=d))


# ---------------------------------------------------------------------------------------------- 1. model self-checks
@pytest.mark.parametrize("H,W,rw,rh", [(16, 16, 1, 1), (32, 32, 2, 2), (16, 64, 2, 1)])
def test_T_has_an_exact_right_inverse_and_the_layout_is_in_place(H, W, rw, rh):
    """T T^+ = I (full row rank), T^+ = A_chroma^+ . IDCT, and coefficient (u, v) of block (I, J) sits at plane position
    (8 I + u, 8 J + v): the DC of every block of a constant image is 8 x the plane value, everything else 0."""
    M = kernel_matrix(BT601)
    D = JpegModel(rw, rh, M, H, W, np.ones(128), 0.0, whole=True)
    L = H * W + 2 * H * W // (rw * rh)
    assert D.T.shape == (L, 3 * H * W) and L % 4 == 0
    err = np.abs(D.T @ D.pinv - np.eye(L)).max()
    print(f"{H} x {W} site {rw}x{rh}: |T T^+ - I| max {err:.2e}")
    assert err < 1e-12
    A = dense_matrix(rw, rh, M, H, W)
    hw, hwn = H * W, H * W // (rw * rh)
    Dy, Dc = block_dct_matrix(H, W), block_dct_matrix(H // rh, W // rw)
    assert np.abs(Dy @ Dy.T - np.eye(hw)).max() < 1e-13 and np.abs(Dc @ Dc.T - np.eye(hwn)).max() < 1e-13
    idct = np.zeros((L, L))
    idct[:hw, :hw], idct[hw:hw + hwn, hw:hw + hwn], idct[hw + hwn:, hw + hwn:] = Dy.T, Dc.T, Dc.T
    assert np.abs(np.linalg.pinv(A) @ idct - D.pinv).max() < 1e-12
    x = np.ones((1, 3, H, W)) * np.array([0.3, -0.2, 0.6])[None, :, None, None]
    c = D.apply_T(x.reshape(1, -1))[0]
    planes = M @ np.array([0.3, -0.2, 0.6])
    want = np.zeros(L)
    want[:hw].reshape(H, W)[::8, ::8] = 8 * planes[0]
    want[hw:hw + hwn].reshape(H // rh, W // rw)[::8, ::8] = 8 * planes[1]
    want[hw + hwn:].reshape(H // rh, W // rw)[::8, ::8] = 8 * planes[2]
    assert np.abs(c - want).max() < 1e-13
    # one pixel lit: only the coefficients of its own blocks answer, and the luma ones are C[u][i] C[v][j] w_Y
    x = np.zeros((1, 3, H, W))
    i0, j0 = 8 + 3, W - 8 + 5
    x[0, 1, i0, j0] = 1.0
    c = D.apply_T(x.reshape(1, -1))[0]
    C = dct_matrix()
    Y = c[:hw].reshape(H, W)
    assert np.abs(Y[8:16, W - 8:] - np.outer(C[:, 3], C[:, 5]) * M[0, 1]).max() < 1e-14
    Y[8:16, W - 8:] = 0
    assert np.abs(Y).max() == 0
    cb = c[hw:hw + hwn].reshape(H // rh, W // rw)
    bi, bj = (i0 // rh) // 8, (j0 // rw) // 8
    assert np.abs(cb[8 * bi:8 * bi + 8, 8 * bj:8 * bj + 8]).max() > 0
    cb[8 * bi:8 * bi + 8, 8 * bj:8 * bj + 8] = 0
    assert np.abs(cb).max() == 0


@pytest.mark.parametrize("H,W,rw,rh", [(16, 16, 1, 1), (32, 32, 2, 2), (16, 64, 2, 1)])
def test_mcu_model_is_the_whole_model(H, W, rw, rh):
    """The per-MCU form that the GPU tests use at sizes whose whole matrix is out of reach is the same operator."""
    M = kernel_matrix(BT601)
    q, delta = steps_of(50)
    whole, mcu = JpegModel(rw, rh, M, H, W, q, delta, whole=True), JpegModel(rw, rh, M, H, W, q, delta)
    rng = np.random.default_rng(7)
    x, xt, et, n = (rng.standard_normal((2, 3 * H * W)) for _ in range(4))
    y = whole.encode(rng.uniform(-1, 1, (2, 3 * H * W)))
    assert np.abs(whole.apply_T(x) - mcu.apply_T(x)).max() < 1e-12
    assert np.abs(whole.apply_pinv(y) - mcu.apply_pinv(y)).max() < 1e-12
    for box in (0.98, 0.0):
        a, b = whole.step(xt, et, n, y, 0.45, 0.6, ETA, 0.3, box), mcu.step(xt, et, n, y, 0.45, 0.6, ETA, 0.3, box)
        assert np.abs(a[1] - b[1]).max() < 1e-12 and abs(a[2] - b[2]) < 1e-3


@pytest.mark.parametrize("rw,rh", SITES)
def test_closed_forms_equal_the_dense_model(rw, rh):
    M = kernel_matrix(BT601)
    D = JpegModel(rw, rh, M, 16, 16, np.ones(128), 0.0, whole=True)
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((2, 768)), rng.standard_normal((2, D.T.shape[0]))
    assert np.abs(closed_T(rw, rh, M, 16, x) - D.apply_T(x)).max() < 1e-12
    assert np.abs(closed_T_pinv(rw, rh, M, 16, y) - D.apply_pinv(y)).max() < 1e-12
    assert closed_T(rw, rh, M, 16, x, np.float32).dtype == np.float32


@pytest.mark.parametrize("rw,rh", SITES)
@pytest.mark.parametrize("quality", [10, 50, 90])
def test_projection_re_encodes_to_the_measured_levels(rw, rh, quality):
    """After x^0 = x0 - T^+(c - clamp(c, y - h, y + h)) with h = 0.98 q / 2, re-quantising T x^0 returns every measured
    level; with h = 0 the step is x0 - T^+(T x0 - y), and the wrapped operator hands the oracle's loop exactly that."""
    d = 32
    M = kernel_matrix(BT601)
    q, delta = steps_of(quality)
    D = JpegModel(rw, rh, M, d, d, q, delta)
    rng = np.random.default_rng(11)
    x_orig = rng.uniform(-1, 1, (2, 3 * d * d))
    y, lv = D.encode(x_orig), D.levels(x_orig)
    x0 = x_orig + 0.1 * rng.standard_normal(x_orig.shape)
    r, share = D.project(D.apply_T(x0), y, 0.98)
    x0h = x0 - D.apply_pinv(r)
    assert np.array_equal(D.levels(x0h), lv) and 0.0 < share < 1.0
    assert not np.array_equal(D.levels(x0), lv)
    r0, _ = D.project(D.apply_T(x0), y, 0.0)
    assert np.abs(r0 - (D.apply_T(x0) - y)).max() == 0
    op = CellOperator(D, y, 0.98)
    t = torch.from_numpy(x0)
    assert (t - op.A_pinv(op.A(t) - torch.from_numpy(y)) - torch.from_numpy(x0h)).abs().max() < 1e-13


# ---------------------------------------------------------------------------------------------- 2. the library's tables
@pytest.fixture(scope="module")
def lib():
    from ddnm_amd import _lib, build
    build.build()
    return _lib.lib()


def library_tables(lib, quality, dc_shift=1):
    q, delta = (ctypes.c_float * 128)(), ctypes.c_float(7.0)
    rc = lib.ddnm_jpeg_quality_tables(quality, dc_shift, q, ctypes.byref(delta))
    return rc if rc else (np.array(q[:], dtype=np.float32), float(delta.value))


@pytest.mark.parametrize("quality", QUALITIES)
def test_quality_tables(lib, quality):
    """ddnm_jpeg_quality_tables == libjpeg's formula over the Annex K tables (Pillow at quality 50) entry by entry, in x
    units (entry / 127.5 in fp32), and its 8-bit entries == the tables Pillow writes at that quality as sorted lists."""
    q, delta = library_tables(lib, quality)
    want = formula_tables(quality, base_tables())
    assert np.array_equal(q, (want.reshape(128) / 127.5).astype(np.float32))
    q8 = np.rint(q.astype(np.float64) * 127.5).astype(np.int64)
    assert np.array_equal(q8, want.reshape(128)) and q8.min() >= 1 and q8.max() <= 255
    py, pc = pillow_tables(quality)
    assert sorted(q8[:64].tolist()) == sorted(py) and sorted(q8[64:].tolist()) == sorted(pc)
    assert delta == float(np.float32(DELTA)) and library_tables(lib, quality, 0)[1] == 0.0
    print(f"Q={quality}: luma {q8[:64].min()}..{q8[:64].max()}, chroma {q8[64:].min()}..{q8[64:].max()}")


def test_quality_tables_refusals(lib):
    for quality in (0, -5, 101, 1000):
        assert library_tables(lib, quality) == -1
    q, delta = (ctypes.c_float * 128)(), ctypes.c_float()
    assert lib.ddnm_jpeg_quality_tables(50, 1, None, ctypes.byref(delta)) == -1
    assert lib.ddnm_jpeg_quality_tables(50, 1, q, None) == -1


# ---------------------------------------------------------------------------------------------- 3. operator, names, flags
def test_operator_tables(lib):
    from ddnm_amd.functions import svd_operators as E
    op = E.JPEG(3, 16, 50, 2, 2, "cpu")
    q, delta = steps_of(50)
    assert op.measurement_size() == 256 + 2 * 64 and op.measurement_image_shape() is None
    assert np.array_equal(op.q.astype(np.float64), q) and op.delta == delta and op.box == 0.98
    assert (op.mcus_per_workgroup(), E.JPEG(3, 16, 50, 1, 1, "cpu").mcus_per_workgroup()) == (8, 16)
    assert op.workgroups(3) == 1 and E.JPEG(3, 48, 50, 2, 2, "cpu").workgroups(3) == 4
    qr, dr = step_rows(q, delta, 2, 2, 16, 16)
    assert np.array_equal(op._q_row.numpy(), qr) and np.array_equal(op._delta_row.numpy(), dr)
    y = torch.from_numpy(qr * 3 + dr)[None]
    assert bool((op.levels(y) == 3).all()) and op.levels(y).dtype == torch.int64
    # the chroma spectrum: the DCT is orthogonal
    ch = E.ChromaSubsample(3, 16, 2, 2, "cpu")
    assert torch.equal(op.singulars(), ch.singulars())
    s444 = E.JPEG(3, 16, 50, 1, 1, "cpu").singulars()
    sv = np.linalg.svd(kernel_matrix(BT601), compute_uv=False)
    assert s444.shape == (768,) and np.abs(np.unique(s444.double().numpy()) - np.sort(sv)).max() < 1e-7
    # qtables override the quality; no level shift on request
    tabs = np.arange(1, 129).reshape(2, 8, 8)
    own = E.JPEG(3, 16, None, 2, 1, "cpu", qtables=tabs, dc_shift=False, box=0.5)
    assert np.array_equal(own.q, (np.arange(1, 129) / 127.5).astype(np.float32)) and own.delta == 0.0 and own.box == 0.5
    for name in ("Lambda", "V", "Vt", "U", "Ut"):
        with pytest.raises(NotImplementedError):
            getattr(op, name)(torch.zeros(1, 384), *([0.5, 0.1, 0.5, ETA] if name == "Lambda" else []))
    with pytest.raises(NotImplementedError):
        op.Lambda_noise(torch.zeros(1, 768), 0.5, 0.1, 0.5, ETA, torch.zeros(1, 768))
    assert not hasattr(op, "ddnm_plus_step")


def test_constructor_refusals(lib):
    from ddnm_amd.functions import svd_operators as E
    with pytest.raises(ValueError, match="channels"):
        E.JPEG(1, 16, 50, 2, 2, "cpu")
    for site in ((4, 1), (1, 2), (4, 4), (8, 8), (3, 3)):
        with pytest.raises(ValueError, match="sites"):
            E.JPEG(3, 32, 50, *site, "cpu")
    with pytest.raises(ValueError, match="MCU"):
        E.JPEG(3, 24, 50, 2, 2, "cpu")
    with pytest.raises(ValueError, match="MCU"):
        E.JPEG(3, 12, 50, 1, 1, "cpu")
    for quality in (0, 101, 50.5):
        with pytest.raises(ValueError, match=r"1\.\.100"):
            E.JPEG(3, 16, quality, 2, 2, "cpu")
    for box in (-0.1, 1.01, float("nan")):
        with pytest.raises(ValueError, match="box"):
            E.JPEG(3, 16, 50, 2, 2, "cpu", box=box)
    for tabs in (np.ones((2, 8, 8)), np.ones((8, 8), np.int64), np.zeros((2, 8, 8), np.int64)):
        with pytest.raises(ValueError, match="qtables"):
            E.JPEG(3, 16, 50, 2, 2, "cpu", qtables=tabs)
    with pytest.raises(ValueError, match="invertible"):
        E.JPEG(3, 16, 50, 2, 2, "cpu", matrix=np.zeros((3, 3)))


def test_build_operator_maps_the_names(lib):
    """jpeg_444 / jpeg_422 / jpeg_420 fix the site, --deg_scale is the integer quality 1..100 and anything else a
    ValueError that names the range.  (Every name ended in `degradation type not supported` before.)"""
    from ddnm_amd.functions import svd_operators as E
    for name, site in (("jpeg_444", (1, 1)), ("jpeg_422", (2, 1)), ("jpeg_420", (2, 2))):
        for scale in (1, 30.0, 100):
            op = E.build_operator(name, scale, _config(32), "cpu")
            assert isinstance(op, E.JPEG) and (op.rw, op.rh) == site and op.quality == int(scale) and op.box == 0.98
        assert E.build_operator(name, 50, _config(32), "cpu", jpeg_box=0.25).box == 0.25
        for scale in (0, 0.0, 101, 30.5, -3, None, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=r"1\.\.100"):
                E.build_operator(name, scale, _config(32), "cpu")
    with pytest.raises(ValueError, match="degradation type not supported"):
        E.build_operator("jpeg_411", 50, _config(32), "cpu")


def _args(**kw):
    base = dict(deg="jpeg_420", deg_scale=30.0, sigma_y=0.0, sigma_y_shot=0.0, sigma_y_map=None, jpeg_box=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_runner_refuses_what_it_cannot_do():
    from ddnm_amd.guided_diffusion import diffusion as D
    D.check_jpeg_flags(_args(), False)
    D.check_jpeg_flags(_args(jpeg_box=0.5), False)
    D.check_jpeg_flags(_args(deg="chroma_420", sigma_y=0.1), True)          # another --deg: nothing to say
    D.check_jpeg_flags(argparse.Namespace(deg="colorization", deg_scale=0.0, sigma_y=0.0), False)   # a namespace without the flags
    for kw, simplified, match in ((dict(sigma_y=0.1), False, "sigma_y 0.1.*bounded, not Gaussian"),
                                  (dict(sigma_y_shot=0.01), False, "sigma_y_shot.*bounded, not Gaussian"),
                                  (dict(sigma_y_map="m.npy"), False, "sigma_y_map.*bounded, not Gaussian"),
                                  (dict(), True, "--simplified with --deg jpeg_420.*SVD path"),
                                  (dict(deg_scale=0.0), False, r"1\.\.100"), (dict(deg_scale=30.5), False, r"1\.\.100"),
                                  (dict(jpeg_box=1.5), False, r"\[0, 1\]"),
                                  (dict(deg="chroma_420", jpeg_box=0.98), False, "--jpeg_box.*chroma_420 does not read it"),
                                  (dict(deg="colorization", jpeg_box=0.0), False, "--jpeg_box")):
        with pytest.raises(ValueError, match=match):
            D.check_jpeg_flags(_args(**kw), simplified)


def test_command_lines_know_the_flag(tmp_path, monkeypatch):
    import importlib.util
    import main
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.chdir(tmp_path)
    argv = ["--ni", "--config", "celeba_hq.yml", "--path_y", "synthetic:1", "--deg", "jpeg_420", "--deg_scale", "30", "-i", "t"]
    assert main.parse_args_and_config(argv)[0].jpeg_box is None
    assert main.parse_args_and_config(argv + ["--jpeg_box", "0.5"])[0].jpeg_box == 0.5
    spec = importlib.util.spec_from_file_location("hq_main_for_jpeg", os.path.join(root, "hq_demo", "main.py"))
    hq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hq)
    with pytest.raises(ValueError, match="jpeg_420.*SVD path"):
        hq.main({}, {"deg": "jpeg_420", "path_y": "x.png"})


# ---------------------------------------------------------------------------------------------- 4. argument validation
def check_jpeg_validation(lib, ptr):
    """Every refusal of the five launching `*_jpeg_*` entry points, with distinct addresses from `ptr` on standing for the
    tensors (never dereferenced: all of it happens before a launch).  DDNM_E_BADARG = -1 comes before DDNM_E_SHAPE = -2."""
    from ddnm_amd._lib import StepScalars
    s = StepScalars()
    s.rng_on = 1
    sp = ctypes.byref(s)
    m = (ctypes.c_float * 9)(*np.asarray(BT601, dtype=np.float32).reshape(-1))
    sing = (ctypes.c_float * 9)(*np.asarray([BT601[0], BT601[1], BT601[1]], dtype=np.float32).reshape(-1))
    good = (ctypes.c_float * 128)(*([0.1] * 128))

    def steps(i, v):
        t = [0.1] * 128
        t[i] = v
        return (ctypes.c_float * 128)(*t)

    bad_q = [steps(0, 0.0), steps(127, -0.1), steps(64, float("nan")), steps(5, float("inf"))]
    P = [ptr + 64 * i for i in range(8)]                    # xt, et, y, -, x0, xt_next, keys / noise, spare
    bad_sites = ((4, 1), (1, 2), (3, 3), (2, 4), (4, 4), (8, 8), (0, 0), (-2, 1))

    def op(fn, a=P[0], b=P[2], B=2, H=16, W=16, rw=2, rh=2, mt=m, q=good, delta=0.0):
        tail = (q, delta) if fn is lib.ddnm_op_jpeg_A_f32 else ()
        return fn(a, b, B, H, W, rw, rh, mt, *tail, None)

    def step(fn, xt=P[0], et=P[1], es=768, nz=None, y=P[2], x0=P[4], xn=P[5], B=2, H=16, W=16, rw=2, rh=2, mt=m, q=good,
             box=0.98, sc=sp):
        return fn(xt, et, es, nz, y, x0, xn, B, H, W, rw, rh, mt, q, box, sc, None)

    for fn in (lib.ddnm_op_jpeg_T_f32, lib.ddnm_op_jpeg_A_f32, lib.ddnm_op_jpeg_pinv_f32):
        call = lambda fn=fn, **kw: op(fn, **kw)      # noqa: E731
        assert call(a=None) == -1 and call(b=None) == -1 and call(mt=None) == -1 and call(mt=sing) == -1, fn.__name__
        assert call(B=0) == -1 and call(B=-2) == -1, fn.__name__
        assert call(a=None, rw=3) == -1 and call(mt=sing, W=6) == -1 and call(B=0, H=24) == -1, fn.__name__      # BADARG first
        for rw, rh in bad_sites:
            assert call(rw=rw, rh=rh) == -2, (fn.__name__, rw, rh)
        assert call(H=24) == -2 and call(W=24) == -2 and call(H=8) == -2 and call(W=8, rw=2, rh=1) == -2, fn.__name__
        assert call(H=0) == -2 and call(W=0) == -2 and call(H=-16) == -2, fn.__name__
    for q in bad_q:
        assert op(lib.ddnm_op_jpeg_A_f32, q=q) == -1 and op(lib.ddnm_op_jpeg_A_f32, q=q, rw=3) == -1
    assert op(lib.ddnm_op_jpeg_A_f32, q=None) == -1 and op(lib.ddnm_op_jpeg_A_f32, delta=float("nan")) == -1
    for fn in (lib.ddnm_step_jpeg_f32, lib.ddnm_step_jpeg_keyed_f32):
        keyed = fn is lib.ddnm_step_jpeg_keyed_f32
        nz = P[6] if keyed else None                          # (a multiple of 16: a valid key table address)
        call = lambda fn=fn, nz=nz, **kw: step(fn, **{"nz": nz, **kw})      # noqa: E731
        for arg in ("xt", "et", "y", "xn", "mt", "q", "sc"):
            assert call(**{arg: None}) == -1, (fn.__name__, arg)
        assert call(B=0) == -1 and call(mt=sing) == -1, fn.__name__
        for q in bad_q:
            assert call(q=q) == -1 and call(q=q, H=24) == -1, fn.__name__
        for box in (-0.01, 1.01, float("nan"), float("inf")):
            assert call(box=box) == -1 and call(box=box, rw=4, rh=1) == -1, (fn.__name__, box)
        # an output that is xt, et or the other output
        assert call(xn=P[0]) == -1 and call(xn=P[1]) == -1 and call(xn=P[4]) == -1, fn.__name__
        assert call(x0=P[0]) == -1 and call(x0=P[1]) == -1 and call(x0=P[0], es=770) == -1, fn.__name__
        for rw, rh in bad_sites:
            assert call(rw=rw, rh=rh) == -2, (fn.__name__, rw, rh)
        assert call(H=24) == -2 and call(W=24) == -2 and call(H=8) == -2 and call(W=8, rw=2, rh=1) == -2, fn.__name__
        assert call(H=0) == -2 and call(es=770) == -2 and call(es=6) == -2, fn.__name__
        if keyed:
            assert call(nz=None) == -1 and call(nz=P[6] + 4) == -1, fn.__name__          # null / misaligned key table
    off = StepScalars()                                       # rng_on = 0 and no noise tensor: no source
    assert step(lib.ddnm_step_jpeg_f32, sc=ctypes.byref(off)) == -1


def test_argument_validation_without_gpu(lib):
    """The entry points refuse bad arguments before touching the device, so the built library answers on a host without
    one; the ABI stays 7."""
    assert lib.ddnm_version() == 7
    check_jpeg_validation(lib, 4096)


def test_hooks_marshal_their_arguments(lib):
    """Host-only dry run (tools/dry_run.py): A, A_linear, A_pinv and ddnm_step reach their entry points with arguments of
    the declared types, for a tensor, an in-kernel and a keyed noise source."""
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
        for rw, rh in SITES:
            op = E.JPEG(3, d, 50, rw, rh, "cpu")
            x = torch.zeros(B, 3, d, d)
            y = op.A(x)
            assert y.shape == (B, d * d + 2 * d * d // (rw * rh)) == op.A_linear(x).shape and op.A_pinv(y).shape == (B, 3 * d * d)
            et6 = torch.zeros(B, 6, d, d)
            s = ops.step_scalars(torch.tensor(0.5), torch.tensor(0.6), ETA)
            out = torch.zeros_like(x), torch.zeros_like(x)
            op.ddnm_step(x, et6[:, :3], torch.zeros_like(x), y, s, *out)
            op.ddnm_step(x, et6[:, :3], None, y, ops.PhiloxNoise(5).stamp(s, 1), None, out[1])
            with pytest.raises(ValueError):
                op.ddnm_step(x, et6[:, :3], None, y[:, :-1], s, *out)
            with pytest.raises(ValueError):
                op.A_pinv(y[:, :-1])
        assert dry.calls == {"ddnm_op_jpeg_A_f32": 3, "ddnm_op_jpeg_T_f32": 3, "ddnm_op_jpeg_pinv_f32": 3, "ddnm_step_jpeg_f32": 6}
    finally:
        _lib._lib, ops._stream, ops._f32c, ops._f16c = saved
