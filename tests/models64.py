"""Plain reference models of the GEMM and Walsh-Hadamard kernels (csrc/gemm_f32.hip, csrc/fwht.hip), importable without
a GPU: float64 where a rounding bound is asserted, float32 in the kernels' own operation order where bit-equality is
the claim.  tests/test_transform_models_host.py keeps them honest on the CPU; the GPU tests (test_gpu_gemm_dispatch.py,
test_gpu_fwht.py, test_gpu_operator_scales.py) compare the kernels against them."""
import math

import torch

U32 = 2.0 ** -24          # unit roundoff of IEEE binary32


# ------------------------------------------------------------------------------------------------ GEMM
def gemm64(A, B, D=None, alpha=1.0, beta=0.0, transa=False, transb=False):
    """C = alpha * op(A) @ op(B) + beta * D in float64 on (possibly strided) views [..., rows, cols] as STORED:
    `transa`: A is stored [K][M]; `transb`: B is stored [N][K] (the ddnm_gemm_desc convention).  D = None counts as 0.
    Returns (C, env) with the error envelope env = |alpha| * (|op(A)| @ |op(B)|) + |beta| * |D|: fp32 accumulation in
    ANY summation order obeys |C_fp32 - C| <= (K + 4) * 2^-24 * env elementwise (K products and K - 1 additions, each
    rounded once, is at most gamma_K; the 4 covers alpha *, beta *, the final addition and one spare)."""
    a = A.double().transpose(-1, -2) if transa else A.double()
    b = B.double().transpose(-1, -2) if transb else B.double()
    prod, env = torch.matmul(a, b), torch.matmul(a.abs(), b.abs())
    C, env = float(alpha) * prod, abs(float(alpha)) * env
    if D is not None:
        d = D.double()
        C, env = C + float(beta) * d, env + abs(float(beta)) * d.abs()
    return C, env


def gemm_bound(K, env):
    return (K + 4) * U32 * env


# ------------------------------------------------------------------------------------------------ Walsh-Hadamard
def hadamard64(n):
    """The n x n Sylvester matrix (entries +-1, natural order) by Kronecker products, float64."""
    assert n >= 1 and n & (n - 1) == 0
    H2 = torch.tensor([[1.0, 1.0], [1.0, -1.0]], dtype=torch.float64)
    H = torch.ones(1, 1, dtype=torch.float64)
    while H.shape[0] < n:
        H = torch.kron(H2, H)
    return H


def _stages(x, dim):
    """Butterfly stages h = 1, 2, ..., n/2 along `dim`, (lower, upper) -> (a + b, a - b), in the dtype of x."""
    x = x.movedim(dim, -1)
    shape, n = x.shape, x.shape[-1]
    h = 1
    while h < n:
        v = x.reshape(*shape[:-1], n // (2 * h), 2, h)
        a, b = v[..., 0, :], v[..., 1, :]
        x = torch.stack([a + b, a - b], dim=-2).reshape(shape)
        h *= 2
    return x.movedim(-1, dim)


def fwht2d_f32(x, mask=None):
    """float32 model of ddnm_fwht2d_f32 / ddnm_fwht2d_masked_f32 on [..., n, n] in the kernels' operation order.
    Unmasked: row stages, column stages, one multiplication by 1/n.  Masked (`mask` broadcastable to x): rows, cols,
    * mask, cols, * 1/n, rows, * 1/n.  Every operation is one IEEE fp32 addition, subtraction or multiplication, and the
    multiplications by 1/n are exact (powers of two), so a kernel that keeps this order is bit-identical to it."""
    assert x.dtype == torch.float32
    n = x.shape[-1]
    inv = torch.tensor(1.0 / n, dtype=torch.float32)
    t = _stages(_stages(x, -1), -2)
    if mask is None:
        return t * inv
    t = _stages(t * mask.to(torch.float32), -2) * inv
    return _stages(t, -1) * inv


def fwht_bound(x, transforms=1):
    """Elementwise bound of `transforms` chained orthonormal 2-D transforms of the planes x [..., n, n] in fp32: every
    output of one transform is a signed sum of all n^2 inputs built by 2 log2(n) additions per element, so its error is
    at most (2 log2(n) + 2) * 2^-24 * (ones @ |X| @ ones) / n (the 2: the exact scalings and one spare).  A second
    transform (the masked form, with one more rounding for the mask product) sees at most the envelope of the first as
    its input, for a mask of magnitude <= 1."""
    n = x.shape[-1]
    ones = torch.ones(n, n, dtype=torch.float64)
    env = ones @ x.double().abs() @ ones / n
    for _ in range(transforms - 1):
        env = ones @ env @ ones / n
    return (transforms * (2 * math.log2(n) + 2) + (transforms - 1)) * U32 * env


# ------------------------------------------------------------------------------------------------ gather / scatter
def wh_gather_model(planes, perm, n_keep):
    """y[b][k*C + c] = planes[b][c][perm[k]] for k*C + c < n_keep (comment above wh_gather_kernel); planes [B, C, N]."""
    B, C, N = planes.shape
    y = torch.empty(B, n_keep, dtype=planes.dtype)
    p = perm.long()
    for j in range(n_keep):
        k, c = divmod(j, C)
        y[:, j] = planes[:, c, p[k]]
    return y


def wh_scatter_model(y, perm, C, N):
    """planes[b][c][perm[k]] = y[b][k*C + c] if k*C + c < n_keep else 0 (comment above wh_scatter_kernel); y [B, n_keep]."""
    B, n_keep = y.shape
    planes = torch.full((B, C, N), float("nan"), dtype=y.dtype)      # the model must cover every entry itself
    p = perm.long()
    for k in range(N):
        for c in range(C):
            j = k * C + c
            planes[:, c, p[k]] = y[:, j] if j < n_keep else 0.0
    return planes
