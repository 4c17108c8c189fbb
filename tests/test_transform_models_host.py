"""The reference models of tests/models64.py against independent formulations, on the CPU: the GPU tests of the GEMM and
Walsh-Hadamard kernels stand on these models, so they are pinned here where no kernel is involved."""
import pytest
import torch

from tests import models64 as M


def gen(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("n", [1, 2, 32, 64, 128, 256])
def test_hadamard_is_symmetric_sign_matrix_and_involution(n):
    H = M.hadamard64(n)
    assert H.shape == (n, n) and H.dtype == torch.float64
    assert torch.equal(H.abs(), torch.ones(n, n, dtype=torch.float64)) and torch.equal(H, H.T)
    assert torch.equal(H @ H, n * torch.eye(n, dtype=torch.float64))              # (H / sqrt n)^2 = I, exactly
    if n >= 4:                                                                     # natural (Sylvester) order
        assert torch.equal(H[1], torch.tensor([1.0, -1.0], dtype=torch.float64).repeat(n // 2))
        assert torch.equal(H[n // 2], torch.cat([torch.ones(n // 2), -torch.ones(n // 2)]).double())


@pytest.mark.parametrize("n", [32, 64, 128, 256])
def test_fwht2d_model_is_the_hadamard_sandwich(n):
    x = gen(3, n, n, seed=n)
    H = M.hadamard64(n)
    got = M.fwht2d_f32(x)
    assert got.dtype == torch.float32
    err = (got.double() - H @ x.double() @ H / n).abs()
    bound = M.fwht_bound(x)
    print(f"fwht2d_f32 n={n}: worst |err|/bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())
    # an involution: twice the model is the input, within the bound of two chained transforms
    back = M.fwht2d_f32(got)
    assert bool(((back.double() - x.double()).abs() <= M.fwht_bound(x, transforms=2)).all())


@pytest.mark.parametrize("n", [32, 128])
def test_fwht2d_masked_model(n):
    x = gen(4, n, n, seed=n + 1)
    H = M.hadamard64(n)
    ones = torch.ones(1, n, n)
    assert bool(((M.fwht2d_f32(x, ones).double() - x.double()).abs() <= M.fwht_bound(x, transforms=2)).all())
    mask = (torch.rand(2, n, n, generator=torch.Generator().manual_seed(3)) < 0.4).float().repeat(2, 1, 1)
    ref = H @ (mask.double() * (H @ x.double() @ H / n)) @ H / n
    err = (M.fwht2d_f32(x, mask).double() - ref).abs()
    assert bool((err <= M.fwht_bound(x, transforms=2)).all())
    assert float(err.max()) > 0.0                      # fp32 model, not the float64 formula in disguise
    # the first half of the masked form is the unmasked transform up to the (exact) scaling: a mask applied by hand
    half = M.fwht2d_f32(x) * mask
    assert torch.equal(M.fwht2d_f32(x, mask), M._stages(M._stages(half, -2) * (1.0 / n), -1))


def test_fwht2d_model_stage_order_on_a_unit_impulse():
    """Stage h pairs (i, i + h): an impulse at (r, c) transforms to the outer product of rows r and c of H, exactly."""
    n = 32
    H = M.hadamard64(n)
    for r, c in [(0, 0), (1, 2), (5, 31), (31, 16)]:
        x = torch.zeros(n, n)
        x[r, c] = 1.0
        assert torch.equal(M.fwht2d_f32(x).double(), torch.outer(H[:, r], H[c]) / n)


@pytest.mark.parametrize("transa", [False, True])
@pytest.mark.parametrize("transb", [False, True])
def test_gemm64_equals_bmm(transa, transb):
    Mm, N, K, batch = 5, 7, 9, 3
    A, B, D = gen(batch, Mm, K, seed=1).double(), gen(batch, K, N, seed=2).double(), gen(batch, Mm, N, seed=3).double()
    ref = -0.5 * torch.bmm(A, B) + 2.0 * D
    As = A.transpose(1, 2).contiguous() if transa else A
    Bs = B.transpose(1, 2).contiguous() if transb else B
    C, env = M.gemm64(As, Bs, D, -0.5, 2.0, transa, transb)
    assert C.dtype == torch.float64 and torch.allclose(C, ref, rtol=0, atol=1e-13)
    assert torch.allclose(env, 0.5 * torch.bmm(A.abs(), B.abs()) + 2.0 * D.abs(), rtol=0, atol=1e-13)
    assert bool((env >= C.abs() - 1e-13).all())
    C0, env0 = M.gemm64(As, Bs, None, 1.0, 3.0, transa, transb)            # D = None: beta has nothing to scale
    assert torch.allclose(C0, torch.bmm(A, B), rtol=0, atol=1e-13) and torch.allclose(env0, torch.bmm(A.abs(), B.abs()))


def test_gemm64_reads_strided_views_and_fp32_obeys_its_bound():
    buf = gen(4000, seed=4)
    A = torch.as_strided(buf, (2, 3, 6, 8), (1000, 8, 50, 1), 3)            # outer / inner batch, padded rows, offset
    B = torch.as_strided(buf, (2, 3, 8, 4), (0, 0, 4, 1), 100)             # shared operand
    C, env = M.gemm64(A, B)
    ref = torch.stack([torch.stack([A[o, i].double() @ B[0, 0].double() for i in range(3)]) for o in range(2)])
    assert torch.allclose(C, ref, rtol=0, atol=1e-13)
    err = (torch.matmul(A, B).double() - C).abs()                           # torch's fp32 product: some summation order
    assert bool((err <= M.gemm_bound(8, env)).all())


def test_gather_scatter_models_are_inverse_on_the_kept_entries():
    C, N, B = 3, 64, 2
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5)).to(torch.int32)
    planes = gen(B, C, N, seed=6)
    for n_keep in (C * N, C * N // 3, 1, C * N - 1, 64):                     # 64 % 3 == 1
        y = M.wh_gather_model(planes, perm, n_keep)
        assert y.shape == (B, n_keep)
        # the reference's own formulation (oracle.operators.WalshHadamardCS.A): permute, (k, c) interleave, cut
        assert torch.equal(y, planes[:, :, perm.long()].permute(0, 2, 1).reshape(B, -1)[:, :n_keep])
        back = M.wh_scatter_model(y, perm, C, N)
        assert not bool(torch.isnan(back).any())
        kept = torch.zeros(C, N, dtype=torch.bool)
        for j in range(n_keep):
            kept[j % C, perm[j // C]] = True
        assert torch.equal(back, torch.where(kept[None], planes, torch.zeros(())))
