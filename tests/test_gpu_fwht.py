"""The Walsh-Hadamard kernels of csrc/fwht.hip through the C ABI, as WalshHadamardCS calls them: every supported size
(n = 32: the stage-by-stage LDS column kernel `fwht_cols_kernel`; n = 64, 128, 256: the register-resident
`fwht_cols_reg_kernel<n>`), unmasked and masked, plus ddnm_wh_gather_f32 / ddnm_wh_scatter_f32 at measurement counts
that are no multiple of the channel count.

Bit-equality is the claim: the kernels do fp32 additions and subtractions in a fixed order and multiply by powers of
two, so they must equal the float32 butterfly model tests/models64.py::fwht2d_f32 bit for bit at all four sizes -- which
also pins the source's statement that its two column kernels are bit-identical.  The float64 Hadamard sandwich is
asserted within the derived bound models64.fwht_bound (measured on the MI355X: worst |err| / bound 0.023, no entry
differing from the float32 model at any size)."""
import pytest
import torch

from tests import models64 as M64

pytestmark = pytest.mark.gpu

SIZES = [32, 64, 128, 256]
E_SHAPE = -2                          # DDNM_E_SHAPE, include/ddnm_hip.h
_REF = {}


def gen(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _input(n):
    """7 planes per size, shared by the plane counts (the first `planes` of them), with the float32 model and the
    float64 sandwich; computed once and left unchanged."""
    if n not in _REF:
        x = gen(7, n, n, seed=300 + n)
        H = M64.hadamard64(n)
        _REF[n] = (x, M64.fwht2d_f32(x), H @ x.double() @ H / n, M64.fwht_bound(x))
    return _REF[n]


def _masked(hip, x, mask, planes_mask):
    planes, n = x.shape[0], x.shape[-1]
    dx, dm = x.cuda().contiguous(), mask.cuda().contiguous()
    out, scratch = torch.full_like(dx, float("nan")), torch.full_like(dx, float("nan"))
    rc = hip.ddnm_fwht2d_masked_f32(dx.data_ptr(), dm.data_ptr(), planes_mask, out.data_ptr(), planes, n,
                                    scratch.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu(), x), "the masked transform changed its input"
    return out.cpu()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("planes", [1, 3, 7])
def test_fwht2d_is_the_butterfly_model_bit_for_bit(hip, n, planes):
    x, model, ref64, bound = _input(n)
    dx = x[:planes].cuda().contiguous()
    out = torch.full((planes + 1, n, n), float("nan"), device="cuda")            # one plane of guard behind the output
    assert hip.ddnm_fwht2d_f32(dx.data_ptr(), out.data_ptr(), planes, n, _stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool(torch.isnan(got[planes]).all()), "the transform wrote past its last plane"
    assert torch.equal(dx.cpu(), x[:planes]), "the out-of-place transform changed its input"
    got = got[:planes]
    err = (got.double() - ref64[:planes]).abs()
    print(f"fwht2d n={n} planes={planes}: worst |err|/bound {float((err / bound[:planes]).max()):.4f}, "
          f"entries differing from the fp32 model {int((got != model[:planes]).sum())}")
    assert bool((err <= bound[:planes]).all())
    assert torch.equal(got, model[:planes])


@pytest.mark.parametrize("n", SIZES)
def test_fwht2d_in_place(hip, n):
    """WalshHadamardCS never calls it in place, but the header does not forbid it and the column pass runs in place."""
    x, model, _, _ = _input(n)
    d = x[:3].cuda().contiguous()
    assert hip.ddnm_fwht2d_f32(d.data_ptr(), d.data_ptr(), 3, n, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(d.cpu(), model[:3])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("planes_mask", [1, 3])
def test_masked_binary_mask_bit_for_bit(hip, n, planes_mask):
    """planes = 6 over planes_mask mask planes: plane p uses mask[p % planes_mask].  A 0 / 1 mask multiplies exactly, fused
    into the next addition or not, so the float32 model must be met bit for bit."""
    x = _input(n)[0][:6]
    mask = (torch.rand(planes_mask, n, n, generator=torch.Generator().manual_seed(n + planes_mask)) < 0.3).float()
    full = mask.repeat(6 // planes_mask, 1, 1)                                    # plane p -> mask[p % planes_mask]
    got = _masked(hip, x, mask, planes_mask)
    H = M64.hadamard64(n)
    ref64 = H @ (full.double() * (H @ x.double() @ H / n)) @ H / n
    err, bound = (got.double() - ref64).abs(), M64.fwht_bound(x, transforms=2)
    print(f"fwht2d_masked n={n} planes_mask={planes_mask}: worst |err|/bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())
    assert torch.equal(got, M64.fwht2d_f32(x, full))
    if planes_mask == 3:                                                          # the three mask planes do differ
        assert not torch.equal(got[0], M64.fwht2d_f32(x[0], mask[1]))


@pytest.mark.parametrize("n", SIZES)
def test_masked_real_mask_and_all_ones_mask(hip, n):
    """A real-valued mask in [0, 1): its product may be contracted into the following addition, so only the derived bound
    of two chained transforms is asserted.  All ones: H H = I, the input comes back within that bound."""
    x = _input(n)[0][:6]
    mask = torch.rand(3, n, n, generator=torch.Generator().manual_seed(7 * n))
    full = mask.repeat(2, 1, 1)
    H = M64.hadamard64(n)
    ref64 = H @ (full.double() * (H @ x.double() @ H / n)) @ H / n
    bound = M64.fwht_bound(x, transforms=2)
    err = (_masked(hip, x, mask, 3).double() - ref64).abs()
    print(f"fwht2d_masked real mask n={n}: worst |err|/bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())
    err1 = (_masked(hip, x, torch.ones(1, n, n), 1).double() - x.double()).abs()
    print(f"fwht2d_masked ones mask n={n}: worst |err|/bound {float((err1 / bound).max()):.4f}")
    assert bool((err1 <= bound).all())


@pytest.mark.parametrize("n", [16, 48, 512])
def test_unsupported_sizes_are_refused(hip, n):
    x = torch.zeros(n * n, device="cuda")
    out = torch.full((n * n,), float("nan"), device="cuda")
    assert hip.ddnm_fwht2d_f32(x.data_ptr(), out.data_ptr(), 1, n, _stream()) == E_SHAPE
    assert hip.ddnm_fwht2d_masked_f32(x.data_ptr(), x.data_ptr(), 1, out.data_ptr(), 1, n, out.data_ptr(),
                                      _stream()) == E_SHAPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ gather / scatter
C_, N_, B_ = 3, 1024, 2
KEEPS = [C_ * N_, C_ * N_ // 3, 1, C_ * N_ - 1]


def _perm():
    return torch.randperm(N_, generator=torch.Generator().manual_seed(11)).to(torch.int32)


@pytest.mark.parametrize("n_keep", KEEPS)
def test_wh_gather_is_the_index_model(hip, n_keep):
    planes, perm = gen(B_, C_, N_, seed=12), _perm()
    y = torch.full((B_ * n_keep + 16,), float("nan"), device="cuda")
    d_planes, d_perm = planes.cuda(), perm.cuda()
    assert hip.ddnm_wh_gather_f32(d_planes.data_ptr(), d_perm.data_ptr(), y.data_ptr(), B_, C_, N_, n_keep,
                                  _stream()) == 0
    torch.cuda.synchronize()
    got = y.cpu()
    assert bool(torch.isnan(got[B_ * n_keep:]).all()), "gather wrote past B * n_keep"
    assert torch.equal(got[:B_ * n_keep].reshape(B_, n_keep), M64.wh_gather_model(planes, perm, n_keep))


@pytest.mark.parametrize("n_keep", KEEPS)
def test_wh_scatter_is_the_index_model_and_covers_every_entry(hip, n_keep):
    y, perm = gen(B_, n_keep, seed=13), _perm()
    planes = torch.full((B_ * C_ * N_ + 16,), float("nan"), device="cuda")
    d_y, d_perm = y.cuda().contiguous(), perm.cuda()
    assert hip.ddnm_wh_scatter_f32(d_y.data_ptr(), d_perm.data_ptr(), planes.data_ptr(), B_, C_, N_, n_keep,
                                   _stream()) == 0
    torch.cuda.synchronize()
    got = planes.cpu()
    assert bool(torch.isnan(got[B_ * C_ * N_:]).all()), "scatter wrote past B * C * N"
    got = got[:B_ * C_ * N_].reshape(B_, C_, N_)
    assert not bool(torch.isnan(got).any()), "scatter left entries of the planes unwritten"
    assert torch.equal(got, M64.wh_scatter_model(y, perm, C_, N_))
