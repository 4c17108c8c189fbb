"""Host-side set-up of the ENGINE operators (the matrices / tables their constructors compute before any kernel
runs) against the behaviour of the reference's operator classes, evaluated on CPU with plain torch: a second,
oracle-independent pin of the constructors.  The reference's outputs on the same seeded inputs are recorded in
tests/golden/reference_pins.npz (tests/golden/make_golden_ref_pins.py); no GPU, no HIP library."""
import os

import numpy as np
import pytest
import torch

from oracle import cases
from tests.helpers import rel


@pytest.fixture(scope="module")
def R(golden_dir):
    """The reference's recorded outputs, by name."""
    g = np.load(os.path.join(golden_dir, "reference_pins.npz"))
    return {k: torch.from_numpy(g[k]) for k in g.files if g[k].dtype.kind == "f"}


def _engine():
    from ddnm_amd.functions import svd_operators as E
    return E


def _planes(v, c, d):
    return v.reshape(v.shape[0], c, d, d)


@pytest.mark.parametrize("factor,d", [(4, 64), (2, 32), (8, 64)])
def test_srconv_matrices(factor, d, R):
    E = _engine()
    k = E.bicubic_kernel(factor)
    eng = E.SRConv(k, 3, d, "cpu", stride=factor)
    x = cases.operator_input(d, 2)
    y_ref = R[f"srconv_{factor}_{d}_y"]                                       # reference SRConv(k, ...).A(x)
    y_eng = (eng.Ae @ _planes(x, 3, d) @ eng.Ae.T).reshape(2, -1)            # what _A's two GEMMs compute
    assert rel(y_eng, y_ref) < 2e-6
    p_ref = R[f"srconv_{factor}_{d}_pinv"]                                    # reference A_pinv(y_ref)
    m = d // factor
    p_eng = (eng.Pe @ _planes(y_ref, 3, m) @ eng.Pe.T).reshape(2, -1)
    assert rel(p_eng, p_ref) < 2e-5
    assert torch.equal(eng.singulars().cpu(), R[f"srconv_{factor}_{d}_singulars"])


@pytest.mark.parametrize("name", ["deblur_uni", "deblur_gauss", "deblur_aniso"])
def test_deblurring_tables(name, R):
    E = _engine()
    d = 32
    cfg = cases.weights.celeba_config(resolution=d)
    eng = E.build_operator(name, 0, cfg, "cpu")
    # reference: Deblurring([1/9] * 9) / Deblurring(gaussian_taps(10, 2)) / Deblurring2D(gaussian_taps(1, 4),
    # gaussian_taps(20, 4)), taps normalised, at d = 32
    x = cases.operator_input(d, 2)
    y_ref = R[f"{name}_y"]
    X = _planes(x, 3, d)
    spec = (eng.V1t @ X @ eng.V2t.T) * eng.G.reshape(1, 3, d, d)               # V1^T X V2, gains
    y_eng = (eng.U1 @ spec @ eng.U2.T).reshape(2, -1)
    assert rel(y_eng, y_ref) < 1e-5
    Y = _planes(y_ref, 3, d)
    p_eng = (eng.V1 @ ((eng.U1t @ Y @ eng.U2t.T) * eng.Ginv.reshape(1, 3, d, d)) @ eng.V2.T).reshape(2, -1)
    assert rel(p_eng, R[f"{name}_pinv"]) < 1e-4
    assert torch.equal(eng.singulars().cpu(), R[f"{name}_singulars"])


def test_cs_matrix(R):
    E = _engine()
    from oracle import operators as O
    gauss = O.gauss_matrix(cases.SEED + 21)             # the reference's CS(3, 64, 0.25) after torch.manual_seed(SEED + 21)
    eng = E.CS(3, 64, 0.25, "cpu", gauss=gauss)
    x = cases.operator_input(64, 2)
    patches = x.reshape(2, 3, 2, 32, 2, 32).permute(0, 1, 2, 4, 3, 5).reshape(2 * 3 * 4, 1024)      # ddnm_patchify_f32
    y_eng = (patches @ eng.M.T).reshape(2, -1)
    assert rel(y_eng, R["cs_y"]) < 2e-6
    assert torch.equal(eng.singulars().cpu(), R["cs_singulars"])


@pytest.mark.parametrize("seed", [0, 1])
def test_inpainting_rank_table(seed, R):
    E = _engine()
    d = 16
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(d, d, generator=g) > 0.3).long()
    r = torch.nonzero(mask.reshape(-1) == 0).long().reshape(-1) * 3
    missing = torch.cat([r, r + 1, r + 2], dim=0)
    eng = E.Inpainting(3, d, missing, "cpu")
    x = torch.randn(2, 3, d, d, generator=g)
    y_ref = R[f"inpainting_rank_{seed}_y"]                                  # reference Inpainting(3, d, missing).A(x)
    # what ddnm_op_inpaint_A_f32 does with the table: y[b, 3*rank[p] + c] = x[b, c, p] for kept pixels
    rank = eng.rank.long()
    y_eng = torch.zeros(2, 3 * eng.n_kept)
    kept = torch.nonzero(rank >= 0).reshape(-1)
    for c in range(3):
        y_eng[:, 3 * rank[kept] + c] = x.reshape(2, 3, -1)[:, c, kept]
    assert torch.equal(y_eng, y_ref)
    assert torch.equal(eng.kept_mask.cpu().reshape(d, d), mask.float())


def test_walsh_hadamard_mask(R):
    E = _engine()
    d = 16
    perm = cases.wh_perm(d)
    eng = E.WalshHadamardCS(3, d, 4, perm, "cpu")
    x = cases.operator_input(d, 2)
    # A^+ A x through the engine's spectral mask: fwht, keep the measured (channel, frequency) entries, fwht
    def fwht2(v):                                             # orthonormal separable WHT of [B,C,d,d]
        H = torch.tensor([[1.0]])
        while H.shape[0] < d:
            H = torch.cat([torch.cat([H, H], 1), torch.cat([H, -H], 1)], 0)
        H = H / d ** 0.5
        return H @ v @ H.T
    spec = fwht2(_planes(x, 3, d)) * eng.mask.reshape(1, 3, d, d)
    got = fwht2(spec).reshape(2, -1)
    want = R["walsh_hadamard_pinv_A"]                          # reference WalshHadamardCS(3, d, 4, perm): A^+ A x
    assert rel(got, want) < 1e-5
    assert eng.n_keep == R["walsh_hadamard_singulars"].shape[0]
