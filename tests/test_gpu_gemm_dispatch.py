"""ddnm_bgemm_f32 on every dispatch branch (csrc/gemm_f32.hip) and ddnm_softmax_rows_f32 at its edges, through ops.bgemm /
ops.softmax_rows_ against float64 (tests/models64.py::gemm64).

The host predicate picks one of three kernels: the 64x64 MFMA tile `bgemm_f32_kernel<1,1>`, the 128x128 tile `<2,2>`
(M, N multiples of 128 and at least 256 such tiles in the launch) and the scalar `bgemm_naive_kernel` (M or N no multiple
of 64, K no multiple of 32, lda / ldb or an A / B batch stride no multiple of 4, A or B not 16-byte aligned).  Every case
names the branch it is meant for and `_branch` (the predicate restated on the actual pointers) asserts that it lands there.

Tolerance: derived, not measured.  fp32 accumulation in any order obeys |C - C64| <= (K + 4) 2^-24 env elementwise with
env = |alpha| |A| |B| + |beta| |D| (models64.gemm64); each case prints its worst |err| / bound.  Every destination buffer is
pre-filled with one bit pattern (a NaN) and must keep it bit for bit outside the M x N windows the launch owns.
Measured on the MI355X: worst |err| / bound over all cases 0.175 (fallback, K = 12), 0.164 on the MFMA tiles."""
import pytest
import torch

from tests import models64 as M64

pytestmark = pytest.mark.gpu

PATTERN = 0x7FC5A5A5                  # a quiet NaN with a payload, as int32: a pad read as D would poison the output
E_SHAPE = -2                          # DDNM_E_SHAPE, include/ddnm_hip.h
GUARD = 64                                                                          # floats after the last window of C


def _natural(rows, cols, inner, pad=0, off=0, gap_outer=0):
    """(ld, outer stride, inner stride, offset) of a packed [outer][inner][rows][cols + pad] operand."""
    ld = cols + pad
    return ld, inner * rows * ld + gap_outer, rows * ld, off


def _extent(lay, outer, inner, rows, cols):
    ld, so, si, off = lay
    return off + (outer - 1) * so + (inner - 1) * si + (rows - 1) * ld + cols


def _view(buf, lay, outer, inner, rows, cols):
    ld, so, si, off = lay
    return torch.as_strided(buf, (outer, inner, rows, cols), (so, si, ld, 1), off)


def _branch(M, N, K, batch, lda, ldb, sA, sB, pA, pB):
    """The host predicate of ddnm_bgemm_f32, restated."""
    aligned = (lda | ldb) % 4 == 0 and (sA[0] | sA[1] | sB[0] | sB[1]) % 4 == 0 and (pA | pB) % 16 == 0
    if M % 64 or N % 64 or K % 32 or not aligned:
        return "naive"
    if M % 128 == 0 and N % 128 == 0 and batch * (M // 128) * (N // 128) >= 256:
        return "t128"
    return "t64"


def run_case(tag, expect, M, N, K, batch, *, inner=1, transa=False, transb=False, A=None, B=None, C=None, D=None,
             alpha=1.0, beta=0.0, positive=False, seed=100):
    """One launch.  A / B / C: (ld, outer stride, inner stride, offset) in floats, default packed; D: None, "alias" (D is
    C: accumulate in place) or such a tuple.  Asserts the branch, the derived bound and the untouched padding."""
    from ddnm_amd import ops
    assert batch % inner == 0
    outer = batch // inner
    ra, ca = (K, M) if transa else (M, K)
    rb, cb = (N, K) if transb else (K, N)
    A = A or _natural(ra, ca, inner)
    B = B or _natural(rb, cb, inner)
    C = C or _natural(M, N, inner)
    g = torch.Generator().manual_seed(seed)

    def draw(n):
        t = torch.randn(n, generator=g)
        return t.abs() + 0.25 if positive else t

    bufA, bufB = draw(_extent(A, outer, inner, ra, ca)), draw(_extent(B, outer, inner, rb, cb))
    nC = _extent(C, outer, inner, M, N) + GUARD
    bufC = torch.full((nC,), PATTERN, dtype=torch.int32).view(torch.float32).clone()
    window = torch.zeros(nC, dtype=torch.bool)
    _view(window, C, outer, inner, M, N).fill_(True)
    assert int(window.sum()) == batch * M * N, "the C windows of the case overlap"
    vA, vB = _view(bufA, A, outer, inner, ra, ca), _view(bufB, B, outer, inner, rb, cb)
    vD = bufD = None
    if D == "alias":
        _view(bufC, C, outer, inner, M, N).copy_(draw(batch * M * N).reshape(outer, inner, M, N))
        vD = _view(bufC, C, outer, inner, M, N).clone()
    elif D is not None:
        bufD = draw(_extent(D, outer, inner, M, N))
        vD = _view(bufD, D, outer, inner, M, N)
    ref, env = M64.gemm64(vA, vB, vD, alpha, beta, transa, transb)

    dA, dB, dC = bufA.cuda(), bufB.cuda(), bufC.cuda()
    dD = None if bufD is None else bufD.cuda()
    pA, pB, pC = dA[A[3]:], dB[B[3]:], dC[C[3]:]
    if D == "alias":
        pD, ldd, sD = pC, C[0], (C[1], C[2])
    elif D is not None:
        pD, ldd, sD = dD[D[3]:], D[0], (D[1], D[2])
    else:
        pD, ldd, sD = None, 0, (0, 0)
    got = _branch(M, N, K, batch, A[0], B[0], (A[1], A[2]), (B[1], B[2]), pA.data_ptr(), pB.data_ptr())
    assert got == expect, f"{tag}: meant for {expect}, the predicate picks {got}"
    ops.bgemm(pA, pB, pC, M, N, K, lda=A[0], ldb=B[0], ldc=C[0], transb=transb, transa=transa, batch=batch, inner=inner,
              sA=(A[1], A[2]), sB=(B[1], B[2]), sC=(C[1], C[2]), D=pD, ldd=ldd, sD=sD, alpha=alpha, beta=beta)
    torch.cuda.synchronize()
    out = dC.cpu()
    assert torch.equal(out.view(torch.int32)[~window], torch.full((int((~window).sum()),), PATTERN, dtype=torch.int32)), \
        f"{tag}: the launch wrote outside its M x N windows"
    res = _view(out, C, outer, inner, M, N).double()
    assert bool(torch.isfinite(res).all()), f"{tag}: non-finite output"
    err, bound = (res - ref).abs(), M64.gemm_bound(K, env)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"bgemm {tag} [{expect}] M={M} N={N} K={K} batch={batch}: worst |err|/bound {ratio:.4f}")
    assert bool((err <= bound).all()), f"{tag}: worst |err| / bound = {ratio:.3f}"
    return ratio


# ------------------------------------------------------------------------------------------------ the three branches
@pytest.mark.parametrize("expect,M,N,K,batch", [
    ("t64", 64, 64, 32, 1),
    ("t64", 128, 192, 96, 3),             # 2 x 3 tile grid: m_tile / n_tile swapped would fail
    ("t64", 128, 128, 64, 255),           # one block short of the <2,2> threshold
    ("t128", 128, 128, 64, 256),
    ("t128", 256, 128, 32, 128),          # mt != nt
])
@pytest.mark.parametrize("transb", [False, True])
def test_mfma_tiles(hip, expect, M, N, K, batch, transb):
    run_case(f"tiles tb={int(transb)}", expect, M, N, K, batch, transb=transb, D=_natural(M, N, 1), alpha=0.5, beta=-1.0)


@pytest.mark.parametrize("expect,M,N,K,batch", [("t64", 128, 192, 96, 3), ("t128", 256, 128, 64, 128),
                                                ("naive", 65, 127, 33, 2)])
def test_positive_operands_show_a_dropped_k_chunk(hip, expect, M, N, K, batch):
    """All operands > 0.25: nothing cancels, so a K chunk (or a single k) left out moves every output by far more than
    the bound."""
    run_case("positive", expect, M, N, K, batch, transb=True, positive=True)
    run_case("positive ta", expect, M, N, K, batch, transa=True, transb=False, positive=True)


BASE = dict(M=64, N=128, K=64, batch=2)


@pytest.mark.parametrize("trigger", ["none", "M63", "M65", "N127", "K33", "lda", "ldb", "ptrA", "ptrB", "strideA"])
@pytest.mark.parametrize("transb", [False, True])
def test_fallback_triggers_one_at_a_time(hip, trigger, transb):
    s = dict(BASE)
    kw = {}
    if trigger == "M63":
        s["M"] = 63
    elif trigger == "M65":
        s["M"] = 65
    elif trigger == "N127":
        s["N"] = 127
    elif trigger == "K33":
        s["K"] = 33
    M, N, K, batch = s["M"], s["N"], s["K"], s["batch"]
    rb, cb = (N, K) if transb else (K, N)
    if trigger == "K33":                                      # pitches stay multiples of 4: K alone departs
        kw["A"] = _natural(M, K, 1, pad=3)
        if transb:
            kw["B"] = _natural(rb, cb, 1, pad=3)
    elif trigger == "N127" and not transb:
        kw["B"] = _natural(rb, cb, 1, pad=1)                  # ldb = 128: N alone departs
    elif trigger == "lda":
        kw["A"] = _natural(M, K, 1, pad=1)                    # lda = K + 1
    elif trigger == "ldb":
        kw["B"] = _natural(rb, cb, 1, pad=2)
    elif trigger == "ptrA":
        kw["A"] = _natural(M, K, 1, pad=4, off=1)             # buf[1:], lda % 4 == 0
    elif trigger == "ptrB":
        kw["B"] = _natural(rb, cb, 1, pad=4, off=1)
    elif trigger == "strideA":
        kw["A"] = _natural(M, K, 1, gap_outer=2)              # sA[0] % 4 == 2
        assert kw["A"][1] % 4 == 2
    expect = "t64" if trigger == "none" else "naive"
    run_case(f"fallback {trigger} tb={int(transb)}", expect, M, N, K, batch, transb=transb,
             C=_natural(M, N, 1, pad=3), D=_natural(M, N, 1, pad=1), alpha=1.25, beta=0.75, **kw)


# ------------------------------------------------------------------------------------------------ transposition
@pytest.mark.parametrize("expect,M,N,K,batch", [("t64", 64, 128, 64, 2), ("t128", 128, 128, 64, 256),
                                                ("naive", 65, 127, 33, 2)])
@pytest.mark.parametrize("transa", [False, True])
@pytest.mark.parametrize("transb", [False, True])
def test_transposition(hip, expect, M, N, K, batch, transa, transb):
    run_case(f"trans ta={int(transa)} tb={int(transb)}", expect, M, N, K, batch, transa=transa, transb=transb)


@pytest.mark.parametrize("expect,M,N,K,batch,pad", [("t64", 128, 64, 96, 2, 4), ("t128", 128, 256, 32, 128, 8),
                                                    ("naive", 64, 64, 32, 2, 1), ("naive", 40, 24, 20, 3, 4)])
def test_transposed_a_with_a_pitch_wider_than_m(hip, expect, M, N, K, batch, pad):
    run_case(f"ta lda=M+{pad}", expect, M, N, K, batch, transa=True, transb=False, A=_natural(K, M, 1, pad=pad),
             C=_natural(M, N, 1, pad=5))


# ------------------------------------------------------------------------------------------------ strides
@pytest.mark.parametrize("expect,Bi,nh,T,hc", [("t64", 2, 2, 64, 64), ("t128", 32, 8, 128, 128), ("naive", 2, 3, 48, 24)])
@pytest.mark.parametrize("transa", [False, True])
def test_classifier_head_layout(hip, expect, Bi, nh, T, hc, transa):
    """The attention backward of the classifier: batch = B * nh with inner = nh; one operand is a head slice of a
    [B][T][3C] buffer (row pitch 3C, heads hc apart), the other a packed per-head matrix, and C is the v-slice of the
    head-interleaved dqkv (`dflat[2 * hc:]`, ldc = 3C, heads 3 hc apart): q and k of every head, and every other head, lie
    between the rows this launch writes and must stay untouched.  transa: the packed operand is P stored [K = T][M = T]
    (dV = P^T dO); otherwise A is the head slice (dP = dO V^T style reads)."""
    Cc = nh * hc
    slice_lay = (3 * Cc, T * 3 * Cc, hc, 0)                   # sA = (T * 3C, hc): head h of image b, rows 3C apart
    c_lay = (3 * Cc, T * 3 * Cc, 3 * hc, 2 * hc)
    if transa:        # A = P^T [T x T] packed, B = the head slice [K = T][N = hc]
        run_case("heads ta", expect, T, hc, T, Bi * nh, inner=nh, transa=True, transb=False, B=slice_lay, C=c_lay)
    else:             # A = the head slice [M = T][K = hc], B = packed [K = hc][N = hc]
        run_case("heads", expect, T, hc, hc, Bi * nh, inner=nh, transb=False, A=slice_lay, C=c_lay)


@pytest.mark.parametrize("expect,M,N,K,outer,inner", [("t64", 64, 128, 64, 2, 3), ("t128", 128, 128, 32, 64, 4),
                                                      ("naive", 30, 20, 12, 2, 3)])
def test_shared_operand_and_d_with_its_own_strides(hip, expect, M, N, K, outer, inner):
    """A shared across the whole batch (both strides 0), B with its own outer / inner strides, D laid out inner-major
    (a different order from C) with a padded pitch."""
    batch = outer * inner
    d_lay = (N + 4, M * (N + 4), outer * M * (N + 4), 0)                   # [inner][outer][M][N + 4]
    run_case("shared A", expect, M, N, K, batch, inner=inner, transb=False, A=(K, 0, 0, 0), D=d_lay, alpha=1.0, beta=2.0)
    run_case("shared B", expect, M, N, K, batch, inner=inner, transb=True, B=(K, 0, 0, 0), D=d_lay, alpha=-1.0, beta=0.5,
             C=_natural(M, N, inner, pad=7))


# ------------------------------------------------------------------------------------------------ alpha / beta / D
@pytest.mark.parametrize("expect,M,N,K,batch", [("t64", 64, 64, 64, 3), ("t128", 128, 128, 32, 256), ("naive", 33, 17, 40, 3)])
def test_alpha_beta_d(hip, expect, M, N, K, batch):
    run_case("D=None beta!=0", expect, M, N, K, batch, transb=True, alpha=1.0, beta=3.0)           # beta has no operand
    run_case("D aliases C", expect, M, N, K, batch, transb=False, D="alias", alpha=1.0, beta=1.0,   # in-place accumulate
             C=_natural(M, N, 1, pad=2))
    run_case("alpha=-0.5", expect, M, N, K, batch, transb=True, D=_natural(M, N, 1), alpha=-0.5, beta=1.0)
    run_case("row-broadcast D", expect, M, N, K, batch, transb=True, D=(0, 0, 0, 0), alpha=1.0, beta=1.0)   # ldd = 0: a bias


# ------------------------------------------------------------------------------------------------ validation
def test_rejected_descriptors_leave_the_output_alone(hip):
    from ddnm_amd import ops
    from ddnm_amd._lib import DDNMHipError
    A, B = torch.ones(6, 64, 32, device="cuda"), torch.ones(6, 32, 64, device="cuda")
    C = torch.full((6 * 64 * 64,), PATTERN, dtype=torch.int32).view(torch.float32).cuda()
    with pytest.raises(DDNMHipError):
        ops.bgemm(A, B, C, 64, 64, 32, lda=32, ldb=64, ldc=64, transb=False, batch=6, inner=4, sA=(64 * 32, 0),
                  sB=(32 * 64, 0), sC=(64 * 64, 0))
    with pytest.raises(DDNMHipError):
        ops.bgemm(A, B, C, 0, 64, 32, lda=32, ldb=64, ldc=64, transb=False, batch=6, sA=(64 * 32, 0), sB=(32 * 64, 0),
                  sC=(64 * 64, 0))
    torch.cuda.synchronize()
    assert bool((C.cpu().view(torch.int32) == PATTERN).all())


# ------------------------------------------------------------------------------------------------ softmax
SCALE = 0.125


def _softmax_case(n, mag, seed):
    rows, ld = 5, n + 3
    x = torch.randn(rows, n, generator=torch.Generator().manual_seed(seed)) * (mag / SCALE)
    buf = torch.full((rows * ld + GUARD,), PATTERN, dtype=torch.int32).view(torch.float32).clone()
    torch.as_strided(buf, (rows, n), (ld, 1)).copy_(x)
    window = torch.zeros(buf.numel(), dtype=torch.bool)
    torch.as_strided(window, (rows, n), (ld, 1)).fill_(True)
    return rows, ld, x, buf, window


@pytest.mark.parametrize("n", [1, 63, 65, 2048])
@pytest.mark.parametrize("mag", [3.0, 80.0])
def test_softmax_rows_edges(hip, n, mag):
    """rows = 5 (the last block of 4 rows is partial), ld = n + 3 with the padding pre-filled, logits of magnitude `mag`
    after the scale.  Reference: float64 softmax.  Bars: the 2e-6 relative L2 of tests/test_gpu_kernels.py, and elementwise
    4 x the largest error of a float32 CPU softmax of the same input against the float64 one (the kernel and the CPU differ
    in expf vs libm and in the reduction order only); rows sum to 1 within (n + 4) 2^-24 (n additions and the division)."""
    from ddnm_amd import ops
    from tests.helpers import rel
    rows, ld, x, buf, window = _softmax_case(n, mag, seed=200 + n)
    ref = torch.softmax(x.double() * SCALE, dim=1)
    cpu32 = torch.softmax(x * SCALE, dim=1)
    dev = buf.cuda()
    ops.softmax_rows_(dev, rows, n, ld, SCALE)
    torch.cuda.synchronize()
    out = dev.cpu()
    assert bool((out.view(torch.int32)[~window] == PATTERN).all()), "softmax wrote into the row padding"
    got = torch.as_strided(out, (rows, n), (ld, 1))
    assert bool(torch.isfinite(got).all())
    e_gpu, e_cpu = float((got.double() - ref).abs().max()), float((cpu32.double() - ref).abs().max())
    l2 = rel(got, ref)
    s_err = float((got.double().sum(1) - 1).abs().max())
    print(f"softmax n={n} mag={mag}: max|err| GPU {e_gpu:.3e}  CPU-fp32 {e_cpu:.3e}  rel-L2 GPU {l2:.3e}  |rowsum-1| {s_err:.3e}")
    assert s_err <= (n + 4) * M64.U32
    assert l2 < 2e-6
    assert e_gpu <= 4 * e_cpu


def test_softmax_rows_rejects_rows_longer_than_2048(hip):
    x = torch.full((2049 + GUARD,), PATTERN, dtype=torch.int32).view(torch.float32).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    assert hip.ddnm_softmax_rows_f32(x.data_ptr(), 1, 2049, 2049, 1.0, stream) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((x.cpu().view(torch.int32) == PATTERN).all())
