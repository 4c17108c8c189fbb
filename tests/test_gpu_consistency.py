"""The data-consistency kernel (ddnm_consistency_f32, ops.consistency) on the GPU against float64 torch on the same
tensors: row lengths around the per-workgroup element count, padded and misaligned rows, valid-entry counts, the
bit-identity of the 16-byte and the element-wise path and of a row alone and inside a batch, and the error codes.

The bounds are derived, not measured: every term |d| and d^2 is formed from the exact fp64 difference of two fp32 values,
so kernel and reference add the same m non-negative terms in different orders, each order within (m - 1) * 2^-53 relative
of the true sum: |got - want| <= m * 2^-52 * want.  The maximum has no rounding but the final one to fp32: equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ELEMS = 2048        # entries of a row per workgroup (csrc/metrics.hip::CONS_ELEMS)
E_BADARG, E_SHAPE = -1, -2


def operands(B, m, seed, row_stride=None, offset=0, pad=float("nan")):
    """Two [B, m] views (row stride `row_stride`, first element `offset` floats into a fresh allocation) of random values:
    y ~ N(0, 1), ax = y + a residual that is 1e-5 N(0, 1) on most entries, O(1) on every 97th and exactly 0 on every
    5th.  Everything outside the views holds `pad`."""
    row_stride = m if row_stride is None else row_stride
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, m, generator=g)
    r = 1e-5 * torch.randn(B, m, generator=g)
    r[:, ::97] = torch.randn(B, (m + 96) // 97, generator=g)
    r[:, ::5] = 0.0
    ax = y + r
    bufs = []
    for t in (ax, y):
        buf = torch.full((B * row_stride + offset + 4,), pad, dtype=torch.float32, device="cuda")
        view = buf[offset:offset + B * row_stride].view(B, row_stride)[:, :m]
        view.copy_(t)
        bufs.append((buf, view))
    return bufs[0][1], bufs[1][1]


def raw(ax, y, counts=None, B=None, m=None, row_stride=None, work_elems=None, null=()):
    """ddnm_consistency_f32 itself on (views of) device tensors; returns (code, l1, sse, maxabs), the outputs prefilled
    with -7 so that a refused call shows it launched nothing.  `null`: names of pointers passed as NULL."""
    from ddnm_amd import _lib
    lib = _lib.lib()
    B = ax.shape[0] if B is None else B
    m = ax.shape[1] if m is None else m
    row_stride = ax.stride(0) if row_stride is None else row_stride
    n = int(lib.ddnm_consistency_workspace_elems(max(B, 1), max(m, 1)))
    assert n == 3 * max(B, 1) * ((max(m, 1) + ELEMS - 1) // ELEMS)
    nb = max(B, 1)
    l1 = torch.full((nb,), -7.0, dtype=torch.float64, device="cuda")
    sse = torch.full((nb,), -7.0, dtype=torch.float64, device="cuda")
    mx = torch.full((nb,), -7.0, dtype=torch.float32, device="cuda")
    work = torch.zeros(n, dtype=torch.float64, device="cuda")
    ptr = dict(ax=ax.data_ptr(), y=y.data_ptr(), l1=l1.data_ptr(), sse=sse.data_ptr(), maxabs=mx.data_ptr(),
               work=work.data_ptr())
    for name in null:
        ptr[name] = None
    cp = counts if counts is None or isinstance(counts, int) else counts.data_ptr()
    code = lib.ddnm_consistency_f32(ptr["ax"], ptr["y"], row_stride, cp, ptr["l1"], ptr["sse"], ptr["maxabs"], ptr["work"],
                                    n if work_elems is None else work_elems, B, m, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code, l1, sse, mx


def reference(ax, y, counts=None):
    """float64 torch on the same tensors: (l1, sse, maxabs as fp32) over the first counts[b] entries of row b."""
    d = ax.double() - y.double()
    if counts is not None:
        keep = torch.arange(ax.shape[1], device=ax.device)[None, :] < torch.as_tensor(counts, device=ax.device)[:, None]
        d = torch.where(keep, d, torch.zeros_like(d))
    return d.abs().sum(1), (d * d).sum(1), d.abs().max(1).values.float()


def check_against_reference(got, want, m, what):
    (l1, sse, mx), (l1_w, sse_w, mx_w) = got, want
    bound = m * 2.0 ** -52
    for name, g, w in (("l1", l1, l1_w), ("sse", sse, sse_w)):
        err = ((g - w).abs() / w.clamp_min(1e-300)).max().item() if bool((w > 0).any()) else float((g - w).abs().max())
        print(f"consistency {what}: {name} relative error {err:.3e} (bound {bound:.3e})")
        assert bool(((g - w).abs() <= bound * w).all()), (what, name, err)
    assert torch.equal(mx, mx_w), what


SHAPES = [(1, 1), (2, 3), (3, ELEMS - 1), (3, ELEMS), (3, ELEMS + 1), (2, 3 * ELEMS + 5)]


@pytest.mark.parametrize("B,m", SHAPES)
def test_kernel_matches_float64_torch(hip, B, m):
    """m = 1; m = 3 with a misaligned second row; one below, at and above one workgroup's entries; three workgroups' worth
    plus 5 -- each contiguous (vector path where row_stride % 4 == 0), with row_stride = m + 3, and offset by one float
    (element-wise path).  The three layouts hold the same values and must give the same bits."""
    from ddnm_amd import ops
    results = {}
    for layout, kw in (("contiguous", {}), ("padded", dict(row_stride=m + 3)), ("offset", dict(offset=1)),
                       ("aligned", dict(row_stride=4 * ((m + 3) // 4)))):
        ax, y = operands(B, m, seed=7 * m + B, **kw)
        assert ax.stride(0) == kw.get("row_stride", m) and (ax.data_ptr() % 16 == 0) == ("offset" not in kw)
        code, l1, sse, mx = raw(ax, y)
        assert code == 0, layout
        assert bool(torch.isfinite(l1).all()) and bool(torch.isfinite(sse).all())       # the NaN around the rows is not read
        check_against_reference((l1, sse, mx), reference(ax, y), m, f"B={B} m={m} {layout}")
        results[layout] = (l1, sse, mx)
    # "aligned" always takes the 16-byte path, "offset" never: same entries, same thread, same order -> same bits
    for layout in ("contiguous", "padded", "offset"):
        for a, b in zip(results[layout], results["aligned"]):
            assert torch.equal(a, b), layout
    ax, y = operands(B, m, seed=7 * m + B)
    l1, sse, mx = ops.consistency(ax.contiguous(), y.contiguous())
    assert (l1.dtype, sse.dtype, mx.dtype) == (torch.float64, torch.float64, torch.float32) and l1.shape == (B,)
    for a, b in zip((l1, sse, mx), results["aligned"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("m", [3, ELEMS + 1, 3 * ELEMS + 5])
def test_counts_keep_the_padding_out(hip, m):
    """counts below m: the entries at and beyond counts[b] are NaN in both operands and must not reach the outputs;
    counts[b] = 0 gives three zeros; counts that are no multiple of 4 end a row inside a 16-byte group."""
    from ddnm_amd import ops
    B = 4
    counts = [m, max(m - 3, 1), 0, (2 * m) // 3]
    for kw in ({}, dict(row_stride=4 * ((m + 3) // 4)), dict(offset=1)):
        ax, y = operands(B, m, seed=m, **kw)
        for b, n in enumerate(counts):
            ax[b, n:] = float("nan")
            y[b, n:] = float("nan")
        c = torch.tensor(counts, dtype=torch.int32, device="cuda")
        code, l1, sse, mx = raw(ax, y, counts=c)
        assert code == 0
        assert bool(torch.isfinite(l1).all()) and bool(torch.isfinite(sse).all()) and bool(torch.isfinite(mx).all())
        assert float(l1[2]) == 0.0 and float(sse[2]) == 0.0 and float(mx[2]) == 0.0
        clean_ax, clean_y = torch.nan_to_num(ax, nan=0.0), torch.nan_to_num(y, nan=0.0)
        check_against_reference((l1, sse, mx), reference(clean_ax, clean_y, counts), m, f"counts m={m} {kw}")
        if not kw:
            got = ops.consistency(ax.contiguous(), y.contiguous(), counts)
            again = ops.consistency(ax.contiguous(), y.contiguous(), c)
            for a, b, d in zip(got, again, (l1, sse, mx)):
                assert torch.equal(a, d) and torch.equal(b, d)
    # a row's valid prefix gives the same bits whatever lies behind it, with and without counts in its batch
    ax, y = operands(1, m, seed=m + 1)
    n = (2 * m) // 3
    if n:
        _, l1_a, sse_a, mx_a = raw(ax, y, counts=torch.tensor([n], dtype=torch.int32, device="cuda"))
        ax[0, n:], y[0, n:] = 0.0, 0.0
        _, l1_b, sse_b, mx_b = raw(ax, y)
        assert torch.equal(l1_a, l1_b) and torch.equal(sse_a, sse_b) and torch.equal(mx_a, mx_b)


@pytest.mark.parametrize("m", [5, ELEMS + 1, 3 * ELEMS + 5])
def test_a_row_is_bit_identical_alone_and_in_a_batch(hip, m):
    ax1, y1 = operands(1, m, seed=3 * m)
    code, l1, sse, mx = raw(ax1, y1)
    assert code == 0 and float(l1[0]) > 0
    for row in range(3):
        ax, y = operands(3, m, seed=3 * m + 1 + row)
        ax[row], y[row] = ax1[0], y1[0]
        code, l1_b, sse_b, mx_b = raw(ax, y)
        assert code == 0
        assert torch.equal(l1_b[row], l1[0]) and torch.equal(sse_b[row], sse[0]) and torch.equal(mx_b[row], mx[0]), row


def test_equal_operands_give_exact_zeros(hip):
    for m in (1, 1000, ELEMS + 7):
        ax, _ = operands(3, m, seed=m)
        code, l1, sse, mx = raw(ax, ax.clone())
        assert code == 0
        assert bool((l1 == 0).all()) and bool((sse == 0).all()) and bool((mx == 0).all())


def test_every_documented_error_code(hip):
    """BADARG: a NULL operand, output or workspace, B < 1, m < 1, row_stride < m, counts in pageable host memory.
    SHAPE: a short workspace, a count outside [0, m] in memory the host can read (pinned), more than 2^31 - 1
    workgroups.  A refused call launches nothing: the outputs keep their fill."""
    from ddnm_amd import _lib, ops
    lib = _lib.lib()
    ax, y = operands(2, 100, seed=1, pad=0.0)

    def refused(code, want, *outs):
        assert code == want
        with pytest.raises(_lib.DDNMHipError):
            _lib.check(code, "ddnm_consistency_f32")
        return all(bool((o == -7.0).all()) for o in outs)

    for name in ("ax", "y", "l1", "sse", "maxabs", "work"):
        code, *outs = raw(ax, y, null=(name,))
        assert refused(code, E_BADARG, *outs), name
    for kw in (dict(B=0), dict(B=-1), dict(m=0), dict(m=-5), dict(row_stride=99)):
        code, *outs = raw(ax, y, **kw)
        assert refused(code, E_BADARG, *outs), kw
    code, *outs = raw(ax, y, work_elems=5)                                      # needs 6
    assert refused(code, E_SHAPE, *outs)
    for bad in ([101, 3], [3, -1]):
        pinned = torch.tensor(bad, dtype=torch.int32).pin_memory()
        code, *outs = raw(ax, y, counts=pinned)
        assert refused(code, E_SHAPE, *outs), bad
    host = np.array([3, 4], dtype=np.int32)                                    # pageable: the kernel could not read it
    code, *outs = raw(ax, y, counts=int(host.ctypes.data))
    assert refused(code, E_BADARG, *outs)
    assert lib.ddnm_consistency_workspace_elems(0, 64) == E_BADARG
    assert lib.ddnm_consistency_workspace_elems(2, 0) == E_BADARG
    assert lib.ddnm_consistency_workspace_elems(2 ** 21, 2 ** 33) == E_SHAPE    # 2^43 workgroups: no such grid
    assert lib.ddnm_consistency_workspace_elems(1, 2 ** 43) == E_SHAPE
    assert lib.ddnm_consistency_workspace_elems(2, 100) == 6
    torch.cuda.synchronize()
    # the Python entry point says the same before any launch
    for bad in ([101, 3], [3, -1], [3]):
        with pytest.raises(ValueError, match="counts"):
            ops.consistency(ax.contiguous(), y.contiguous(), bad)
    with pytest.raises(ValueError, match="consistency"):
        ops.consistency(ax.contiguous(), y.contiguous()[:, :50])
