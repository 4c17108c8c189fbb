"""A convolution whose plan splits K runs unsplit when the caller brings no scratch (csrc/conv_common.h::conv_run_ksplit),
and refuses when it is to emit statistics without scratch.  ops.conv2d always supplies the scratch, so the launchers are
called here directly, on the descriptor ops.conv2d built: B = 1, 16 x 16, Cin = Cout = 128, the smallest shape whose
plan splits -- except in the 1x1 GEMM family, whose K chunks are 64 channels and whose plan wants two chunks per slice:
there Cin = 256 is the smallest that splits (at 128 the workspace query returns 0).  Tolerances: the ones
tests/test_gpu_kernels.py, tests/test_gpu_adm.py (fp16 operands, 2e-3) and tests/test_gpu_s16.py (split-fp16 forms, 8e-7)
apply to the family against the unrounded reference."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, H, C = 1, 16, 128
#          family: (launcher, workspace query, weights ops.conv2d is given, ksize, Cin, tolerance)
FAMILIES = {
    "f32": ("ddnm_conv2d_f32", "ddnm_conv2d_f32_workspace_floats", None, 3, C, 3e-6),
    "f16": ("ddnm_conv3x3_f16_f32", "ddnm_conv3x3_f16_workspace_floats", "f16", 3, C, 2e-3),
    "s16": ("ddnm_conv3x3_s16_f32", "ddnm_conv3x3_s16_workspace_floats", "s16", 3, C, 8e-7),
    "gather_s16": ("ddnm_conv_gather_s16_f32", "ddnm_conv_gather_s16_workspace_floats", "s16", 3, C, 8e-7),
    "1x1_f16": ("ddnm_conv1x1_f16_f32", "ddnm_conv1x1_f16_workspace_floats", "f16", 1, 2 * C, 2e-3),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_split_plan_without_scratch_runs_unsplit(hip, family, monkeypatch):
    from ddnm_amd import ops
    launcher, ws_query, kind, k, cin, tol = FAMILIES[family]
    g = torch.Generator(device="cuda").manual_seed(5)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    a, w, bias = rn(B, H, H, cin) * 1.5, rn(C, cin, k, k) / (k * cin ** 0.5), rn(C)
    gn = None if k == 1 else (rn(B, cin) * 0.3 + 1.0, rn(B, cin) * 0.3)      # (the 1x1 GEMM has no GroupNorm prologue)
    x = a.double()
    if gn is not None:
        x = x * gn[0].double()[:, None, None, :] + gn[1].double()[:, None, None, :]
        x = x * torch.sigmoid(x)
    ref = F.conv2d(x.permute(0, 3, 1, 2), w.double(), bias.double(), padding=k // 2).permute(0, 2, 3, 1)

    # the descriptor as ops.conv2d builds it: the launch is intercepted, the launcher is chosen here
    built = []
    monkeypatch.setattr(ops, "_launch", lambda fn, d, label, record: built.append(d))
    scale = ops.s16_weight_scale(w)
    w32, w16 = ops.pack_conv_weight(w), ops.pack_conv_weight_f16(w)      # (named: the descriptor holds their addresses)
    ws16 = (ops.pack_conv_weight_s16(w, scale), scale, None) if k == 3 else None
    ops.conv2d(a, w32, C, k, bias=bias, gn=gn, gn_silu=True, weight_f16=w16 if kind == "f16" else None,
               weight_s16=ws16 if kind == "s16" else None)
    (d,) = built
    need = getattr(hip, ws_query)(ctypes.byref(d))
    assert need > 0, "the case must split K"
    run = getattr(hip, launcher)
    ws = torch.empty(need, dtype=torch.float32, device="cuda")
    outs = {}
    for scratch in (True, False):
        out = torch.full((B, H, H, C), float("nan"), device="cuda")
        d.out, d.stats_out = out.data_ptr(), None
        d.workspace, d.workspace_floats = (ws.data_ptr(), need) if scratch else (None, 0)
        assert run(ctypes.byref(d), ops._stream()) == 0
        outs[scratch] = out
    for scratch, out in outs.items():
        err = ((out.double() - ref).norm() / ref.norm()).item()
        print(f"{family}: scratch={scratch} rel-L2 vs fp64 {err:.3e} (tolerance {tol:g})")
        assert err < tol, (family, scratch, err)
    # statistics were sized for the split plan: without scratch the launch is refused, not run unsplit
    stats = torch.empty(B * H * H * C * 2, dtype=torch.float32, device="cuda")
    d.stats_out, d.workspace, d.workspace_floats = stats.data_ptr(), None, 0
    assert run(ctypes.byref(d), ops._stream()) == -1
    del w32, w16, ws16
