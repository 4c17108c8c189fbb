#!/usr/bin/env python
"""Host-only dry run of an engine path (development tool, no GPU): the real shared library is loaded, its PLANNING entry
points (`*_supported`, `*_stats_tiles`, `*_workspace_floats`, `ddnm_gn_nchunk`, ...) run as usual -- they are host code --
and every LAUNCHING entry point (last argument = stream) is replaced by a stub that returns 0.  Tensors live on the CPU
and hold garbage; what is exercised is the Python plumbing: shapes, dtypes, descriptor marshalling, workspace sizes,
dictionary keys.  Usage:  python tools/dry_run.py [classifier|adm|celeba] ...
"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddnm_amd import _lib, ops  # noqa: E402

HOST_ONLY = ("_supported", "_stats_tiles", "_workspace_floats", "_nchunk", "_tile_n", "_fuses_skip", "_fuses_fin",
             "_persistent", "_act_scale", "ddnm_version", "ddnm_error_string", "ddnm_build_digest", "ddnm_sizeof",
             "ddnm_chroma_constants", "ddnm_jpeg_quality_tables")


class DryLib:
    def __init__(self, real):
        self._real = real
        self.calls = {}
        self.on_launch = None      # optional hook(name, args) of every launching call (tools/record_launch_trace.py)
        self.real = ()             # launching entry points that run for real: descriptors they REFUSE (no launch follows)

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if any(name.endswith(s) or name == s for s in HOST_ONLY):
            return fn
        if name in self.real:
            def refuse(*args):
                if self.on_launch is not None:
                    self.on_launch(name, args)
                code = fn(*args)
                assert code < 0, f"{name}: expected a refusal, got {code}"
                return code
            return refuse

        def stub(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            if self.on_launch is not None:
                self.on_launch(name, args)
            res, argtypes = _lib.PROTOTYPES[name]
            assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for {len(argtypes)} parameters"
            for a, t in zip(args, argtypes):      # what ctypes would reject at call time
                if t in (ctypes.c_int32, ctypes.c_int64):
                    assert isinstance(a, int), f"{name}: {a!r} passed for an integer parameter"
                elif t is ctypes.c_float:
                    assert isinstance(a, (int, float)), f"{name}: {a!r} passed for a float parameter"
            return 0
        return stub


def install():
    real = _lib.lib()
    dry = DryLib(real)
    _lib._lib = dry
    ops._stream = lambda: 0
    ok = lambda t, name: t          # noqa: E731
    f32c, f16c = ops._f32c, ops._f16c

    def f32(t, name):
        assert t.dtype == torch.float32 and t.is_contiguous(), (name, t.dtype, t.is_contiguous())
        return t

    def f16(t, name):
        assert t.dtype == torch.float16 and t.is_contiguous(), (name, t.dtype, t.is_contiguous())
        return t
    ops._f32c, ops._f16c = f32, f16
    del ok, f32c, f16c
    return dry


def make_classifier(size=256, kind="h16"):
    from ddnm_amd.guided_diffusion.classifier import classifier_defaults, create_classifier
    kw = classifier_defaults()
    kw["image_size"] = size
    clf = create_classifier(**kw)
    clf.device = torch.device("cpu")
    g = torch.Generator().manual_seed(1)
    clf.load_state_dict({k: torch.randn(v, generator=g) * 0.05 for k, v in clf.state_dict_shapes().items()})
    if kind != "fp32":
        os.environ["DDNM_CLS_GEN1"] = "1" if kind == "gen1" else "0"
        clf.convert_to_fp16()
    return clf


def classifier_pass(clf, B=2, size=256):
    """One logits pass and one gradient pass (make_cond_fn) of `clf`."""
    from ddnm_amd.guided_diffusion.classifier import make_cond_fn
    x = torch.randn(B, 3, size, size)
    t = torch.full((B,), 500.0)
    y = torch.full((B,), 951, dtype=torch.long)
    logits = clf(x, t)
    assert logits.shape == (B, 1000)
    grad = make_cond_fn(clf, 1.0)(x, t, y)
    assert grad.shape == x.shape and grad.dtype == torch.float32, (grad.shape, grad.dtype)


def classifier(B=2, size=256, kind="h16"):
    clf = make_classifier(size, kind)
    classifier_pass(clf, B, size)
    return clf


def stub_device_queries():
    """What the networks and ops.conv2d ask of a device beyond the library: the current stream, the operand bound."""
    import types
    torch.cuda.current_stream = lambda *a: types.SimpleNamespace(cuda_stream=0)      # (the networks key their scratch on it)
    ops.amax_bound = lambda a0, a1=None: torch.empty(ops.tensor_of(a0).shape[0] * ops.AMAX_N)      # (a launch: stubbed anyway)


def engine_modes(batches, mfma32=False):
    """The eight engine modes of profiles/host_scaffold_launch_lists.md, each at every batch size of `batches`, as
    (name, network, run) with `run()` = one pass; `mfma32` adds the celeba `Model` on the all-fp32 engine.  Call install()
    first.  Shared by tools/record_conv_plans.py and tools/record_launch_trace.py."""
    import bench
    from ddnm_amd.guided_diffusion.models import Model
    from ddnm_amd.guided_diffusion.unet import create_model
    stub_device_queries()

    def forward(net, B):
        return lambda: net(torch.empty(B, 3, 256, 256), torch.full((B,), 500.0))
    for name, kw in [("celeba", {})] + ([("celeba_mfma32", {"split16": False})] if mfma32 else []):
        cel = Model(bench.make_config(), device="cpu", **kw)
        cel.load_state_dict(cel.random_state_dict(1234))
        for B in batches:
            yield f"{name}_b{B}", cel, forward(cel, B)
    for kind in ("fp32", "h16", "gen1"):
        os.environ["DDNM_ADM_GEN1"] = "1" if kind == "gen1" else "0"
        adm = create_model(image_size=256, num_channels=256, num_res_blocks=2, attention_resolutions="32,16,8",
                           num_head_channels=64, learn_sigma=True, use_scale_shift_norm=True, resblock_updown=True)
        adm.device = torch.device("cpu")
        adm.load_state_dict(adm.random_state_dict(1))
        if kind != "fp32":
            adm.convert_to_fp16()
        for B in batches:
            yield f"adm_{kind}_b{B}", adm, forward(adm, B)
    for kind in ("fp32", "h16", "gen1"):
        for B in batches:
            clf = make_classifier(256, kind)
            yield f"cls_{kind}_b{B}", clf, lambda: classifier_pass(clf, B, 256)


if __name__ == "__main__":
    dry = install()
    what = sys.argv[1] if len(sys.argv) > 1 else "classifier"
    if what == "classifier":
        for kind in ("h16", "gen1", "fp32"):
            for size, B in ((256, 2), (64, 3), (256, 32)):
                dry.calls.clear()
                classifier(B=B, size=size, kind=kind)
                n = sum(dry.calls.values())
                print(f"classifier {kind} {size}px B={B}: {n} launches; " +
                      ", ".join(f"{k.replace('ddnm_', '')} x{v}" for k, v in sorted(dry.calls.items(), key=lambda kv: -kv[1])[:8]))
