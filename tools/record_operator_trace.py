#!/usr/bin/env python
"""Records what the degradation operators LAUNCH, for tests/test_operator_trace.py (development tool, no GPU needed).
Sibling of tools/record_launch_trace.py, whose `Tracer` row format it reuses (entry point, every scalar argument and
descriptor field, floats as bit patterns, one row per launching call, distinct rows stored once).  Usage, on a checkout
of the commit whose behaviour is to be pinned:

    python tools/record_operator_trace.py | gzip -9n > tests/golden/operator_trace.json.gz

(`--replay`, what tests/test_operator_trace.py passes: the same output without asking git where it was recorded.)

Under tools/dry_run.py the operators of ddnm_amd/functions/svd_operators.py run on CPU tensors and every launching entry
point is a stub.  A CASE is one method call (or a short sequence: begin_run + step, begin_plus_run + step) on one
operator, recorded as its rows, the exception (type, message) where it raises, and what it returned (shape and dtype of a
tensor: `singulars` launches nothing; class and length of an operator).  Image size 64, batch 2 (batch 1 once per
operator, for `A`): the smallest size every operator accepts (CS: a multiple of 32 with several patches per side,
Walsh-Hadamard: a power of two, sr_bicubic x4: a 16 x 16 measurement).

Pointer labels, resolved AFTER the call (every tensor whose address went into a launch is kept alive until then, so no
address is seen twice within a case): `arg:<name>` for a tensor the case passed in (a KeyedPhiloxNoise's key table:
`arg:noise`), `ret` for the returned tensor, `const<k>:<shape>:<dtype>` for the operator's own tensors -- whatever is
reachable from vars(op) through dicts, tuples and lists (operators among them: a Composition's parts), numbered by first
use within the case, so that renaming a private cache does not change a row -- with a content hash behind the integer
tables (rank tables, index tables, `perm`), 0 for NULL, `x` for anything else (`+<bytes>`: an address inside).

The table replays on another x86 host: float tables are not hashed, and nothing in a row depends on LAPACK's last bits --
`torch.svd` is wrapped for this process so that its factors are rounded to a grid of 2^-10 and the sign of every
left-singular vector is fixed by its first entry (launches are stubs, accuracy is immaterial; the scalars that come out
of a host SVD -- the `s` of a 1 x n measurement row that ends up in lambda, d1, d2, and U[0, 0] -- are then the same
everywhere).  The global generator is seeded before `CS` draws its Gaussian matrix, and `perm` is passed explicitly.
`KeyedPhiloxNoise.table()` asks torch.cuda.current_device() for a CPU device: stubbed like the current stream.

`GeneralA` is NOT in the trace: its constructor moves a CPU matrix to "cuda".  Its guard are the GeneralA cases of
tests/test_gpu_kernels.py.  What a trace cannot see is the data flow between temporaries (which scratch buffer feeds
which launch); the GPU tests of the operators hold that.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dry_run  # noqa: E402
import record_launch_trace as rlt  # noqa: E402
from ddnm_amd import ops  # noqa: E402
from ddnm_amd.functions import svd_operators as E  # noqa: E402

D, B = 64, 2
A_COEF, ETA = 0.8, 0.85
POINTS = {"below": (0.2, 0.05), "above": (0.2, 0.9), "sigma_y_0": (0.0, 0.5)}       # (sigma_y, sigma_t)
SURFACE = ("A_pinv", "V", "Vt", "U", "Ut", "add_zeros", "At", "A_pinv_eta")
NOISES = ("tensor", "philox", "keyed")
ERRORS = (ValueError, NotImplementedError, RuntimeError, TypeError, AttributeError, AssertionError)


def _span(t):
    st = t.untyped_storage()
    return t.data_ptr(), st.data_ptr() + st.nbytes()


def _tensors(obj, seen):
    """Every tensor reachable from vars(obj) through dicts, tuples, lists and operators."""
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors(v, seen)
    elif isinstance(obj, (tuple, list)):
        for v in obj:
            yield from _tensors(v, seen)
    elif isinstance(obj, (E.A_functions, E.InpaintingBank, ops.KeyedPhiloxNoise)) and id(obj) not in seen:
        seen.add(id(obj))
        yield from _tensors(vars(obj), seen)


class OperatorTracer(rlt.Tracer):
    """rlt.Tracer whose pointer labels are resolved after the call (`take`)."""

    def label(self, p):
        return ("@", p) if p else 0

    def take(self, op, fn, args):
        """(rows, [type, message] or None, description of what fn() returned)."""
        self.rows, kept, err, ret = [], [], None, None
        saved = ops._p, getattr(E, "_p", None)

        def p(t):
            kept.append(t)
            return saved[0](t)
        ops._p = p
        if saved[1] is not None:
            E._p = p
        try:
            ret = fn()
        except ERRORS as e:
            err = [type(e).__name__, str(e)]
        finally:
            ops._p = saved[0]
            if saved[1] is not None:
                E._p = saved[1]
        named = [(f"arg:{k}", t) for k, v in args.items() for t in _tensors(v, set())]
        if isinstance(ret, torch.Tensor):
            named.append(("ret", ret))
        consts, numbers = list(_tensors(op, set())) if op is not None else [], {}

        def inside(t, addr):
            lo, hi = _span(t)
            return lo <= addr < hi

        def resolve(addr):
            for name, t in named:
                if inside(t, addr):
                    return name + (f"+{addr - t.data_ptr()}" if addr != t.data_ptr() else "")
            for t in [t for t in consts if t.data_ptr() == addr] + consts:      # the tensor itself before one that holds it
                if inside(t, addr):
                    key = t.data_ptr()
                    if key not in numbers:
                        lab = f"const{len(numbers)}:{json.dumps(list(t.shape), separators=(',', ':'))}:{_dtype(t)}"
                        if not t.dtype.is_floating_point:
                            lab += ":" + hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()[:12]
                        numbers[key] = lab
                    return numbers[key] + (f"+{addr - key}" if addr != key else "")
            return "x"

        def walk(v):
            if isinstance(v, tuple) and len(v) == 2 and v[0] == "@":
                return resolve(v[1])
            return [walk(e) for e in v] if isinstance(v, list) else v
        rows = [walk(r) for r in self.rows]
        del kept
        return rows, err, _describe(ret)


def _dtype(t):
    return {torch.float32: "f32", torch.int32: "i32", torch.int64: "i64", torch.float64: "f64"}.get(t.dtype, str(t.dtype))


def _describe(ret):
    if isinstance(ret, torch.Tensor):
        return [list(ret.shape), _dtype(ret)]
    if isinstance(ret, (E.A_functions, E.InpaintingBank)):
        return [type(ret).__name__, len(ret) if hasattr(ret, "__len__") else None]
    return None if ret is None else repr(ret)


def install():
    """(dry library, tracer) with the device queries stubbed and torch.svd made reproducible (module docstring)."""
    dry = dry_run.install()
    dry_run.stub_device_queries()
    torch.cuda.current_device = lambda: 0
    dry.on_launch = OperatorTracer()
    svd = torch.svd

    def coarse_svd(a, some=True, compute_uv=True):
        U, S, V = svd(a, some=some, compute_uv=compute_uv)
        k = S.shape[-1]
        sign = torch.where(U[0, :k] < 0, -1.0, 1.0)
        U, V = U.clone(), V.clone()
        U[:, :k] *= sign
        V[:, :k] *= sign
        return tuple(torch.round(t * 1024) / 1024 for t in (U, S, V))
    torch.svd = coarse_svd
    return dry, dry.on_launch


# ------------------------------------------------------------------------------------------------ inputs
def _config(channels=3, size=D):
    return types.SimpleNamespace(data=types.SimpleNamespace(channels=channels, image_size=size))


def _mask2d(k=0):
    """0 = missing: a rectangular hole whose size depends on k (the masks of a bank keep different pixel counts)."""
    m = np.ones((D, D), dtype=np.float32)
    m[8 + k:40, 16:48 - 3 * k] = 0
    return m


def _missing(mask):
    r = torch.nonzero(torch.from_numpy(mask).reshape(-1) == 0).long().reshape(-1) * 3
    return torch.cat([r, r + 1, r + 2], dim=0)


def _ysize(op):
    return op.y_dim if isinstance(op, E.PerImageInpainting) else op.measurement_size()


def _spectral_size(op):
    return op.channels * op.img_dim ** 2


def _scalars():
    return ops.step_scalars(torch.tensor(0.5), torch.tensor(0.6), ETA)


def _et(b, c, view):
    return torch.zeros(b, 2 * c, D, D)[:, :c] if view else torch.zeros(b, c, D, D)


def _noise(kind, s, b, c):
    if kind == "tensor":
        return torch.zeros(b, c, D, D)
    if kind == "philox":
        return ops.PhiloxNoise(1234, image_base=3).kernel_arg(s, 7)
    return ops.KeyedPhiloxNoise([11 + i for i in range(b)], [5 + i for i in range(b)]).kernel_arg(s, 7)


# ------------------------------------------------------------------------------------------------ cases
def operators(tmp):
    """[(name, constructor)]: every --deg of build_operator, the simplified path's operators, SuperResolution variants."""
    from ddnm_amd.guided_diffusion.diffusion import Diffusion

    def mask_file(name, arr):
        path = os.path.join(name, "exp", "inp_masks", "mask.npy")          # relative: a message may quote it
        os.makedirs(os.path.join(tmp, os.path.dirname(path)), exist_ok=True)
        np.save(os.path.join(tmp, path), arr)
        return path
    m2 = mask_file("m2", _mask2d())
    m3 = mask_file("m3", np.stack([_mask2d(k) for k in range(3)]))
    m1 = mask_file("m1", np.ones(D * D, dtype=np.float32))
    perm = torch.arange(D * D - 1, -1, -1)

    def build(deg, scale, **kw):
        def make():
            torch.manual_seed(0)
            cwd = os.getcwd()
            os.chdir(tmp)
            try:
                return E.build_operator(deg, scale, _config(), "cpu", **kw)
            finally:
                os.chdir(cwd)
        return make

    def simplified(deg, where, scale=4.0):
        def make():
            cwd = os.getcwd()
            os.chdir(os.path.join(tmp, where.split(os.sep)[0]))                # it reads exp/inp_masks/mask.npy of the run directory
            try:
                me = types.SimpleNamespace(args=types.SimpleNamespace(deg=deg, deg_scale=scale), config=_config(),
                                           device="cpu")
                return Diffusion._simplified_operator(me)
            finally:
                os.chdir(cwd)
        return make
    return [
        ("sr_bicubic", build("sr_bicubic", 4)), ("deblur_aniso", build("deblur_aniso", 0)),
        ("deblur_gauss", build("deblur_gauss", 0)), ("deblur_uni", build("deblur_uni", 0)),
        ("sr_averagepooling", build("sr_averagepooling", 4)), ("colorization", build("colorization", 0)),
        ("denoising", build("denoising", 0)), ("cs_blockbased", build("cs_blockbased", 0.25)),
        ("cs_walshhadamard", build("cs_walshhadamard", 0.25, perm=perm)),
        ("inpainting", build("inpainting", 0, mask_path=m2)), ("inpainting_bank", build("inpainting", 0, mask_path=m3)),
        ("inpainting_1d_mask_file", build("inpainting", 0, mask_path=m1)),
        ("simplified_colorization", simplified("colorization", m2)), ("simplified_inpainting", simplified("inpainting", m2)),
        ("simplified_inpainting_bank", simplified("inpainting", m3)), ("simplified_mask_color_sr", simplified("mask_color_sr", m2)),
        ("pixel_mask", lambda: E.PixelMask(3, D, torch.from_numpy(_mask2d()), "cpu")),
        ("sr_ratio8", lambda: E.SuperResolution(3, D, 8, "cpu")), ("sr_ratio2", lambda: E.SuperResolution(3, D, 2, "cpu")),
        ("sr_channels1", lambda: E.SuperResolution(1, D, 4, "cpu")),
        ("inpainting_channels1", lambda: E.Inpainting(1, D, _missing(_mask2d()), "cpu")),
        ("inpainting_bank_channels1", lambda: E.InpaintingBank(1, D, np.stack([_mask2d()]), "cpu")),
        ("inpainting_per_channel_mask", lambda: E.Inpainting(3, D, torch.tensor([0]), "cpu")),
        ("cs_size_48", lambda: E.CS(3, 48, 0.25, "cpu")),
    ]


def _call(op, method, **args):
    """One case: (operator that names the constants, thunk, arguments)."""
    return op, (lambda: getattr(op, method)(*args.values())), args


def step_case(op, kind, view, b=B, y=None, begin=False, et=None):
    c = op.channels
    s = _scalars()
    args = dict(xt=torch.zeros(b, c, D, D), et=_et(b, c, view) if et is None else et, noise=_noise(kind, s, b, c),
                y=torch.zeros(b, _ysize(op)) if y is None else y, x0_out=torch.zeros(b, c, D, D),
                xt_next=torch.zeros(b, c, D, D))

    def run():
        if begin:
            op.begin_run(args["y"])
        op.ddnm_step(args["xt"], args["et"], args["noise"], args["y"], s, args["x0_out"], args["xt_next"])
    return op, run, args


def plus_case(op, kind, view, begin_b=B, b=B, ylen=None, begin=True):
    c = op.channels
    s = _scalars()
    args = dict(y=torch.zeros(begin_b, _ysize(op) if ylen is None else ylen), xt=torch.zeros(b, c, D, D),
                et=_et(b, c, view), noise=_noise(kind, s, b, c), x0_out=torch.zeros(b, c, D, D),
                xt_next=torch.zeros(b, c, D, D))

    def run():
        if begin:
            op.begin_plus_run(args["y"])
        op.ddnm_plus_step(args["xt"], args["et"], args["noise"], s, 0.2, 0.3, ETA, args["x0_out"], args["xt_next"])
    return op, run, args


def operator_cases(name, op):
    """[(case name, (operator, thunk, arguments))] of one operator: every method of the surface, Lambda / Lambda_noise at the
    three coefficient points, ddnm_step with every noise kind and et layout, the DDNM+ hook where the class has one."""
    img = lambda b=B: torch.zeros(b, op.channels, D, D)                  # noqa: E731
    y = lambda b=B: torch.zeros(b, _ysize(op))                           # noqa: E731
    spec = lambda b=B: torch.zeros(b, _spectral_size(op))                # noqa: E731
    inputs = {"A_pinv": y, "V": spec, "Vt": img, "U": y, "Ut": y, "add_zeros": y, "At": y}
    out = [("A", _call(op, "A", vec=img())), ("A_b1", _call(op, "A", vec=img(1)))]
    out += [(m, _call(op, m, vec=inputs[m]())) for m in SURFACE if m != "A_pinv_eta"]
    out += [("A_pinv_eta", _call(op, "A_pinv_eta", vec=y(), eta=0.5)), ("singulars", _call(op, "singulars"))]
    for point, (sigma_y, sigma_t) in POINTS.items():
        out.append((f"Lambda_{point}", _call(op, "Lambda", vec=spec(), a=A_COEF, sigma_y=sigma_y, sigma_t=sigma_t, eta=ETA)))
        out.append((f"Lambda_noise_{point}", _call(op, "Lambda_noise", vec=spec(), a=A_COEF, sigma_y=sigma_y, sigma_t=sigma_t,
                                                   eta=ETA, epsilon=spec())))
    if callable(getattr(op, "ddnm_plus_step", None)):
        out.append(("plus_step_before_begin", plus_case(op, "tensor", False, begin=False)))
    for kind in NOISES:
        for view in (False, True):
            out.append((f"ddnm_step_{kind}{'_et_view' if view else ''}", step_case(op, kind, view)))
            if callable(getattr(op, "ddnm_plus_step", None)):
                out.append((f"plus_{kind}{'_et_view' if view else ''}", plus_case(op, kind, view)))
    out.append(("ddnm_step_et_layout", step_case(op, "tensor", False, et=torch.zeros(B, D, D, op.channels).permute(0, 3, 1, 2))))
    if callable(getattr(op, "ddnm_plus_step", None)):
        out.append(("plus_step_other_batch", plus_case(op, "tensor", False, begin_b=B, b=1)))
        out.append(("plus_begin_row_length", plus_case(op, "tensor", False, ylen=_ysize(op) - 4)))
    if isinstance(op, E.WalshHadamardCS):
        out.append(("ddnm_step_inside_begin_run", step_case(op, "tensor", False, begin=True)))
    if isinstance(op, E.PerImageInpainting):
        out.append(("A_pinv_row_length", _call(op, "A_pinv", vec=torch.zeros(B, op.y_dim - 4))))
        out.append(("ddnm_step_row_length", step_case(op, "tensor", False, y=torch.zeros(B, op.y_dim - 4))))
        out.append(("A_batch", _call(op, "A", vec=img(3))))
        out.append(("A_pinv_batch", _call(op, "A_pinv", vec=y(3))))
        out.append(("Lambda_batch", _call(op, "Lambda", vec=spec(3), a=A_COEF, sigma_y=0.2, sigma_t=0.05, eta=ETA)))
        out.append(("Lambda_noise_batch", _call(op, "Lambda_noise", vec=spec(3), a=A_COEF, sigma_y=0.2, sigma_t=0.05, eta=ETA,
                                                epsilon=spec(3))))
        out.append(("ddnm_step_batch", step_case(op, "tensor", False, b=3)))
    return [(f"{name}.{c}", case) for c, case in out]


def rebatched_cases(name, op, b):
    """The short list for an operator that narrow / concat built from others (the full one runs on for_images)."""
    return [(f"{name}.A", _call(op, "A", vec=torch.zeros(b, 3, D, D))),
            (f"{name}.A_pinv", _call(op, "A_pinv", vec=torch.zeros(b, op.y_dim))),
            (f"{name}.Lambda", _call(op, "Lambda", vec=torch.zeros(b, 3 * D * D), a=A_COEF, sigma_y=0.2, sigma_t=0.05, eta=ETA)),
            (f"{name}.ddnm_step", step_case(op, "keyed", True, b=b))]


def cases(tracer, tmp):
    """Yields (case name, rows, error, returned) in the recorded order."""
    built = {}
    for name, make in operators(tmp):
        rows, err, ret = tracer.take(None, lambda: built.__setitem__(name, make()) or built[name], {})
        yield f"{name}.build", rows, err, ret
    assert E.Deblurring.begin_plus_run is None and E.Deblurring.ddnm_plus_step is None
    bank = built.pop("inpainting_bank")
    for name, op in built.items():
        for case_name, (o, fn, args) in operator_cases(name, op):
            yield (case_name,) + tracer.take(o, fn, args)
    # per-image inpainting: for_images, narrow, concat, a concat of parts
    made = {}

    def derive(key, fn):
        rows, err, ret = tracer.take(bank, lambda: made.__setitem__(key, fn()) or made[key], {})
        return f"inpainting_bank.{key}", rows, err, ret
    yield derive("for_images", lambda: bank.for_images([0, 1]))
    yield derive("for_images_b1", lambda: bank.for_images([5]))
    yield derive("for_images_none", lambda: bank.for_images([]))
    for case_name, (o, fn, args) in operator_cases("per_image", made["for_images"]):
        yield (case_name,) + tracer.take(o, fn, args)
    yield derive("narrow", lambda: made["for_images"].narrow(1, 2))
    yield derive("narrow_refused", lambda: made["for_images"].narrow(1, 3))
    yield derive("concat", lambda: E.PerImageInpainting.concat([made["for_images"], made["for_images_b1"]]))
    yield derive("concat_one", lambda: E.PerImageInpainting.concat([made["for_images_b1"]]))
    yield derive("concat_of_parts", lambda: E.PerImageInpainting.concat([made["narrow"], made["for_images"].narrow(0, 1),
                                                                        made["for_images_b1"]]))
    for key, b in (("for_images_b1", 1), ("narrow", 1), ("concat", 3), ("concat_of_parts", 3)):
        for case_name, (o, fn, args) in rebatched_cases(f"per_image_{key}", made[key], b):
            yield (case_name,) + tracer.take(o, fn, args)
    # the GEMM branch of _site_matmul (more than 16 entries per site) refuses every layout but the contiguous site-major one
    v, M = torch.zeros(B, 3 * D * D), torch.zeros(64, 64)
    yield ("site_matmul_64_strided",) + tracer.take(None, lambda: E._site_matmul(v, M, 192, 64, 3 * D * D, 1, 192, True),
                                                    dict(vec=v, M=M))
    yield ("site_matmul_64",) + tracer.take(None, lambda: E._site_matmul(v, M, 192, 64, 3 * D * D, 64, 1, True), dict(vec=v, M=M))


if __name__ == "__main__":
    dry, tracer = install()
    rows, out = rlt.Table(), {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, trace, err, ret in cases(tracer, tmp):
            assert name not in out, name
            out[name] = {"rows": [rows.index(r) for r in trace], "error": err, "returned": ret}
    commit, dirty = "replay", ""
    if "--replay" not in sys.argv[1:]:          # tests/test_operator_trace.py compares the cases, not where they were recorded
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
        dirty = subprocess.run(["git", "status", "--porcelain", "ddnm_amd"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    print(f"{len(out)} cases, {sum(len(c['rows']) for c in out.values())} launches, {len(rows.items)} distinct rows",
          file=sys.stderr)
    used = sorted({r[0] for r in rows.items})
    lines = "[\n" + ",\n".join(json.dumps(i, separators=(",", ":")) for i in rows.items) + "\n]"

    def block(d):
        return "{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}" for k, v in d.items()) + "\n}"
    sys.stdout.write(f'{{"recorded_at":{json.dumps(commit + (" (ddnm_amd modified)" if dirty else ""))},\n'
                     f'"entry_points":{block({n: rlt.signature(n) for n in used})},\n"rows":{lines},\n'
                     f'"cases":{block(out)}}}\n')
