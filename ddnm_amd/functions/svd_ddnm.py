"""DDNM reverse-diffusion loop on MI355X.

Drop-in for `functions/svd_ddnm.py::ddnm_diffusion` (:19-78): same name, same
positional arguments `(x, model, b, eta, A_funcs, y, cls_fn, classes, config)`,
same return value `([x_0], [x0_pred_last])`.

What differs from the reference is everything the reference does per step on the
host: it rebuilds alpha-bar with a cumprod every step (:10-13,43-44), ping-pongs
every intermediate through CPU memory (:45,67-68,72,76 -- two implicit device
syncs per step) and launches ~60 tiny ATen kernels for the projection.  Here
alpha-bar is tabulated once on the host, all state stays in HBM, and a step is:
UNet forward (ddnm_amd.guided_diffusion.models) + ONE fused HIP kernel (or a
short fixed chain for the SVD-free forms of sr_bicubic / cs_walshhadamard).

Reference quirks kept on purpose: float timesteps
990, 980, ...; classifier guidance evaluated on the initial noise `x` with the
hard-coded class 951 (:7,49-52); time travel re-noises the UN-projected x0
prediction (:72-74).

ONE driver, `_reverse_loop`, runs the loop of all three samplers
(`ddnm_diffusion`, `ddnm_plus_diffusion`, and `simplified_loop` of
guided_diffusion/diffusion.py): the jump schedule and alpha-bar table, the
coercion of `x` / `y`, `x0_t` and the two ping-pong buffers, the per-run tables,
classifier guidance on its side stream, the model call, the time-travel
re-noise and the `record` probe.  A sampler supplies its per-run operator set-up
(`begin`) and ONE `step(it, xt, et, y, noise, x0_t, out)` callable: the reverse
step from eps to `x0_t` and `out`.

Noise reaches the loop as an object with two methods.  `kernel_arg(s, k)` is
what a step kernel takes as `noise` for loop iteration k: a tensor (`_TapeNoise`,
`_AtenNoise`), or -- after stamping (on, k) into the step scalars `s` -- None
(`ops.PhiloxNoise`) or the object itself (`ops.KeyedPhiloxNoise`, which owns the
key table); then the kernel draws N(0, I) itself.  `tensor(k, like)` is the same
draw as a tensor (time-travel re-noise, the generic DDNM+ chain).  An iteration
calls one of the two, once.

The samplers' `noise` argument (optional) is an explicit tape: tensor [n_iters, B, 3, H, W] or a list of
tensors, consumed one per loop iteration (the parity path).  Without it the
N(0, I) draw of the reference's `torch.randn_like(x)` (svd_ddnm.py:65,74) happens
INSIDE the step kernels (`ops.PhiloxNoise`: Philox4x32-10 + Box-Muller, counter =
(element, iteration, global image index), key = the torch seed and a per-call
counter): no noise tensor is written and read back, and no ATen kernel runs in
the loop.  `noise=ops.PhiloxNoise(seed, image_base)` pins seed and the global
index of the batch's first image (sharded runs); DDNM_NOISE=torch restores the
ATen draw from the device generator.  `noise=ops.KeyedPhiloxNoise(keys, image_ctrs)`
gives every image its own key and counter: a batch of independently seeded images
(e.g. several loader batches fused into one call) restored in one run, each image
drawing exactly what it draws when restored alone.

`return_cpu` (default True) matches the reference, which hands back CPU tensors
(`xs[-1]`, `x0_preds[-1]` were `.to('cpu')`, svd_ddnm.py:67-68,76-78); the runner, the
benchmark and the parity tests pass False and keep the result in HBM.  `record(k, name, tensor)`
is an optional probe called with the device tensors `x0_t` / `xt_next` after iteration k.
"""
import collections
import contextlib
import os

import torch

from .. import _lib, ops
from .svd_operators import HN_OPERATORS, A_functions, NoiseModel, _axpby

class_num = 951      # svd_ddnm.py:7


def compute_alpha(beta, t):
    """alpha_bar_t as in svd_ddnm.py:10-13 (fp32 cumprod over [0, beta]); t = -1 -> 1."""
    beta = torch.cat([torch.zeros(1).to(beta.device), beta], dim=0)
    return (1 - beta).cumprod(dim=0).index_select(0, t + 1).view(-1, 1, 1, 1)


def get_schedule_jump(T_sampling, travel_length, travel_repeat):
    """RePaint-style jump schedule (svd_ddnm.py:167-206), with the reference's sanity checks."""
    budget = {j: travel_repeat - 1 for j in range(0, T_sampling - travel_length, travel_length)}
    t, ts = T_sampling, []
    while t >= 1:
        t -= 1
        ts.append(t)
        if budget.get(t, 0) > 0:
            budget[t] -= 1
            for _ in range(travel_length):
                t += 1
                ts.append(t)
    ts.append(-1)
    assert ts[0] > ts[1], (ts[0], ts[1])
    assert ts[-1] == -1, ts[-1]
    for a, b in zip(ts[:-1], ts[1:]):
        assert abs(a - b) == 1, (a, b)
    for v in ts:
        assert -1 <= v <= T_sampling, (v, T_sampling)
    return ts


class _AlphaTable:
    """alpha-bar for t in [-1, T) tabulated once on the host in fp32 (same arithmetic as compute_alpha)."""

    def __init__(self, b):
        bc = b.detach().float().cpu()
        full = torch.cat([torch.zeros(1), bc], dim=0)
        self.ab = (1 - full).cumprod(dim=0)

    def __call__(self, t):
        return self.ab[t + 1]


def _guided_eps(et, grad, coef):
    """eps[:, :3] - sqrt(1 - abar_t) * cls_fn(x, t, y)   (svd_ddnm.py:51-52; note the guidance is evaluated on the
    INITIAL noise x, not on x_t -- reference quirk kept)."""
    n = et.shape[0]
    chw = 3 * et.shape[2] * et.shape[3]
    out = torch.empty(n, 3, et.shape[2], et.shape[3], dtype=torch.float32, device=et.device)
    grad = grad.float().contiguous()
    _lib.check(_lib.lib().ddnm_axpby_strided_f32(et.data_ptr(), et.stride(0), grad.data_ptr(), out.data_ptr(), n, chw,
                                                 1.0, -coef, ops._stream()), "ddnm_axpby_strided_f32")
    return out


def _reverse_times(times, skip):
    """The float-timestep values (990, 980, ...) of the schedule's reverse steps, in loop order."""
    return [a * skip for a, c in zip(times[:-1], times[1:]) if c < a]


def _step_tables(times, skip, n, device, with_classes):
    """Per-run device constants of the loop: one row [n] of the float timestep per distinct reverse-step time (the
    reference builds `torch.ones(n) * i` every step, svd_ddnm.py:40) and the constant class vector (:50).  ONE host-to-
    device copy per run; the loop then only takes views -- no fill kernel (and no other ATen arithmetic) per step."""
    uniq = sorted(set(_reverse_times(times, skip)))
    table = torch.tensor([[float(v)] * n for v in uniq], dtype=torch.float32).to(device, non_blocking=False) if uniq else None
    index = {v: k for k, v in enumerate(uniq)}
    cls = torch.tensor([class_num] * n, dtype=torch.long).to(device) if with_classes else None
    return (lambda i: table[index[i]]), cls


_SIDE_STREAMS = {}


def _side_stream(device, priority):
    key = (torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device(), priority)
    st = _SIDE_STREAMS.get(key)
    if st is None:
        st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=device, priority=priority)
    return st


class _GuidanceAhead:
    """Classifier guidance on its own HIP stream, ahead of the UNet.

    The reference evaluates `cls_fn(x, t, classes)` on the INITIAL noise `x` (svd_ddnm.py:49-52; quirk kept), so the
    guidance term of a step depends only on (x, t, class) -- not on x_t, i.e. not on the UNet chain.  Its ~600 launches
    (classifier forward + explicit input-gradient backward, many of them latency-bound with a handful of workgroups)
    therefore run on a second stream while the first stream runs the UNet; the main stream waits on an event right before
    it combines the two.  Since round 4 the guidance terms of G consecutive reverse steps (DDNM_CLS_GROUP, default 4) are
    evaluated in one pass over the batch [x; ...; x] with the timestep vector [t_k ... t_k, t_k+1 ... t_k+1, ...] (the
    classifier conditions per sample, so this IS the reference's computation for each of the steps): the low-resolution
    half of the classifier is a chain of launches whose time does not depend on the batch, and one chain now serves G
    steps.  Same inputs, same arithmetic; the launch plans of a batch of G n differ from those of n in summation order
    only (fp32: ~1e-7).  DDNM_CLS_GROUP=1 evaluates step by step (bit-identical to the serial order), DDNM_CLS_OVERLAP=0
    restores the serial order on the main stream."""

    def __init__(self, cls_fn, x, n, t_values, t_of=None, cls=None):
        self.cls_fn, self.x, self.n = cls_fn, x, n
        self.t_of, self.cls = t_of, cls
        self.t_values, self.pos = t_values, 0
        self.serial = os.environ.get("DDNM_CLS_OVERLAP") == "0"
        # steps per guidance pass: DDNM_CLS_GROUP (default 4: c5 at B = 8 on one MI355X 2.92 / 3.00 / 3.03 / 3.04 images/s
        # for 1 / 2 / 3 / 4, same box; 1 or 0 = step by step, bit-identical to the serial order).  ONLY the engine's own cond_fn is grouped (`make_cond_fn` marks it): a foreign callable
        # -- e.g. the reference's torch-autograd closure -- sees exactly the reference's calls (n images, one timestep),
        # because grouping multiplies its activation memory by G and assumes a strictly per-sample classifier.
        grp = int(os.environ.get("DDNM_CLS_GROUP", "4"))
        if grp < 1 or getattr(cls_fn, "ddnm_engine", None) is None:
            grp = 1
        # ... capped so that the replicated batch stays within what one convolution launch can address (2 GiB per
        # tensor): 32 images for the fp32-tensor engines (128 channels at 256 x 256), 64 for the fp16-activation one
        cap = int(getattr(getattr(cls_fn, "ddnm_engine", None), "max_group_batch", 32))
        self.group = max(1, min(grp, len(t_values), max(1, cap // n))) if (not self.serial and n > 0) else 1
        self.queue = collections.deque()
        if self.group > 1:
            # per-run constants of the grouped evaluation, built on the main stream before the side stream forks: the
            # replicated batch, its class vector and ONE host-to-device table of the grouped timestep vectors
            G = self.group
            self.xg = torch.cat([x] * G, 0)
            rows = []
            for i in range(0, len(t_values), G):
                ts = list(t_values[i:i + G])
                ts = ts + [ts[-1]] * (G - len(ts))                   # a ragged last group uses the first len(ts) * n rows only
                rows.append([float(tv) for tv in ts for _ in range(n)])
            self.tg = torch.tensor(rows, dtype=torch.float32).to(x.device)
            self.clsg = torch.tensor([class_num] * (G * n), dtype=torch.long).to(x.device)
        if not self.serial:
            self.main = torch.cuda.current_stream()
            # high priority: the guidance pass is a long chain of small dependent launches (latency-bound), the UNet a
            # sequence of chip-filling ones -- the chain must not queue behind them, the big kernels soak up the rest
            # ONE side stream per (device, priority) for the life of the process: the convolution / GroupNorm workspaces
            # are keyed by the stream handle, a fresh stream per call would grow them by one set per batch
            # (measured on c5, one MI355X: high priority 2.85 -> 2.99 images/s for step-by-step evaluation; with four steps
            # per pass the chain has four UNet steps to hide behind and normal priority is ahead, 3.034 vs 3.011)
            self.side = _side_stream(x.device, -1 if self.group == 1 else 0)
            self.side.wait_stream(self.main)             # x (and the operator's set-up) are complete
            self._launch()

    def _launch(self):
        if self.pos >= len(self.t_values):
            return
        tv = self.t_values[self.pos]
        G = self.group
        if G > 1:
            g = min(G, len(self.t_values) - self.pos)            # steps served by this pass
            m = g * self.n
            with torch.cuda.stream(self.side):
                # (the engine's cond_fn is told that the batch is g copies of x: t-independent layers run once)
                gg = self.cls_fn(self.xg[:m], self.tg[self.pos // G][:m], self.clsg[:m], replicas=g)
                ev = torch.cuda.Event()
                ev.record(self.side)
            for j in range(g):
                self.queue.append((self.t_values[self.pos + j], gg[j * self.n:(j + 1) * self.n], ev, gg))
            self.pos += g
            return
        self.pos += 1
        with torch.cuda.stream(self.side):
            if self.t_of is not None:        # views of the per-run tables (built on the main stream before this one forked)
                t, cls = self.t_of(tv), self.cls
            else:
                t = torch.full((self.n,), float(tv), device=self.x.device, dtype=torch.float32)
                cls = torch.full((self.n,), class_num, dtype=torch.long, device=self.x.device)
            g = self.cls_fn(self.x, t, cls)
            ev = torch.cuda.Event()
            ev.record(self.side)
        self.queue.append((tv, g, ev, g))

    def grad(self, tv, t, cls):
        """Gradient of the reverse step at timestep `tv` (called AFTER the UNet forward of that step was enqueued)."""
        if self.serial:
            return self.cls_fn(self.x, t, cls)
        tq, g, ev, owner = self.queue.popleft()
        assert tq == tv, (tq, tv)
        self.main.wait_event(ev)
        owner.record_stream(self.main)                    # allocated on the side stream, consumed on the main one
        if len(self.queue) <= max(0, self.group - 1):
            # the next evaluation starts under this step's tail; a grouped pass (G times the work) is launched when the
            # FIRST term of the previous group is consumed, so it has G UNet steps to hide behind
            self._launch()
        return g

    def close(self):
        if not self.serial:
            self.main.wait_stream(self.side)


_PHILOX_CALLS = [0]


def _philox_for_call(like):
    """Key of an un-pinned run (`noise=None`): a 64-bit hash of the device generator's FULL seed (torch.manual_seed /
    torch.cuda.manual_seed_all set it, like the reference's main.py:139-143), a per-call counter -- consecutive restorations
    draw different noise -- and the rank of the calling process, so that the ranks of a sharded programmatic run do not draw
    identical noise for different images.  Callers that want rank-count-independent results pin the generator:
    `noise=ops.PhiloxNoise(seed, image_base=<global index of image 0>)`, as the runner does; DDNM_NOISE=torch = ATen draws."""
    seed = int(torch.cuda.initial_seed() if like.is_cuda else torch.initial_seed())
    _PHILOX_CALLS[0] += 1
    rank = torch.distributed.get_rank() if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 0
    z = (seed * 0x9E3779B97F4A7C15 + _PHILOX_CALLS[0] * 0xBF58476D1CE4E5B9 + (rank + 1) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return ops.PhiloxNoise(z ^ (z >> 31))


class _TensorNoise:
    """A noise source whose draws are tensors; `like` is the template of the kernel-form draw (x: fp32, contiguous)."""

    def __init__(self, like):
        self.like = like.float().contiguous()

    def kernel_arg(self, s, k):
        return self.tensor(k, self.like)


class _TapeNoise(_TensorNoise):
    """An explicit tape, read `tape[k]` once per loop iteration (BatchNoise / FusedTape draw sequentially)."""

    def __init__(self, tape, like):
        super().__init__(like)
        self.tape = tape

    def tensor(self, k, like):
        n = self.tape[k]
        if n.device != like.device or n.dtype != torch.float32 or not n.is_contiguous():
            n = n.to(device=like.device, dtype=torch.float32).contiguous()
        return n


class _AtenNoise(_TensorNoise):
    """The reference's draw: one `torch.randn_like` per loop iteration from the device generator."""

    def tensor(self, k, like):
        return torch.randn_like(like)


def _noise_source(noise, like):
    """The noise source (`kernel_arg(s, k)` / `tensor(k, like)`, see the module docstring) of a sampler's `noise`
    argument: a Philox object as it is, a per-call Philox key for None (the ATen draw with DDNM_NOISE=torch), else a tape."""
    if isinstance(noise, (ops.PhiloxNoise, ops.KeyedPhiloxNoise)):
        return noise
    if noise is not None:
        return _TapeNoise(noise, like)
    return _AtenNoise(like) if os.environ.get("DDNM_NOISE") == "torch" else _philox_for_call(like)


_Iter = collections.namedtuple("_Iter", "k i at at_next")       # loop index, float timestep, alpha-bar of t and of t'


def _reverse_loop(x, model, b, y, config, noise, step, begin=None, cls_fn=None, record=None):
    """The reverse loop of every sampler here -> (x_0, last un-projected x0 prediction), both on x's device.

    `noise` is a noise source; `begin(y)`, when given, is the operator's per-run set-up and gets the SAME `y` tensor that
    every step gets (WalshHadamardCS keys its A^+ y on that object).  `step(it, xt, et, y, noise, x0_t, out)` is one
    reverse step: `it` = _Iter(k, i, at, at_next), `et` the model's eps -- guided when `cls_fn` is given, the [:, :3]
    view of a learn_sigma output -- and it writes the x0 prediction to `x0_t` and x_t' to `out`, drawing its noise as
    `noise.kernel_arg(s, it.k)` or `noise.tensor(it.k, x0_t)`.  The caller's `x` is never written."""
    tt = config.time_travel
    skip = config.diffusion.num_diffusion_timesteps // tt.T_sampling
    times = get_schedule_jump(tt.T_sampling, tt.travel_length, tt.travel_repeat)
    alpha = _AlphaTable(b)
    n = x.size(0)
    x = x.float().contiguous()
    y = y.reshape(n, -1).float().contiguous()
    if begin is not None:
        begin(y)           # per-run constants of the operator (e.g. A^+ y); never cached across runs
    xt = x
    x0_t = torch.empty_like(x)
    bufs = [torch.empty_like(x), torch.empty_like(x)]
    have_x0 = False
    with torch.no_grad(), contextlib.ExitStack() as stack:
        t_of, cls = _step_tables(times, skip, n, x.device, cls_fn is not None)
        if cls_fn is not None:
            guide = _GuidanceAhead(cls_fn, x, n, _reverse_times(times, skip), t_of, cls)
            stack.callback(guide.close)          # also when the loop raises: the main stream re-joins the side stream
        for k, (i, j) in enumerate(zip(times[:-1], times[1:])):
            i, j = i * skip, j * skip
            if j < 0:
                j = -1
            at_next = alpha(j)
            out = bufs[k & 1]
            if j < i:      # reverse step
                at = alpha(i)
                t = t_of(i)
                if cls_fn is None:
                    et = model(xt, t)
                else:
                    et = _guided_eps(model(xt, t, cls), guide.grad(i, t, cls), float((1 - at).sqrt()))
                if et.size(1) == 6:
                    et = et[:, :3]               # read through its strides, no copy
                step(_Iter(k, i, at, at_next), xt, et, y, noise, x0_t, out)
                have_x0 = True
            else:          # time-travel back (svd_ddnm.py:70-76)
                assert have_x0
                ops.renoise(x0_t, noise.tensor(k, x0_t), float(at_next.sqrt()), float((1 - at_next).sqrt()), out=out)
            xt = out
            if record is not None:
                record(k, "x0_t", x0_t)
                record(k, "xt_next", xt)
    return xt, x0_t


def _finish(xt, x0_t, return_cpu):
    if return_cpu:
        return [xt.to("cpu")], [x0_t.to("cpu")]
    return [xt], [x0_t]


def ddnm_diffusion(x, model, b, eta, A_funcs, y, cls_fn=None, classes=None, config=None, noise=None, return_cpu=True,
                   record=None):
    if not x.is_cuda:
        raise RuntimeError("ddnm_amd.ddnm_diffusion runs on the GPU only (no CPU fallback); got a CPU tensor")
    fused = isinstance(A_funcs, A_functions)

    def step(it, xt, et, y, noise, x0_t, out):
        s = ops.step_scalars(it.at, it.at_next, eta)
        if fused:
            A_funcs.ddnm_step(xt, et, noise.kernel_arg(s, it.k), y, s, x0_t, out)
        else:          # foreign operator object: its own A / A_pinv, our elementwise kernels
            ops.step_x0(xt, et, s, out=x0_t)
            proj = A_funcs.A_pinv(A_funcs.A(x0_t.reshape(x0_t.size(0), -1)) - y).reshape(*x0_t.size())
            ops.step_combine(x0_t, proj.float().contiguous(), None, noise.kernel_arg(s, it.k), et, s, out=out)

    xt, x0_t = _reverse_loop(x, model, b, y, config, _noise_source(noise, x), step,
                             begin=getattr(A_funcs, "begin_run", None), cls_fn=cls_fn, record=record)
    return _finish(xt, x0_t, return_cpu)


def ddnm_plus_diffusion(x, model, b, eta, A_funcs, y, sigma_y, cls_fn=None, classes=None, config=None, noise=None,
                        return_cpu=True, record=None):
    """DDNM+ for noisy measurements: drop-in for `functions/svd_ddnm.py::ddnm_plus_diffusion` (:80-164).

      x0|t  = (x_t - eps*sqrt(1-abar_t)) / sqrt(abar_t)                                  (Eq. 12)
      x0^   = x0|t - Lambda( A^+ (A x0|t - y) )                                          (Eq. 17)
      x_t-1 = sqrt(abar') x0^ + Lambda_noise( N(0,I), eps )                              (Eq. 51)

    with the operator's `Lambda` / `Lambda_noise` (spectral lambda_t and noise mixing).  Every product is a
    HIP kernel; per step: UNet forward, x0 kernel, A / A^+ kernels, Lambda, Lambda_noise, combine.  An operator with a
    non-None `ddnm_plus_step` hook (SRConv, Deblurring2D: no Lambda in the reference) runs the whole operator part of the
    step in its spectral planes instead: `begin_plus_run(y)` once, then x0 kernel, two two-sided GEMMs and one fused kernel
    per step (svd_operators._SpectralPlus).  `sigma_y` is the noise level on the engine's [-1, 1] scale, or a
    `svd_operators.NoiseModel`: its scalar form runs what the float runs, shot + read noise and noise maps run the
    one-launch `ddnm_plus_step_hn` of Mosaic / Denoising (every other operator: ValueError)."""
    if not x.is_cuda:
        raise RuntimeError("ddnm_amd.ddnm_plus_diffusion runs on the GPU only (no CPU fallback)")
    plus_step = getattr(A_funcs, "ddnm_plus_step", None)     # SRConv / Deblurring2D: the step fused in the spectral planes
    begin = A_funcs.begin_plus_run if plus_step is not None else None
    # `sigma_y` as a NoiseModel: the scalar form IS the float (same launches); shot + read noise and noise maps run the
    # operator's one-launch per-entry step (Mosaic, Denoising: U = I and singular value 1, where the model is exact)
    hn_step = None
    if isinstance(sigma_y, NoiseModel):
        model_y = sigma_y
        if model_y.is_scalar:
            sigma_y = model_y.sigma_engine()
        else:
            hn_step = getattr(A_funcs, "ddnm_plus_step_hn", None)
            if hn_step is None:
                raise ValueError(f"per-entry measurement noise (a {model_y.kind} NoiseModel) is supported by {HN_OPERATORS}, "
                                 f"not by {type(A_funcs).__name__}: pass a scalar sigma_y")
            begin = lambda y: A_funcs.begin_plus_run(y, model_y)

    def step(it, xt, et, y, noise, x0_t, out):
        a, sigma_t = it.at_next.sqrt(), (1 - it.at_next).sqrt()
        s = ops.step_scalars(it.at, it.at_next, eta)
        if hn_step is not None:
            hn_step(xt, et, noise.kernel_arg(s, it.k), s, float(sigma_t), eta, x0_t, out)
            return
        if plus_step is not None:
            plus_step(xt, et, noise.kernel_arg(s, it.k), s, sigma_y, float(sigma_t), eta, x0_t, out)
            return
        et = et.contiguous()                     # a copy only of the [:, :3] view of a learn_sigma output
        ops.step_x0(xt, et, s, out=x0_t)
        resid = _axpby(A_funcs.A(x0_t), y, 1.0, -1.0)
        corr = A_funcs.Lambda(A_funcs.A_pinv(resid), a, sigma_y, sigma_t, eta).reshape(x0_t.shape)
        nz = A_funcs.Lambda_noise(noise.tensor(it.k, x0_t), a, sigma_y, sigma_t, eta, et).reshape(x0_t.shape)
        s.c1, s.c2, s.lam = 1.0, 0.0, 1.0        # x_t-1 = sqrt(abar') (x0 - corr) + 1 * nz
        ops.step_combine(x0_t, corr, None, nz, et, s, out=out)

    # begin_plus_run: y^ of THIS call's measurement; never cached across runs
    xt, x0_t = _reverse_loop(x, model, b, y, config, _noise_source(noise, x), step,
                             begin=begin, cls_fn=cls_fn, record=record)
    return _finish(xt, x0_t, return_cpu)
