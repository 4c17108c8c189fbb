"""CPU tests of the samplers' shared reverse-loop driver (svd_ddnm._reverse_loop) and of the noise-source interface.

The driver runs on CPU tensors with a stub model, a stub step and `ops.renoise` replaced by its torch expression, on the
smallest schedule that has time travel and a ragged tail: T_sampling = 5 of 1000 timesteps, travel 1 / 2, B = 2, 3x4x4."""
import types

import pytest
import torch

from ddnm_amd import ops
from ddnm_amd.functions import svd_ddnm
from oracle import cases

B, SHAPE, SKIP = 2, (2, 3, 4, 4), 200
NS = types.SimpleNamespace
CFG = NS(diffusion=NS(num_diffusion_timesteps=1000), time_travel=NS(T_sampling=5, travel_length=1, travel_repeat=2))
TIMES = svd_ddnm.get_schedule_jump(5, 1, 2)


def expected_iterations():
    """(k, kind, i, at, at_next) straight from get_schedule_jump and _AlphaTable; a re-noise has no `i` / `at`."""
    alpha = svd_ddnm._AlphaTable(cases.betas())
    rows = []
    for k, (a, c) in enumerate(zip(TIMES[:-1], TIMES[1:])):
        at_next = alpha(c * SKIP if c >= 0 else -1).item()
        rows.append((k, "reverse", a * SKIP, alpha(a * SKIP).item(), at_next) if c < a else (k, "renoise", None, None, at_next))
    return rows


class StrictTape:
    """A tape that may be read at k = 0, 1, 2, ... only, once each."""

    def __init__(self, n):
        g = torch.Generator().manual_seed(7)
        self.items, self.next_k = [torch.randn(SHAPE, generator=g) for _ in range(n)], 0

    def __getitem__(self, k):
        assert k == self.next_k, f"tape read at {k}, expected {self.next_k}"
        self.next_k += 1
        return self.items[k]


class Run:
    """One CPU run of the driver; records what the model, the step and the re-noise see."""

    def __init__(self, monkeypatch, use_tensor=False, fail_at=None, cls_fn=None):
        self.rows, self.events, self.probe = [], [], []
        self.x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(1))
        self.x_before = self.x.clone()
        self.y = torch.randn(B, 3, 2, 2, generator=torch.Generator().manual_seed(2))
        self.tape = StrictTape(len(TIMES) - 1)
        self.noise = svd_ddnm._TapeNoise(self.tape, self.x)
        self.use_tensor, self.fail_at, self.cls_fn = use_tensor, fail_at, cls_fn
        self.prev_out = self.x
        monkeypatch.setattr(ops, "renoise", self.renoise)

    def model(self, xt, t, cls=None):
        assert xt is self.prev_out                       # x_t of an iteration is the previous iteration's output
        self.events.append(("model", float(t[0])))
        self.t = t
        self.eps = torch.cat([0.1 * xt, xt], 1)          # a learn_sigma output: the step must see its [:, :3] view
        return self.eps

    def check_out(self, out, *others):
        for o in others + (self.x,):
            assert out.data_ptr() != o.data_ptr()
        self.prev_out = out

    def step(self, it, xt, et, y, noise, x0_t, out):
        if it.k == self.fail_at:
            raise KeyError("step failed")
        assert xt is self.prev_out and noise is self.noise and y is self.y_seen
        assert self.t.shape == (B,) and bool((self.t == float(it.i)).all())
        assert et.shape == SHAPE and (self.cls_fn is not None or et.data_ptr() == self.eps.data_ptr())
        self.check_out(out, xt, x0_t)
        s = ops.step_scalars(it.at, it.at_next, 0.85)
        nz = noise.tensor(it.k, x0_t) if self.use_tensor else noise.kernel_arg(s, it.k)
        assert torch.equal(nz, self.tape.items[it.k])
        x0_t.copy_((xt - et * s.sqrt_1m_at) / s.sqrt_at)
        out.copy_(s.sqrt_at_next * x0_t + s.c1 * nz + s.c2 * et)
        self.rows.append((it.k, "reverse", it.i, it.at.item(), it.at_next.item()))

    def renoise(self, x0, noise, a, b, out=None):
        k = self.tape.next_k - 1                         # the draw of this iteration was just read
        assert torch.equal(noise, self.tape.items[k]) and x0 is self.x0_t
        self.check_out(out, x0, self.prev_out)
        out.copy_(a * x0 + b * noise)
        self.rows.append((k, "renoise", a, b))

    def begin(self, y):
        self.y_seen = y

    def record(self, k, name, t):
        self.probe.append((k, name))
        if name == "x0_t":
            self.x0_t = t

    def go(self):
        return svd_ddnm._reverse_loop(self.x, self.model, cases.betas(), self.y, CFG, self.noise, self.step,
                                      begin=self.begin, cls_fn=self.cls_fn, record=self.record)


@pytest.mark.parametrize("use_tensor", [False, True])
def test_driver_iterations_buffers_and_tape(monkeypatch, use_tensor):
    r = Run(monkeypatch, use_tensor)
    want = expected_iterations()
    # the schedule of this test does travel back and ends on the ragged step to t = -1
    assert [w[1] for w in want].count("renoise") == 4 and want[-1][1] == "reverse" and want[-1][4] == 1.0
    xt, x0_t = r.go()
    # (a) every iteration, in order, with the alpha-bar values of the table
    got = [row if row[1] == "reverse" else (row[0], "renoise", None, None, row[2:]) for row in r.rows]
    want = [w if w[1] == "reverse" else w[:4] + ((float(torch.tensor(w[4]).sqrt()), float((1 - torch.tensor(w[4])).sqrt())),)
            for w in want]
    assert got == want
    assert r.probe == [(k, n) for k in range(len(want)) for n in ("x0_t", "xt_next")]
    # (b) checked per iteration in Run.check_out; the results are the driver's own buffers, x is untouched, y was
    # coerced once ([B, -1]) and that one tensor went to `begin` and to every step
    assert xt is r.prev_out and x0_t is r.x0_t and x0_t.data_ptr() != xt.data_ptr()
    assert torch.equal(r.x, r.x_before) and r.y_seen.shape == (B, 12) and torch.equal(r.y_seen, r.y.reshape(B, -1))
    # (c) StrictTape raises on a repeated or out-of-order read; every iteration read it
    assert r.tape.next_k == len(TIMES) - 1


def test_guidance_side_stream_is_rejoined_when_a_step_raises(monkeypatch):
    made = []

    class Guide:
        def __init__(self, cls_fn, x, n, t_values, t_of, cls):
            self.t_values, self.cls, self.closed, self.events = list(t_values), cls, 0, run.events
            assert cls_fn is run.cls_fn and n == B and torch.equal(x, run.x)
            assert bool((t_of(t_values[0]) == float(t_values[0])).all())
            made.append(self)

        def grad(self, tv, t, cls):
            assert cls is self.cls and self.events[-1] == ("model", float(tv))      # after that step's model call
            self.events.append(("grad", tv))
            return torch.zeros(SHAPE)

        def close(self):
            self.closed += 1

    monkeypatch.setattr(svd_ddnm, "_GuidanceAhead", Guide)
    monkeypatch.setattr(svd_ddnm, "_guided_eps", lambda et, grad, coef: (et[:, :3] - coef * grad).contiguous())
    run = Run(monkeypatch, fail_at=2, cls_fn=lambda x, t, y: None)
    with pytest.raises(KeyError, match="step failed"):
        run.go()
    (g,) = made
    assert g.closed == 1
    assert g.t_values == [a * SKIP for a, c in zip(TIMES[:-1], TIMES[1:]) if c < a]
    assert g.cls.tolist() == [svd_ddnm.class_num] * B
    assert run.events == [("model", 800.0), ("grad", 800), ("model", 800.0), ("grad", 800)]     # k = 0, 2; k = 1 re-noises
    # and once on the way out of a run that ends normally
    run = Run(monkeypatch, cls_fn=lambda x, t, y: None)
    run.go()
    assert len(made) == 2 and made[1].closed == 1


def test_noise_sources_share_one_interface(monkeypatch):
    like = torch.zeros(SHAPE)
    alpha = svd_ddnm._AlphaTable(cases.betas())

    def scalars():
        return ops.step_scalars(alpha(800), alpha(600), 0.85)

    tape = [torch.full(SHAPE, float(k), dtype=torch.float64) for k in range(3)]
    src, s = svd_ddnm._noise_source(tape, like), scalars()
    assert isinstance(src, svd_ddnm._TapeNoise)
    got = src.kernel_arg(s, 1)
    assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, tape[1].float()) and s.rng_on == 0
    assert torch.equal(src.tensor(2, like), tape[2].float())
    f32 = [torch.randn(SHAPE)]
    assert svd_ddnm._TapeNoise(f32, like).kernel_arg(s, 0) is f32[0]           # nothing to coerce: the tape's own tensor

    monkeypatch.setenv("DDNM_NOISE", "torch")
    src, s = svd_ddnm._noise_source(None, like), scalars()
    assert isinstance(src, svd_ddnm._AtenNoise)
    torch.manual_seed(5)
    got = [src.kernel_arg(s, 0), src.tensor(1, like)]
    torch.manual_seed(5)
    assert all(torch.equal(g, torch.randn_like(like)) for g in got) and s.rng_on == 0      # one draw each, in order
    monkeypatch.delenv("DDNM_NOISE")

    ph, s = ops.PhiloxNoise(0x1234567890ABCDEF, image_base=3), scalars()
    assert svd_ddnm._noise_source(ph, like) is ph and ph.kernel_arg(s, 7) is None
    assert (s.rng_on, s.rng_iter, s.rng_seed_lo, s.rng_seed_hi, s.rng_image_base) == (1, 7, 0x90ABCDEF, 0x12345678, 3)
    src, s = svd_ddnm._noise_source(None, like), scalars()                      # un-pinned: a per-call Philox key
    assert isinstance(src, ops.PhiloxNoise) and src.kernel_arg(s, 4) is None and (s.rng_on, s.rng_iter) == (1, 4)

    keyed, s = ops.KeyedPhiloxNoise([11, 12], [0, 1]), scalars()
    assert svd_ddnm._noise_source(keyed, like) is keyed and keyed.kernel_arg(s, 9) is keyed
    assert (s.rng_on, s.rng_iter) == (1, 9)
