"""CPU float64 models and input builders shared by the attention edge tests (test_attn_model_host.py without a GPU,
test_gpu_attention_edges.py on one).

`attn16_model_*` restate what csrc/attn16.hip and csrc/attn16_bwd.hip document, in float64, rounding to fp16 exactly
where the kernels do; they do NOT reproduce the kernels' fp32 accumulation order or the one-ulp v_exp_f32.  `exact_*`
are the plain float64 functions (softmax attention, gradients by torch autograd).  All tensors are per head:
[..., T, d] float64 holding the (fp16-exact) input values.

Input builders are seeded (torch.Generator only) and cached: a case is built once and must be left unchanged."""
import functools
import math

import torch

KT = 64                                     # keys per tile of attn16.hip / attn16_bwd.hip
SCALE_LOG2_F32 = float(torch.tensor(0.125, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32))
LOG2E = 1.4426950408889634


def r16(x):
    """Round to fp16, back in float64."""
    return x.to(torch.float16).to(torch.float64)


def ulp16(x):
    """Spacing of fp16 at |x| (float64 tensor): 2^(e - 10) for a normal x, 2^-24 below 2^-14."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10.0)


# ----------------------------------------------------------------------------- exact float64
def exact_logits(q, k, scale):
    return (q @ k.transpose(-1, -2)) * scale


def exact_attention(q, k, v, scale):
    """softmax(q k^T scale) v and the base-2 log-sum-exp of the scaled logits."""
    s = exact_logits(q, k, scale)
    return torch.softmax(s, dim=-1) @ v, torch.logsumexp(s, dim=-1) * LOG2E


def exact_attention_grads(q, k, v, dO, scale):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    o, _ = exact_attention(q, k, v, scale)
    (o * dO).sum().backward()
    return q.grad, k.grad, v.grad


# ----------------------------------------------------------------------------- fp64 model of attn16.hip / attn16_bwd.hip
def attn16_model_fwd(q, k, v):
    """Online softmax per 64-key tile in the base-2 domain: P = fp16(exp2(s * scale_log2 - m)), l sums the ROUNDED P, the
    running output is rescaled by alpha; out = fp16(o / l), lse = m + log2 l (stored as fp32)."""
    T = k.shape[-2]
    s2 = (q @ k.transpose(-1, -2)) * SCALE_LOG2_F32
    m = torch.full(q.shape[:-1], -1e30, dtype=torch.float64)
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    for t0 in range(0, T, KT):
        st = s2[..., t0:t0 + KT]
        m_new = torch.maximum(m, st.amax(dim=-1))
        alpha = torch.exp2(m - m_new)
        p = r16(torch.exp2(st - m_new[..., None]))
        l = l * alpha + p.sum(dim=-1)
        o = o * alpha[..., None] + p @ v[..., t0:t0 + KT, :]
        m = m_new
    lse = (m + torch.log2(l)).to(torch.float32).to(torch.float64)
    return r16(o / l[..., None]), lse


def attn16_model_bwd(q, k, v, o16, lse, dO, return_ds=False):
    """D = sum_d dO * O (the fp16 O), P = exp2(s * scale_log2 - lse); fp16(P) is the operand of dv, fp16(P (dP - D)) the
    operand of dq / dk; results rounded to fp16."""
    D = (dO * o16).sum(dim=-1, keepdim=True)
    p = torch.exp2((q @ k.transpose(-1, -2)) * SCALE_LOG2_F32 - lse[..., None])
    dp = dO @ v.transpose(-1, -2)
    ds = p * (dp - D)
    ds16 = r16(ds)
    dv = r16(r16(p).transpose(-1, -2) @ dO)
    dq = r16((ds16 @ k) * 0.125)
    dk = r16((ds16.transpose(-1, -2) @ q) * 0.125)
    if return_ds:
        return dq, dk, dv, ds
    return dq, dk, dv


# ----------------------------------------------------------------------------- per-block judgement
def block_errors(got, ref, rows=32):
    """||got - ref|| / ||ref|| per block of `rows` consecutive tokens: [..., T, d] -> [..., T / rows]."""
    got, ref = got.double(), ref.double()
    sh = ref.shape[:-2] + (ref.shape[-2] // rows, rows * ref.shape[-1])
    num = (got - ref).reshape(sh).norm(dim=-1)
    return num / (ref.reshape(sh).norm(dim=-1) + 1e-300)


def worst_block(got, ref, rows=32):
    return float(block_errors(got, ref, rows).max())


# ----------------------------------------------------------------------------- layouts
def pack_legacy(q, k, v):
    """[B, nh, T, 64] x 3 -> qkv [B, T, 3 * 64 nh], channel = head * 192 + {q, k, v} (attn16.hip)."""
    B, nh, T, d = q.shape
    return torch.stack([q, k, v], dim=3).permute(0, 2, 1, 3, 4).reshape(B, T, nh * 3 * d).contiguous()


def unpack_legacy(t, nh):
    """[B, T, 3 * 64 nh] -> three [B, nh, T, 64]."""
    B, T, _ = t.shape
    x = t.reshape(B, T, nh, 3, 64).permute(3, 0, 2, 1, 4)
    return x[0], x[1], x[2]


def heads_to_tokens(o):
    """[B, nh, T, 64] -> [B, T, 64 nh]."""
    B, nh, T, d = o.shape
    return o.permute(0, 2, 1, 3).reshape(B, T, nh * d).contiguous()


def tokens_to_heads(o, nh):
    B, T, _ = o.shape
    return o.reshape(B, T, nh, 64).permute(0, 2, 1, 3)


# ----------------------------------------------------------------------------- input builders
def _gen(*key):
    h = 0
    for x in key:
        h = (h * 1000003 + (int(x) if not isinstance(x, str) else sum(map(ord, x)))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(h)


def pi_map(T):
    """pi(i) = (77 i + 13) mod T: a bijection whenever gcd(77, T) = 1 (every T of the attn16 tests; at T = 224 it is a
    7-to-1 map onto every 7th key, which a forward-only test can still use).  Consecutive queries land 77 keys
    apart, so the 32 queries of a block meet every tile and every position inside a group of 16 keys."""
    return (77 * torch.arange(T) + 13) % T


@functools.lru_cache(maxsize=None)
def permutation_case(T, d, c, scale, lead=(), seed=0, vkind="unit", vmag=1.0):
    """Keys are rows of +-1, q_i = c k_{pi(i)}: the softmax of query i is one-hot on key pi(i) (logit c d scale against
    c (k_pi . k_j) scale).  v: fp16-exact magnitudes in [0.5, 2) with random sign ("unit"), or vmag * Gaussian."""
    g = _gen("perm", T, d, int(c * 16), seed, *lead)
    k = (torch.randint(0, 2, lead + (T, d), generator=g) * 2 - 1).double()
    pi = pi_map(T)
    q = c * k[..., pi, :]
    if vkind == "unit":
        mant = 1.0 + torch.randint(0, 1024, lead + (T, d), generator=g).double() / 1024.0
        expo = torch.randint(-1, 1, lead + (T, d), generator=g).double()
        sign = (torch.randint(0, 2, lead + (T, d), generator=g) * 2 - 1).double()
        v = sign * mant * torch.exp2(expo)
    else:
        v = (torch.randn(lead + (T, d), generator=g) * vmag).float().double()
    return {"q": q, "k": k, "v": v, "pi": pi, "scale": scale}


def permutation_margins(case):
    """(smallest logit margin of the target key in nats, largest off-target probability, largest off-target mass)."""
    s = exact_logits(case["q"], case["k"], case["scale"])
    T = s.shape[-1]
    tgt = torch.zeros(T, T, dtype=torch.bool)
    tgt[torch.arange(T), case["pi"]] = True
    target = s[..., tgt].reshape(s.shape[:-1])
    off = s.masked_fill(tgt, -float("inf"))
    margin = (target - off.amax(dim=-1)).min()
    p = torch.softmax(s, dim=-1).masked_fill(tgt, 0.0)
    return float(margin), float(p.max()), float(p.sum(dim=-1).max())


@functools.lru_cache(maxsize=None)
def drift_case(T, d, rising, scale=0.125, sigma=0.8, step=0.15, lead=(), seed=0, half=True):
    """Gaussian q, k, v (amplitude sigma) plus one shared unit direction u: q_i += beta u, k_j += beta t_j u with t_j
    growing linearly from 0 to 1 over the keys (falling: from 1 to 0), beta^2 scale = step (T - 1) -- the logit of every
    query drifts by `step` nats per key.  The Gaussian parts of q and k are projected orthogonal to u, so that the drift is
    the same for every query.  The row maximum of every query then lies in the last (first) 64-key tile."""
    g = _gen("drift", T, d, int(rising), seed, *lead)
    u = torch.randn(d, generator=g).double()
    u = u / u.norm()
    proj = lambda x: x - (x @ u)[..., None] * u                       # noqa: E731
    q = proj(sigma * torch.randn(lead + (T, d), generator=g).double())
    k = proj(sigma * torch.randn(lead + (T, d), generator=g).double())
    v = sigma * torch.randn(lead + (T, d), generator=g).double()
    beta = math.sqrt(step * max(T - 1, 1) / scale)
    t = torch.arange(T).double() / max(T - 1, 1)
    if not rising:
        t = 1.0 - t
    q = q + beta * u
    k = k + beta * t[:, None] * u
    rnd = r16 if half else (lambda x: x.float().double())
    return {"q": rnd(q), "k": rnd(k), "v": rnd(v), "scale": scale}


@functools.lru_cache(maxsize=None)
def flat_case(T, d, lead=(), seed=0, half=True):
    """q = 0: an exactly flat softmax, every output row is the mean of v over the tokens.  v = Gaussian + a per-channel
    offset of +-1, so that no mean is a cancellation residue (|mean| > 0.25, asserted by the host test): `to one fp16 ulp of
    the mean` then leaves room for the fp32 accumulation of T terms."""
    g = _gen("flat", T, d, seed, *lead)
    rnd = r16 if half else (lambda x: x.float().double())
    k = rnd(torch.randn(lead + (T, d), generator=g).double())
    off = (torch.randint(0, 2, lead + (1, d), generator=g) * 2 - 1).double()
    v = rnd(0.5 * torch.randn(lead + (T, d), generator=g).double() + off)
    return {"q": torch.zeros_like(k), "k": k, "v": v}


@functools.lru_cache(maxsize=None)
def gaussian_case(T, d, amp, lead=(), seed=0):
    """i.i.d. Gaussian q, k, v of amplitude amp, rounded to fp16."""
    g = _gen("gauss", T, d, int(amp * 100), seed, *lead)
    q, k, v = (r16(amp * torch.randn(lead + (T, d), generator=g).double()) for _ in range(3))
    return {"q": q, "k": k, "v": v}


@functools.lru_cache(maxsize=None)
def grad_case(T, d, lead=(), seed=0):
    """An output gradient on the grid 2^-8 Z (|x| < 8): fp16-exact, and exact under a scaling by 2^-6 .. 2^6."""
    g = _gen("grad", T, d, seed, *lead)
    x = torch.randn(lead + (T, d), generator=g).double().clamp(-7.5, 7.5)
    return torch.round(x * 256.0) / 256.0
