"""The conditions the GPU attention edge tests (test_gpu_attention_edges.py) rely on, asserted from the exact float64
reference alone -- no GPU: the one-hot margins of the permutation cases, the tile of the row maximum of the drift cases,
the non-degenerate means of the flat case, and the agreement of the fp64 model of attn16.hip / attn16_bwd.hip with the
exact reference at the fp16-probability bars of the existing whole-tensor tests."""
import math

import pytest
import torch

from tests import attn_model as AM
from tests.helpers import rel

ATTN16_T = (64, 128, 192, 320, 384)
ATTN16_NH = (1, 3)                                   # C = 64, 192
FUSED_C = (128, 256, 384, 512)
FUSED_T = (32, 96, 160, 224, 256)
PERM_SEED_T1024 = 1                                  # lead = (): the seed at which T = 1024 meets the 27-nat condition


def test_pi_is_a_bijection_where_the_backward_tests_need_one():
    for T in ATTN16_T + (1024, 32, 96, 160, 256):
        assert sorted(AM.pi_map(T).tolist()) == list(range(T))
    # every 32-query block reaches every position inside a group of 16 keys and every 64-key tile (all but one of the six
    # tiles at T = 384)
    for T in ATTN16_T:
        pi = AM.pi_map(T).reshape(T // 32, 32)
        for blk in pi:
            assert len(set((blk // 64).tolist())) >= min(T // 64, 5)
            assert set((blk % 16).tolist()) == set(range(16))


@pytest.mark.parametrize("T", ATTN16_T + (1024,))
def test_attn16_permutation_case_is_one_hot(T):
    """c = 8, d = 64, scale = 1/8: margin >= 27 nats, largest off-target probability <= 2^-26 (it rounds to zero in fp16,
    whose smallest subnormal is 2^-24).  Measured: margins 28 .. 32 nats, off-target <= 6.9e-13."""
    leads = [(2, nh) for nh in ATTN16_NH] if T != 1024 else [()]
    for lead in leads:
        cs = AM.permutation_case(T, 64, 8.0, 0.125, lead=lead, seed=PERM_SEED_T1024 if T == 1024 else 0)
        margin, pmax, _ = AM.permutation_margins(cs)
        assert margin >= 27.0 and pmax <= 2.0 ** -26, (T, lead, margin, pmax)
        assert cs["v"].abs().min() >= 0.5 and cs["v"].abs().max() < 2.0 and torch.equal(AM.r16(cs["v"]), cs["v"])


@pytest.mark.parametrize("T", ATTN16_T)
def test_attn16_large_logit_case(T):
    """c = 62.5: the target logit is 500 nats and every other logit at least 200 nats below it (measured: >= 218)."""
    for nh in ATTN16_NH:
        cs = AM.permutation_case(T, 64, 62.5, 0.125, lead=(2, nh))
        s = AM.exact_logits(cs["q"], cs["k"], 0.125)
        margin, pmax, _ = AM.permutation_margins(cs)
        assert float(s.max()) == 500.0 and margin >= 200.0 and pmax < 1e-80, (margin, pmax)


@pytest.mark.parametrize("C", FUSED_C)
def test_fused_permutation_case_is_one_hot(C):
    """c = 4, d = C, scale = C^-0.5: margin >= 27 nats, off-target probability <= 2^-26 (times 2^14 it is below half the
    smallest fp16 subnormal).  Measured: margin >= 28.99 nats, off-target <= 2.6e-13 (C = 128)."""
    for T in FUSED_T:
        cs = AM.permutation_case(T, C, 4.0, C ** -0.5, lead=(2,), vkind="gauss")
        margin, pmax, mass = AM.permutation_margins(cs)
        assert margin >= 27.0 and pmax <= 2.0 ** -26, (C, T, margin, pmax)
        assert mass * 2.0 ** 14 < 2.0 ** -25


@pytest.mark.parametrize("rising", [True, False])
def test_drift_cases_put_the_row_maximum_in_the_intended_tile(rising):
    for T in ATTN16_T:
        for nh in ATTN16_NH:
            cs = AM.drift_case(T, 64, rising, lead=(2, nh))
            tile = AM.exact_logits(cs["q"], cs["k"], 0.125).argmax(dim=-1) // AM.KT
            assert bool((tile == (T // AM.KT - 1 if rising else 0)).all()), (T, nh)
    C, T = 512, 256
    cs = AM.drift_case(T, C, rising, scale=C ** -0.5, sigma=4.0 / C ** 0.25, lead=(2,), half=False)
    tile = AM.exact_logits(cs["q"], cs["k"], cs["scale"]).argmax(dim=-1) // AM.KT
    assert bool((tile == (T // AM.KT - 1 if rising else 0)).all())


def test_flat_case_means_are_no_cancellation_residue():
    for T in ATTN16_T:
        for nh in ATTN16_NH:
            v = AM.flat_case(T, 64, lead=(2, nh))["v"]
            assert float(v.mean(dim=-2).abs().min()) > 0.25
            # fp32 accumulation of T terms against one fp16 ulp of the mean: T 2^-24 mean|v| << 2^-11 |mean|
            assert float((T * 2.0 ** -24 * v.abs().mean(dim=-2) / AM.ulp16(v.mean(dim=-2))).max()) < 0.1
    for C in FUSED_C:
        for T in FUSED_T:
            v = AM.flat_case(T, C, lead=(2,), half=False)["v"]
            assert float(v.mean(dim=-2).abs().min()) > 0.25


@pytest.mark.parametrize("T,nh", [(64, 3), (192, 1), (384, 3)])
def test_attn16_model_agrees_with_the_exact_reference(T, nh):
    """On Gaussian inputs the model stays within the whole-tensor bars of the existing GPU tests (2e-3 for the output and
    lse, 4e-3 for the gradients): its fp16 roundings are the ones those bars were set for."""
    cs = AM.gaussian_case(T, 64, 1.5, lead=(2, nh))
    o, lse = AM.exact_attention(cs["q"], cs["k"], cs["v"], 0.125)
    om, lm = AM.attn16_model_fwd(cs["q"], cs["k"], cs["v"])
    assert rel(om, o) < 2e-3 and float((lm - lse).abs().max()) < 2e-3
    cs = AM.gaussian_case(T, 64, 0.8, lead=(2, nh))
    dO = AM.grad_case(T, 64, lead=(2, nh))
    om, lm = AM.attn16_model_fwd(cs["q"], cs["k"], cs["v"])
    want = AM.exact_attention_grads(cs["q"], cs["k"], cs["v"], dO, 0.125)
    got = AM.attn16_model_bwd(cs["q"], cs["k"], cs["v"], om, lm, dO)
    for name, a, b in zip("qkv", got, want):
        assert rel(a, b) < 4e-3, (name, rel(a, b))
    # the tile loop of the model is the plain softmax when nothing is rounded: one tile or six, the same lse
    assert float((lm - AM.exact_attention(cs["q"], cs["k"], cs["v"], 0.125)[1]).abs().max()) < 2e-3


def test_model_roundings_are_where_the_kernels_round():
    """A one-hot row: P is exactly 1 on the target and 0 elsewhere, so the model returns v[pi] bit for bit and lse = the
    target's base-2 logit; a flat row: lse = log2 T and the output is the fp16 mean."""
    cs = AM.permutation_case(192, 64, 8.0, 0.125, lead=(2, 1))
    om, lm = AM.attn16_model_fwd(cs["q"], cs["k"], cs["v"])
    assert torch.equal(om, cs["v"][..., cs["pi"], :])
    assert float((lm - 64.0 * AM.LOG2E).abs().max()) < 2.0 ** -20 * 64.0 * AM.LOG2E
    fc = AM.flat_case(192, 64, lead=(2, 1))
    om, lm = AM.attn16_model_fwd(fc["q"], fc["k"], fc["v"])
    assert float((lm - math.log2(192)).abs().max()) < 2.0 ** -20
    mean = AM.r16(fc["v"].mean(dim=-2, keepdim=True)).expand_as(om)
    assert bool(((om - mean).abs() <= AM.ulp16(mean)).all())
