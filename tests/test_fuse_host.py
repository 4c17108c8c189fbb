"""CPU tests of batch fusing (DDNM_FUSE_BATCHES) and per-image Philox keys: the keyed entry points are exported and
prototyped, the runner's grouping of loader batches, the key table of ops.KeyedPhiloxNoise, and the keyed draw rule
against the numpy Philox oracle."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYED = ["ddnm_randn_philox_keyed_f32", "ddnm_step_combine_keyed_f32", "ddnm_step_sr_avgpool_keyed_f32",
         "ddnm_step_color_keyed_f32", "ddnm_step_inpaint_keyed_f32", "ddnm_step_denoise_keyed_f32"]


def test_keyed_entry_points_are_declared_prototyped_and_exported():
    from ddnm_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ddnm_hip.h")).read(), flags=re.S)
    build.build()
    lib = _lib.lib()
    for name in KEYED:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name
    # the keyed step entry points take the unkeyed ones' arguments, the key table in place of the noise tensor
    for name in KEYED[1:]:
        assert _lib.PROTOTYPES[name] == _lib.PROTOTYPES[name.replace("_keyed_f32", "_f32")], name
    assert lib.ddnm_version() == _lib.ABI_VERSION == 7


def _groups(n_items, batch_size, rank, world, k):
    from ddnm_amd.guided_diffusion.diffusion import fuse_groups
    return [[bi for bi, _, _ in g] for g in fuse_groups(n_items, batch_size, rank, world, k)]


def test_fuse_groups_one_rank():
    assert _groups(6, 1, 0, 1, 4) == [[0, 1, 2, 3], [4, 5]]              # ragged tail
    assert _groups(6, 1, 0, 1, 3) == [[0, 1, 2], [3, 4, 5]]
    assert _groups(5, 2, 0, 1, 2) == [[0, 1], [2]]                       # ragged last loader batch
    assert _groups(6, 1, 0, 1, 1) == [[i] for i in range(6)]
    from ddnm_amd.guided_diffusion.diffusion import fuse_groups
    # (batch index, first image, batch size): image indices in the loader order (the runner adds --subset_start)
    assert fuse_groups(5, 2, 0, 1, 4) == [[(0, 0, 2), (1, 2, 2), (2, 4, 1)]]


def test_fuse_groups_deal_mode():
    # batch_size < world: batch bi belongs to rank bi % world; consecutive OWNED batches fuse
    assert _groups(7, 1, 0, 2, 2) == [[0, 2], [4, 6]]
    assert _groups(7, 1, 1, 2, 2) == [[1, 3], [5]]
    assert _groups(7, 1, 0, 3, 2) == [[0, 3], [6]]
    assert _groups(7, 1, 1, 3, 2) == [[1, 4]]
    assert _groups(7, 1, 2, 3, 3) == [[2, 5]]
    assert _groups(10, 2, 1, 3, 4) == [[1, 4]]                            # 5 batches of 2, 3 ranks
    assert _groups(10, 1, 0, 2, 3) == [[0, 2, 4], [6, 8]]
    owned = sorted(bi for r in range(3) for g in _groups(11, 1, r, 3, 4) for bi in g)
    assert owned == list(range(11))                                       # every batch once, over all ranks


def test_fuse_groups_split_mode_is_not_fused():
    # batch_size >= world > 1: every rank restores a slice of every batch -> one batch per group
    assert _groups(8, 4, 0, 2, 4) == [[0], [1]]
    assert _groups(8, 4, 1, 2, 4) == [[0], [1]]
    assert _groups(9, 3, 2, 3, 2) == [[0], [1], [2]]


def test_fuse_switch(monkeypatch):
    from ddnm_amd.guided_diffusion.diffusion import fuse_batches
    monkeypatch.delenv("DDNM_FUSE_BATCHES", raising=False)
    assert fuse_batches() == 1
    monkeypatch.setenv("DDNM_FUSE_BATCHES", "8")
    assert fuse_batches() == 8
    monkeypatch.setenv("DDNM_FUSE_BATCHES", "0")
    with pytest.raises(ValueError):
        fuse_batches()


def test_keyed_noise_key_table_from_per_batch_sources():
    from ddnm_amd import ops
    from ddnm_amd.guided_diffusion.diffusion import _mix64
    srcs = [ops.PhiloxNoise(_mix64(0, bi), image_base=base) for bi, base in ((3, 0), (4, 2))]
    kn = ops.KeyedPhiloxNoise.from_sources([(srcs[0], 0), (srcs[0], 1), (srcs[1], 0)])
    assert len(kn) == 3
    t = kn._host.numpy().view(np.uint32)
    assert t.shape == (3, 4)
    for row, (src, i) in zip(t, [(srcs[0], 0), (srcs[0], 1), (srcs[1], 0)]):
        assert list(row) == [src.seed_lo, src.seed_hi, src.image_base + i, 0]
    assert ops.KeyedPhiloxNoise.concat([(srcs[1], 5)]).image_ctrs == [7]
    with pytest.raises(ValueError):
        ops.KeyedPhiloxNoise([1, 2], [0])
    s = kn.stamp(ops.StepScalars(), 17)
    assert s.rng_iter == 17 and s.rng_on == 1


def keyed_oracle(keys, ctrs, n, iteration):
    """The keyed draw rule: image b, element r = normal4(key_b, r // 4, iteration, ctr_b)[r % 4], any n."""
    from oracle import philox
    rows = []
    for key, ctr in zip(keys, ctrs):
        v = philox.normal4(key & 0xFFFFFFFF, key >> 32, np.arange((n + 3) // 4), iteration, ctr).reshape(-1)
        rows.append(v[:n])
    return np.stack(rows, 0)


@pytest.mark.parametrize("n", [5, 6, 7, 8, 145314 % 64 + 64])
def test_keyed_rule_extends_the_per_batch_draw(n):
    """Rows {seed, seed, base + b} of the keyed rule are the per-batch draw (oracle.philox.randn) on every whole block of
    four, and an odd length is the prefix of the next multiple of four."""
    from oracle import philox
    seed, base = 0x1234_5678_9ABC_DEF0, 3
    got = keyed_oracle([seed] * 3, [base, base + 1, base + 2], n, 7)
    n4 = (n + 3) // 4 * 4
    ref = philox.randn(seed, 3, n4, 7, image_base=base)
    np.testing.assert_array_equal(got, ref[:, :n])
    mixed = keyed_oracle([seed, seed ^ 1, seed], [0, 0, 9], n, 7)
    np.testing.assert_array_equal(mixed[2], philox.randn(seed, 1, n4, 7, image_base=9)[0, :n])
    assert not np.array_equal(mixed[0], mixed[1])
