"""`Model.load_state_dict` of the celeba network leaves behind what it left when tests/golden/weight_table.json.gz was
recorded (tools/record_weight_table.py): per case the keys of the weight dictionary, every tensor in it -- also inside the
(pack, scale, skip pack) tuples -- by dtype, shape and a hash of its bytes, every float by its bits, and `s16_dropped` in
order.  The cases trip each of the loader's two split-fp16 guards on each kind of launch.  No GPU needed: packing and the
guards are host code.  A refactor of the loader must leave the table alone: a difference means the loader is wrong.

The loader also converts every checkpoint tensor once (test_every_weight_is_fetched_once)."""
import collections
import gzip
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_weight_table as rec  # noqa: E402

CASES = dict(rec.cases())


@pytest.fixture(scope="module")
def table():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "weight_table.json.gz"), "rt") as f:
        return json.load(f)


def test_recorder_still_generates_the_recorded_cases(table):
    assert list(CASES) == list(table["cases"])


@pytest.mark.parametrize("case", list(CASES))
def test_loader_leaves_what_was_recorded(table, case):
    want = table["cases"][case]
    got = json.loads(json.dumps(rec.digest(CASES[case]())))        # (tuples as lists, like the stored table)
    assert got["s16_dropped"] == want["s16_dropped"]
    assert set(got["w"]) == set(want["w"]), sorted(set(got["w"]) ^ set(want["w"]))
    diff = [k for k in want["w"] if got["w"][k] != want["w"][k]]
    assert not diff, f"{len(diff)} keys differ, first: {diff[0]} = {got['w'][diff[0]]}, recorded {want['w'][diff[0]]}"


def test_table_trips_both_guards_on_every_kind_of_launch(table):
    """What the cases are there for: the first guard on conv1, conv2 and qkv; the second on conv1, a conv2 + shortcut pair,
    an un-fused shortcut after the first took its conv2, proj_out, a downsample and an upsample convolution."""
    dropped = {n: c["s16_dropped"] for n, c in table["cases"].items()}
    assert dropped["bench_split16_True"] == dropped["small_base"] == dropped["small_spec"] == []
    assert dropped["bench_split16_False"] is None
    assert dropped["small_spec_outlier_layers"] == ["down.1.block.0.conv1", "up.1.upsample.conv"]
    assert dropped["small_spec_outlier_shortcut"] == ["down.1.block.0.conv2"]
    assert dropped["small_gamma_norm2"] == ["down.0.block.0.conv2"]
    assert dropped["small_gamma_norm1_of_shortcut_block"] == ["down.1.block.0.conv1"]
    assert dropped["small_gamma_attn_norm"] == ["mid.attn_1.qkv"]
    assert dropped["small_spec_outlier_shortcut_gamma_norm2"] == ["down.1.block.0.conv2", "down.1.block.0.nin_shortcut"]
    assert dropped["small_spec_outlier_proj_out_downsample"] == ["mid.attn_1.proj_out", "down.0.downsample.conv"]
    w = table["cases"]["small_spec_outlier_shortcut_gamma_norm2"]["w"]
    assert "down.1.block.0.conv1.s16" in w and "up.1.upsample.conv.s16_subpixel" in w
    assert not any(k.endswith(".s16") for k in table["cases"]["bench_split16_False"]["w"])


class _Counting(dict):
    def __init__(self, *a):
        super().__init__(*a)
        self.lookups = collections.Counter()

    def __getitem__(self, k):
        self.lookups[k] += 1
        return super().__getitem__(k)


def test_every_weight_is_fetched_once():
    """One load of the benchmark's checkpoint looks every convolution weight up once -- the fp32 pack, the split pack, the
    fused pack and the guards share the converted tensor -- except the attention q / k / v weights, which the operand
    scales of the fused attention kernel read a second time on the host.  (942 lookups for 450 tensors before the loader
    packed from one table of launches.)"""
    import bench
    from ddnm_amd.guided_diffusion.models import Model
    m = Model(bench.make_config(), device="cpu", split16=True)
    sd = _Counting(m.random_state_dict(1234))
    m.load_state_dict(sd)
    total = sum(sd.lookups.values())
    print(f"{len(sd)} tensors, {total} lookups")
    assert set(sd.lookups) == set(sd)
    for k, v in sd.items():
        if v.dim() == 4:
            qkv = k.rsplit(".", 2)[-2] in ("q", "k", "v")
            assert sd.lookups[k] <= (2 if qkv else 1), (k, sd.lookups[k])
    assert total < 942
