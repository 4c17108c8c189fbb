#!/usr/bin/env python
"""Records what `Model.load_state_dict` of the celeba network LEAVES BEHIND, for tests/test_weight_table.py (development
tool, no GPU: every case loads with device="cpu"; packing and the two split-fp16 guards are host code).  Usage, on a
checkout of the commit whose behaviour is to be pinned:

    python tools/record_weight_table.py | gzip -9n > tests/golden/weight_table.json.gz

Per case (cases()): the keys of `Model.w` (sorted: insertion order is not pinned), per key a digest of the value --
a tensor as [dtype, shape, sha256 prefix of its bytes], a tuple element by element, a float as the bit pattern of the
double, None as null -- and the list `s16_dropped`, in order.  Cases: the benchmark's configuration on both engines,
and the test configuration of tests/test_s16_dynamic_range_host.py with state dicts that trip each guard on each kind
of launch (a GroupNorm gamma x 3000: the normalised-operand guard; outlier columns: the weight-range guard).
"""
import hashlib
import json
import os
import struct
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RB = "down.1.block.0"       # a ResnetBlock with a 1x1 shortcut (128 -> 256 channels) of the test configuration


def digest_value(v):
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        raw = v.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy()
        return [str(v.dtype), list(v.shape), hashlib.sha256(memoryview(raw)).hexdigest()[:16]]
    if isinstance(v, (tuple, list)):
        return [digest_value(e) for e in v]
    if isinstance(v, float):
        return "f64:" + struct.pack(">d", v).hex()
    raise TypeError(f"no digest for {type(v).__name__}")


def digest(model):
    """What a case stores of a loaded `Model` (`s16_dropped` exists on the split-fp16 engine only)."""
    return {"w": {k: digest_value(model.w[k]) for k in sorted(model.w)}, "s16_dropped": getattr(model, "s16_dropped", None)}


def _scaled(sd, **factors):
    out = dict(sd)
    for k, f in factors.items():
        out[k] = sd[k] * f
    return out


def cases():
    """[(name, () -> loaded Model)]; the state dicts are built once per configuration."""
    import bench
    from ddnm_amd.guided_diffusion.models import Model
    from oracle import cases as oracle_cases
    from tests import s16_model as sm
    memo = {}

    def bench_sd():
        if "bench" not in memo:
            memo["bench"] = Model(bench.make_config(), device="cpu").random_state_dict(1234)
        return memo["bench"]

    def small_sd():
        if "small" not in memo:
            memo["small"] = small(True).random_state_dict(seed=7)
        return memo["small"]

    def small(split16=True):
        cfg = oracle_cases.weights.celeba_config(resolution=64, ch=128, ch_mult=(1, 2, 2), attn_resolutions=(16,))
        return Model(cfg, device="cpu", split16=split16)

    def gamma(name):
        return {name + ".weight": 3000.0}
    variants = [
        ("base", lambda sd: sd),
        ("spec", lambda sd: sm.spec_state_dict(sd, 0)),
        ("spec_outlier_layers", lambda sd: sm.spec_state_dict(sd, 0, sm.OUTLIER_LAYERS)),
        ("spec_outlier_shortcut", lambda sd: sm.spec_state_dict(sd, 0, (RB + ".nin_shortcut",))),
        ("gamma_norm2", lambda sd: _scaled(sd, **gamma("down.0.block.0.norm2"))),
        ("gamma_norm1_of_shortcut_block", lambda sd: _scaled(sd, **gamma(RB + ".norm1"))),
        ("gamma_attn_norm", lambda sd: _scaled(sd, **gamma("mid.attn_1.norm"))),
        ("spec_outlier_shortcut_gamma_norm2", lambda sd: _scaled(sm.spec_state_dict(sd, 0, (RB + ".nin_shortcut",)),
                                                                 **gamma(RB + ".norm2"))),
        ("spec_outlier_proj_out_downsample", lambda sd: sm.spec_state_dict(sd, 0, ("mid.attn_1.proj_out",
                                                                                   "down.0.downsample.conv"))),
    ]
    out = [(f"bench_split16_{s}", lambda s=s: Model(bench.make_config(), device="cpu", split16=s).load_state_dict(bench_sd()))
           for s in (True, False)]
    out += [(f"small_{name}", lambda make=make: small().load_state_dict(make(small_sd()))) for name, make in variants]
    return out


if __name__ == "__main__":
    table = {}
    for name, load in cases():
        table[name] = digest(load())
        print(f"{name}: {len(table[name]['w'])} keys, s16_dropped = {table[name]['s16_dropped']}", file=sys.stderr)
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(["git", "status", "--porcelain", "ddnm_amd"], cwd=ROOT, capture_output=True, text=True).stdout.strip()

    def case(d):              # one key per line: a later re-record shows up key by key
        rows = ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}" for k, v in d["w"].items())
        return f'{{"s16_dropped":{json.dumps(d["s16_dropped"])},\n"w":{{\n{rows}\n}}}}'
    sys.stdout.write(f'{{"recorded_at":{json.dumps(commit + (" (ddnm_amd modified)" if dirty else ""))},\n"cases":{{\n' +
                     ",\n".join(f"{json.dumps(n)}:{case(d)}" for n, d in table.items()) + "\n}}\n")
