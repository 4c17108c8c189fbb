#!/usr/bin/env python
"""sha256 of the gfx950 code object of every file of build.SOURCES (development tool, no GPU): the proof that a host-only
change left the device code alone.  Usage:  python tools/code_object_hashes.py TREE [TREE ...]

Every TREE (a checkout of this repository) is copied to ONE staging directory before it is compiled with build.FLAGS,
because hipcc derives the compilation-unit id it plants in the code object (`__hip_cuid_*`) from the source's absolute
path and the command line: two trees compiled where they lie never compare equal.  For the same reason misc.hip gets a
fixed DDNM_BUILD_DIGEST here (a host-side string).  Prints one markdown table row per source.
"""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddnm_amd import build  # noqa: E402

LLVM = os.path.join(os.path.dirname(os.path.realpath(build._hipcc())), "..", "llvm", "bin")


def hashes(tree, stage):
    for sub in ("ddnm_amd/csrc", "include"):
        shutil.rmtree(os.path.join(stage, sub), ignore_errors=True)
        shutil.copytree(os.path.join(tree, sub), os.path.join(stage, sub))
    cflags = [f for f in build.FLAGS if f != "-shared"]

    def one(src):
        base = os.path.join(stage, src)
        extra = ['-DDDNM_BUILD_DIGEST="0"'] if src == "misc.hip" else []
        subprocess.run([build._hipcc()] + cflags + extra + ["-c", os.path.join(stage, "ddnm_amd/csrc", src), "-o", base + ".o"],
                       check=True, capture_output=True)
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={base}.fat", base + ".o", os.devnull],
                       check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={base}.fat", f"--output={base}.co"], check=True)
        with open(base + ".co", "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()
    with ThreadPoolExecutor(max_workers=8) as ex:
        return dict(zip(build.SOURCES, ex.map(one, build.SOURCES)))


if __name__ == "__main__":
    trees = sys.argv[1:]
    stage = os.path.join(tempfile.gettempdir(), "ddnm_code_object_stage")      # fixed: the ids depend on it
    cols = [hashes(os.path.abspath(t), stage) for t in trees]
    shutil.rmtree(stage, ignore_errors=True)
    print("| source | " + " | ".join(trees) + " | equal |")
    print("|---|" + "---|" * (len(trees) + 1))
    for s in build.SOURCES:
        hs = [c[s] for c in cols]
        print(f"| `{s}` | " + " | ".join(f"`{h[:16]}`" for h in hs) + f" | {'yes' if len(set(hs)) == 1 else 'NO'} |")
    sys.exit(0 if all(len({c[s] for c in cols}) == 1 for s in build.SOURCES) else 1)
