#!/usr/bin/env python
"""sha256 of the gfx950 code object of every file of build.SOURCES (development tool, no GPU): the proof that a host-only
change left the device code alone.  Usage:  python tools/code_object_hashes.py [--isa] [--sources a.hip,b.hip] TREE [TREE ...]

Every TREE (a checkout of this repository) is copied to ONE staging directory before it is compiled with build.FLAGS,
because hipcc derives the compilation-unit id it plants in the code object (`__hip_cuid_*`) from the source's absolute
path and the command line: two trees compiled where they lie never compare equal.  For the same reason misc.hip gets a
fixed DDNM_BUILD_DIGEST here (a host-side string).  Prints one markdown table row per source.

--isa: for a change that MOVES device code without meaning to change it.  Adds, per kernel of every source whose code
object differs between the trees, the instruction count, the sha256 of the mnemonic stream (first token of every
instruction of `llvm-objdump -d`) and the resource notes of `llvm-readelf --notes` (VGPRs, AGPRs, SGPRs, LDS bytes,
scratch bytes, SGPR / VGPR spills), and a tier per source: A = byte-identical code object, B = every kernel has the same
count, mnemonic hash and notes (what differs is register numbers and the operand order of commutative instructions),
C = anything else.  Exit status 0 only when every source is A (or, with --isa, A or B).
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddnm_amd import build  # noqa: E402

LLVM = os.path.join(os.path.dirname(os.path.realpath(build._hipcc())), "..", "llvm", "bin")
NOTES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
         "sgpr_spill_count", "vgpr_spill_count")


def kernel_isa(co):
    """{kernel: (instruction count, sha256 of the mnemonic stream, resource notes in the order of NOTES)} of a code object"""
    notes, cur = {}, None
    for line in subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout.splitlines():
        if line.startswith("  - ."):
            cur = {}                                            # a new entry of amdhsa.kernels (its .args nest deeper)
        m = re.match(r"(?:  - |    )\.(\w+):\s+(\S+)\s*$", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                notes[m.group(2)] = cur
    streams, sym = {}, None
    for line in subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout.splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:$", line)
        if m:
            sym = m.group(1)
        elif sym in notes and line[:1].isspace() and line.strip():
            streams.setdefault(sym, []).append(line.split()[0])
    return {k: (len(streams.get(k, ())), hashlib.sha256("\n".join(streams.get(k, ())).encode()).hexdigest(),
                tuple(n.get(f, "-") for f in NOTES)) for k, n in notes.items()}


def hashes(tree, stage, sources, isa):
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
            return hashlib.sha256(f.read()).hexdigest(), (kernel_isa(base + ".co") if isa else None)
    with ThreadPoolExecutor(max_workers=8) as ex:
        return dict(zip(sources, ex.map(one, sources)))


if __name__ == "__main__":
    args = sys.argv[1:]
    isa = "--isa" in args
    sources = list(build.SOURCES)
    if "--sources" in args:
        i = args.index("--sources")
        sources = args[i + 1].split(",")
        del args[i:i + 2]
    trees = [a for a in args if a != "--isa"]
    stage = os.path.join(tempfile.gettempdir(), "ddnm_code_object_stage")      # fixed: the ids depend on it
    cols = [hashes(os.path.abspath(t), stage, sources, isa) for t in trees]
    shutil.rmtree(stage, ignore_errors=True)
    print("| source | " + " | ".join(trees) + " | equal |" + (" tier |" if isa else ""))
    print("|---|" + "---|" * (len(trees) + 1 + isa))
    tiers = {}
    for s in sources:
        hs = [c[s][0] for c in cols]
        tiers[s] = "A" if len(set(hs)) == 1 else ("B" if isa and all(c[s][1] == cols[0][s][1] for c in cols) else "C")
        print(f"| `{s}` | " + " | ".join(f"`{h[:16]}`" for h in hs) + f" | {'yes' if len(set(hs)) == 1 else 'NO'} |" + (f" {tiers[s]} |" if isa else ""))
    if isa:
        print("\n| source | kernel | tree | instructions | mnemonic sha256 | " + " | ".join(NOTES) + " |")
        print("|---|---|---|---|---|" + "---|" * len(NOTES))
        for s in sources:
            if tiers[s] == "A":
                continue
            for k in sorted(set().union(*(c[s][1] for c in cols))):
                for t, c in zip(trees, cols):
                    n, h, notes = c[s][1].get(k, (0, "-", ("-",) * len(NOTES)))
                    print(f"| `{s}` | `{k}` | {t} | {n} | `{h[:16]}` | " + " | ".join(notes) + " |")
    sys.exit(0 if all(t != "C" for t in tiers.values()) else 1)
