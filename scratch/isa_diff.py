#!/usr/bin/env python3
"""Are two trees the same device program?  Builds the gfx950 ISA listings of the three translation units that include
lmpc_solve_kernel.hip (lmpc_lib, lmpc_lib_minreg, lmpc_lib_w2: the Makefile's FLAGS plus --cuda-device-only -S), once for the
product and once with -DLMPC_DEBUG_HOOKS, from both trees, and compares them function by function -- instructions, .amdhsa_*
directives and the amdhsa.kernels metadata entry -- after replacing the per-compilation __hip_cuid_<hash> symbol by a constant.

Per function it reports one of
    identical               every line equal
    renamed registers only  equal after a consistent one-to-one renaming of registers (v / s / a, singles and ranges): opcodes,
                            order, immediates, offsets, wait counts and metadata are equal; the number of differing lines is given
    different               anything else (the two versions are written to <out>/diff/ for a look with diff)
and exits 1 if any function is different or missing.  Meant for refactors of the solve kernel: the check needs no GPU.

usage: isa_diff.py TREE_A TREE_B [--out DIR] [--jobs N (<= 16)] [--reuse] [--units lmpc_lib_w2,...] [--no-dbg] [--rename OLD=NEW ...]
  --reuse keeps listings already under <out>/a or <out>/b (a parent built once serves many comparisons)
  --rename OLD=NEW (repeatable) states that tree B calls NEW what tree A calls OLD: every occurrence of OLD in listing A -- mangled
    names or prefixes of them, e.g. _Z14lmpc_polish_w2=_Z19lmpc_polish_call_w2 -- is replaced before the split, so that a renamed
    function and the callers that name it are compared by content instead of reported missing
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys

UNITS = {"lmpc_lib": [], "lmpc_lib_minreg": ["-mllvm", "-amdgpu-sched-strategy=iterative-minreg"], "lmpc_lib_w2": []}
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "-Wall"]
CSRC = "racing-lmpc-ros2_amd/csrc"

CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
FUNC = re.compile(r"^\s*\.type\s+(\S+),@function")
META = re.compile(r"^  - \.")  # an entry of the amdhsa.kernels list
META_NAME = re.compile(r"^\s+\.name:\s+(\S+)")
REG = re.compile(r"\b([vsa])(?:(\d+)|\[(\d+):(\d+)\])(?![\w\[])")


def build(tree, out, unit, dbg, reuse):
    path = os.path.join(out, unit + ("_dbg" if dbg else "") + ".s")
    if reuse and os.path.exists(path) and os.path.getsize(path) > 0:
        return path
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + FLAGS + UNITS[unit] + (["-DLMPC_DEBUG_HOOKS"] if dbg else []) + ["--cuda-device-only", "-S", "-o", path, unit + ".hip"]
    subprocess.run(cmd, cwd=os.path.join(tree, CSRC), check=True)
    return path


def split(path, renames=()):
    """listing -> {name: lines}: one part per function (body and kernel descriptor), one per metadata entry, the rest as '(module)'"""
    parts = {"(module)": []}
    cur = parts["(module)"]
    meta = None
    for line in open(path):
        line = CUID.sub("__hip_cuid_X", line.rstrip("\n"))
        for old, new in renames:
            line = line.replace(old, new)
        m = FUNC.match(line)
        if m:
            cur = parts.setdefault(m.group(1), [])
            meta = None
        elif line.startswith("\t.amdgpu_metadata") or line.startswith("amdhsa.") or line.startswith("\t.end_amdgpu_metadata"):
            cur = parts["(module)"]
            meta = None
        elif META.match(line):
            meta = []
            cur = meta
        cur.append(line)
        if meta is not None:
            n = META_NAME.match(line)
            if n:  # the entry's name comes after its arguments: file what was gathered under it
                cur = parts.setdefault(n.group(1), [])
                cur.extend(meta)
                meta = None
    return parts


def renamed_only(a, b):
    """number of differing lines if b is a with registers consistently renamed, else -1"""
    if len(a) != len(b):
        return -1
    fwd, bwd, n = {}, {}, 0
    for la, lb in zip(a, b):
        if la == lb and not REG.search(la):
            continue
        ra, rb = REG.findall(la), REG.findall(lb)
        if len(ra) != len(rb) or REG.sub("R", la) != REG.sub("R", lb):
            return -1
        for (ca, sa, loa, hia), (cb, sb, lob, hib) in zip(ra, rb):
            xa = [int(sa)] if sa else list(range(int(loa), int(hia) + 1))
            xb = [int(sb)] if sb else list(range(int(lob), int(hib) + 1))
            if ca != cb or bool(sa) != bool(sb) or len(xa) != len(xb):
                return -1
            for ia, ib in zip(xa, xb):
                if fwd.setdefault((ca, ia), ib) != ib or bwd.setdefault((ca, ib), ia) != ia:
                    return -1
        n += la != lb
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--out", default="isa_diff_out")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--reuse", action="store_true")
    ap.add_argument("--units", default=",".join(UNITS))
    ap.add_argument("--no-dbg", action="store_true")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    units = args.units.split(",")
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    cfgs = [(u, d) for u in units for d in ([False] if args.no_dbg else [False, True])]
    outs = {"a": os.path.join(args.out, "a"), "b": os.path.join(args.out, "b")}
    for d in list(outs.values()) + [os.path.join(args.out, "diff")]:
        os.makedirs(d, exist_ok=True)
    trees = {"a": os.path.abspath(args.tree_a), "b": os.path.abspath(args.tree_b)}
    with concurrent.futures.ThreadPoolExecutor(max(1, min(16, args.jobs))) as pool:
        # the main unit takes minutes, the others seconds: start the long ones first
        jobs = {(s, u, d): pool.submit(build, trees[s], os.path.abspath(outs[s]), u, d, args.reuse)
                for u, d in sorted(cfgs, key=lambda x: x[0] != "lmpc_lib") for s in "ab"}
        paths = {k: f.result() for k, f in jobs.items()}
    bad = 0
    for u, d in cfgs:
        tag = u + ("_dbg" if d else "")
        pa, pb = split(paths[("a", u, d)], renames), split(paths[("b", u, d)])
        print("== %s: %d / %d lines" % (tag, sum(map(len, pa.values())), sum(map(len, pb.values()))))
        for name in list(pa) + [n for n in pb if n not in pa]:
            if name not in pa or name not in pb:
                print("  MISSING in %s   %s" % ("a" if name not in pa else "b", name))
                bad += 1
                continue
            a, b = pa[name], pb[name]
            if a == b:
                verdict = "identical"
            else:
                n = renamed_only(a, b)
                if n >= 0:
                    verdict = "renamed registers only (%d lines)" % n
                else:
                    bad += 1
                    verdict = "different (%d / %d lines)" % (len(a), len(b))
                    for s, x in (("a", a), ("b", b)):
                        with open(os.path.join(args.out, "diff", "%s.%s.%s.s" % (tag, name[:120], s)), "w") as f:
                            f.write("\n".join(x) + "\n")
            print("  %-34s %s" % (verdict, name))
    print("RESULT: %s" % ("every function identical or renamed registers only" if not bad else "%d function(s) different or missing" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
