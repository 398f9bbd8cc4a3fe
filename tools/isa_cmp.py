#!/usr/bin/env python3
"""Compare the gfx950 machine code of every kernel of two builds.

    tools/isa_cmp.py <tree or dir of .s> <tree or dir of .s> [--keep DIR] [-j N] [--rename OLD=NEW ...]

A tree is a checkout of this repository: every .hip / .cpp in its build.py's
SOURCES is compiled device-only to assembly (-S) with build.py's flags.  A
directory without ar_slam_amd/build.py is taken as a set of .s files made that
way.  For every kernel (.amdhsa_kernel) the text between `<symbol>:` and the
following `.Lfunc_end<n>:` is normalized -- comment and directive lines
dropped, the function index taken out of `.LBB<n>_` labels -- and hashed;
kernels are matched across the two sides by mangled name, whichever file they
live in.  --rename OLD=NEW replaces OLD by NEW in the first side's names before
the match, for a change that moves a type of a kernel's signature to another
namespace: the mangled name spells the type, the code does not.  Printed per
kernel: line count, hash, and the resource lines of the code object's metadata
(VGPRs, SGPRs, spills, scratch and LDS bytes).

Exit status 0: every kernel is present on both sides with identical code and
resources.  A diff of two builds; needs hipcc, no GPU.
"""
import argparse
import concurrent.futures
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

RESOURCES = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("sgpr_spill", ".sgpr_spill_count"),
             ("vgpr_spill", ".vgpr_spill_count"), ("scratch", ".private_segment_fixed_size"),
             ("lds", ".group_segment_fixed_size"))


def normalize(body):
    """The instruction and label lines of a function body, comments and directives dropped,
    `.LBB<n>_<m>` rewritten to `.LBB_<m>` (n is the function's index in its file)."""
    out = []
    for line in body.splitlines():
        line = line.split(";", 1)[0].strip()
        if not line or (line.startswith(".") and not line.startswith(".LBB")):
            continue
        out.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def kernels_of(asm):
    """{mangled name: {"lines", "hash", resources...}} of one assembly file's kernels."""
    found = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M):
        m = re.search(r"^" + re.escape(name) + r":.*?\n(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S)
        if not m:
            raise ValueError(f"no body for kernel {name}")
        lines = normalize(m.group(1))
        found[name] = {"lines": len(lines), "hash": digest(lines)}
    # the metadata note: one YAML map per kernel, fields in alphabetical order around .name
    for block in re.split(r"^\s*- \.agpr_count:", asm, flags=re.M)[1:]:
        m = re.search(r"^\s*\.name:\s+(\S+)", block, re.M)
        if not m or m.group(1) not in found:
            continue
        for key, field in RESOURCES:
            v = re.search(r"^\s*" + re.escape(field) + r":\s+(\d+)", block, re.M)
            found[m.group(1)][key] = int(v.group(1)) if v else -1
    return found


def _build_module(tree):
    spec = importlib.util.spec_from_file_location("arslam_build_" + hashlib.md5(tree.encode()).hexdigest(),
                                                  os.path.join(tree, "ar_slam_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_tree(tree, out, jobs):
    """Device-only -S compile of the tree's SOURCES into out/; returns the .s paths."""
    here = _build_module(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    there = _build_module(tree)
    csrc = os.path.join(tree, "ar_slam_amd", "csrc")
    flags = here.hip_flags(tree, "isa_cmp")
    os.makedirs(out, exist_ok=True)

    def one(src):
        dst = os.path.join(out, os.path.splitext(src)[0] + ".s")
        cmd = [here.hipcc()] + flags + (["-x", "hip"] if src.endswith(".cpp") else []) + \
              ["--cuda-device-only", "-S", os.path.join(csrc, src), "-o", dst]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{p.stdout}")
        return dst

    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        return list(ex.map(one, there.SOURCES))


def load_side(path, keep, jobs):
    path = os.path.abspath(path)
    if os.path.exists(os.path.join(path, "ar_slam_amd", "build.py")):
        files = compile_tree(path, keep, jobs)
    else:
        files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith(".s"))
    kernels = {}
    for f in files:
        with open(f) as fh:
            for name, k in kernels_of(fh.read()).items():
                if name in kernels:
                    raise ValueError(f"kernel {name} defined twice ({kernels[name]['file']}, {f})")
                kernels[name] = dict(k, file=os.path.basename(f))
    return kernels


def fmt(k):
    res = " ".join(f"{key}={k.get(key, -1)}" for key, _ in RESOURCES)
    return f"{k['file']:<18} lines={k['lines']:<6} {k['hash']} {res}"


def compare(a, b, out=sys.stdout):
    """Print the table; the number of kernels that are missing on one side or differ."""
    bad = 0
    for name in sorted(set(a) | set(b)):
        ka, kb = a.get(name), b.get(name)
        if ka and kb and all(ka[f] == kb[f] for f in ka if f != "file"):
            print(f"same     {name}\n           {fmt(kb)}", file=out)
            continue
        bad += 1
        print(f"{'DIFFERS ' if ka and kb else 'MISSING '} {name}", file=out)
        print(f"         a {fmt(ka) if ka else '-'}\n         b {fmt(kb) if kb else '-'}", file=out)
    print(f"{len(set(a) | set(b))} kernels, {bad} missing or different", file=out)
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--keep", help="keep the assembly files under DIR/a and DIR/b")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="replace OLD by NEW in the first side's kernel names before matching")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        base = args.keep or tmp
        a = load_side(args.a, os.path.join(base, "a"), args.j)
        b = load_side(args.b, os.path.join(base, "b"), args.j)
    for old, new in (r.split("=", 1) for r in args.rename):
        a = {name.replace(old, new): k for name, k in a.items()}
    return 1 if compare(a, b) else 0


if __name__ == "__main__":
    sys.exit(main())
