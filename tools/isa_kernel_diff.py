#!/usr/bin/env python3
"""Kernel-by-kernel companion of tools/isa_diff.sh, for a change that ADDS kernels to a translation unit: isa_diff.sh compares
whole device assemblies, which then differ by construction.  This compiles one source of csrc/ to gfx950 device assembly, once
from <rev> and once from the working tree, with the Makefile's flags, and compares the body of every kernel of <rev> whose mangled
name contains <filter> with the working tree's kernel of the same name.  Basic-block labels carry the function's position in the
file (``.LBB<k>_<n>``), so <k> is masked; ``--rename NEW=OLD`` rewrites a piece of the working tree's mangled names first (a new
defaulted template parameter changes the mangling of the old instantiations).  Exits non-zero if a kernel is missing or differs.
Needs no GPU.

    python tools/isa_kernel_diff.py HEAD~1 ctc_lexbeam.hip ctc_lexbeam_kernel \\
        --rename ILb0ELb0ELb0EE=ILb0ELb0EE --rename ILb1ELb0ELb0EE=ILb1ELb0EE --rename ILb1ELb1ELb0EE=ILb1ELb1EE
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-pass-failed", "-fPIC", "--cuda-device-only", "-S"]


def assembly(tree, source):
    out = subprocess.run([HIPCC, *FLAGS, source, "-o", "-"], cwd=os.path.join(tree, "early_exit_transformer_amd", "csrc"), check=True,
                         capture_output=True, text=True).stdout
    return "\n".join(line for line in out.split("\n") if "__hip_cuid_" not in line)


def kernels(text, flt):
    found = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        if flt in m.group(1):
            found[m.group(1)] = re.sub(r"BB\d+_", "BBk_", m.group(2))
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rev")
    ap.add_argument("source", help="a file of early_exit_transformer_amd/csrc")
    ap.add_argument("filter", help="substring of the mangled kernel names to compare")
    ap.add_argument("--rename", action="append", default=[], metavar="NEW=OLD")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as work:
        old, new = os.path.join(work, "old"), os.path.join(work, "new")
        os.makedirs(old)
        archive = subprocess.run(["git", "-C", ROOT, "archive", args.rev, "early_exit_transformer_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=archive, check=True)
        shutil.copytree(os.path.join(ROOT, "early_exit_transformer_amd", "csrc"), os.path.join(new, "early_exit_transformer_amd", "csrc"),
                        ignore=shutil.ignore_patterns("build", "*.so"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(new, "include"))
        was, text = kernels(assembly(old, args.source), args.filter), assembly(new, args.source)
    for pair in args.rename:
        a, b = pair.split("=")
        text = text.replace(a, b)
    now = kernels(text, args.filter)
    status = 0
    for name, body in sorted(was.items()):
        verdict = "MISSING" if name not in now else "same" if now[name] == body else "DIFFERENT"
        status |= verdict != "same"
        print(f"{verdict:9s} {len(body.splitlines()):6d} lines  {name[:100]}")
    for name in sorted(set(now) - set(was)):
        print(f"{'new':9s} {len(now[name].splitlines()):6d} lines  {name[:100]}")
    if not was:
        print(f"no kernel of {args.rev} matches {args.filter!r}")
        status = 1
    sys.exit(status)


if __name__ == "__main__":
    main()
