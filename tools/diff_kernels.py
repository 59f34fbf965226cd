#!/usr/bin/env python3
"""Which kernels of a translation unit compile to different instructions in two source trees (no device needed).

    python tools/diff_kernels.py OTHER_TREE [UNIT ...]        # e.g. a checkout of the parent commit; default unit: fos_fista

Each unit (fastoptsolver_amd/csrc/UNIT.hip) is compiled for gfx950, device side only, to assembly in both trees; per kernel
the instruction text is compared after comments, debug directives and the function-numbered basic-block labels (.LBBn_m: n
shifts when a kernel is added in front) are normalised.  Prints the kernels that differ, that exist in one tree only, and
exits 1 if an existing kernel differs.  This is how "the existing instantiations compile to what they compiled to" is
checked when a template gains a form."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernels(tree, unit, out):
    src = os.path.join(tree, "fastoptsolver_amd", "csrc", unit + ".hip")
    subprocess.run(["hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-fvisibility=hidden", "--cuda-device-only", "-S",
                    "-o", out, src], check=True, stderr=subprocess.DEVNULL)
    found = {}
    with open(out) as fh:
        text = fh.read()
    for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)\n\s*s_endpgm", text, re.M | re.S):
        body = re.sub(r";.*", "", m.group(2))
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        body = re.sub(r"\.Ltmp\d+|\.loc.*|\.file.*", "", body)
        body = re.sub(r"[ \t]+$", "", body, flags=re.M)                   # the comment column moves with the label's width
        found[m.group(1)] = body
    return found


def main(argv):
    if len(argv) < 2:
        print(__doc__)
        return 2
    other, units = argv[1], argv[2:] or ["fos_fista"]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for unit in units:
            a, b = kernels(other, unit, os.path.join(tmp, "a.s")), kernels(ROOT, unit, os.path.join(tmp, "b.s"))
            differ = sorted(k for k in a if k in b and a[k] != b[k])
            print(f"{unit}: {len(a)} kernels there, {len(b)} here, {len(differ)} differ; only there: {sorted(set(a) - set(b))}; "
                  f"only here: {sorted(set(b) - set(a))}")
            for k in differ:
                print("  differs:", k)
            bad += len(differ)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
