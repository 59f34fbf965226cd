"""CPU guard: the coverage table of the L-BFGS kernels (tests/_menu_lbfgs.py) names every __global__ of
csrc/lbfgs_kernels.hpp in every instantiation the four translation units launch, and restates the dispatch constants of the
source correctly.

Parsed: every `__global__` of the header (with its template parameters and their defaults), every hipLaunchKernelGGL of the
four .hip files whose kernel is one of them - template arguments included, a launch inside a `#define NAME(ARG)` macro
counted once per use of the macro with the argument put in."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import _menu_lbfgs as ml

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fastoptsolver_amd", "csrc")
HEADER = os.path.join(CSRC, "lbfgs_kernels.hpp")
UNITS = tuple(os.path.join(CSRC, u + ".hip") for u in ("fos_plan", "fos_comm", "fos_fista", "fos_lbfgs"))


def _text(path):
    with open(path) as fh:
        return re.sub(r"//[^\n]*", "", fh.read())


def globals_of(header=HEADER):
    """{kernel: [default of every template parameter, None where it has none]} for every __global__ of the header."""
    t = _text(header)
    out = {}
    for m in re.finditer(r"(template\s*<([^<>]*)>\s*)?(?:static\s+)?__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(", t):
        params = []
        if m.group(2) is not None:
            for p in m.group(2).split(","):
                params.append(p.split("=")[1].strip() if "=" in p else None)
        out[m.group(3)] = params
    return out


def _first_arg(text, i):
    """The first argument of the call whose opening parenthesis is at text[i]."""
    depth, j = 0, i
    while True:
        ch = text[j]
        depth += ch in "(<" and 1 or 0
        depth -= ch in ")>" and 1 or 0
        if ch == "," and depth == 1:
            return text[i + 1:j]
        j += 1


def _launches(text):
    for m in re.finditer(r"hipLaunchKernelGGL\s*\(", text):
        arg = _first_arg(text, m.end() - 1).strip()
        while arg.startswith("(") and arg.endswith(")"):
            arg = arg[1:-1].strip()
        k = re.fullmatch(r"(?:fos::)?(\w+)\s*(?:<(.*)>)?", arg, flags=re.S)
        if k is None:                       # a launch through a function pointer (the dispatch tables of the A passes)
            continue
        yield k.group(1), tuple(a.strip() for a in k.group(2).split(",")) if k.group(2) else ()


def parse(header=HEADER, units=UNITS):
    """The set of (kernel, template arguments) the units launch, for the kernels of the header."""
    kernels = globals_of(header)
    cells = set()
    for path in units:
        t = _text(path)
        # a launch inside a one-argument macro: counted per use, with the argument substituted
        for m in re.finditer(r"#define\s+(\w+)\((\w+)\)((?:[^\n]*\\\n)*[^\n]*)\n(.*?)#undef\s+\1", t, flags=re.S):
            name, par, body, scope = m.groups()
            body = body.replace("\\\n", " ")
            for use in re.finditer(r"\b" + name + r"\(\s*(\w+)\s*\)", scope):
                for kern, targs in _launches(re.sub(r"\b" + par + r"\b", use.group(1), body)):
                    cells.add((kern, targs))
        plain = re.sub(r"#define\s+\w+\(\w+\)(?:[^\n]*\\\n)*[^\n]*\n", "", t)
        for kern, targs in _launches(plain):
            cells.add((kern, targs))
        # no kernel of the header is named anywhere but as the kernel of a launch (none hides in a table of pointers)
        sites = [k for k, _ in _launches(t)]
        for kern in kernels:
            assert len(re.findall(r"\b" + kern + r"\b", t)) == sites.count(kern), (path, kern)
    out = set()
    for kern, targs in cells:
        if kern not in kernels:
            continue
        defaults = kernels[kern]
        assert len(targs) <= len(defaults), (kern, targs)
        full = tuple(targs) + tuple(defaults[len(targs):])
        assert None not in full, (kern, targs)
        out.add((kern, full))
    return out


def _describe(cells):
    return "\n  ".join(f"{k}<{', '.join(t)}>" for k, t in sorted(cells))


def check_coverage(header=HEADER, units=UNITS):
    src, table = parse(header, units), ml.cells()
    msg = [f"{what}:\n  {_describe(c)}" for what, c in (("instantiations without a row in tests/_menu_lbfgs.py", src - table),
                                                          ("rows without a launch in the source", table - src)) if c]
    missing = set(globals_of(header)) - {k for k, _ in src}
    if missing:
        msg.append("kernels of the header that nothing launches: " + ", ".join(sorted(missing)))
    assert not msg, "\n".join(msg)


def test_table_covers_every_launched_instantiation():
    check_coverage()
    assert len(globals_of()) == 19
    assert len(ml.ROWS) == len(ml.cells()) == 8 + 2 + 3 + 3 + 2 + 2 + 3 + 2 + 6


def test_every_row_has_cases_or_says_why_not():
    from tests import _lbfgs_cases as lc
    for row in ml.ROWS:
        assert bool(row["cases"]) != bool(row["unreachable"]), ml.row_id(row)
        if row["check"] == "driver":
            assert all(name in lc.BY_NAME for name in row["cases"]), ml.row_id(row)
        if row["check"] == "lockstep":
            assert all(name in lc.GROUPS for name in row["cases"]), ml.row_id(row)
    assert [ml.row_id(r) for r in ml.ROWS if r["unreachable"]] == ["lbfgs_two_loop_multi-0"]


def test_constants_match_the_source():
    th, tl = _text(HEADER), _text(UNITS[3])
    consts = {}
    for names in re.findall(r"constexpr\s+int\s+((?:\w+\s*=\s*\d+\s*,?\s*)+);", th):
        consts.update({k: int(v) for k, v in re.findall(r"(\w+)\s*=\s*(\d+)", names)})
    assert (consts["LB_THREADS"], consts["LB_MAXHIST"]) == (ml.LB_THREADS, ml.LB_MAXHIST)
    assert (consts["VL_MAXH"], consts["VL_COLS"], consts["VL_THREADS"], consts["VL_PSTRIDE"], consts["VL_MAXPARTS"]) == \
        (ml.VL_MAXH, ml.VL_COLS, ml.VL_THREADS, ml.VL_PSTRIDE, ml.VL_MAXPARTS)
    assert re.search(r"__shared__\s+double\s+coef\[LB_MAXHIST\]", th) and re.search(r"__shared__\s+double\s+rho\[LB_MAXHIST\]", th)
    # the bucket limits and alignment masks of both two-loop entry points, and their history cap
    chains = re.findall(r"if\s*\(vec\s*&&\s*n\s*<=\s*(\d+)\)\s*FOS_TL\((\d)\);\s*else\s+if\s*\(vec\s*&&\s*n\s*<=\s*(\d+)\)\s*FOS_TL\((\d)\);\s*"
                        r"else\s+if\s*\(vec\s*&&\s*n\s*<=\s*(\d+)\)\s*FOS_TL\((\d)\);\s*else\s+FOS_TL\(0\);", tl)
    assert len(chains) == 2
    for c in chains:
        assert tuple((int(c[i]), int(c[i + 1])) for i in (0, 2, 4)) == ml.BUCKETS
    masks = [int(v) for v in re.findall(r"const\s+bool\s+vec\s*=\s*\(n\s*%\s*4\s*==\s*0\)\s*&&.*?&\s*(\d+)u\)\s*==\s*0", tl, flags=re.S)]
    assert masks == [ml.ALIGN["float"] - 1, ml.ALIGN["double"] - 1]
    assert len(re.findall(r"hist\s*>\s*fos::LB_MAXHIST", tl)) == 2 and len(re.findall(r"hist\s*>\s*fos::VL_MAXH", tl)) == 2
    # both drivers: the whole-chip direction from n >= 2048, n % 4 picks the two-loop form below, M = 10 pairs
    assert len(re.findall(r"if\s*\(n\s*>=\s*%d\)\s*\{" % ml.CHIP_MIN_N, tl)) == 2
    assert re.search(r"fused_first_trial\s*=\s*n\s*>=\s*%d\s*&&\s*nit\s*>\s*0" % ml.CHIP_MIN_N, tl)
    assert re.search(r"c\.fuse\[k\]\s*=\s*n\s*>=\s*%d\s*&&\s*col\[j\]\.nit\s*>\s*0" % ml.CHIP_MIN_N, tl)
    assert re.findall(r"constexpr\s+int\s+M\s*=\s*(\d+)", tl) == [str(ml.DRIVER_M)] * 2
    assert re.search(r"\}\s*else\s+if\s*\(vec\)\s*FOS_TL\(1\);\s*else\s+FOS_TL\(0\);", tl) and re.search(r"const\s+bool\s+vec\s*=\s*\(n\s*%\s*4\s*==\s*0\);", tl)
    # the grid of the element-wise kernels: every launch of one in this unit uses grid_1d(n, 256, 1024)
    grids = re.findall(r"grid_1d\(\s*n\s*,\s*(\d+)\s*,\s*(\d+)\s*\)", tl)
    assert len(grids) == 5 and set(grids) == {(str(ml.AX_BLOCK), str(ml.AX_CAP))}
    body = re.search(r"int\s+grid_1d\(int64_t\s+n,\s*int\s+per_block,\s*int\s+cap\)\s*\{(.*?)\n\}", _text(UNITS[0]), flags=re.S).group(1)
    assert re.search(r"\(n\s*\+\s*per_block\s*-\s*1\)\s*/\s*per_block", body) and "cap" in body
    # vl_parts and the scratch length
    assert re.search(r"std::min<int64_t>\(\(n\s*\+\s*fos::VL_COLS\s*-\s*1\)\s*/\s*fos::VL_COLS,\s*fos::VL_MAXPARTS\)", tl)
    assert re.search(r"\(int64_t\)vl_parts\(n\)\s*\*\s*fos::VL_PSTRIDE", tl)


def test_case_lengths_follow_the_constants():
    """Every case lands on the instantiation it is filed under, and the edges the issue names are there."""
    (b1, _), (b2, _), (b4, _) = ml.BUCKETS
    for vt in ("float", "double"):
        rows = [r for r in ml.ROWS if r["kernel"] == "lbfgs_two_loop_kernel" and r["targs"][0] == vt]
        seen, forms = set(), set()
        for r in rows:
            nq = int(r["targs"][1])
            row_forms = set()
            for c in r["cases"]:
                assert ml.two_loop_nq(c["n"], c["off"] == 0) == nq, (ml.row_id(r), c)
                assert all(0 <= h <= ml.LB_MAXHIST and cap >= h and (head < cap or cap == 0) for h, cap, head in c["cfgs"])
                assert c["n"] > ml.TINY or all(h <= min(c["n"], 2) for h, _, _ in c["cfgs"]), (ml.row_id(r), c)
                seen.add((c["n"], c["off"]))
                row_forms |= set(c["cfgs"])
            assert {h for h, _, _ in row_forms} == set(ml.HISTS), ml.row_id(r)        # every history length on every row
            forms |= row_forms
        want = {(n, 0) for n in (1, 3, 4, 1023 * 4, b1 - 4, b1, b1 + 4, b2, b2 + 4, b4, b4 + 4)}
        assert want <= seen, want - seen
        assert any(n % 4 and n < b1 for n, _ in seen) and any(n % 4 and b1 < n < b2 for n, _ in seen)
        assert any(n % 4 and b2 < n < b4 for n, _ in seen) and any(n > 70000 for n, _ in seen)
        assert any(off == 1 and n % 4 == 0 for n, off in seen)
        for h in ml.HISTS[1:]:
            caps = {(cap == hh, tag) for hh, cap, head in forms if hh == h
                    for tag, on in (("head0", head == 0), ("last", head == cap - 1)) if on}
            assert {(True, "head0"), (False, "head0"), (True, "last"), (False, "last")} <= caps, (h, caps)
            assert any(head + hh > cap for hh, cap, head in forms if hh == h) or h == 1               # the live window wraps
    full = ml.VL_COLS * ml.VL_MAXPARTS
    for r in ml.ROWS:
        if r["check"] != "direction":
            continue
        ns = {c["n"] for c in r["cases"]}
        assert {1, ml.VL_COLS - 1, ml.VL_COLS, ml.VL_COLS + 1, ml.VL_THREADS - 1, ml.VL_THREADS, ml.VL_THREADS + 1, full - 1, full,
                full + 1, 2 * full + 1} <= ns and max(ns) > 70000
        assert ml.direction_parts(full) == ml.VL_MAXPARTS == ml.direction_parts(full + 1) and ml.direction_parts(full - 1) == ml.VL_MAXPARTS
        for c in r["cases"]:
            assert [h for h, _, _ in c["cfgs"]] == list(range(min(c["n"], ml.VL_MAXH) + 1 if c["n"] <= ml.TINY else ml.VL_MAXH + 1)), c
    both = [c for r in ml.ROWS if r["check"] == "direction" for c in r["cases"]]
    for n in {c["n"] for c in both}:
        assert {c["gd"] for c in both if c["n"] == n} == {True, False}, n           # gd_out given and NULL at every length
        assert {bool(c["tail"]) for c in both if c["n"] == n} == {True, False}, n   # work exact and with a NaN tail
    ax = {c["n"] for r in ml.ROWS if r["check"] == "axpby" for c in r["cases"]}
    assert ml.AX_BLOCK * ml.AX_CAP + 3 in ax and max(ax) > 2 * ml.AX_BLOCK * ml.AX_CAP and 1 in ax
    assert ml.axpby_grid(ml.AX_BLOCK * ml.AX_CAP + 3) == ml.AX_CAP
    st = {c["n"] for r in ml.ROWS if r["check"] == "stats" for c in r["cases"]}
    assert {1, 63, 64, 1023, 1024, 1025, 70001} <= st


def _fma(a, b, c):
    """a*b + c with ONE rounding (exact rational arithmetic; int / int division is correctly rounded)."""
    v = Fraction(a) * Fraction(b) + Fraction(c)
    return v.numerator / v.denominator


@pytest.mark.parametrize("ytype", ["double", "float"])
def test_axpby_inputs_tell_a_contracted_sum_from_separate_roundings(ytype):
    """The bitwise test of vec_axpby_f64_kernel can only see an fma contraction where the contracted result differs.
    Measured on 4000 elements (exact rational fma): contracting b*y into the sum differs in 61.7 % (y double) / 61.2 %
    (y float) of the elements, contracting a*x in 59.5 % / 59.2 %; at least a quarter is required."""
    a, x, b, y = ml.axpby_inputs(4000, 5, ytype)
    want = b * y + a * x                                    # NumPy: two rounded products, one rounded sum
    by, ax = b * y, a * x
    share_by = np.mean([_fma(b, float(y[i]), float(ax[i])) != want[i] for i in range(x.size)])
    share_ax = np.mean([_fma(a, float(x[i]), float(by[i])) != want[i] for i in range(x.size)])
    assert share_by >= 0.25 and share_ax >= 0.25, (share_by, share_ax)


def test_guard_names_a_missing_row_and_a_new_instantiation(tmp_path):
    with open(UNITS[3]) as fh:
        text = fh.read()
    for old, new, cell in (
            ("  else if (vec && n <= 16384) FOS_TL(4);\n  else FOS_TL(0);\n#undef FOS_TL\n  LAUNCH_CHECK();\n  return FOS_OK;\n}\n\nint fos_lbfgs_two_loop_dd",
             "  else FOS_TL(0);\n#undef FOS_TL\n  LAUNCH_CHECK();\n  return FOS_OK;\n}\n\nint fos_lbfgs_two_loop_dd", "lbfgs_two_loop_kernel<float, 4>"),
            ("fos::vec_stats_kernel<double>, dim3(1)", "fos::vec_stats_kernel<double, double>, dim3(1)", "vec_stats_kernel<double, float>"),
            ("fos::lbfgs_two_loop_multi_kernel<1>", "fos::lbfgs_two_loop_multi_kernel<2>", "lbfgs_two_loop_multi_kernel<2>")):
        assert text.count(old) == 1, old
        fake = tmp_path / "fos_lbfgs.hip"
        fake.write_text(text.replace(old, new))
        with pytest.raises(AssertionError) as err:
            check_coverage(units=UNITS[:3] + (str(fake),))
        assert cell in str(err.value), (cell, str(err.value))
