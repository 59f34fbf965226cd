"""CPU guard: the coverage table (tests/_menu.py) names every single-pass kernel instantiation the planner can launch.

The initialisers of kMenu, kDdMenu, kTallRows* and kTall* are parsed from csrc/fos_plan.hip; the set of cells they
instantiate must equal the table's, and every case the planner selects by capacity (fp64 geometries, column-block
widths) or by layout (tall load forms) must land on its own cell.  An entry added without a test, or a capacity moved
without moving its test, fails here."""
import os
import re

import pytest

from tests import _menu

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fastoptsolver_amd", "csrc", "fos_plan.hip")

# variants by macro (the column-block pair is in every kMenu entry)
MACRO_VARIANTS = {
    "ENTRY": ("with_g", "resid", "cb"),
    "ENTRY_D": ("with_g", "resid", "dual", "cb"),
    "ENTRY_NB_IL": ("with_g", "resid", "dual", "cb", "with_g_il", "resid_il", "dual_il"),
    "ENTRY_DRAIN": ("with_g", "resid", "dual", "cb", "with_g_il", "resid_il", "dual_il"),
    "ENTRY_IL_ND": ("with_g", "resid", "cb", "with_g_il", "resid_il"),
}
TALL_FORMS = {"f32": ("DIRECT", "VEC", "STAGE", "STAGE4"), "bf16": ("DIRECT", "STAGE")}
DTYPE = {"F32": "f32", "BF16": "bf16"}


def _initialiser(text, name):
    """Body of `const MenuEntry|DdEntry <name>[...] = { ... };` (comments stripped)."""
    m = re.search(r"const\s+\w+\s+" + re.escape(name) + r"\s*(?:\[[^\]]*\])*\s*=\s*\{", text)
    if m is None:
        raise AssertionError(f"{name}: initialiser not found")
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[m.end():i - 1]


def _args(s):
    return [a.strip() for a in s.split(",")]


def parse(path=SRC):
    """{'menu': [(dtype, th, k, r, macro)], 'dd': [(dtype, th, k, r, il)], 'tall_rows': {dtype: [lanes]},
    'tall': {dtype: [(capacity, form)]}, 'cells': set of (table, dtype, geometry, variant)} of the source at `path`."""
    with open(path) as fh:
        text = re.sub(r"//[^\n]*", "", fh.read())
    out = dict(menu=[], dd=[], tall_rows={}, tall={}, cells=set())
    cells = out["cells"]
    for macro, args in re.findall(r"\b(ENTRY\w*)\s*\(([^()]*)\)", _initialiser(text, "kMenu")):
        a = _args(args)
        dtype, th, k, r = DTYPE[a[0].replace("FOS_", "")], int(a[2]), int(a[3]), int(a[4])
        out["menu"].append((dtype, th, k, r, macro))
        for v in MACRO_VARIANTS[macro]:
            cells.add(("kMenu", dtype, _menu.geo(th, k, r), v))
    body = _initialiser(text, "kDdMenu")
    for item in re.finditer(r"\b(DD_ENTRY\w*)\s*\(([^()]*)\)|\{\s*FOS_(\w+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,([^{}]*)\}", body):
        if item.group(1):
            a = _args(item.group(2))
            dtype, th, k, r = DTYPE[a[0].replace("FOS_", "")], int(a[2]), int(a[3]), int(a[4])
            il = item.group(1).endswith("_IL")
        else:
            dtype, th, k, r = DTYPE[item.group(3)], int(item.group(4)), int(item.group(5)), int(item.group(6))
            il = len(re.findall(r"fused_launch_dd\s*<", item.group(7))) == 2
        out["dd"].append((dtype, th, k, r, il))
        for v in ("dd", "dd_il") if il else ("dd",):
            cells.add(("kDdMenu", dtype, _menu.geo(th, k, r), v))
    for suffix, dtype in (("F32", "f32"), ("Bf16", "bf16")):
        lanes = [int(x) for x in re.findall(r"\bTALLR\s*\([^,()]*,[^,()]*,\s*(\d+)\s*\)", _initialiser(text, "kTallRows" + suffix))]
        out["tall_rows"][dtype] = lanes
        for lpr in lanes:
            for v in _menu.TALL_VARIANTS:
                cells.add(("kTallRows" + suffix, dtype, f"lpr{lpr}", v))
        forms = TALL_FORMS[dtype]
        entries = []           # one per table position, row-major
        for macro, args in re.findall(r"\b(TALL_ROW|TALLQ|TALL)\s*\(([^()]*)\)", _initialiser(text, "kTall" + suffix)):
            a = _args(args)
            if macro == "TALL_ROW":
                entries += [int(a[2])] * len(forms)
            elif macro == "TALL":
                entries.append(int(a[2]))
                assert a[3].endswith("TL_" + forms[(len(entries) - 1) % len(forms)]), (suffix, a, "load form out of its column")
            else:
                entries.append(_menu.TL_MAX_N)          # the row-per-quad kernel serves up to 64 columns
        out["tall"][dtype] = [(c, forms[i % len(forms)]) for i, c in enumerate(entries)]
        for c, form in out["tall"][dtype]:
            for v in _menu.TALL_VARIANTS:
                cells.add(("kTall" + suffix, dtype, f"{c}/{form}", v))
    return out


def _describe(cells):
    return "\n  ".join("/".join(c) for c in sorted(cells))


def check_coverage(path=SRC):
    """Raise AssertionError naming every cell of the source at `path` without a row in tests/_menu.py (and every row
    without a cell)."""
    src = parse(path)["cells"]
    table = _menu.cells()
    missing, stale = src - table, table - src
    msg = [f"{what}:\n  {_describe(c)}" for what, c in (("cells without a row in tests/_menu.py", missing),
                                                          ("rows without a cell in the source", stale)) if c]
    assert not msg, "\n".join(msg)


def test_table_covers_every_instantiated_cell():
    check_coverage()


def test_entry_lists_match_the_source():
    """Order matters: default_entry / ensure_dd take the FIRST entry whose capacity fits."""
    src = parse()
    assert src["menu"] == [e[:5] for e in _menu.MENU]
    assert src["dd"] == list(_menu.DD_MENU)
    assert src["tall_rows"] == {d: list(v) for d, v in _menu.TALL_ROWS.items()}
    for dtype, forms in _menu.TALL_FORMS.items():
        assert src["tall"][dtype] == [(c, f) for c in _menu.TALL_CAPS for f in forms]


def test_every_reachable_row_has_cases_and_unreachable_rows_say_why():
    for row in _menu.ROWS:
        assert bool(row["cases"]) != bool(row["unreachable"]), _menu.row_id(row)
    assert len(_menu.reachable()) + sum(1 for r in _menu.ROWS if r["unreachable"]) == len(_menu.ROWS)


def _sibling(path=SRC):
    with open(path) as fh:
        text = re.sub(r"//[^\n]*", "", fh.read())
    out = {}
    for args in re.findall(r"\bENTRY_DRAIN\s*\(([^()]*)\)", _initialiser(text, "kMenu")):
        a = _args(args)
        out[(DTYPE[a[0].replace("FOS_", "")], int(a[2]), int(a[3]))] = (int(a[6]), int(a[7]))
    return out


def test_drained_entries_name_their_dual_sibling():
    sib = _sibling()
    assert sib == {(d, th, k): s for d, th, k, r, macro, s in _menu.MENU if macro == "ENTRY_DRAIN"}
    for (dtype, th, k), (th2, k2) in sib.items():
        assert _menu.cap(dtype, th2, k2) == _menu.cap(dtype, th, k)      # the sibling covers the same n


def _tall_cell(dtype, n, lda, aligned):
    """tall_entry() of fos_plan.hip: (table, geometry) of a tall plan."""
    epc = _menu.EPC[dtype]
    suffix = "F32" if dtype == "f32" else "Bf16"
    if n % epc == 0 and lda % epc == 0 and aligned and n // epc > 4:
        chunks = n // epc
        return "kTallRows" + suffix, f"lpr{8 if chunks <= 8 else 16 if chunks <= 16 else 32}"
    cap = 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64
    contiguous = lda == n
    if dtype == "f32":
        vec = n % 4 == 0 and lda % 4 == 0 and aligned
        form = "VEC" if vec else ("STAGE4" if aligned and cap < 64 else "STAGE") if contiguous else "DIRECT"
    else:
        form = "STAGE" if contiguous else "DIRECT"
    return "kTall" + suffix, f"{cap}/{form}"


def _lda(dtype, c):
    if c["m"] == 1:
        return c["n"]
    e = _menu.EPC[dtype]
    return c["n"] + {"compact": 0, "misaligned": 0, "strided": 2 * e, "ragged": 1, "cbview": 2 * e}[c["layout"]]


def test_selected_cases_land_on_their_cell():
    """Capacities and layouts are the planner's choice, not the test's: every such case must select its own cell
    (capacities from the parsed source)."""
    src = parse()
    menu, dd = src["menu"], src["dd"]
    for row in _menu.reachable():
        for c in row["cases"]:
            dtype, n, where = row["dtype"], c["n"], (_menu.row_id(row), c)
            assert c["m"] * _lda(dtype, c) * _menu.ESZ[dtype] <= _menu.MAX_BYTES, where
            if row["table"] == "kDdMenu":
                i = _menu.first_fit(dd, dtype, n)
                assert i is not None and _menu.geo(*dd[i][1:4]) == row["geometry"], where
                assert n > _menu.TLR_MAX_N[dtype] and n % _menu.EPC[dtype] == 0, where      # a streaming plan
            elif row["variant"] == "cb":
                w = _menu.cb_width(n)
                i = _menu.first_fit(menu, dtype, w)
                assert i is not None and _menu.geo(*menu[i][1:4]) == row["geometry"], where
                assert n > _menu.TLR_MAX_N[dtype] and n % _menu.EPC[dtype] == 0 and c["layout"] == "cbview", where
            elif row["table"] == "kMenu":
                th, k, r = row["tune"]
                assert n <= _menu.cap(dtype, th, k) and n % _menu.EPC[dtype] == 0, where       # tune accepts it
                assert c["no_tall"] == (n <= _menu.TLR_MAX_N[dtype]), where
            else:
                aligned = c["layout"] != "misaligned"
                assert n <= _menu.TLR_MAX_N[dtype], where
                assert _tall_cell(dtype, n, _lda(dtype, c), aligned) == (row["table"], row["geometry"]), where


def test_tail_cases_cut_a_row_step():
    for row in _menu.reachable():
        r = row.get("tune", (0, 0, 1))[2]
        for c in row["cases"]:
            if c["tail"]:
                rpw = -(-c["m"] // c["wg"])
                last = c["m"] - (c["wg"] - 1) * rpw
                assert 0 < last < rpw and -(-c["m"] // rpw) == c["wg"], (_menu.row_id(row), c)
                if r > 1:
                    assert rpw % r and last % r, (_menu.row_id(row), c)


def test_guard_names_a_new_entry_without_a_test(tmp_path):
    """The guard itself: an entry added to a copy of the source without a row in the table fails, naming its cells."""
    with open(SRC) as fh:
        text = fh.read()
    anchor = "ENTRY_IL_ND(FOS_BF16, fos::bf16_t, 512, 6, 1, 2),"
    assert anchor in text
    fake = tmp_path / "fos_plan.hip"
    fake.write_text(text.replace(anchor, anchor + " ENTRY_NB_IL(FOS_BF16, fos::bf16_t, 1024, 4, 1, 2, 2),"))
    with pytest.raises(AssertionError) as err:
        check_coverage(str(fake))
    msg = str(err.value)
    for v in MACRO_VARIANTS["ENTRY_NB_IL"]:
        assert f"kMenu/bf16/1024x4x1/{v}" in msg
    moved = tmp_path / "moved.hip"
    moved.write_text(text.replace("DD_ENTRY(FOS_F32, float, 64, 3, 2, false)", "DD_ENTRY(FOS_F32, float, 64, 4, 2, false)"))
    with pytest.raises(AssertionError):
        check_coverage(str(moved))
