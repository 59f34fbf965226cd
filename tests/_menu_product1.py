"""The product-1 cells csrc/fos_plan.hip instantiates (a helper: no tests in here), beside the tests/_menu*.py tables.

fos_plan.hip writes the launchable forms of product 1 once, as the list FOS_P1_FORMS of X(STORE_R, BBLOCK, FOLD, LOSS, WEIGHT)
lines, and expands it with FOS_P1_ENTRY into kBatchForms: per form an fp32 and a bf16 kernel at RB 1 and RB 2.  cells() reads
both macros and returns every (table, dtype, geometry, variant) cell under the labels of the four coverage tables; the table
follows from the form: WEIGHT -> p1w (tests/_menu_weighted.py), else LOSS_LOGISTIC -> p1l (_menu_logit.py), else a fold mask ->
p1f (_menu_cv.py), else p1 (_menu_multi.py)."""
import os
import re

from tests import _menu_multi as mm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fastoptsolver_amd", "csrc")
PLAN, FISTA = os.path.join(CSRC, "fos_plan.hip"), os.path.join(CSRC, "fos_fista.hip")

KERNELS = {"residual_batch_mfma_kernel": ("f32", 1), "residual_batch_mfma_bf16_kernel": ("bf16", 2)}   # dtype, index of STORE_R
PARAMS = ("S", "B", "F", "L", "W")
FOLD = {"FOLD_OFF": "", "FOLD_TRAIN": "train-", "FOLD_HELD": "heldout-"}
LOSS = {"LOSS_SQUARED": "squared", "LOSS_LOGISTIC": "logistic"}


def _text(path):
    with open(path) as fh:
        return re.sub(r"//[^\n]*", "", fh.read())


def _body(text, start):
    """The brace-balanced body that follows the first match of `start` (which ends before its opening brace)."""
    m = re.search(start, text)
    assert m is not None, start
    i = text.index("{", m.end())
    depth, j = 1, i + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        j += 1
    return text[i + 1:j - 1]


def _macro(text, name):
    """The body of `#define name(...)`, its line continuations joined."""
    m = re.search(r"#define\s+" + name + r"\s*\(([^)]*)\)((?:[^\n]*\\\n)*[^\n]*)", text)
    assert m is not None, name
    return [s.strip() for s in m.group(1).split(",")], m.group(2).replace("\\\n", " ")


def forms(plan=PLAN):
    """The lines of FOS_P1_FORMS as (store, bblock, fold, loss, weight) tuples of their source tokens."""
    _, body = _macro(_text(plan), "FOS_P1_FORMS")
    out = [tuple(s.strip() for s in args.split(",")) for args in re.findall(r"\bX\s*\(([^()]*)\)", body)]
    assert out and all(len(f) == len(PARAMS) for f in out), out
    return out


def label(form):
    """(table, variant) of a form."""
    store, bblock, fold, loss, weight = form
    assert store in ("true", "false") and bblock in ("true", "false") and weight in ("true", "false"), form
    sr = ("store" if store == "true" else "resid") + ("-B" if bblock == "true" else "")
    if weight == "true":
        return "p1w", LOSS[loss] + "/" + FOLD[fold] + sr
    if loss != "LOSS_SQUARED":
        assert loss == "LOSS_LOGISTIC", form
        return "p1l", FOLD[fold] + sr
    if fold != "FOLD_OFF":
        return "p1f", FOLD[fold][:-1] + "-" + sr
    return "p1", sr


def instantiations(plan=PLAN):
    """One (table, dtype, geometry, variant) per kernel the table instantiates, in source order (a list: duplicates show)."""
    params, body = _macro(_text(plan), "FOS_P1_ENTRY")
    assert tuple(params) == PARAMS, params
    assert re.search(r"\{\s*S\s*,\s*B\s*,\s*fos::F\s*,\s*fos::L\s*,\s*W\s*\}", body), "the form of an entry is {S, B, fos::F, fos::L, W}"
    kernels = re.findall(r"fos::(residual_batch_mfma(?:_bf16)?_kernel)\s*<([^<>]*)>", body)
    assert kernels, body
    out = []
    for form in forms(plan):
        table, variant = label(form)
        for kern, args in kernels:
            dtype, skip = KERNELS[kern]
            a = [s.strip() for s in args.split(",")]
            assert a[skip:] == ["S", "B", "fos::F", "fos::L", "W"], (kern, a)
            if dtype == "bf16":
                assert int(a[1]) == mm.TILE_COLS["bf16"], a
            out.append((table, dtype, f"RB{int(a[0])}", variant))
    return out


def cells(plan=PLAN, table=None):
    """The set of cells, of all four tables or of one."""
    return {c for c in instantiations(plan) if table is None or c[0] == table}


def describe(cells_):
    return "\n  ".join("/".join(c) for c in sorted(cells_))


def check_coverage(table, menu_cells, menu_file, plan=PLAN):
    """The cells of `table` in the source are the cells of its coverage table."""
    src = cells(plan, table)
    msg = [f"{what}:\n  {describe(c)}" for what, c in ((f"cells without a row in {menu_file}", src - menu_cells),
                                                       ("rows without a cell in the source", menu_cells - src)) if c]
    assert not msg, "\n".join(msg)


def check_partition(groups, plan=PLAN):
    """`groups` (table -> the cells of its coverage table) are together exactly the instantiations of the source: 72 kernels,
    none left over, none twice."""
    inst = instantiations(plan)
    assert len(inst) == len(set(inst)) == 4 * len(forms(plan)) == 72, describe(c for c in set(inst) if inst.count(c) > 1)
    assert all(c[0] == t for t, g in groups.items() for c in g)
    union = set().union(*groups.values())
    assert union == set(inst), describe(union ^ set(inst))
    assert sum(len(g) for g in groups.values()) == len(union)


def launcher(plan=PLAN):
    """The body of the one launcher, after the checks every guard makes of it: the grid is batch_grid's (whose 128 x CUs
    threshold the route mm.rb restates), and the fp32 / bf16 branch exists once, each side launching the entry's kernel of the
    grid's tile variant on the grid's workgroups."""
    tp = _text(plan)
    grid = _body(tp, r"static\s+BatchGrid\s+batch_grid\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"const\s+int\s+variant\s*=\s*rows_total\s*>=\s*%d\s*\*\s*\(int64_t\)\s*p->ncu\s*\?\s*1\s*:\s*0" % mm.RB2_ROWS_PER_CU, grid)
    assert len(re.findall(r"\bint\s+launch_batch_product\w*\s*\(", tp)) == 1
    body = _body(tp, r"int\s+launch_batch_product\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"const\s+BatchGrid\s+g\s*=\s*batch_grid\s*\(\s*p\s*,\s*L\.rows\s*\)", body)
    launches = re.findall(r"hipLaunchKernelGGL\s*\(\s*e\.(\w+)\s*\[\s*g\.variant\s*\]\s*,\s*dim3\(\(unsigned\)g\.nwg\)", body)
    assert launches == ["bf16", "f32"] and body.count("hipLaunchKernelGGL") == 2 and len(re.findall(r"\bg\.gpw\b", body)) == 2
    return body
