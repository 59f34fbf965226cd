"""Coverage table of the logistic instantiations of product 1 (a helper: no tests in here), beside tests/_menu_cv.py.

A logistic problem (fos_problem_set_loss) launches product 1 with the logistic epilogue, with or without a fold mask: one
row per launchable cell (table, dtype, geometry, variant) with the cases that reach it.  tests/test_kernel_menu_logit.py
keeps the set of cells in step with the logistic forms of the product-1 form list of csrc/fos_plan.hip and checks on the CPU that
every case lands on its cell; tests/test_gpu_logit.py runs every case against the fp64 reference of tests/_logit.py.

table  geometry  variant        instantiation, chosen by
p1l    RB1, RB2  store          residual_batch_mfma_kernel<RB, true, false, FOLD_OFF, LOSS_LOGISTIC> (f32) and
                                residual_batch_mfma_bf16_kernel<RB, 128, true, false, FOLD_OFF, LOSS_LOGISTIC> (bf16): every row
                                panel of a lockstep iteration of fos_fista_run_multi (logistic_path) - RB 2 from 128 x CUs rows
p1l    RB1, RB2  resid          <RB, false, false, FOLD_OFF, LOSS_LOGISTIC>: fos_residual_batch (logistic_objective), all rows
p1l    RB1, RB2  train-store    <RB, true, false, FOLD_TRAIN, LOSS_LOGISTIC>: every row panel of fos_fista_run_multi_folds (logistic_cv)
p1l    RB1, RB2  heldout-resid  <RB, false, false, FOLD_HELD, LOSS_LOGISTIC>: fos_residual_batch_folds, all rows at once

The cases are the shapes of tests/_menu_cv.py (imported, not restated): the smallest at which the epilogue and its mask can go
wrong.  The row thresholds scale with the device's CU count: build(cus); ROWS = build(256) names the cells."""
from tests import _menu_cv as mc, _menu_multi as mm
from tests._menu import row_id  # noqa: F401  (ids of the rows, as the other tables)

VARIANTS = ("store", "resid", "train-store", "heldout-resid")
shapes = mc.shapes
fold_ids = mc.fold_ids


def case_cells(dtype, case, cus):
    """The cells a case launches: logistic_path and logistic_cv per row panel, logistic_objective and the held-out pass on
    all rows."""
    out = set()
    for rows in mm.panels(case["m"], cus):
        out.add(("p1l", dtype, f"RB{mm.rb(rows, cus)}", "store"))
        out.add(("p1l", dtype, f"RB{mm.rb(rows, cus)}", "train-store"))
    out.add(("p1l", dtype, f"RB{mm.rb(case['m'], cus)}", "resid"))
    out.add(("p1l", dtype, f"RB{mm.rb(case['m'], cus)}", "heldout-resid"))
    return out


def build(cus):
    rows = []
    for dtype in ("f32", "bf16"):
        named = shapes(dtype, cus)
        for geometry in ("RB1", "RB2"):
            for variant in VARIANTS:
                cell = ("p1l", dtype, geometry, variant)
                cases = [dict(c, name=k) for k, c in named.items() if cell in case_cells(dtype, c, cus)]
                rows.append(dict(table="p1l", dtype=dtype, geometry=geometry, variant=variant, cases=cases))
    return rows


ROWS = build(mm.GPU_CUS)


def cells(rows=None):
    return {(r["table"], r["dtype"], r["geometry"], r["variant"]) for r in (ROWS if rows is None else rows)}
