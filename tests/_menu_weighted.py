"""Coverage table of the weighted instantiations of product 1 (a helper: no tests in here), beside tests/_menu_logit.py.

A problem with row weights (fos_row_weights_bind) launches product 1 with the weight in its epilogue, for either loss and with
or without a fold mask: one row per launchable cell (table, dtype, geometry, variant) with the cases that reach it.
tests/test_kernel_menu_weighted.py keeps the set of cells in step with the weighted forms of the product-1 form list of
csrc/fos_plan.hip and checks on the CPU that every case lands on its cell; tests/test_gpu_weighted.py runs every case against
the fp64 reference of tests/_weighted.py.

table  geometry  variant                 instantiation, chosen by
p1w    RB1, RB2  LOSS/store              residual_batch_mfma_kernel<RB, true, false, FOLD_OFF, LOSS, true> (f32) and
                                         residual_batch_mfma_bf16_kernel<RB, 128, true, false, FOLD_OFF, LOSS, true> (bf16): every
                                         row panel of fos_fista_run_multi (fista_path / logistic_path on a weighted handle)
p1w    RB1, RB2  LOSS/resid              <RB, false, false, FOLD_OFF, LOSS, true>: fos_residual_batch, all rows
p1w    RB1, RB2  LOSS/train-store        <RB, true, false, FOLD_TRAIN, LOSS, true>: every row panel of fos_fista_run_multi_folds
p1w    RB1, RB2  LOSS/heldout-resid      <RB, false, false, FOLD_HELD, LOSS, true>: fos_residual_batch_folds, all rows at once

LOSS is squared or logistic.  The cases are the shapes of tests/_menu_cv.py (imported, not restated); the row thresholds scale
with the device's CU count: build(cus); ROWS = build(256) names the cells."""
from tests import _menu_cv as mc, _menu_multi as mm
from tests._menu import row_id  # noqa: F401  (ids of the rows, as the other tables)

LOSSES = ("squared", "logistic")
FORMS = ("store", "resid", "train-store", "heldout-resid")
VARIANTS = tuple(f"{loss}/{form}" for loss in LOSSES for form in FORMS)
shapes = mc.shapes
fold_ids = mc.fold_ids


def case_cells(dtype, case, cus):
    """The cells a case launches for either loss: the path and the cross-validation per row panel, the objective and the
    held-out pass on all rows."""
    out = set()
    for loss in LOSSES:
        for rows in mm.panels(case["m"], cus):
            out.add(("p1w", dtype, f"RB{mm.rb(rows, cus)}", f"{loss}/store"))
            out.add(("p1w", dtype, f"RB{mm.rb(rows, cus)}", f"{loss}/train-store"))
        out.add(("p1w", dtype, f"RB{mm.rb(case['m'], cus)}", f"{loss}/resid"))
        out.add(("p1w", dtype, f"RB{mm.rb(case['m'], cus)}", f"{loss}/heldout-resid"))
    return out


def build(cus):
    rows = []
    for dtype in ("f32", "bf16"):
        named = shapes(dtype, cus)
        for geometry in ("RB1", "RB2"):
            for variant in VARIANTS:
                cell = ("p1w", dtype, geometry, variant)
                cases = [dict(c, name=k) for k, c in named.items() if cell in case_cells(dtype, c, cus)]
                rows.append(dict(table="p1w", dtype=dtype, geometry=geometry, variant=variant, cases=cases))
    return rows


ROWS = build(mm.GPU_CUS)


def cells(rows=None):
    return {(r["table"], r["dtype"], r["geometry"], r["variant"]) for r in (ROWS if rows is None else rows)}
