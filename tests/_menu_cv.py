"""Coverage table of the fold instantiations of product 1 (a helper: no tests in here), beside tests/_menu_multi.py.

K-fold cross-validation in lockstep (fos_fista_run_multi_folds, fos_residual_batch_folds) launches product 1 with a fold
mask in its epilogue: one row per launchable cell (table, dtype, geometry, variant) with the cases that reach it.
tests/test_kernel_menu_cv.py keeps the set of cells in step with the fold forms of the product-1 form list of
csrc/fos_plan.hip and checks on the CPU that every case lands on its cell; tests/test_gpu_cv.py runs every case against the
fp64 oracle on the gathered rows.

table  geometry  variant        instantiation, chosen by
p1f    RB1, RB2  train-store    residual_batch_mfma_kernel<RB, true, false, FOLD_TRAIN> (f32) and
                                residual_batch_mfma_bf16_kernel<RB, 128, true, false, FOLD_TRAIN> (bf16): every row panel of a
                                lockstep iteration of fos_fista_run_multi_folds - RB 2 from 128 x CUs panel rows
p1f    RB1, RB2  heldout-resid  the same kernels <RB, false, false, FOLD_HELD>: fos_residual_batch_folds, all rows at once

A case is (m, n, folds, nalpha): folds = (kind, K) with kind "interleaved" (i % K), "contiguous" (fista_cv's int K) or
"random" (ids from a seeded generator); K x nalpha columns in groups of 16.  The row thresholds scale with the device's CU
count: build(cus); ROWS = build(256) names the cells."""
import numpy as np

from tests import _menu_multi as mm
from tests._menu import row_id  # noqa: F401  (ids of the rows, as the other tables)

WIDTH = {"f32": 68, "bf16": 72}            # the narrowest streaming width: 64 columns plus one 16-byte chunk
VARIANTS = ("train-store", "heldout-resid")


def shapes(dtype, cus):
    """The smallest shapes at which the mask can go wrong, by name."""
    w = WIDTH[dtype]
    return {
        # less than one row tile plus 3, the narrowest width, a lane's 4 rows alternating folds
        "one_tile": dict(m=67, n=w, folds=("interleaved", 2), nalpha=2),
        # fold edges 201 / 401 / ... inside a lane's 4-row group and inside a 16-row block; clamped columns; 15 columns
        "edges": dict(m=1001, n=200, folds=("contiguous", 5), nalpha=3),
        # the 128-row tile just past its threshold
        "rb2": dict(m=mm.RB2_ROWS_PER_CU * cus + 1, n=w, folds=("random", 3), nalpha=3),
        # two panels, the second shorter than a row tile: the ids offset with the panel, product 2's accumulate form
        "panels": dict(m=mm.PANEL_ROWS_PER_CU * cus + 37, n=w, folds=("interleaved", 4), nalpha=3),
    }


def fold_ids(case, seed=0):
    """The fold id of every row of a case (int64 ndarray)."""
    kind, K = case["folds"]
    m = case["m"]
    if kind == "interleaved":
        return np.arange(m) % K
    if kind == "contiguous":
        return np.repeat(np.arange(K), [m // K + (1 if f < m % K else 0) for f in range(K)])
    ids = np.random.default_rng(1000 + seed).integers(0, K, size=m)
    ids[:K] = np.arange(K)                 # no fold empty whatever the draw
    return ids


def case_cells(dtype, case, cus):
    """The cells fista_cv launches for a case: train-store per row panel, heldout-resid on all rows."""
    out = {("p1f", dtype, f"RB{mm.rb(rows, cus)}", "train-store") for rows in mm.panels(case["m"], cus)}
    out.add(("p1f", dtype, f"RB{mm.rb(case['m'], cus)}", "heldout-resid"))
    return out


def build(cus):
    rows = []
    for dtype in ("f32", "bf16"):
        named = shapes(dtype, cus)
        for geometry in ("RB1", "RB2"):
            for variant in VARIANTS:
                cell = ("p1f", dtype, geometry, variant)
                cases = [dict(c, name=k) for k, c in named.items() if cell in case_cells(dtype, c, cus)]
                rows.append(dict(table="p1f", dtype=dtype, geometry=geometry, variant=variant, cases=cases))
    return rows


ROWS = build(mm.GPU_CUS)


def cells(rows=None):
    return {(r["table"], r["dtype"], r["geometry"], r["variant"]) for r in (ROWS if rows is None else rows)}
