"""CPU guard: the coverage table of the fold instantiations of product 1 (tests/_menu_cv.py) names every cell of the launch
tables kF32Folds / kBf16Folds (csrc/fos_plan.hip), every case lands on the cells it is filed under, and the launcher picks
the tile variant the table's route restates."""
import os
import re

import pytest

from tests import _menu_cv as mc, _menu_multi as mm
from tests.test_kernel_menu import _initialiser
from tests.test_kernel_menu_multi import PLAN, _body, _text, CU_COUNTS

FOLD = {"fos::FOLD_TRAIN": "train", "fos::FOLD_HELD": "heldout", "fos::FOLD_OFF": "off"}


def parse(plan=PLAN):
    """The set of (table, dtype, geometry, variant) cells the two fold tables instantiate."""
    tp = _text(plan)
    cells = set()
    for name, kern, dtype, skip in (("kF32Folds", "residual_batch_mfma_kernel", "f32", 1),
                                    ("kBf16Folds", "residual_batch_mfma_bf16_kernel", "bf16", 2)):
        found = re.findall(kern + r"\s*<([^<>]*)>", _initialiser(tp, name))
        assert found, name
        for args in found:
            a = [s.strip() for s in args.split(",")]
            assert len(a) == skip + 3, (name, a)
            if dtype == "bf16":
                assert int(a[1]) == mm.TILE_COLS["bf16"], a
            assert a[skip + 1] == "false", (name, a, "the fold forms read the problem's own b")
            cells.add(("p1f", dtype, f"RB{int(a[0])}", FOLD[a[skip + 2]] + ("-store" if a[skip] == "true" else "-resid")))
    return cells


def _describe(cells):
    return "\n  ".join("/".join(c) for c in sorted(cells))


def check_coverage(plan=PLAN):
    src, table = parse(plan), mc.cells()
    msg = [f"{what}:\n  {_describe(c)}" for what, c in (("cells without a row in tests/_menu_cv.py", src - table),
                                                          ("rows without a cell in the source", table - src)) if c]
    assert not msg, "\n".join(msg)


def test_table_covers_every_instantiated_cell():
    check_coverage()
    assert len(mc.ROWS) == len(mc.cells()) == 2 * 2 * 2          # dtype x RB x {train-store, heldout-resid}


def test_fold_cells_stay_out_of_the_unmasked_tables():
    """kF32Batch / kBf16Batch hold no fold form: tests/test_kernel_menu_multi.py parses them for the unmasked cells."""
    tp = _text(PLAN)
    for name in ("kF32Batch", "kBf16Batch"):
        assert "FOLD" not in _initialiser(tp, name), name


def test_launcher_shares_the_grid_of_the_unmasked_product():
    """The RB route of the table (mm.rb) is launch_batch_product's: both launchers take it from batch_grid."""
    tp = _text(PLAN)
    grid = _body(tp, r"static\s+BatchGrid\s+batch_grid\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"const\s+int\s+variant\s*=\s*rows_total\s*>=\s*%d\s*\*\s*\(int64_t\)\s*p->ncu\s*\?\s*1\s*:\s*0" % mm.RB2_ROWS_PER_CU, grid)
    for fn in ("launch_batch_product", "launch_batch_product_folds"):
        body = _body(tp, r"int\s+" + fn + r"\s*\([^)]*\)\s*(?=\{)")
        assert re.search(r"batch_grid\s*\(\s*p\s*,\s*rows_total\s*\)", body), fn
    body = _body(tp, r"int\s+launch_batch_product_folds\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"kBf16Folds\s*\[\s*g\.variant\s*\]", body) and re.search(r"kF32Folds\s*\[\s*g\.variant\s*\]", body)
    assert len(re.findall(r"rout\s*\?\s*v[qf]\.store_train\s*:\s*v[qf]\.resid_held", body)) == 2


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_cases_land_on_their_cell(cus):
    for row in mc.build(cus):
        cell = (row["table"], row["dtype"], row["geometry"], row["variant"])
        assert row["cases"], (cus, cell)
        for c in row["cases"]:
            assert cell in mc.case_cells(row["dtype"], c, cus), (cus, cell, c)
            assert c["n"] % {"f32": 4, "bf16": 8}[row["dtype"]] == 0 and 64 < c["n"] <= mm.MFMA_MAX_N
            ids = mc.fold_ids(c)
            K = c["folds"][1]
            assert len(ids) == c["m"] and set(ids.tolist()) == set(range(K)) and K * c["nalpha"] >= 1
    named = mc.shapes("f32", cus)
    assert named["one_tile"]["m"] == mm.TILE_ROWS + 3 and named["one_tile"]["n"] == mm.TILE_COLS["f32"] + 4
    assert mm.rb(named["rb2"]["m"], cus) == 2 and mm.rb(named["rb2"]["m"] - 2, cus) == 1     # just past the threshold
    tail = mm.panels(named["panels"]["m"], cus)
    assert len(tail) == 2 and tail[1] < mm.TILE_ROWS
    edges = mc.fold_ids(named["edges"])
    cuts = [int(i) for i in range(1, len(edges)) if edges[i] != edges[i - 1]]
    assert cuts == [201, 401, 601, 801] and all(c % 4 and c % 16 for c in cuts)           # inside a 4-row group and a 16-row block
    assert named["edges"]["folds"][1] * named["edges"]["nalpha"] == 15 and named["edges"]["n"] % 64


def test_guard_names_a_deleted_instantiation(tmp_path):
    """The guard itself: an instantiation removed from, changed in or added to a copy of the source fails by name."""
    with open(PLAN) as fh:
        text = fh.read()
    for old, new, cell in (
            ("fos::residual_batch_mfma_kernel<2, false, false, fos::FOLD_HELD>}", "nullptr}", "p1f/f32/RB2/heldout-resid"),
            ("    {fos::residual_batch_mfma_bf16_kernel<1, 128, true, false, fos::FOLD_TRAIN>,\n", "    {nullptr,\n",
             "p1f/bf16/RB1/train-store"),
            ("{fos::residual_batch_mfma_kernel<1, true, false, fos::FOLD_TRAIN>,", "{fos::residual_batch_mfma_kernel<1, true, false, fos::FOLD_HELD>,",
             "p1f/f32/RB1/heldout-store"),
            ("     fos::residual_batch_mfma_bf16_kernel<2, 128, false, false, fos::FOLD_HELD>},\n",
             "     fos::residual_batch_mfma_bf16_kernel<4, 128, false, false, fos::FOLD_HELD>},\n", "p1f/bf16/RB4/heldout-resid")):
        assert text.count(old) == 1, old
        fake = tmp_path / "fos_plan.hip"
        fake.write_text(text.replace(old, new))
        with pytest.raises(AssertionError) as err:
            check_coverage(plan=str(fake))
        assert cell in str(err.value), (cell, str(err.value))
