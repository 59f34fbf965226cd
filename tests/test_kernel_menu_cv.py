"""CPU guard: the coverage table of the fold instantiations of product 1 (tests/_menu_cv.py) names every unweighted squared
form with a fold mask in the form list of csrc/fos_plan.hip (tests/_menu_product1.py reads it), every case lands on the cells it
is filed under, and the launcher picks the tile variant the table's route restates."""
import re

import pytest

from tests import _menu_cv as mc, _menu_multi as mm, _menu_product1 as p1
from tests.test_kernel_menu_multi import PLAN, CU_COUNTS


def check_coverage(plan=PLAN):
    p1.check_coverage("p1f", mc.cells(), "tests/_menu_cv.py", plan)


def test_table_covers_every_instantiated_cell():
    check_coverage()
    assert len(mc.ROWS) == len(mc.cells()) == 2 * 2 * 2          # dtype x RB x {train-store, heldout-resid}


def test_launcher_shares_the_grid_of_the_unmasked_product():
    """The RB route of the table (mm.rb) is batch_grid's, for every form: one launcher, and the fold form follows from rout."""
    body = p1.launcher()
    assert re.search(r"L\.fold_of_row\s*\?\s*\(\s*L\.rout\s*\?\s*fos::FOLD_TRAIN\s*:\s*fos::FOLD_HELD\s*\)\s*:\s*fos::FOLD_OFF", body)
    assert len(re.findall(r"L\.fold_of_row\s*,\s*held\s*,", body)) == 2                  # ids and held block reach both launches
    assert re.search(r"const\s+fos::FoldHeld\s+held\s*=\s*L\.held\s*\?\s*\*L\.held\s*:\s*fos::FoldHeld\{\}", body)


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
            ("  X(false, false, FOLD_HELD, LOSS_SQUARED, false)        \\\n", "", "p1f/f32/RB2/heldout-resid"),
            ("  X(true, false, FOLD_TRAIN, LOSS_SQUARED, false)        \\\n", "", "p1f/bf16/RB1/train-store"),
            ("  X(true, false, FOLD_TRAIN, LOSS_SQUARED, false)        \\\n", "  X(true, false, FOLD_HELD, LOSS_SQUARED, false)         \\\n",
             "p1f/f32/RB1/heldout-store"),
            ("    fos::residual_batch_mfma_bf16_kernel<2, 128, S, B, fos::F, fos::L, W>}},\n",
             "    fos::residual_batch_mfma_bf16_kernel<4, 128, S, B, fos::F, fos::L, W>}},\n", "p1f/bf16/RB4/heldout-resid"),
            ("{fos::residual_batch_mfma_kernel<1, S, B, fos::F, fos::L, W>,", "{fos::residual_batch_mfma_kernel<2, S, B, fos::F, fos::L, W>,",
             "p1f/f32/RB1/train-store")):
        assert text.count(old) == 1, old
        fake = tmp_path / "fos_plan.hip"
        fake.write_text(text.replace(old, new))
        with pytest.raises(AssertionError) as err:
            check_coverage(plan=str(fake))
        assert cell in str(err.value), (cell, str(err.value))
