"""CPU guard: the coverage table of the logistic instantiations of product 1 (tests/_menu_logit.py) names every unweighted
logistic form in the form list of csrc/fos_plan.hip (tests/_menu_product1.py reads it), every case lands on the cells it is filed
under, and the one launcher takes the logistic form from the problem's loss."""
import re

import pytest

from tests import _menu_logit as ml, _menu_multi as mm, _menu_product1 as p1
from tests.test_kernel_menu_multi import PLAN, CU_COUNTS


def check_coverage(plan=PLAN):
    p1.check_coverage("p1l", ml.cells(), "tests/_menu_logit.py", plan)


def test_table_covers_every_instantiated_cell():
    check_coverage()
    assert len(ml.ROWS) == len(ml.cells()) == 2 * 2 * 4          # dtype x RB x {store, resid, train-store, heldout-resid}


def test_launcher_shares_the_grid_of_the_other_products():
    body = p1.launcher()
    # the logistic form only where b enters: fos_gram_apply (use_b = 0) gets the squared form on any problem
    assert re.search(r"\(\s*L\.use_b\s*&&\s*p->loss\s*==\s*FOS_LOSS_LOGISTIC\s*\)\s*\?\s*fos::LOSS_LOGISTIC\s*:\s*fos::LOSS_SQUARED", body)
    assert re.search(r"const\s+int\s+use_b\s*=\s*\(\s*L\.use_b\s*&&\s*L\.b\s*\)\s*\?\s*1\s*:\s*0", body)
    assert len(re.findall(r"L\.b\s*,\s*use_b\s*,\s*L\.rows\s*,", body)) == 2
    assert len(re.findall(r"L\.fold_of_row\s*,\s*held\s*,", body)) == 2


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_cases_land_on_their_cell(cus):
    for row in ml.build(cus):
        cell = (row["table"], row["dtype"], row["geometry"], row["variant"])
        assert row["cases"], (cus, cell)
        for c in row["cases"]:
            assert cell in ml.case_cells(row["dtype"], c, cus), (cus, cell, c)
            assert c["n"] % {"f32": 4, "bf16": 8}[row["dtype"]] == 0 and 64 < c["n"] <= mm.MFMA_MAX_N
    named = ml.shapes("f32", cus)
    assert mm.rb(named["rb2"]["m"], cus) == 2 and mm.rb(named["one_tile"]["m"], cus) == 1
    assert len(mm.panels(named["panels"]["m"], cus)) == 2


def test_guard_names_a_deleted_instantiation(tmp_path):
    """The guard itself: an instantiation removed from or changed in a copy of the source fails by name."""
    with open(PLAN) as fh:
        text = fh.read()
    for old, new, cell in (
            ("  X(false, false, FOLD_HELD, LOSS_LOGISTIC, false)       \\\n", "", "p1l/f32/RB2/heldout-resid"),
            ("  X(true, false, FOLD_OFF, LOSS_LOGISTIC, false)         \\\n", "", "p1l/bf16/RB1/store"),
            ("  X(false, false, FOLD_OFF, LOSS_LOGISTIC, false)        \\\n", "  X(true, false, FOLD_OFF, LOSS_LOGISTIC, false)         \\\n",
             "p1l/f32/RB1/resid"),
            ("    fos::residual_batch_mfma_bf16_kernel<2, 128, S, B, fos::F, fos::L, W>}},\n",
             "    fos::residual_batch_mfma_bf16_kernel<4, 128, S, B, fos::F, fos::L, W>}},\n", "p1l/bf16/RB4/train-store"),
            ("{fos::residual_batch_mfma_kernel<1, S, B, fos::F, fos::L, W>,", "{fos::residual_batch_mfma_kernel<2, S, B, fos::F, fos::L, W>,",
             "p1l/f32/RB1/store")):
        assert text.count(old) == 1, old
        fake = tmp_path / "fos_plan.hip"
        fake.write_text(text.replace(old, new))
        with pytest.raises(AssertionError) as err:
            check_coverage(plan=str(fake))
        assert cell in str(err.value), (cell, str(err.value))
    old = "  X(false, false, FOLD_HELD, LOSS_LOGISTIC, false)       \\\n"
    fake.write_text(text.replace(old, old.replace("LOSS_LOGISTIC", "LOSS_SQUARED ")))      # now twice in the list: a p1f cell
    with pytest.raises(AssertionError):
        check_coverage(plan=str(fake))
    with pytest.raises(AssertionError):
        p1.check_partition({}, plan=str(fake))
