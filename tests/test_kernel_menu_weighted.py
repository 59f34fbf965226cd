"""CPU guard: the coverage table of the weighted instantiations of product 1 (tests/_menu_weighted.py) names every form with
WEIGHT on in the form list of csrc/fos_plan.hip (tests/_menu_product1.py reads it), every case lands on the cells it is filed
under, the one launcher hands the weights to both of its launches, and the one guard helper refuses weights as well as the
logistic loss."""
import os
import re

import pytest

from tests import _logit_guard as gd, _menu_weighted as mw, _menu_multi as mm, _menu_product1 as p1
from tests.test_kernel_menu_multi import PLAN, _body, _text, CU_COUNTS


def check_coverage(plan=PLAN):
    p1.check_coverage("p1w", mw.cells(), "tests/_menu_weighted.py", plan)


def test_table_covers_every_instantiated_cell():
    check_coverage()
    assert len(mw.ROWS) == len(mw.cells()) == 2 * 2 * 2 * 4      # dtype x RB x loss x {store, resid, train-store, heldout-resid}


def test_launcher_shares_the_grid_of_the_other_products():
    body = p1.launcher()
    assert re.search(r"L\.row_weight\s*!=\s*nullptr\s*\}", body)                          # WEIGHT, the last flag of the form
    assert len(re.findall(r"L\.fold_of_row\s*,\s*held\s*,\s*L\.row_weight\s*\)", body)) == 2      # the weights reach both launches


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_cases_land_on_their_cell(cus):
    for row in mw.build(cus):
        cell = (row["table"], row["dtype"], row["geometry"], row["variant"])
        assert row["cases"], (cus, cell)
        for c in row["cases"]:
            assert cell in mw.case_cells(row["dtype"], c, cus), (cus, cell, c)
            assert c["n"] % {"f32": 4, "bf16": 8}[row["dtype"]] == 0 and 64 < c["n"] <= mm.MFMA_MAX_N
    named = mw.shapes("f32", cus)
    assert (named["one_tile"]["m"], named["edges"]["m"], named["edges"]["n"]) == (67, 1001, 200)
    assert named["rb2"]["m"] == 128 * cus + 1 and mm.rb(named["rb2"]["m"], cus) == 2 and mm.rb(named["one_tile"]["m"], cus) == 1
    tail = mm.panels(named["panels"]["m"], cus)
    # the second panel: the weights offset with the panel, and a 4-row group that reaches past the last row
    assert named["panels"]["m"] == 256 * cus + 37 and len(tail) == 2 and tail[1] == 37 and tail[1] % 4


def test_guard_names_a_deleted_instantiation(tmp_path):
    """The guard itself: an instantiation removed from or changed in a copy of the source fails by name."""
    with open(PLAN) as fh:
        text = fh.read()
    for old, new, cell in (
            ("  X(false, false, FOLD_HELD, LOSS_LOGISTIC, true)\n", "  X(false, false, FOLD_HELD, LOSS_LOGISTIC, false)\n",
             "p1w/f32/RB2/logistic/heldout-resid"),
            ("  X(true, false, FOLD_OFF, LOSS_SQUARED, true)           \\\n", "", "p1w/bf16/RB1/squared/store"),
            ("  X(false, false, FOLD_OFF, LOSS_SQUARED, true)          \\\n", "  X(true, false, FOLD_OFF, LOSS_SQUARED, true)           \\\n",
             "p1w/f32/RB1/squared/resid"),
            ("    fos::residual_batch_mfma_bf16_kernel<2, 128, S, B, fos::F, fos::L, W>}},\n",
             "    fos::residual_batch_mfma_bf16_kernel<4, 128, S, B, fos::F, fos::L, W>}},\n", "p1w/bf16/RB4/logistic/train-store"),
            ("{fos::residual_batch_mfma_kernel<1, S, B, fos::F, fos::L, W>,", "{fos::residual_batch_mfma_kernel<2, S, B, fos::F, fos::L, W>,",
             "p1w/f32/RB1/squared/store")):
        assert text.count(old) == 1, old
        fake = tmp_path / "fos_plan.hip"
        fake.write_text(text.replace(old, new))
        with pytest.raises(AssertionError) as err:
            check_coverage(plan=str(fake))
        assert cell in str(err.value), (cell, str(err.value))
    old = "  X(true, false, FOLD_TRAIN, LOSS_SQUARED, true)         \\\n"
    assert text.count(old) == 1
    fake.write_text(text.replace(old, old.replace("true) ", "false)")))                    # now twice in the list: a p1f cell
    with pytest.raises(AssertionError):
        check_coverage(plan=str(fake))
    with pytest.raises(AssertionError):
        p1.check_partition({}, plan=str(fake))


def test_the_one_guard_refuses_the_loss_and_the_weights():
    defs = []
    for unit in os.listdir(gd.CSRC):
        if unit.endswith((".hip", ".hpp")):
            with open(os.path.join(gd.CSRC, unit)) as fh:
                defs += re.findall(r"^int\s+" + gd.GUARD + r"\s*\([^;{]*\)\s*\{", fh.read(), flags=re.M)
    assert len(defs) == 1, defs
    body = _body(_text(PLAN), r"int\s+" + gd.GUARD + r"\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"p->loss\s*!=\s*FOS_LOSS_SQUARED", body) and re.search(r"p->row_weight\s*!=\s*nullptr", body)
    assert len(re.findall(r"FOS_ERR_UNSUPPORTED", body)) == 2 and "fos_row_weights_bind" in body      # a message of its own
    # the weighted dispatch sits in the serving entry points only: no refusing body mentions the weights
    for name in sorted(gd.REFUSES):
        assert "row_weight" not in gd.body_of(name), name
