"""CPU guard: the coverage table of the logistic instantiations of product 1 (tests/_menu_logit.py) names every cell of the
launch tables kF32Logit / kBf16Logit (csrc/fos_plan.hip), every case lands on the cells it is filed under, and the launcher
takes its grid from batch_grid as the other product-1 launchers do."""
import re

import pytest

from tests import _menu_logit as ml, _menu_multi as mm
from tests.test_kernel_menu import _initialiser
from tests.test_kernel_menu_multi import PLAN, _body, _text, CU_COUNTS

FOLD = {"fos::FOLD_TRAIN": "train-", "fos::FOLD_HELD": "heldout-", "fos::FOLD_OFF": ""}


def parse(plan=PLAN):
    """The set of (table, dtype, geometry, variant) cells the two logistic tables instantiate."""
    tp = _text(plan)
    cells = set()
    for name, kern, dtype, skip in (("kF32Logit", "residual_batch_mfma_kernel", "f32", 1),
                                    ("kBf16Logit", "residual_batch_mfma_bf16_kernel", "bf16", 2)):
        found = re.findall(kern + r"\s*<([^<>]*)>", _initialiser(tp, name))
        assert found, name
        for args in found:
            a = [s.strip() for s in args.split(",")]
            assert len(a) == skip + 4, (name, a)
            if dtype == "bf16":
                assert int(a[1]) == mm.TILE_COLS["bf16"], a
            assert a[skip + 1] == "false", (name, a, "the logistic forms read one label vector")
            assert a[skip + 3] == "fos::LOSS_LOGISTIC", (name, a)
            cells.add(("p1l", dtype, f"RB{int(a[0])}", FOLD[a[skip + 2]] + ("store" if a[skip] == "true" else "resid")))
    return cells


def _describe(cells):
    return "\n  ".join("/".join(c) for c in sorted(cells))


def check_coverage(plan=PLAN):
    src, table = parse(plan), ml.cells()
    msg = [f"{what}:\n  {_describe(c)}" for what, c in (("cells without a row in tests/_menu_logit.py", src - table),
                                                          ("rows without a cell in the source", table - src)) if c]
    assert not msg, "\n".join(msg)


def test_table_covers_every_instantiated_cell():
    check_coverage()
    assert len(ml.ROWS) == len(ml.cells()) == 2 * 2 * 4          # dtype x RB x {store, resid, train-store, heldout-resid}


def test_logistic_cells_stay_out_of_the_other_tables():
    """kF32Batch / kBf16Batch / kF32Folds / kBf16Folds hold no logistic form: their guards parse a fixed argument count."""
    tp = _text(PLAN)
    for name in ("kF32Batch", "kBf16Batch", "kF32Folds", "kBf16Folds"):
        assert "LOSS" not in _initialiser(tp, name), name


def test_launcher_shares_the_grid_of_the_other_products():
    tp = _text(PLAN)
    body = _body(tp, r"int\s+launch_batch_product_logit\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"batch_grid\s*\(\s*p\s*,\s*rows_total\s*\)", body)
    assert re.search(r"kBf16Logit\s*\[\s*g\.variant\s*\]", body) and re.search(r"kF32Logit\s*\[\s*g\.variant\s*\]", body)
    assert len(re.findall(r"fold_of_row\s*\?\s*\(\s*rout\s*\?\s*v[qf]\.train_store\s*:\s*v[qf]\.held_resid\s*\)\s*:\s*"
                          r"\(\s*rout\s*\?\s*v[qf]\.store\s*:\s*v[qf]\.resid\s*\)", body)) == 2


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
            ("     fos::residual_batch_mfma_kernel<2, false, false, fos::FOLD_HELD, fos::LOSS_LOGISTIC>},\n", "     nullptr},\n",
             "p1l/f32/RB2/heldout-resid"),
            ("    {fos::residual_batch_mfma_bf16_kernel<1, 128, true, false, fos::FOLD_OFF, fos::LOSS_LOGISTIC>,\n", "    {nullptr,\n",
             "p1l/bf16/RB1/store"),
            ("     fos::residual_batch_mfma_kernel<1, false, false, fos::FOLD_OFF, fos::LOSS_LOGISTIC>,\n",
             "     fos::residual_batch_mfma_kernel<1, true, false, fos::FOLD_OFF, fos::LOSS_LOGISTIC>,\n", "p1l/f32/RB1/resid"),
            ("     fos::residual_batch_mfma_bf16_kernel<2, 128, true, false, fos::FOLD_TRAIN, fos::LOSS_LOGISTIC>,\n",
             "     fos::residual_batch_mfma_bf16_kernel<4, 128, true, false, fos::FOLD_TRAIN, fos::LOSS_LOGISTIC>,\n",
             "p1l/bf16/RB4/train-store")):
        assert text.count(old) == 1, old
        fake = tmp_path / "fos_plan.hip"
        fake.write_text(text.replace(old, new))
        with pytest.raises(AssertionError) as err:
            check_coverage(plan=str(fake))
        assert cell in str(err.value), (cell, str(err.value))
    fake = tmp_path / "fos_plan.hip"
    fake.write_text(text.replace("fos::LOSS_LOGISTIC>},\n};\nstruct F32LogitVariant", "fos::LOSS_SQUARED>},\n};\nstruct F32LogitVariant"))
    with pytest.raises(AssertionError):
        check_coverage(plan=str(fake))
