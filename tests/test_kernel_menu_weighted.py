"""CPU guard: the coverage table of the weighted instantiations of product 1 (tests/_menu_weighted.py) names every cell of the
launch tables kF32Weighted / kBf16Weighted (csrc/fos_plan.hip), every case lands on the cells it is filed under, the launcher
takes its grid from batch_grid as the other product-1 launchers do, and the one guard helper refuses weights as well as the
logistic loss."""
import os
import re

import pytest

from tests import _logit_guard as gd, _menu_weighted as mw, _menu_multi as mm
from tests.test_kernel_menu import _initialiser
from tests.test_kernel_menu_multi import PLAN, _body, _text, CU_COUNTS

FOLD = {"fos::FOLD_TRAIN": "train-", "fos::FOLD_HELD": "heldout-", "fos::FOLD_OFF": ""}
LOSS = {"fos::LOSS_SQUARED": "squared", "fos::LOSS_LOGISTIC": "logistic"}


def parse(plan=PLAN):
    """The set of (table, dtype, geometry, variant) cells the two weighted tables instantiate."""
    tp = _text(plan)
    cells = set()
    for name, kern, dtype, skip in (("kF32Weighted", "residual_batch_mfma_kernel", "f32", 1),
                                    ("kBf16Weighted", "residual_batch_mfma_bf16_kernel", "bf16", 2)):
        found = re.findall(kern + r"\s*<([^<>]*)>", _initialiser(tp, name))
        assert found, name
        for args in found:
            a = [s.strip() for s in args.split(",")]
            assert len(a) == skip + 5, (name, a)
            if dtype == "bf16":
                assert int(a[1]) == mm.TILE_COLS["bf16"], a
            assert a[skip + 1] == "false", (name, a, "the weighted forms are not combined with several right-hand sides")
            assert a[skip + 4] == "true", (name, a, "every form of the weighted tables has WEIGHT on")
            cells.add(("p1w", dtype, f"RB{int(a[0])}",
                       LOSS[a[skip + 3]] + "/" + FOLD[a[skip + 2]] + ("store" if a[skip] == "true" else "resid")))
    return cells


def _describe(cells):
    return "\n  ".join("/".join(c) for c in sorted(cells))


def check_coverage(plan=PLAN):
    src, table = parse(plan), mw.cells()
    msg = [f"{what}:\n  {_describe(c)}" for what, c in (("cells without a row in tests/_menu_weighted.py", src - table),
                                                          ("rows without a cell in the source", table - src)) if c]
    assert not msg, "\n".join(msg)


def test_table_covers_every_instantiated_cell():
    check_coverage()
    assert len(mw.ROWS) == len(mw.cells()) == 2 * 2 * 2 * 4      # dtype x RB x loss x {store, resid, train-store, heldout-resid}


def test_weighted_cells_stay_out_of_the_other_tables():
    """The six earlier tables keep their initialisers: their guards parse a fixed argument count."""
    tp = _text(PLAN)
    for name in ("kF32Batch", "kBf16Batch", "kF32Folds", "kBf16Folds", "kF32Logit", "kBf16Logit"):
        for args in re.findall(r"_kernel\s*<([^<>]*)>", _initialiser(tp, name)):
            assert len(args.split(",")) <= (6 if "Bf16" in name else 5), (name, args)


def test_launcher_shares_the_grid_of_the_other_products():
    tp = _text(PLAN)
    body = _body(tp, r"int\s+launch_batch_product_weighted\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"batch_grid\s*\(\s*p\s*,\s*rows_total\s*\)", body)
    assert re.search(r"kBf16Weighted\s*\[\s*g\.variant\s*\]", body) and re.search(r"kF32Weighted\s*\[\s*g\.variant\s*\]", body)
    assert len(re.findall(r"fold_of_row\s*\?\s*\(\s*rout\s*\?\s*v[qf]\.train_store\s*:\s*v[qf]\.held_resid\s*\)\s*:\s*"
                          r"\(\s*rout\s*\?\s*v[qf]\.store\s*:\s*v[qf]\.resid\s*\)", body)) == 2
    assert len(re.findall(r"fold_of_row\s*,\s*hb\s*,\s*row_weight\s*\)", body)) == 2      # the weights reach both launches


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
            ("      fos::residual_batch_mfma_kernel<2, false, false, fos::FOLD_HELD, fos::LOSS_LOGISTIC, true>}}},\n", "      nullptr}}},\n",
             "p1w/f32/RB2/logistic/heldout-resid"),
            ("    {{{fos::residual_batch_mfma_bf16_kernel<1, 128, true, false, fos::FOLD_OFF, fos::LOSS_SQUARED, true>,\n", "    {{{nullptr,\n",
             "p1w/bf16/RB1/squared/store"),
            ("      fos::residual_batch_mfma_kernel<1, false, false, fos::FOLD_OFF, fos::LOSS_SQUARED, true>,\n",
             "      fos::residual_batch_mfma_kernel<1, true, false, fos::FOLD_OFF, fos::LOSS_SQUARED, true>,\n", "p1w/f32/RB1/squared/resid"),
            ("      fos::residual_batch_mfma_bf16_kernel<2, 128, true, false, fos::FOLD_TRAIN, fos::LOSS_LOGISTIC, true>,\n",
             "      fos::residual_batch_mfma_bf16_kernel<4, 128, true, false, fos::FOLD_TRAIN, fos::LOSS_LOGISTIC, true>,\n",
             "p1w/bf16/RB4/logistic/train-store")):
        assert text.count(old) == 1, old
        fake = tmp_path / "fos_plan.hip"
        fake.write_text(text.replace(old, new))
        with pytest.raises(AssertionError) as err:
            check_coverage(plan=str(fake))
        assert cell in str(err.value), (cell, str(err.value))
    fake = tmp_path / "fos_plan.hip"
    old = "fos::FOLD_OFF, fos::LOSS_SQUARED, true>,\n      fos::residual_batch_mfma_kernel<1, false"
    assert text.count(old) == 1
    fake.write_text(text.replace(old, old.replace("true>", "false>")))
    with pytest.raises(AssertionError):
        check_coverage(plan=str(fake))


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
