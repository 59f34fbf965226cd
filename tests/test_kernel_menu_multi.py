"""CPU guard: the coverage table of the multi-vector kernels (tests/_menu_multi.py) names every instantiation the
dispatchers can launch, and every case lands on the cell it is filed under.

Parsed from csrc/fos_plan.hip and csrc/fos_fista.hip: the four arrays of find_multi, the unmasked squared forms of the
product-1 table (tests/_menu_product1.py), kPairDdMulti (and the two product-2 launches of run_pair_dd_multi), the switch of
launch_cluster_pass, the ACC pairs of the product-2 launches of launch_gram_panel, and the thresholds the table's route
functions restate (the 4096 / 8192 split, 128 x CUs and 256 x CUs rows, the cluster's strip width and row count)."""
import os
import re

import numpy as np
import pytest

from tests import _data, _menu, _menu_cv, _menu_logit, _menu_multi as mm, _menu_product1 as p1, _menu_weighted
from tests._menu_product1 import CSRC, FISTA, PLAN, _body, _text
from tests.test_kernel_menu import _initialiser

CU_COUNTS = (256, 64, 128, 304)          # 304: (CUs / 8) % cs != 0 - no cluster form on such a device


def _flag(args, i):
    return len(args) > i and args[i] == "true"


def parse(plan=PLAN, fista=FISTA):
    """The set of (table, dtype, geometry, variant) cells the two sources instantiate."""
    tp, tf = _text(plan), _text(fista)
    cells = set()
    # find_multi: every multi_launch<THREADS, K, NVEC[, BBLOCK]> of its arrays
    body = _body(tp, r"MultiLaunch\s+find_multi\s*\([^)]*\)\s*(?=\{)")
    arrays = re.findall(r"static\s+const\s+MultiLaunch\s+(\w+)\s*\[\s*\d+\s*\]\s*=\s*\{([^}]*)\}", body)
    assert len(arrays) == 4, [a[0] for a in arrays]
    for _, init in arrays:
        for args in re.findall(r"multi_launch\s*<([^<>]*)>", init):
            a = [s.strip() for s in args.split(",")]
            cells.add(("valu", "f32", f"{int(a[0])}x{int(a[1])}", f"nvec{int(a[2])}" + ("-B" if _flag(a, 3) else "")))
    cells |= p1.cells(plan, "p1")
    # product 2 of the lockstep run and of fos_gram_apply
    body = _body(tf, r"static\s+int\s+launch_gram_panel\s*\([^)]*\)\s*(?=\{)")
    for acc in re.findall(r"FOS_GRAM\s*\(\s*float\s*,\s*(true|false)\s*\)", body):
        cells.add(("p2", "f32", "gram", "acc" if acc == "true" else "first"))
    for acc in re.findall(r"gram_batch_mfma_bf16_kernel\s*<\s*(true|false)\s*>", body):
        cells.add(("p2", "bf16", "gram", "acc" if acc == "true" else "first"))
    # the one-read form
    body = _body(tp, r"int\s+launch_cluster_pass\s*\([^)]*\)\s*(?=\{)")
    for case, cs in re.findall(r"case\s+(\d+)\s*:\s*return\s+launch_cluster_pass_cs\s*<\s*(\d+)\s*>", body):
        assert case == cs
        cells.add(("cluster", "f32", f"cs{int(cs)}", "pass"))
    # the fp64 pair: one entry per storage type, each with product 1 and both forms of product 2
    run = _body(tp, r"int\s+run_pair_dd_multi\s*\([^)]*\)\s*(?=\{)")
    dd_p1 = re.findall(r"residual_dd_mfma_kernel\s*<\s*T\s*>", run)
    accs = re.findall(r"gram_dd_mfma_kernel\s*<\s*T\s*,\s*(true|false)\s*>", run)
    for t in re.findall(r"run_pair_dd_multi\s*<\s*([\w:]+)\s*>", _initialiser(tp, "kPairDdMulti")):
        dtype = {"float": "f32", "fos::bf16_t": "bf16"}[t]
        for _ in dd_p1:
            cells.add(("dd", dtype, "residual", "p1"))
        for acc in accs:
            cells.add(("dd", dtype, "gram", "acc" if acc == "true" else "first"))
    return cells


def _describe(cells):
    return "\n  ".join("/".join(c) for c in sorted(cells))


def check_coverage(plan=PLAN, fista=FISTA):
    src, table = parse(plan, fista), mm.cells()
    msg = [f"{what}:\n  {_describe(c)}" for what, c in (("cells without a row in tests/_menu_multi.py", src - table),
                                                          ("rows without a cell in the source", table - src)) if c]
    assert not msg, "\n".join(msg)


def test_table_covers_every_instantiated_cell():
    check_coverage()
    assert len(mm.ROWS) == len(mm.cells()) == 12 + 8 + 8 + 4 + 3 + 2 + 4


def test_the_four_tables_share_out_the_product_1_cells():
    """The p1 rows here and the tables of the fold, logistic and weighted forms are together the 72 kernels of the source."""
    groups = {"p1": {c for c in mm.cells() if c[0] == "p1"}, "p1f": _menu_cv.cells(), "p1l": _menu_logit.cells(),
              "p1w": _menu_weighted.cells()}
    assert [len(groups[t]) for t in ("p1", "p1f", "p1l", "p1w")] == [16, 8, 16, 32]
    p1.check_partition(groups)


def test_thresholds_match_the_source():
    """The constants the route functions of the table restate."""
    tp = _text(PLAN)
    find = _body(tp, r"MultiLaunch\s+find_multi\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"if\s*\(\s*nv\s*<\s*2\s*\|\|\s*nv\s*>\s*4\s*\)\s*return\s+nullptr", find)
    split = re.findall(r"if\s*\(\s*n\s*<=\s*(\d+)\s*\)\s*return\s*\(\s*bblock\s*\?\s*(\w+)\s*:\s*(\w+)\s*\)", find)
    assert [(int(c), a, b) for c, a, b in split] == [(mm.VALU_CAP[256], "small_rhs", "small"), (mm.VALU_CAP[512], "big_rhs", "big")]
    assert re.search(r"const\s+int\s+variant\s*=\s*rows_total\s*>=\s*%d\s*\*\s*\(int64_t\)\s*p->ncu\s*\?\s*1\s*:\s*0" % mm.RB2_ROWS_PER_CU, tp)
    assert re.search(r"const\s+int64_t\s+rows\s*=\s*%d\s*\*\s*\(int64_t\)\s*p->ncu\s*;\s*p->multi\.panel_rows\s*=\s*std::min<int64_t>\(rows,\s*\(p->m\s*\+\s*255\)\s*/\s*256\s*\*\s*256\)" % mm.PANEL_ROWS_PER_CU, tp)
    assert re.search(r"p->dm\.panel_rows\s*=\s*std::min<int64_t>\(%d\s*\*\s*\(int64_t\)\s*p->ncu,\s*\(p->m\s*\+\s*255\)\s*/\s*256\s*\*\s*256\)" % mm.PANEL_ROWS_PER_CU, tp)
    assert re.search(r"cs_need\s*<=\s*2\s*\?\s*0\s*:\s*cs_need\s*<=\s*4\s*\?\s*4\s*:\s*cs_need\s*<=\s*8\s*\?\s*8\s*:\s*cs_need\s*<=\s*16\s*\?\s*16\s*:\s*0", tp)
    assert re.search(r"\(p->ncu\s*/\s*8\)\s*%\s*cs\s*==\s*0\s*&&\s*p->m\s*>=\s*\(int64_t\)\(p->ncu\s*/\s*cs\)\s*\*\s*fos::CP_ROWS\s*\*\s*"
                     + str(mm.CP_MIN_PANELS), tp)
    assert re.search(r"p->n\s*<=\s*%d" % mm.MFMA_MAX_N, _body(tp, r"bool\s+pair_dd_multi_supported\s*\([^)]*\)\s*(?=\{)"))
    consts = {}
    for hdr in ("batch_trial.hpp", "gram_batch.hpp", "gram_batch_dd.hpp", "cluster_pass.hpp", "reduce_update.hpp"):
        for names in re.findall(r"constexpr\s+int\s+((?:\w+\s*=\s*\d+\s*,?\s*)+);", _text(os.path.join(CSRC, hdr))):
            consts.update({k: int(v) for k, v in re.findall(r"(\w+)\s*=\s*(\d+)", names)})
    assert (consts["GB_COLS"], consts["GQ_COLS"], consts["BQ_COLS"]) == (mm.TILE_COLS["f32"], mm.TILE_COLS["bf16"], mm.TILE_COLS["bf16"])
    assert consts["GB_ROWS"] == consts["DM_ROWS"] == consts["BT_ROWS"] == mm.TILE_ROWS and consts["DM_COLS"] == mm.DM_COLS
    assert (consts["CP_W"], consts["CP_ROWS"], consts["BT_NV"]) == (mm.CP_W, mm.CP_ROWS, mm.NV_MAX)


def test_every_row_has_cases_or_says_why_not():
    for cus in CU_COUNTS:
        for row in mm.build(cus):
            assert bool(row["cases"]) != bool(row["unreachable"]), (cus, mm.row_id(row))
    assert all(r["unreachable"] is None for r in mm.ROWS)           # every cell is reachable on the device the table names
    shut = [mm.row_id(r) for r in mm.build(304) if r["unreachable"]]
    assert shut == ["cluster-f32-cs4-pass", "cluster-f32-cs8-pass", "cluster-f32-cs16-pass"]


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_cases_land_on_their_cell(cus):
    """Whatever the CU count: every case launches the cell it is filed under, fits its cap, and sits at the edge it is
    there for."""
    for row in mm.build(cus):
        cell = (row["table"], row["dtype"], row["geometry"], row["variant"])
        dtype = row["dtype"]
        for c in row["cases"]:
            where = (cus, mm.row_id(row), c)
            assert cell in mm.case_cells(row, c, cus), (where, mm.case_cells(row, c, cus))
            assert mm.case_bytes(row, c) <= mm.cap_bytes(row), where
            assert c["n"] % _menu.EPC[dtype] == 0 and 64 < c["n"] <= mm.MFMA_MAX_N and 1 <= c["nv"] <= mm.NV_MAX, where
            if row["table"] == "valu":
                th, k, r = c["tune"]
                assert c["n"] <= _menu.cap("f32", th, k) and not mm.is_tall("f32", c["n"]), where
                assert _menu.MENU[_menu.first_fit(_menu.MENU, "f32", c["n"])][1:4] == (th, k, r), where
            if row["table"] == "cluster":
                assert mm.cluster_size(c["m"], c["n"], cus) == int(row["geometry"][2:]), where
        if not row["cases"]:
            continue
        ms = [c["m"] for c in row["cases"]]
        if row["geometry"] == "RB2":
            assert all(mm.rb(m, cus) == 2 and len(mm.panels(m, cus)) == 1 for m in ms), (cus, mm.row_id(row))
            assert min(ms) - 1 == mm.RB2_ROWS_PER_CU * cus and mm.rb(min(ms) - 2, cus) == 1   # just past the threshold
        if row["geometry"] == "RB1" or row["variant"] == "first":
            assert all(mm.rb(m, cus) == 1 and len(mm.panels(m, cus)) == 1 for m in ms), (cus, mm.row_id(row))
            assert 1 in ms and any(1 < m < 64 for m in ms) and any(m > 64 and m % 64 == 1 for m in ms), (cus, mm.row_id(row))
        if row["variant"] == "acc":
            tails = []
            for c in row["cases"]:
                p = mm.panels(c["m"], cus)
                assert len(p) == 2, (cus, mm.row_id(row), c)
                rps = mm.split_rows(dtype, c["m"], c["n"], cus, mm.DM_COLS if row["table"] == "dd" else None)
                tails.append((p[1], -(-p[1] // rps), p[1] % rps))
            assert any(t[0] < 64 for t in tails), tails                               # a second panel below one row tile
            assert any(t[1] >= 2 and t[2] % 64 for t in tails), tails                 # several row splits, the last partial
        if row["table"] == "p2" and row["variant"] == "first":
            assert any(-(-c["m"] // mm.split_rows(dtype, c["m"], c["n"], cus)) >= 2 and
                       c["m"] % mm.split_rows(dtype, c["m"], c["n"], cus) % 64 for c in row["cases"]), (cus, mm.row_id(row))


def test_valu_tail_cases_give_the_last_workgroup_a_short_share():
    for row in mm.ROWS:
        for c in row["cases"]:
            if c["tail"]:
                rpw = -(-c["m"] // c["wg"])
                last = c["m"] - (c["wg"] - 1) * rpw
                assert 0 < last < rpw and -(-c["m"] // rpw) == c["wg"], (mm.row_id(row), c)


def test_the_groups_no_test_launched_are_rows():
    """The instantiations the table was written for are cells with cases."""
    have = {mm.row_id(r) for r in mm.ROWS if r["cases"]}
    want = [f"valu-f32-512x4-nvec{v}{s}" for v in (2, 3, 4) for s in ("", "-B")] + \
        ["p2-bf16-gram-acc", "p1-bf16-RB2-store", "p1-bf16-RB2-store-B", "p1-f32-RB2-resid-B", "p1-bf16-RB2-resid-B",
         "dd-bf16-gram-acc", "dd-f32-gram-acc", "dd-f32-residual-p1", "dd-bf16-residual-p1"]
    assert set(want) <= have, set(want) - have


def test_lockstep_forms():
    assert mm.lockstep_form("f32", 4096, 2, "b") == mm.lockstep_form("f32", 8192, 4, "B") == "valu"
    assert mm.lockstep_form("f32", 8196, 3, "b") == mm.lockstep_form("bf16", 4096, 3, "b") == "mfma"
    assert mm.lockstep_form("f32", 128, 3, "b") == "mfma"                             # a tall plan has no VALU multi pass
    assert mm.lockstep_form("f32", 8196, 2, "b") == mm.lockstep_form("bf16", 512, 2, "B") == "refused"
    assert mm.lockstep_form("f32", 512, 1, "b") == "single" and mm.lockstep_form("f32", 512, 1, "B") == "refused"


def test_guard_names_a_deleted_instantiation(tmp_path):
    """The guard itself: an instantiation removed from (or added to) a copy of the source without moving its row fails."""
    with open(PLAN) as fh:
        text = fh.read()
    for old, new, cell in (
            ("multi_launch<512, 4, 3>, ", "", "valu/f32/512x4/nvec3"),
            ("  X(false, true, FOLD_OFF, LOSS_SQUARED, false)          \\\n", "", "p1/bf16/RB2/resid-B"),
            ("  X(true, true, FOLD_OFF, LOSS_SQUARED, false)           \\\n", "  X(true, true, FOLD_TRAIN, LOSS_SQUARED, false)         \\\n",
             "p1/f32/RB1/store-B"),
            ("fos::residual_batch_mfma_kernel<2, S, B, fos::F, fos::L, W>}", "fos::residual_batch_mfma_kernel<4, S, B, fos::F, fos::L, W>}",
             "p1/f32/RB4/resid"),
            ("    case 16: return launch_cluster_pass_cs<16>(p);\n", "", "cluster/f32/cs16/pass"),
            ("    {FOS_BF16, run_pair_dd_multi<fos::bf16_t>},\n", "", "dd/bf16/gram/acc"),
            ("multi_launch<512, 4, 4, true>}", "multi_launch<512, 4, 4, true>, multi_launch<1024, 4, 4, true>}", "valu/f32/1024x4/nvec4-B")):
        assert text.count(old) == 1, old
        fake = tmp_path / "fos_plan.hip"
        fake.write_text(text.replace(old, new))
        with pytest.raises(AssertionError) as err:
            check_coverage(plan=str(fake))
        assert cell in str(err.value), (cell, str(err.value))
    with open(FISTA) as fh:
        text = fh.read()
    old = "if (accumulate) FOS_GRAM(float, true); else FOS_GRAM(float, false);"
    assert text.count(old) == 1
    fake = tmp_path / "fos_fista.hip"
    fake.write_text(text.replace(old, "FOS_GRAM(float, false);"))
    with pytest.raises(AssertionError) as err:
        check_coverage(fista=str(fake))
    assert "p2/f32/gram/acc" in str(err.value)


def test_column_tolerances_equal_the_single_column_bounds():
    """_data.fp32_pass_tolerances_cols is fp32_pass_tolerances column by column (one b, a block of them, none)."""
    rng = np.random.default_rng(5)
    for m, n, k in ((7, 12, 3), (300, 260, 4)):
        A, Y, B = rng.standard_normal((m, n)), rng.standard_normal((n, k)), rng.standard_normal((m, k))
        for blk in (None, B[:, 0], B):
            cols = [None if blk is None else blk if blk.ndim == 1 else blk[:, j] for j in range(k)]
            R = A @ Y - (0.0 if blk is None else blk if blk.ndim == 2 else blk[:, None])
            G, rr = A.T @ R, (R * R).sum(axis=0)
            g_tol, rr_tol = _data.fp32_pass_tolerances_cols(A, Y, blk, G, rr)
            for j in range(k):
                g1, r1 = _data.fp32_pass_tolerances(A, Y[:, j], cols[j], G[:, j], rr[j])
                assert g_tol[j] == pytest.approx(g1, rel=1e-12) and rr_tol[j] == pytest.approx(r1, rel=1e-12)
