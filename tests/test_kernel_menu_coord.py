"""CPU guard: the coverage table of the coordinate update cells (tests/_menu_coord.py) is in step with the one separable update
launch behind run_multi_mfma and with the COORD form of the update body, and its shapes are the ones the update can go wrong at."""
import pytest

from tests import _menu_coord as mc, _menu_cv
from tests._menu_product1 import _text
from tests.test_kernel_menu_multi import CU_COUNTS


def test_table_covers_every_coordinate_cell():
    mc.check_coverage()
    assert len(mc.cells()) == 2 * 3 * 2               # dtype x form x prox kind


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_shapes(cus):
    for dtype, gran in (("f32", 4), ("bf16", 8)):
        named = mc.shapes(dtype, cus)
        assert set(named) == set(_menu_cv.shapes(dtype, cus)) | {"whole_wgs"}
        for k, c in _menu_cv.shapes(dtype, cus).items():
            assert (named[k]["m"], named[k]["n"]) == (c["m"], c["n"])         # imported, not restated
        assert named["whole_wgs"]["n"] % 64 == 0                              # whole 64-column update workgroups
        tail = named["one_tile"]["n"] % 64
        assert tail == gran and tail // 4 == (1 if dtype == "f32" else 2)      # the last workgroup owns one quad (fp32)
        assert 0 < named["edges"]["n"] % 64 < 64
        assert all(c["n"] % gran == 0 and 64 < c["n"] <= 16384 for c in named.values())


def test_guard_names_a_removed_branch(tmp_path):
    """The guard itself: the coordinate form, the per-column prox kind or a prox kind of the body removed from a copy of the source
    fails naming the cell."""
    fista, upd = _text(mc.FISTA), _text(mc.UPDATE)
    cuts = (
        (fista, "fos_fista.hip", "has_coord(p) ? fos::fista_update_multi_kernel<true>", "false ? fos::fista_update_multi_kernel<true>", "upd/bf16/one-launch-controlled/PROX_ENET"),
        (fista, "fos_fista.hip", "    mu.prox_bits |= (f->prm.prox_kind == fos::PROX_ENET ? 1 : 0) << v;\n", "", "upd/f32/mixed-families-plain/PROX_L1"),
        (upd, "reduce_update.hpp", "      if (prm.prox_kind == PROX_ENET) xn *= 1.0 / (1.0 + tau * a2p);\n", "", "upd/f32/one-launch-plain/PROX_ENET"),
    )
    for text, name, old, new, cell in cuts:
        assert text.count(old) == 1, old
        fake = tmp_path / name
        fake.write_text(text.replace(old, new))
        kw = {"fista": str(fake)} if name.endswith(".hip") else {"update": str(fake)}
        with pytest.raises(AssertionError) as err:
            mc.check_coverage(**kw)
        assert cell in str(err.value), (cell, str(err.value))
