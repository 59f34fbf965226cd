"""CPU: the arithmetic behind the two-product features on a cluster-planned problem (tests/_cluster_planned.py).

The restatement of plan_multi_mfma's split arithmetic is pinned to the source, and the refusal of two_product_splits
(csrc/fos_fista.hip: "the cluster layout of this problem has too few slabs for the two-product form") is swept over the CU
counts of tests/test_kernel_menu_multi.py."""
import numpy as np
import pytest

from tests import _cluster_planned as cp, _coord as cd, _menu_multi as mm
from tests._menu_product1 import FISTA, PLAN
from tests.test_kernel_menu_multi import CU_COUNTS

LARGE_M = 1 << 20
WIDTHS = range(2049, mm.MFMA_MAX_N + 1, 4)


@pytest.fixture(scope="module", autouse=True)
def _release_the_recipes():
    """The cached designs of the controlled case (0.4 GB of host memory per shape) go when the module is done."""
    yield
    cp.data.cache_clear()


def test_restatement_matches_the_source():
    cp.check_source()


def test_restatement_equals_the_kernel_menu_table():
    """Where tests/_menu_multi.py restates the same quantities, the two agree."""
    for cus in CU_COUNTS:
        for m, n in list(cp.SHAPES.values()) + [(131072, 4096), (65536, 8192), (LARGE_M, 6148), (300, 132)]:
            lay = cp.two_product_layout(m, n, cus)
            assert lay["rows_per_split"] == mm.split_rows("f32", m, n, cus), (cus, m, n)
            assert len(mm.panels(m, cus)) == -(-m // lay["panel_rows"]) and max(mm.panels(m, cus)) == min(m, lay["panel_rows"]), (cus, m, n)
            assert 1 <= lay["gram_splits"] <= lay["splits"], (cus, m, n, lay)


def test_the_shapes_are_cluster_planned_on_the_device_the_table_names():
    for name, (m, n) in cp.SHAPES.items():
        assert mm.cluster_size(m, n, mm.GPU_CUS) == cp.EXPECTED_CS[name], name
        assert m * n * 4 <= 140 * 10 ** 6, name
        assert not cp.refused(m, n, mm.GPU_CUS), name
    m, n = cp.SHAPES["cs4"]
    assert m % (mm.PANEL_ROWS_PER_CU) and n == 4 * mm.CP_W                   # a ragged last row panel under full strips
    m, n = cp.SHAPES["cs8"]
    assert -(-n // mm.CP_W) < 8 and n % mm.CP_W                              # members without a column, a strip that ends inside a block


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_the_refusal_of_two_product_splits_is_unreachable(cus):
    """For every fp32 width the cluster form can be planned at (2049 .. 16384 columns, steps of 4), at the fewest rows the planner
    accepts and at 2^20 rows, the cluster layout holds at least as many slab sets as the two-product form has row splits: the
    refusal never fires on 64, 128, 256 or 304 CUs (304 plans no cluster form at all).

    Why: there are CUs / cs clusters with cs <= 16, so at least CUs / 16 slab sets; the two-product form wants at most
    ceil(2 CUs / strips) splits with strips = ceil(n / 64) >= 33 from 2049 columns on - at most ceil(2 CUs / 33) <= CUs / 16.  So
    no GPU cell for the refusal exists at any size: none is added to tests/test_gpu_cluster_planned.py."""
    fired = []
    planned = 0
    for n in WIDTHS:
        m_min = cp.min_cluster_rows(n, cus)
        if m_min is None:
            assert mm.cluster_size(LARGE_M, n, cus) == 0
            continue
        assert mm.cluster_size(m_min, n, cus) and not mm.cluster_size(m_min - 1, n, cus), (cus, n)
        for m in (m_min, LARGE_M):
            planned += 1
            if cp.refused(m, n, cus):
                fired.append((cus, n, m))
    assert not fired, fired[:10]
    assert (planned == 0) == (cus == 304)


def test_split_arithmetic_at_the_shapes():
    """The numbers behind the GPU cells on 256 CUs: 8, 7 and 2 row splits of product 2 against 64, 32 and 16 slab sets."""
    got = {name: (cp.two_product_layout(m, n, 256)["gram_splits"], cp.clusters(m, n, 256)) for name, (m, n) in cp.SHAPES.items()}
    assert got == {"cs4": (8, 64), "cs8": (7, 32), "cs16": (2, 16)}, got


def test_guard_names_an_edited_constant(tmp_path):
    """An edited constant in a copy of the source fails the pin."""
    with open(PLAN) as fh:
        plan = fh.read()
    with open(FISTA) as fh:
        fista = fh.read()
    for text, path, old, new in (
            (plan, "fos_plan.hip", "std::max<int64_t>(1, p->multi.panel_rows / 256)", "std::max<int64_t>(1, p->multi.panel_rows / 128)"),
            (plan, "fos_plan.hip", "int64_t splits = std::max<int64_t>(1, (2 * (int64_t)p->ncu + strips - 1) / strips);\n  splits = std::min<int64_t>(splits, std::max<int64_t>(1, p->multi.panel_rows",
             "int64_t splits = std::max<int64_t>(1, (4 * (int64_t)p->ncu + strips - 1) / strips);\n  splits = std::min<int64_t>(splits, std::max<int64_t>(1, p->multi.panel_rows"),
            (plan, "fos_plan.hip", "p->multi.gram_splits = p->multi.cp_clusters;", "p->multi.gram_splits = 2 * p->multi.cp_clusters;"),
            (fista, "fos_fista.hip", "if (*g_splits > p->multi.gram_splits)", "if (*g_splits >= p->multi.gram_splits)")):
        assert text.count(old) == 1, old
        fake = tmp_path / path
        fake.write_text(text.replace(old, new))
        with pytest.raises(AssertionError):
            cp.check_source(**{"plan" if path == "fos_plan.hip" else "fista": str(fake)})


@pytest.mark.parametrize("name", ["cs4", "cs8"])
def test_the_controlled_case_decides_by_a_margin(name):
    """The preconditions of the device-controlled test on the oracle's run alone: a weight that stops early, one that runs to the
    end, a genuine restart, and every restart and stop decision further from its threshold than fp32 can move it."""
    refs = cp.control_references(name)
    cp.check_control(refs)
    assert cp.control_margin(refs) >= cp.MIN_CONTROL_MARGIN > cd.MARGIN
    assert len(refs) == cp.CONTROL_WEIGHTS == 16


@pytest.mark.parametrize("cell", list(cp.CERT_CELLS))
@pytest.mark.parametrize("name", ["cs4", "cs8"])
def test_the_certificate_cells_meet_their_preconditions(name, cell):
    """Both arms of the scale and of the conjugate are live and no gap is rounding noise, on the fp64 certificate alone."""
    ref = cp.check_certificate_case(name, cell)
    print(f"{name} {cell}: scales {np.round(ref['scale'], 3).tolist()}, smallest gap / magnitude {(ref['gap'] / ref['mag_gap'])[1:].min():.2e}")
    cp.certificate_case.cache_clear()


@pytest.mark.parametrize("cell", ["resampled_path", "resampled_weighted_logistic_path", cp.RESAMPLE_PLAIN])
@pytest.mark.parametrize("name", ["cs4", "cs8"])
def test_the_resampled_fits_have_left_zero(name, cell):
    """Every reference fit of a resampled path cell has zero and non-zero coefficients after ITERS iterations under the bound
    max_i c_ij L: the GPU comparison is not one of vectors that never left 0, and the penalty bites."""
    cs = cp.resample_case(name, cell)
    C = cs["counts"]
    assert C.shape == (cp.SHAPES[name][0], len(cs["L"])) and (cs["L"] >= cp.data(name)["L"]).all()
    if cell == "resampled_path":
        assert C.max() >= 3 and (C.sum(axis=0) == C.shape[0]).all()       # bootstrap columns: a step several times shorter
    else:
        assert set(np.unique(C)) == {0, 1}
    for r in range(C.shape[1]):
        for a in range(len(cs["alphas"])):
            x = cp.resample_reference(name, cell, r, a)
            assert (x == 0).any() and (x != 0).any(), (r, a, int((x != 0).sum()))
    print(f"{name} {cell}: largest count per resample {C.max(axis=0).tolist()}")


@pytest.mark.parametrize("name", ["cs4", "cs8"])
def test_the_resampled_controlled_case_keeps_half_of_its_cells(name):
    """The (resample, weight) cells of the controlled resampled run that the fp64 reference decides fp32-proof: at least half of
    the 32, with an early stop, a full run and a genuine restart among them."""
    C, weights, kept = cp.resample_control_case(name)
    cp.check_resample_control(kept)
    assert len(weights) == cp.CONTROL_WEIGHTS and set(np.unique(C)) == {0, 1}
    print(f"{name}: {len(kept)} of 32 cells kept, iterations {[(ra, r['k']) for ra, r in sorted(kept.items())]}")
    cp.resample_control_case.cache_clear()


def test_recipe_helpers():
    assert cp.picks(1) == [0] and cp.picks(3) == [0, 1, 2] and cp.picks(16) == [0, 8, 15]
    ids = cp.fold_ids(50, 3, 1)
    assert set(ids.tolist()) == {0, 1, 2}
    start, gw = cp.group_layout(4096)
    assert start[-1] == 4096 and gw is None and (60, 70) in set(zip(start[:-1].tolist(), start[1:].tolist()))
    for m, n in cp.SHAPES.values():
        assert cp.lipschitz_bound(m, n) > (np.sqrt(m) + np.sqrt(n) + 6.6) ** 2
