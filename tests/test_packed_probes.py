"""The probes of the packed gradient pass (tests/_packed_probes.py) on the CPU: the NumPy model of the three launches passes
every probe check of every matrix - the bounds are proven here, on the reference alone - every named fault of the model fails
at least one, and the faults that touch only below-window elements or the lowest binades of the window PASS the norm check the
GPU suite had before (tests/test_packed_gpu.py: rel < 1e-5 on standard_normal data with eight planted elements): the gap the
probes close.  tests/test_gpu_packed_probes.py runs the same checks on the device."""
import numpy as np
import pytest

from tests import _data, _forms as F, _packed_probes as PP
from tests.test_packed_format import roundtrip

# (edges515x144: the narrowest width the packed plan serves - 9 live threads of 512 - which tests/test_gpu_packed_probes.py finds
# by asking the planner; edges515x80: narrower than any plan serves, for the mirror alone)
MATRICES = ["edges37x16368", "edges260x4112", "edges1x16384", "edges515x144", "edges515x80", "heavy", "low", "high", "unsampled"]
# where each fault is looked for: the matrix whose probes reach it
FAULT_CASE = {f: "edges260x4112" for f in PP.FAULTS}
FAULT_CASE.update(csc_past_64_dropped="heavy", csr_last_dropped="heavy")


def runners(case, fault=None):
    model = PP.Model(case, fault)
    return model.probe, lambda **kw: model.run(None, **kw)


@pytest.mark.parametrize("name", MATRICES)
def test_model_passes_every_probe(name):
    case = PP.case(name)
    worst_row, worst_col = PP.all_checks(case, *runners(case))
    print(f"{name}: window {case.e0}, share {case.share:.2e}, worst row error / bound {worst_row:.2f}, column rr {worst_col:.2f}")
    assert worst_row <= 1.0 and worst_col <= 1.0


def test_model_passes_on_another_slab_split():
    """Row i in slab 0 (its placeholder and its correction meet in fp64) and in another slab (they meet in the fp32 slab sum)."""
    case = PP.case("edges260x4112")
    for nslab in (1, 7):
        model = PP.Model(case, nslab=nslab)
        PP.all_checks(case, model.probe)


def test_heavy_over_the_cap_is_refused_and_its_probes_are_exact_too():
    case = PP.case("heavy_over_cap")
    assert case.packed is None and 1.19e-3 < case.share < 1.25e-3
    PP.sum_probe_b(case)
    PP.sum_probe_y(case)                                    # (the helper asserts the exactness of every partial sum)


@pytest.mark.parametrize("fault", PP.FAULTS)
def test_every_fault_fails_a_probe(fault):
    case = PP.case(FAULT_CASE[fault])
    with pytest.raises(AssertionError):
        PP.all_checks(case, *runners(case, fault))


def _old_case():
    from tests.test_packed_gpu import _case
    return _case(260, 4112)


@pytest.mark.parametrize("fault", PP.QUIET_FAULTS)
def test_quiet_faults_pass_the_old_norm_check(fault):
    """The whole-gradient check of tests/test_packed_gpu.py::test_packed_gradient on its own matrix, with the fault: passes."""
    A, b, y, (g_ref, rr_ref), _ = _old_case()
    case = PP.Case("old", A)
    clean, _ = PP.Model(case).run(b, y, 0.3)
    g, rr = PP.Model(case, fault).run(b, y, 0.3)
    assert not np.array_equal(g, clean)                    # the fault is there ...
    assert _data.rel(g.astype(np.float64), g_ref) < PP.TOL and rr == pytest.approx(rr_ref, rel=PP.TOL)     # ... and not seen
    assert _data.rel(clean.astype(np.float64), g_ref) < PP.TOL


def test_loud_faults_fail_the_old_norm_check_or_need_the_probes():
    """For the record: which of the other faults the old check would have caught on its matrix (no exception list there is
    longer than two, none is read in the momentum form)."""
    A, b, y, (g_ref, rr_ref), _ = _old_case()
    case = PP.Case("old", A)
    seen = {f for f in PP.FAULTS if _data.rel(PP.Model(case, f).run(b, y, 0.3)[0].astype(np.float64), g_ref) >= PP.TOL}
    assert not seen & set(PP.QUIET_FAULTS)
    assert not seen & {"csc_past_64_dropped", "bprime_y_is_x_cur"}
    print("the old norm check sees:", sorted(seen))


@pytest.mark.parametrize("name", MATRICES)
def test_every_matrix_round_trips(name):
    case = PP.case(name)
    nex, e0 = roundtrip(case.A, case.threads)
    assert nex == int(case.out.sum()) and e0 == case.e0
    if case.n <= 8192:                                      # a copy laid out for the wider geometry: dead threads from n / 16 on
        assert roundtrip(case.A, 1024) == (nex, e0)


def test_dropping_d_moves_the_forms_run():
    """tests/test_gpu_packed_forms.py relies on this: on its heavy-tailed S-f32 matrix (window 114, 9e-4 exceptions: packed)
    a pass that dropped D altogether - FISTA on the decoded P instead of A - ends the 8-iteration window at least 100 x TOL
    from the oracle, for both weights of the cells.  Planted magnitudes uniform(16, 256) suffice: no larger value was needed."""
    A, b, L, lam = PP.forms_data(256)
    case = PP.Case("forms", A)
    assert case.e0 == 114 and 8.5e-4 < case.share < 9.5e-4, (case.e0, case.share)
    P64 = PP.Model(case, "d_dropped").P64
    assert np.array_equal(PP.Model(case).P64, P64) and not np.array_equal(P64, A)
    for cls in ("plain", "backtracking"):
        for w, (f1, a2) in enumerate(F.weights(PP.FORMS_FAMILY, cls)):
            prm = F.class_params(PP.FORMS_FAMILY, cls, w)[0]
            bt = cls == "backtracking"
            x = F.oracle_states(A, b, L, prm, f1 * lam, a2, F.WINDOW, backtracking=bt)[-1]["x"]
            x_fault = F.oracle_states(P64, b, L, prm, f1 * lam, a2, F.WINDOW, backtracking=bt)[-1]["x"]
            moved = _data.rel(x_fault, x)
            print(f"{cls} weights {w}: D dropped moves the run by {moved:.2e}")
            assert moved >= 100 * F.TOL, (cls, w, moved)
    # the momentum form: b' formed from x_cur instead of y (no probe of Problem.gemv_pair reaches it on the device: the cells of
    # tests/test_gpu_packed_forms.py are what catches it there) moves the plain run as far
    for w, (f1, a2) in enumerate(F.weights(PP.FORMS_FAMILY, "plain")):
        prm = F.class_params(PP.FORMS_FAMILY, "plain", w)[0]
        assert prm["mode"] == "fista" and prm["prox"] == "l1"
        x = F.oracle_states(A, b, L, prm, f1 * lam, a2, F.WINDOW)[-1]["x"]
        assert _data.rel(PP.fista_with_pass(A, b, L, f1 * lam, a2, F.WINDOW, P64), x) < 1e-12      # the three launches, right
        moved = _data.rel(PP.fista_with_pass(A, b, L, f1 * lam, a2, F.WINDOW, P64, bprime_from_x_cur=True), x)
        print(f"plain weights {w}: b' from x_cur moves the run by {moved:.2e}")
        assert moved >= 100 * F.TOL, (w, moved)
    # the stopped cell: the oracle stops on the ratio rule strictly inside the window, well clear of the threshold
    prm = F.stop_params(PP.FORMS_FAMILY)
    for f1, a2 in F.weights(PP.FORMS_FAMILY, "controlled"):
        last = F.oracle_states(A, b, L, prm, f1 * lam, a2, F.WINDOW)[-1]
        assert last["stopped"] == F.STOP_RATIO and 0 < last["k"] < F.WINDOW
        assert abs(last["this"] / last["prev"] - prm["tol_ratio"]) > 0.05
