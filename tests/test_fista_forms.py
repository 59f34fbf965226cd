"""CPU guard of the table of FISTA run forms (tests/_forms.py): every exported entry point that takes a fos_fista handle is
a form, an inspector or one of the few that cannot change a handle; the host mirror is assigned only by its helpers; the
families' shapes fall where the table says on every CU count; and a wrong transition at any switch iteration the GPU cells
use moves the final iterate by at least 100 x the tolerance those cells check (tests/test_gpu_fista_forms.py)."""
import functools
import math
import os
import re

import numpy as np
import pytest

from oracle import fos_oracle as orc
from tests import _data, _forms as F
from tests.test_kernel_menu_multi import CSRC, CU_COUNTS, FISTA, _text

HEADER = os.path.join(os.path.dirname(CSRC), "..", "include", "fos.h")
HANDLE_DECL = re.compile(r"\b(fos_fista_\w+)\s*\(\s*fos_fista\s*\*\s*(?:const\s*\*\s*)?\w+")


def handle_exports(header=HEADER, fista=FISTA):
    """Exported functions whose first parameter is fos_fista* or fos_fista* const*, from the header and from the source."""
    in_header = set(HANDLE_DECL.findall(_text(header)))
    in_source = set(re.findall(r"^(?:int|int64_t|double\*|float\*)\s+(fos_fista_\w+)\s*\(\s*fos_fista\s*\*", _text(fista), re.M))
    return in_header, in_source


def check_exports(header=HEADER, fista=FISTA, forms=None):
    forms = F.FORMS if forms is None else forms
    in_header, in_source = handle_exports(header, fista)
    assert in_source == in_header, ("handle entry points of fos_fista.hip and fos.h differ", sorted(in_source ^ in_header))
    named = {e for row in forms.values() for e in row} | {e for row in F.INSPECTORS.values() for e in row} | set(F.PASSIVE)
    msg = [f"{what}: {sorted(c)}" for what, c in (("entry points without a row in tests/_forms.py", in_header - named),
                                                   ("rows naming an entry point the header does not export",
                                                    named - in_header - {"fos_fista_create"})) if c]     # (its handle is the result)
    assert not msg, "\n".join(msg)


def test_every_handle_entry_point_is_a_form_an_inspector_or_passive():
    check_exports()
    every = set(re.findall(r"\b(fos_fista_\w+)\s*\(", _text(HEADER)))
    # the batch entry points take matrices, not a handle; create returns one
    assert every - handle_exports()[0] == set(F.NOT_A_HANDLE) | {"fos_fista_create"}
    assert set(F.PASSIVE) == {"fos_fista_create", "fos_fista_destroy", "fos_fista_x", "fos_fista_gbuf", "fos_fista_history_workspace"}


def test_guard_names_a_new_entry_point_and_a_removed_row(tmp_path):
    text = _text(HEADER)
    fake = tmp_path / "fos.h"
    fake.write_text(text + "\nint fos_fista_run_twice(fos_fista* f, int iters);\n")
    fake_src = tmp_path / "fos_fista.hip"
    fake_src.write_text(_text(FISTA) + "\nint fos_fista_run_twice(fos_fista* f, int iters) { return 0; }\n")
    with pytest.raises(AssertionError) as err:
        check_exports(header=str(fake), fista=str(fake_src))
    assert "fos_fista_run_twice" in str(err.value)
    for row, gone in (("run_history", "fos_fista_run_history"), ("run_multi_folds", "fos_fista_run_multi_folds"),
                      ("run_chip", "fos_fista_run_chip"), ("graddual_update", "fos_fista_grad_dual")):
        with pytest.raises(AssertionError) as err:
            check_exports(forms={k: v for k, v in F.FORMS.items() if k != row})
        assert gone in str(err.value), row


def mirror_assignments(fista=FISTA):
    """(function, field) of every assignment to a mirror field in fos_fista.hip."""
    text = re.sub(r"//[^\n]*", "", _text(fista))
    heads = [(m.start(), m.group(1)) for m in re.finditer(r"^(?:static\s+|template[^\n]*\n\s*static\s+)?(?:[\w:]+[\s\*&]+)+(\w+)\s*\(", text, re.M)]
    out = set()
    for m in re.finditer(r"(?:\bf|\bfs\[\w+\])->(%s)\s*(?:[-+*]?=)(?!=)" % "|".join(F.MIRROR_FIELDS), text):
        owner = [name for pos, name in heads if pos < m.start()][-1]
        out.add((owner, m.group(1)))
    return out


def test_the_mirror_is_assigned_only_by_its_helpers(tmp_path):
    found = mirror_assignments()
    assert {fn for fn, _ in found} == set(F.MIRROR_WRITERS), sorted(found)
    assert {fld for _, fld in found} == set(F.MIRROR_FIELDS)
    # the two writers outside the helpers touch tau_on_device only (besides reset)
    assert {fld for fn, fld in found if fn in ("fos_fista_set_tau", "run_device_driven")} == {"tau_on_device"}
    with open(os.path.join(CSRC, "fos_internal.hpp")) as fh:
        comment = fh.read()
    assert "begin_plain ... hand_to_device" in comment and "create / reset" in comment
    # the guard itself: an entry point that writes a flag on its own fails by name
    fake = tmp_path / "fos_fista.hip"
    fake.write_text(_text(FISTA).replace("  *iters_done = 0;\n", "  *iters_done = 0;\n  f->y_valid = false;\n", 1))
    assert ("fos_fista_run_resident", "y_valid") in mirror_assignments(str(fake))


def _const(name, text):
    m = re.search(r"\b%s\s*=\s*([^;,]+)[;,]" % name, text)
    assert m, name
    return int(eval(m.group(1), {"__builtins__": {}}))


def test_planner_constants_match_the_source():
    rs = _text(os.path.join(CSRC, "resident.hpp"))
    for name in ("RS_MAX_N", "RS_MAX_M", "RS_MAX_A", "RS_CHUNK", "RS_SMALL_M"):
        assert _const(name, rs) == getattr(F, name), name
    cr = _text(os.path.join(CSRC, "chip_resident.hpp"))
    assert _const("CR_LDS_BUDGET", cr) == F.CR_LDS_BUDGET
    assert re.search(r"cr_rows_cap\(int nc\)\s*\{\s*return\s*\(CR_LDS_BUDGET - 1024\)\s*/\s*\(\(nc \+ 4\) \* 4 \+ 4\);", cr)
    fz = _text(os.path.join(CSRC, "fused_step.hpp"))
    assert _const("FZ_OWN_MAX", fz) == F.FZ_OWN_MAX and _const("FZ_ROWS", fz) == F.FZ_ROWS
    src = _text(FISTA)
    assert re.search(r"p->n %% %d != 0\s*\|\|\s*p->n > %d" % (F.FUSED_COLS, F.FUSED_MAX_N), src)
    assert re.search(r"p->m < %d \* \(int64_t\)G" % F.FUSED_ROWS_PER_CU, src)
    assert re.search(r"p->n > 16 \|\| p->comm \|\| p->m < 512 \|\| p->m > cap \* \(int64_t\)p->ncu", src)
    assert re.search(r"p->m >= 512 && iters >= 8 &&\s*\(p->n <= 8 \? p->m <= 131072 : \(p->n <= 16 && p->m <= 32768\)\)", src)
    assert re.search(r"const bool small = p->n <= fos::RS_CHUNK && p->m <= fos::RS_SMALL_M", src)


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_families_fall_where_the_table_says(cus):
    fam = F.families(cus)
    for name in ("S-f32", "S-bf16"):
        s = fam[name]
        assert not F.resident_fits(s["m"], s["n"]) and s["n"] > F.TALL_MAX_N and not F.chip_serves(s["m"], s["n"], cus, s["dtype"])
        assert F.fused_serves(s["m"], s["n"], cus, s["dtype"]) == (name == "S-f32")
        assert s["m"] % F.FZ_ROWS != 0                                   # a partial last 4-row panel
        assert not F.fused_serves(F.FUSED_ROWS_PER_CU * cus - 1, s["n"], cus)   # the smallest m the fused step serves, plus 3
    t = fam["T"]
    assert not F.resident_fits(t["m"], t["n"]) and t["n"] <= F.TALL_MAX_N and F.chip_serves(t["m"], t["n"], cus)
    # plain run takes the chip loop by itself only from 8 iterations on: the cells' calls (at most 3) stay on the two launches
    assert all(not F.chip_region(t["m"], t["n"], it) for it in (1, 2, 3)) and F.chip_region(t["m"], t["n"], 8)
    lds, reg = fam["R-lds"], fam["R-reg"]
    assert F.resident_fits(lds["m"], lds["n"]) and not F.register_resident(lds["m"], lds["n"])
    assert F.register_resident(reg["m"], reg["n"])
    A, _, _ = _data.problem("tiny")
    assert A.shape == (lds["m"], lds["n"])


def test_table_is_consistent():
    fam = F.families(256)
    assert {k[0] for k in F.SERVED} == set(fam)
    for (family, cls), forms in F.SERVED.items():
        assert cls in fam[family]["classes"] and len(forms) >= 2 and len(set(forms)) == len(forms), (family, cls)
        assert set(forms) <= set(F.universe(family, cls)), (family, cls)
        assert "reset" not in forms
    for family, spec in fam.items():
        assert {c for f, c in F.SERVED if f == family} == set(spec["classes"]), family
    # every form is served somewhere, every inspector cell has a form to run on
    assert {f for forms in F.SERVED.values() for f in forms} == set(F.FORMS) - {"reset"}
    cells = F.count_cells()
    print("cells per family:", cells, "total", sum(cells.values()))
    assert all(v > 0 for v in cells.values())


@functools.lru_cache(maxsize=None)
def _data_of(family):
    return F.make_data(family, 256, F.bf16_round_np if family == "S-bf16" else None)


def test_numpy_solver_equals_the_oracle():
    for family in ("R-lds", "T"):
        A, b, L, lam = _data_of(family)
        a1, a2 = 0.1 * lam, 0.5
        n = A.shape[1]
        x = F.faulty_run(A, b, L, dict(mode="fista", prox="l1"), a1, a2, 12)
        assert _data.rel(x, orc.fista(A, b, "elasticnet", a1, a2, max_iter=12, L=L)) < 1e-12
        x = F.faulty_run(A, b, L, dict(mode="fista", prox="l1", adaptive_restart=True, restart_threshold=0.8), a1, a2, 12)
        assert _data.rel(x, orc.fista(A, b, "elasticnet", a1, a2, max_iter=12, L=L, adaptive_restart=True, restart_threshold=0.8)) < 1e-12
        x = F.faulty_run(A, b, L, dict(mode="delta", prox="l1", delta=3.0), a1, a2, 12)
        assert _data.rel(x, orc.fista_delta(A, b, "elasticnet", a1, a2, 3.0, max_iter=12, L=L)) < 1e-12
        x = F.faulty_run(A, b, L, dict(mode="ista", prox="enet"), a1, a2, 12)
        x_o = orc.ista(np.zeros(n), lambda z: 0.5 * float(np.sum((A @ z - b) ** 2)), lambda z: A.T @ (A @ z - b),
                       lambda v, t: orc.prox_elastic_net(v, t, a1, a2), L, max_iter=12)
        assert _data.rel(x, x_o) < 1e-12
        prm = dict(mode="fista", prox="l1", **F.BACKTRACKING)
        x = F.faulty_run(A, b, L, prm, a1, a2, 12, backtracking=True)
        assert _data.rel(x, orc.fista(A, b, "elasticnet", a1, a2, max_iter=12, L=L, backtracking=True, **F.BACKTRACKING)) < 1e-12
        # ... and the iteration-by-iteration oracle the GPU cells compare with ends where orc.fista does
        st = F.oracle_states(A, b, L, prm, a1, a2, 12, backtracking=True)
        assert np.array_equal(st[-1]["x"], orc.fista(A, b, "elasticnet", a1, a2, max_iter=12, L=L, backtracking=True, **F.BACKTRACKING))


@pytest.mark.parametrize("family", sorted(F.families(256)))
def test_a_wrong_transition_moves_the_answer(family):
    """Every fault that applies to a class, injected at each switch iteration the cells use, changes the final iterate of the
    8-iteration window by at least 100 x TOL relative, for both weights of the cells.  ISTA carries no momentum: none of the
    faults applies to it (its cells check k, the step norms and the iterate itself).
    Controlled class: a genuine restart falls inside the window (every run also restarts after its first iteration, whose
    ratio is infinite), the run does not stop in it, and the sticky cells' tolerance stops it inside a request of 5.  A
    restart leaves beta = 0 for the next two iterations, where a lagging or restarted momentum IS the right one: the faults
    are injected at the switch iterations whose beta is positive in the oracle's run (at least one per weight); at the others
    the cells rest on status(): restarts, t_prev and beta are compared exactly.
    Backtracking class: genuine shrinks on both sides of every switch, no step-underflow search in the window; a step that
    reverts to its first value repeats shrinks the oracle does not make."""
    A, b, L, lam = _data_of(family)
    worst, left_out = None, set()
    for cls in F.families(256)[family]["classes"]:
        bt = cls == "backtracking"
        for w, (f1, a2) in enumerate(F.weights(family, cls)):
            a1 = f1 * lam
            for prm in F.class_params(family, cls, w):
                clean = F.faulty_run(A, b, L, prm, a1, a2, F.WINDOW, backtracking=bt)
                states = F.oracle_states(A, b, L, prm, a1, a2, F.WINDOW, backtracking=bt)
                assert _data.rel(clean, states[-1]["x"]) < 1e-12
                switches = F.switch_iterations()
                if cls == "controlled":
                    assert states[-1]["restarts"] >= 2 and states[-1]["stopped"] == F.STOP_NONE, (family, f1)
                    ratios = [s["this"] / s["prev"] for s in states[2:]]
                    assert min(abs(r - prm["restart_threshold"]) for r in ratios) > 1e-3, (family, f1, ratios)   # fp32-proof decisions
                    assert min(ratios) > 10 * prm["tol_ratio"]
                    stop = F.oracle_states(A, b, L, F.stop_params(family), a1, a2, 5)
                    assert stop[-1]["stopped"] == F.STOP_RATIO and 0 < stop[-1]["k"] < 5, (family, f1, stop[-1]["k"])
                    # a skipped switch iteration: its cells are carried by status() - t_prev there is not the t of a run
                    # that never restarted, so a missed or an extra restart shows in the t_prev / beta / restarts checks
                    never = F.oracle_states(A, b, L, dict(prm, restart_threshold=math.inf), a1, a2, F.WINDOW)
                    for at in switches:
                        if states[at]["beta"] == 0.0:
                            assert states[at]["t"] != never[at]["t"] or at <= 2, (family, f1, at)
                            assert states[at]["restarts"] >= 1
                            left_out.add(("controlled: every fault", at))
                    switches = [at for at in switches if states[at]["beta"] > 0.0]
                    assert switches, (family, f1)
                if bt:
                    ls = [s["ls"] for s in states[1:]]
                    assert max(ls) < 16, (family, prm["name"], ls)           # one batch of 16 candidates decides every search
                    for sw in sorted({nx for nx, _ in F.COUNTS}):
                        assert sum(ls[:sw]) > 0 and sum(ls[sw:]) > 0, (family, prm["name"], f1, ls)
                for fault in F.faults_of(prm, cls):
                    for at in switches:
                        counts = []
                        moved = _data.rel(F.faulty_run(A, b, L, prm, a1, a2, F.WINDOW, fault=fault, at=at, backtracking=bt,
                                                       shrinks=counts), clean) / F.TOL
                        if fault == "tau_reverts":
                            # the search finds the lost step again (that is what a search is for): the fault shows as the
                            # shrinks it repeats - the cells compare the counts and the step itself
                            assert states[at]["tau"] < states[0]["tau"] and counts[at] > ls[at], (family, prm["name"], f1, at)
                            left_out.add(("backtracking: tau_reverts (held to repeated shrinks, not to the iterate)", at))
                            continue
                        if worst is None or moved < worst[0]:
                            worst = (moved, cls, prm["name"], f1, fault, at)
    print(f"{family}: smallest fault-to-tolerance ratio {worst[0]:.0f} ({worst[1:]}); not in this minimum: {sorted(left_out) or 'nothing'}")
    assert worst[0] >= 100.0, worst


def test_the_oracle_reaches_a_step_underflow_and_the_switched_searches_do_not():
    """The stalled cells of the GPU file: the oracle's search of iteration STALL_K (S-f32, F.STALL) is a step underflow - far
    more shrinks than the 16 candidates of a batch - after searches a batch decides.  The set_tau cells: with the step doubled
    at the switch every search of the window is still decided by one batch."""
    A, b, L, lam = _data_of("S-f32")
    f1, a2 = F.STALL_WEIGHTS
    ls = [s["ls"] for s in F.oracle_states(A, b, L, F.STALL, f1 * lam, a2, F.STALL_K + 1, backtracking=True)[1:]]
    assert max(ls[:F.STALL_K]) < F.BATCH and ls[F.STALL_K] >= 40, ls
    for family in ("S-f32", "S-bf16"):
        A, b, L, lam = _data_of(family)
        for w, (f1, a2) in enumerate(F.BT_WEIGHTS):
            for prm in F.class_params(family, "backtracking", w):
                base = F.oracle_states(A, b, L, prm, f1 * lam, a2, F.WINDOW, backtracking=True)
                for nx, _ in F.COUNTS:
                    sw = F.oracle_states(A, b, L, prm, f1 * lam, a2, F.WINDOW, backtracking=True, tau_switch=(nx, 2.0 * base[nx]["tau"]))
                    ls = [s["ls"] for s in sw[1:]]
                    assert max(ls) < F.BATCH and ls[nx] > base[nx + 1]["ls"], (family, prm["name"], w, nx, ls)
