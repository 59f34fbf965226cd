"""CPU: the table of tests/_handle_pairs.py - the cells of the ordered-pair tests of tests/test_gpu_handle_pairs.py.

1. every entry point of include/*.h that binds or changes a handle's configuration is a step of some move (or has a stated
   reason not to be one), so that a new setter fails here until it has a cell;
2. every lockstep entry point is reached by a cell, and every `int fos_*(` the headers declare is such an entry point, a binding
   entry point or excused with a reason (tests/_handle_pairs.NOT_LOCKSTEP): a new header fails here until it has cells;
3. move is legal for every ordered pair of configurations: replayed against a host model of the refusal rules, which is itself
   pinned to the guards of csrc/fos_plan.hip;
4. the fp64 references of all cells run at the padded shape and meet their own preconditions: penalties that bite, the branch
   shares of the Huber and squared-hinge losses, fp32-proof decisions of the controlled cell, a grown and certified working set,
   certificates with a scale inside (0, 1) and the scale 1 whose gaps stand 100 times clear of fp32 rounding, a certified path
   whose every decision does;
5. the configurations that fos_duality_gap refuses are the guards of its source, each with a cell."""
import numpy as np
import pytest

from tests import _handle_pairs as hp, _link as lk


def _moves():
    cfgs = sorted({c.cfg for c in hp.ALL_CELLS.values()} | {hp.PLAIN})
    return [(x, y) for x in cfgs for y in cfgs if x != y]


def test_every_binding_entry_point_is_a_step_of_a_move():
    found = hp.binding_entry_points()
    assert {"fos_problem_set_loss", "fos_problem_set_link_loss", "fos_problem_set_multinomial", "fos_row_weights_bind", "fos_coord_bind",
            "fos_feature_groups_bind", "fos_problem_replan"} <= found, found
    used = {entry for x, y in _moves() for entry, _ in hp.plan_move(x, y)} - {"target", "grouped"}
    assert used.isdisjoint(hp.NOT_A_MOVE) and used | set(hp.NOT_A_MOVE) == found, (sorted(found - used - set(hp.NOT_A_MOVE)),
                                                                                  sorted((used | set(hp.NOT_A_MOVE)) - found))
    assert set(hp.GUARDS) == used
    # both directions of every binding, and every loss as the one that is set
    steps = {(entry, arg if isinstance(arg, bool) else arg[0]) for x, y in _moves() for entry, arg in hp.plan_move(x, y)
             if entry not in ("target", "grouped")}
    for entry in ("fos_row_weights_bind", "fos_coord_bind", "fos_feature_groups_bind"):
        assert {(entry, True), (entry, False)} <= steps, entry
    assert {hp.SETTER[loss] for loss in hp.LOSS_IDS} == set(hp.SETTER.values())
    assert {(hp.SETTER[loss], loss) for loss in hp.LOSS_IDS} <= steps


def test_every_lockstep_entry_point_is_reached_by_a_cell():
    reached = {e for c in hp.CELLS.values() for e in c.reaches}
    assert reached == set(hp.LOCKSTEP_ENTRY_POINTS), set(hp.LOCKSTEP_ENTRY_POINTS) ^ reached
    declared = set()
    import glob
    import os
    import re
    for path in glob.glob(os.path.join(hp.INCLUDE, "*.h")):
        with open(path) as fh:
            declared |= set(re.findall(r"\bint\s+(fos_\w+)\s*\(", fh.read()))
    assert reached <= declared, reached - declared
    # ... and the other way round: what the headers declare is reached by a cell, binds, or is excused with a reason
    assert declared == hp.declared_entry_points()
    hp.check_entry_points()
    for header, names in (("fos_resample.h", ("fos_fista_run_multi_resampled", "fos_gradient_batch_resampled", "fos_gram_apply_resampled")),
                          ("fos_multinomial_ws.h", ("fos_multinomial_gradient_batch", "fos_multinomial_kkt_scan", "fos_multinomial_duality_gap"))):
        with open(os.path.join(hp.INCLUDE, header)) as fh:
            assert set(re.findall(r"\bint\s+(fos_\w+)\s*\(", fh.read())) == set(names) <= reached, header


def test_an_entry_point_without_a_cell_fails_the_closed_check(tmp_path):
    """Each of the six entry points of fos_resample.h and fos_multinomial_ws.h fails check_entry_points once no cell reaches it,
    and so does a copy of the headers that declares an entry point which is neither reached nor excused; a declaration that binds
    (fos_*_bind, fos_problem_set_*) is left to test_every_binding_entry_point_is_a_step_of_a_move."""
    import copy
    import os
    import shutil
    new = ("fos_fista_run_multi_resampled", "fos_gradient_batch_resampled", "fos_gram_apply_resampled",
           "fos_multinomial_gradient_batch", "fos_multinomial_kkt_scan", "fos_multinomial_duality_gap")
    for entry in new:
        cells = {name: copy.copy(c) for name, c in hp.CELLS.items()}
        for c in cells.values():
            c.reaches = tuple(e for e in c.reaches if e != entry)
        with pytest.raises(AssertionError):
            hp.check_entry_points(cells=cells)
    fake = tmp_path / "include"
    shutil.copytree(hp.INCLUDE, fake)
    hp.check_entry_points(include=str(fake))                      # the copy as it is passes
    with open(fake / "fos_next.h", "w") as fh:
        fh.write('#include "fos.h"\nint fos_fista_run_multi_next(fos_fista* const* fs, int nv, int iters);\n')
    with pytest.raises(AssertionError, match="fos_fista_run_multi_next"):
        hp.check_entry_points(include=str(fake))
    os.remove(fake / "fos_next.h")
    with open(fake / "fos_resample.h") as fh:                       # a declaration that goes: the table names an entry point no header has
        text = fh.read()
    assert text.count("int fos_gram_apply_resampled(") == 1
    with open(fake / "fos_resample.h", "w") as fh:
        fh.write(text.replace("int fos_gram_apply_resampled(", "int fos_gram_apply_resampled_v2("))
    with pytest.raises(AssertionError):
        hp.check_entry_points(include=str(fake))


def test_the_host_model_is_the_guards_of_the_source():
    hp.check_guards()


def test_the_refusing_configurations_are_the_guards_of_the_certificate():
    hp.check_duality_guards()
    for cell in hp.ALL_CELLS.values():                     # a cell that drops fos_duality_gap from its reaches fails here
        if isinstance(cell, (hp.DualityGap, hp.CertifiedPath)):
            assert {"fos_duality_gap", "fos_gradient_batch"} <= set(cell.reaches) and cell.sized_by_panels, cell.name
    assert "fos_duality_gap" in hp.LOCKSTEP_ENTRY_POINTS


def test_a_changed_guard_of_the_certificate_fails_the_pin(tmp_path):
    """A guard of fos_duality_gap that is reworded, dropped or added in a copy of the source fails check_duality_guards."""
    with open(hp.FISTA) as fh:
        text = fh.read()
    new_guard = '  if (p->row_weight) return fail(FOS_ERR_UNSUPPORTED, "fos_duality_gap: row weights are bound");\n  // 1. the gradient block'
    for old, new in (('"fos_duality_gap: box bounds (fos_coord_bind) are bound;', '"fos_duality_gap: bounds are bound;'),
                     ("  if (has_fgroups(p))\n    return fail(FOS_ERR_UNSUPPORTED, \"fos_duality_gap:", "  if (false)\n    return fail(FOS_ERR_UNSUPPORTED, \"fos_duality_gap:"),
                     ("  // 1. the gradient block", new_guard)):
        assert text.count(old) == 1, old
        fake = tmp_path / "fos_fista.hip"
        fake.write_text(text.replace(old, new))
        with pytest.raises(AssertionError):
            hp.check_duality_guards(str(fake))


def test_every_move_is_legal_and_minimal():
    for x, y in _moves():
        model = hp.HostModel(x)
        steps = hp.plan_move(x, y)
        for entry, arg in steps:
            model.step(entry, arg)                         # raises Refused
        assert (model.loss, model.coord, model.groups) == (y.loss, bool(y.coord), y.groups), (x, y)
        entries = [e for e, _ in steps]
        assert len(entries) == len(set(entries)), (x, y, steps)        # every entry point at most once
        # only what differs: a binding that X and Y share is not touched
        assert ("fos_row_weights_bind" in entries) == (x.weights != y.weights)
        assert ("fos_coord_bind" in entries) == (x.coord != y.coord)                  # "bounds" <-> "factors": the one rebind
        assert ("fos_feature_groups_bind" in entries) == (x.groups != y.groups)
        assert any(e in hp.SETTER.values() for e in entries) == ((x.loss, x.classes) != (y.loss, y.classes))
        assert ("target" in entries) == (hp.target_key(x) != hp.target_key(y))
    # the model does refuse the orders plan_move avoids
    for bad in ([("fos_feature_groups_bind", True), ("fos_coord_bind", True)], [("fos_coord_bind", True), ("fos_feature_groups_bind", True)],
                [("fos_feature_groups_bind", True), ("fos_problem_set_multinomial", ("multinomial", 3))],
                [("fos_problem_set_multinomial", ("multinomial", 3)), ("fos_feature_groups_bind", True)]):
        model = hp.HostModel()
        with pytest.raises(hp.Refused):
            for entry, arg in bad:
                model.step(entry, arg)


def test_the_table_has_the_cells_and_the_pairs():
    assert len(hp.CELLS) == 42 and len(hp.PAIRS) == 42 * 41 and len(hp.ALL_CELLS) == 46
    sized = [n for n, c in hp.CELLS.items() if c.sized_by_panels]
    assert len(hp.PANEL_PAIRS) == len(hp.PAIRS) - (42 - len(sized)) * (41 - len(sized))
    for name in ("cv", "groups_cv", "logistic_objective5", "huber_objective16", "multinomial3_path5", "multinomial7_grouped_path2",
                 "working_set", "kkt_excess", "gap16", "gap3", "weights_gap5", "logistic_gap16", "huber_gap5", "hinge_weights_gap5",
                 "positive_factors_gap16", "certified_path",
                 "resampled_path5", "resampled_gradient16", "multinomial3_gap5", "multinomial7_grouped_working_set"):
        assert name in sized
    assert len(sized) == 24 and len(hp.PANEL_PAIRS) == 42 * 41 - 18 * 17
    for wide, narrow in hp.WIDTHS.values():
        a, b = hp.ALL_CELLS[wide], hp.ALL_CELLS[narrow]
        assert a.count * (a.cfg.classes or 1) != b.count * (b.cfg.classes or 1) and a.cfg._replace(classes=0) == b.cfg._replace(classes=0)


@pytest.mark.parametrize("kind", hp.KINDS)
@pytest.mark.parametrize("cell", list(hp.ALL_CELLS))
def test_the_reference_meets_its_preconditions(cell, kind):
    d = hp.data("padded", kind)
    c = hp.ALL_CELLS[cell]
    ref = c.ref(d)
    c.precondition(d, ref)
    for k, v in ref.items():
        if isinstance(v, np.ndarray) and v.dtype.kind == "f":
            assert np.isfinite(v).all(), (cell, k)
    if isinstance(c, hp.Path) and not isinstance(c, hp.Controlled):
        assert ref["x"].shape[0] == c.count
    if isinstance(c, hp.Controlled):
        ctl, weights = c.chosen(d)
        print(f"controlled {kind}: {ctl}, {len(weights)} weights, iterations {ref['info'][:, 0].tolist()}")
        assert 5 <= len(weights) <= 16
    if isinstance(c, hp.ResampledControlled):
        ctl, kept = c.chosen(d)
        print(f"{cell} {kind}: {ctl}, {len(kept)} of {c.RESAMPLES * c.WEIGHTS} pairs, iterations {ref['info'][:, 0].tolist()}")
        assert 2 * len(kept) >= c.RESAMPLES * c.WEIGHTS                      # at least half of the cell's pairs remain
    if isinstance(c, hp.MultinomialWorkingSet):
        print(f"{cell} {kind}: sizes {ref['sizes'].tolist()}, worst excess {ref['worst']:.4f}, smallest margin {ref['margin']:.2e}")
    if isinstance(c, hp.WorkingSet):
        print(f"{cell} {kind}: sizes {ref['sizes'].tolist()}, worst excess {ref['worst']:.4f}, smallest margin {ref['margin']:.2e}, gap {ref['gap']:.2e}")


@pytest.mark.parametrize("kind", hp.KINDS)
def test_the_targets_of_the_losses(kind):
    d = hp.data("padded", kind)
    assert d["A"].shape == hp.PADDED and set(np.unique(d["y01"])) == {0.0, 1.0} and set(np.unique(d["ysign"])) == {-1.0, 1.0}
    assert set(np.unique(d["y3"])) == {0.0, 1.0, 2.0} and set(np.unique(d["y7"])) == set(float(c) for c in range(7))
    assert (d["p"] == 0).any() and (d["gw"] == 0).any() and d["w"].max() == hp.WEIGHT_MAX and (d["w"] == 0).any()
