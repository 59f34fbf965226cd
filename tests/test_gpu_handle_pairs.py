"""GPU: every ordered pair of lockstep configurations on ONE problem handle (tests/_handle_pairs.py has the cells, the moves and
the fp64 references; tests/test_handle_pairs.py checks that table on the CPU).

fos_problem_set_loss / _set_link_loss / _set_multinomial, fos_row_weights_bind and fos_coord_bind say "nothing to invalidate",
fos_feature_groups_bind and fos_problem_replan re-bind or drop buffers beside the bindings that stay, and every lockstep call of a
handle shares its workspace.  Five parts, per storage type (f32, bf16):

1. each cell on a fresh handle: served (asserted), within the project's 1e-5 of its fp64 reference (the sums within the bounds of
   their fp32 passes), and a second fresh handle gives the same bits - the precondition of everything below;
2. every ordered pair (X, Y), X != Y: configure(X), call(X), move(X, Y), call(Y), move(Y, X), call(X) on one handle; Y's result
   and the second X's are bit for bit those of the fresh handles, and after each move the getters report the configuration just
   set.  All 1722 pairs at the padded shape; at the two-panel shape the pairs in which X or Y is a CV, objective, working-set,
   certificate or multinomial cell (buffers sized by the panel count);
3. a replan with the bindings in place: call(X), move(X, Y), replan(), call(Y) gives the fresh bits, replan(interleave=True)
   stays within 1e-5 of the reference where the plan then deals the rows round-robin (at these shapes it does not: the fresh
   bits), and back gives the fresh bits again; the getters still report Y;
4. the same call at another width: path 16 -> path 3 -> path 16 on the plain, factor and logistic configurations, C = 7 (14
   columns) -> C = 3 (15 columns) -> C = 7 on the multinomial one, the certificate of 16 columns -> 3 -> 16 (the columns >= nv of
   its 4 x 16 answer are 0 each time);
5. a refused certificate between two calls: for every configuration of the table that fos_duality_gap refuses (bounds, feature
   groups, bounds under the weighted logistic and under the Huber loss, the three multinomial ones) call(X), fos_duality_gap through the C ABI -
   FOS_ERR_UNSUPPORTED with the guard's text, nothing launched -, call(X): the fresh bits both times, getters and plan unchanged.

The certificate cells (fos_duality_gap on 16, 3, 5, 16, 5, 5 and 16 columns of a seeded block with one zero column, on the
plain, weighted, logistic, Huber, weighted squared-hinge and positive-factor configurations, and certified_path) are checked on
the fresh handle against tests/_duality.certificate - primal, dual and gap within 1e-5 of the magnitude of their terms, the scale
to 1e-12, gap == primal - dual, G within the bound of fos_gradient_batch - and against tests/_duality.certified.

No pair comparison has a tolerance and nothing skips.  Before the resampled cells (below): 33 cells (36 with the narrow twins of
part 4), 1056 ordered pairs per storage type at the padded shape and 900 at the two-panel shape; the 452 tests took 41 to 47 s on the MI355X (the 328 tests of
25 cells, 600 and 444 pairs before the certificate cells: 32 s in the same session; the slowest test 0.69 s then, and the
slowest that the certificate cells add, the two-panel pairs of certified_path on bf16, 0.62 s).

What fails when the library is wrong (five temporary edits, each run against this file on the MI355X).  No defect was found, and
four of the five edits change no bit - each removes one of two layers that keep an unused column harmless:
- xp_pack_kernel / xq_pack_kernel copy columns j >= nv of the caller's block: nothing fails, and nothing can from Python -
  Problem._block16 hands the library an n_dev x 16 block that is zero beyond nv, so the copy writes the same zeros;
- softmax_link_kernel and pointwise_link_kernel leave columns >= nv of the panel as they came in: nothing fails - the lockstep
  zeroes the candidate block at every call and writes y into columns < nv only, so product 1 leaves exact zeros there for a
  link loss (Z = A Y, no b), and the updates read columns < nv of product 2 alone;
- fos_problem_set_loss keeps link_param: nothing fails, and nothing can - the parameter is read on a Huber or squared-hinge
  handle only (fos_problem_get_link_loss answers 0 otherwise), and the one way to such a handle, fos_problem_set_link_loss, sets
  it;
- stage_b16_kernel leaves columns >= nv of ws.b16 unwritten: nothing fails - those columns of R, of the slabs and of the sums
  are whatever the allocation held, and every reader (updates, q_part) is bounded by nv: columns never meet in either product;
- no memset of the candidate block in run_multi_mfma (the edit of tests/test_gpu_cluster_planned.py): 207 of the 328 tests
  fail, 57 of them in part 1 (first test_cell_on_a_fresh_handle[path16-panels-bf16]) with NaN iterates against the reference -
  the rows n .. n_pad of the block and the columns >= nv keep what the allocation held.

Four more temporary edits, of fos_duality_gap's host part alone (values only), each run once against this file,
tests/test_gpu_cluster_planned.py and tests/test_gpu_duality.py with the certificate cells in place:
- launch_dual_link passes p->b and p->row_weight without + row0: 100 of the 452 tests fail, all at the two-panel shape and
  every padded one passes - the 16 fresh certificate cells there (first test_cell_on_a_fresh_handle[gap16-panels-f32], against
  fp64), their 16 replans, the 66 two-panel pair tests and the two width runs.  The cluster-planned file passes: 8200 and 4200
  rows are one panel.  tests/test_gpu_duality.py fails in its 12 two-panel end-to-end cases;
- product 1 of fos_duality_gap also sets L.row_weight: 148 fail - the fresh weights_gap5 and hinge_weights_gap5 cells at both
  shapes against fp64 (first test_cell_on_a_fresh_handle[weights_gap5-padded-f32]), and through their missing fresh results
  every pair test; the unweighted cells pass.  The weighted logistic cell of the cluster-planned file fails, the squared one
  passes;
- the dual_scale_kernel launch is skipped: 200 fail, and not only "Y after X" as expected - ws.dual_col also carries the penalty
  and the conjugate of the ridge term to the finish, so every certificate is wrong from the first call on a fresh handle (first
  test_cell_on_a_fresh_handle[gap16-padded-f32], against fp64);
- nparts is not advanced between panels (the second panel's partial sums overwrite the first's): the same 100 tests as under
  the first edit fail, first test_cell_on_a_fresh_handle[gap16-panels-f32]; one-panel shapes pass.

The resampled cells (include/fos_resample.h: resampled_path5 with the out-of-bag sums and its 16-column twin, the weighted
logistic path of 16 columns on 0/1 counts, the Huber path under factors and the lower bound 0, the feature-group path,
fos_gradient_batch_resampled on the weighted squared-hinge handle, resampled_lipschitz on 18 resamples, the controlled run) and the
two of include/fos_multinomial_ws.h (certificate and KKT excess of five fits at C = 3, the grouped working-set path at C = 7) go
through all five parts like the others: 42 cells (46 with the twins of part 4), 1722 ordered pairs per storage type at the padded
shape and 1416 at the two-panel shape; the 572 tests take 82 to 86 s on the MI355X at 256 CUs with no skip (452 tests in 41 to 47 s
before these cells; the slowest test, the two-panel pairs of multinomial7_grouped_working_set, 2.2 s).  No defect was found.

Five temporary edits of the resampled host code (values only, every read inside the buffers of the call), each run once against
this file, tests/test_gpu_cluster_planned.py and tests/test_gpu_resample.py:
- use_cluster of run_multi_mfma without `&& !counts`: nothing fails here, and nothing can - no shape of this table is planned
  for the cluster form.  tests/test_gpu_cluster_planned.py fails in 6 tests (listed there);
- launch_resample_link takes counts without + row0: 118 of the 572 tests fail, all at the two-panel shape - the 16 fresh
  resampled cells (first test_cell_on_a_fresh_handle[resampled_path5-panels-f32], against fp64: the second panel is 37 rows
  long and already moves a fit beyond 1e-5), 14 replans, the 84 two-panel pair tests, the resampled width run and the refused
  certificate on resampled_huber_bounds_path3.  tests/test_gpu_resample.py fails in its 24 two-panel cases;
- launch_resample_link takes p->row_weight without + row0: 96 fail, all at the two-panel shape - the fresh weighted cells
  (resampled_logistic_weights_path16, resampled_gradient16, resampled_lipschitz, both storage types), their replans and the 84
  two-panel pair tests; the unweighted resampled cells pass.  tests/test_gpu_resample.py fails in 10 two-panel cases (the
  gradient, sums and Gram cases, which hold weighted cells, and the weighted out-of-bag cases);
- gradient_walk does not advance nparts (every panel's partial sums are copied to the start of ws.grad_part and the fold reads
  the last panel's count): 96 fail, all at the two-panel shape - the fresh cells with sums (resampled_path5, resampled_path16 and
  resampled_gradient16: the out-of-bag and in-bag sums against fp64; the iterates and G are right), their replans, the width run and
  the 84 two-panel pair tests.  tests/test_gpu_resample.py fails in 12 two-panel cases, the four new out-of-bag ones among them;
- the resampled branch of run_multi_mfma leaves L.row_weight set (the weight enters product 1 and the link: applied twice): 142
  fail - resampled_logistic_weights_path16 fresh at both shapes against fp64, and through its missing fresh result every pair
  test; no other weighted resampled cell goes through run_multi_mfma (resampled_gradient16 and resampled_lipschitz are the
  gradient walk and the Gram operator).  tests/test_gpu_resample.py fails test_path_matches_the_reference on the weighted
  squared and logistic handles, tests/test_gpu_cluster_planned.py its weighted logistic resampled cell on both shapes."""
import time

import pytest
import torch

from tests import _handle_pairs as hp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


class Bench:
    """The contexts and the fresh results of the module: one device matrix per (shape, storage type), one result per cell."""

    def __init__(self, fos):
        self.fos, self.ctxs, self.results = fos, {}, {}
        self.cus = fos.prepare(torch.zeros(8, 8, device="cuda")).plan()["cus"]

    def ctx(self, name, kind):
        if (name, kind) not in self.ctxs:
            self.ctxs[(name, kind)] = hp.Ctx(self.fos, hp.data(name, kind, self.cus))
        return self.ctxs[(name, kind)]

    def on_fresh(self, c, cell):
        P = c.fresh()
        c.move(P, hp.PLAIN, cell)
        c.check_getters(P, cell.cfg, ("fresh", cell.name))
        return c.run(cell, P)

    def fresh(self, name, kind, cell):
        """The result of the cell on a fresh handle, checked against its fp64 reference; computed once per module."""
        key = (name, kind, cell.name)
        if key not in self.results:
            c = self.ctx(name, kind)
            out = self.on_fresh(c, cell)
            cell.check(c.d, out)
            self.results[key] = out
        return self.results[key]


@pytest.fixture(scope="module")
def bench(fos):
    t0 = time.perf_counter()
    b = Bench(fos)
    yield b
    torch.cuda.synchronize()
    print(f"\nhandle pairs: {len(b.results)} fresh results, {time.perf_counter() - t0:.1f} s in all")
    b.ctxs.clear()
    b.results.clear()
    hp.data.cache_clear()
    hp._reference.cache_clear()
    torch.cuda.empty_cache()


_differs = hp.same_bits


# ---- 1. each cell on a fresh handle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", hp.KINDS)
@pytest.mark.parametrize("shape", hp.SHAPES)
@pytest.mark.parametrize("cell", list(hp.ALL_CELLS))
def test_cell_on_a_fresh_handle(bench, cell, shape, kind):
    c, cl = bench.ctx(shape, kind), hp.ALL_CELLS[cell]
    if shape == "padded":
        assert (c.d["m"], c.d["n"]) == hp.PADDED
        P = c.fresh()
        assert P.n == 37 and P.n_dev == (72 if kind == "bf16" else 68) and P.sample_weight is None
    first = bench.fresh(shape, kind, cl)                   # served, and within the bounds of its fp64 reference
    again = bench.on_fresh(c, cl)
    assert _differs(again, first) is None, (cell, _differs(again, first))


# ---- 2. every ordered pair -----------------------------------------------------------------------------------------------------------
def _pair(bench, c, shape, kind, x, y):
    """The six steps of a pair on one handle; the list of what differed from the fresh handles."""
    X, Y = hp.CELLS[x], hp.CELLS[y]
    fx, fy = bench.fresh(shape, kind, X), bench.fresh(shape, kind, Y)
    P = c.fresh()
    c.move(P, hp.PLAIN, X)
    bad = []
    for step, (cell, want, move) in enumerate(((X, fx, None), (Y, fy, (X, Y)), (X, fx, (Y, X)))):
        if move is not None:
            c.move(P, *move)
            c.check_getters(P, cell.cfg, (x, y, step))
        d = _differs(c.run(cell, P), want)
        if d is not None:
            bad.append((f"{x} -> {y}", ("first X", "Y after X", "X after Y")[step], d))
    return bad


@pytest.mark.parametrize("kind", hp.KINDS)
@pytest.mark.parametrize("x", list(hp.CELLS))
def test_every_ordered_pair_at_the_padded_shape(bench, x, kind):
    c = bench.ctx("padded", kind)
    bad = [b for (a, y) in hp.PAIRS if a == x for b in _pair(bench, c, "padded", kind, x, y)]
    assert not bad, bad


@pytest.mark.parametrize("kind", hp.KINDS)
@pytest.mark.parametrize("x", list(hp.CELLS))
def test_the_pairs_of_the_panel_sized_buffers_at_the_two_panel_shape(bench, x, kind):
    c = bench.ctx("panels", kind)
    assert c.d["m"] > 256 * bench.cus                      # two row panels, the second short
    bad = [b for (a, y) in hp.PANEL_PAIRS if a == x for b in _pair(bench, c, "panels", kind, x, y)]
    assert not bad, bad


# ---- 3. a replan with the bindings in place ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", hp.KINDS)
@pytest.mark.parametrize("shape", hp.SHAPES)
@pytest.mark.parametrize("y", list(hp.CELLS))
def test_replan_with_the_bindings_in_place(bench, y, shape, kind):
    c, Y = bench.ctx(shape, kind), hp.CELLS[y]
    X = hp.CELLS["huber_path5" if Y.cfg.loss == "logistic" else "logistic_path16"]        # a cell of another loss
    assert X.cfg.loss != Y.cfg.loss
    fy = bench.fresh(shape, kind, Y)
    P = c.fresh()
    c.move(P, hp.PLAIN, X)
    c.run(X, P)
    c.move(P, X, Y)
    P.replan()
    c.check_getters(P, Y.cfg, (y, "replan"))
    out = c.run(Y, P)
    assert _differs(out, fy) is None, (y, "after replan()", _differs(out, fy))
    P.replan(interleave=True)
    c.check_getters(P, Y.cfg, (y, "interleave"))
    out = c.run(Y, P)
    if P.plan()["interleave"]:                             # the row order changes the summation: the reference's bounds
        Y.check(c.d, out)
    else:                                                  # the planner does not deal these rows round-robin: the same sums
        assert _differs(out, fy) is None, (y, "after replan(interleave=True)", _differs(out, fy))
    P.replan(interleave=False)
    c.check_getters(P, Y.cfg, (y, "back"))
    out = c.run(Y, P)
    assert _differs(out, fy) is None, (y, "after replan(interleave=False)", _differs(out, fy))


# ---- 4. the same call at another width -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", hp.KINDS)
@pytest.mark.parametrize("shape", hp.SHAPES)
@pytest.mark.parametrize("config", list(hp.WIDTHS))
def test_the_same_call_at_another_width(bench, config, shape, kind):
    c = bench.ctx(shape, kind)
    wide, narrow = (hp.ALL_CELLS[n] for n in hp.WIDTHS[config])
    fw, fn = bench.fresh(shape, kind, wide), bench.fresh(shape, kind, narrow)
    P = c.fresh()
    at = hp.PLAIN
    for cell, want in ((wide, fw), (narrow, fn), (wide, fw), (narrow, fn)):
        c.move(P, at, cell)
        at = cell.cfg
        c.check_getters(P, cell.cfg, (config, cell.name))
        out = c.run(cell, P)
        assert _differs(out, want) is None, (config, cell.name, _differs(out, want))


# ---- 5. a refused certificate between two calls ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", hp.KINDS)
@pytest.mark.parametrize("shape", hp.SHAPES)
@pytest.mark.parametrize("cell", list(hp.REFUSED))
def test_a_refused_certificate_leaves_the_handle_alone(bench, cell, shape, kind):
    import ctypes as C
    c, X = bench.ctx(shape, kind), hp.REFUSED[cell]
    want = bench.fresh(shape, kind, X)
    P = c.fresh()
    c.move(P, hp.PLAIN, X)
    assert _differs(c.run(X, P), want) is None
    getters, plan = c.getters(P), P.plan()
    block = torch.zeros(P.n_dev, 16, device="cuda")
    G = torch.full((2, P.n_dev), 9.0, device="cuda")
    out64 = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
    a = (C.c_double * 2)(0.5, 0.25)
    with P.ctx():
        rc = P.lib.fos_duality_gap(C.c_void_p(block.data_ptr()), 2, a, a, P.h, C.c_void_p(G.data_ptr()), C.c_void_p(out64.data_ptr()))
    message = P.lib.fos_last_error().decode()
    assert rc == hp.FOS_ERR_UNSUPPORTED and hp.refusal(X.cfg) in message, (rc, message)
    torch.cuda.synchronize()
    assert bool((G == 9.0).all()) and bool((out64 == 7.0).all())           # nothing was launched
    assert c.getters(P) == getters and P.plan() == plan
    c.check_getters(P, X.cfg, (cell, "refused"))
    assert _differs(c.run(X, P), want) is None, (cell, "after the refusal", _differs(c.run(X, P), want))
