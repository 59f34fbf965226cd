"""The two-product features of the matrix-core lockstep on cluster-planned problems (tests/_cluster_planned.py).

A problem planned for the one-read cluster form (replan(cluster=True); the planner's own choice at 131072 x 4096 and 65536 x
8192) keeps one slab set per cluster, an exchange ring and flag words, and every feature - several right-hand sides, fold masks,
the logistic and multinomial losses, row weights, penalty factors and bounds, the group penalty, feature groups, the working-set
gradient batch, the duality-gap certificate - runs the two-product form on that layout.  Three things are checked at the smallest shapes the cluster form is
served at:

1. every feature on a cluster-planned problem Pc against the same call on a two-product problem Pt on the same device matrix:
   bit for bit (both plans compute panel rows, rows per split and the split count by the same expressions and the same kernels
   sum the same slabs in the same order: only the allocation differs), and against the family's fp64 reference at the first,
   middle and last weight;
2. the forms alternating on one problem: plain path (cluster form), feature (two products), plain path again, in every order,
   and a replan in the middle; the same with the certificate (fos_duality_gap of 16 columns, squared loss and weighted
   logistic) in the feature's place - every certificate bit for bit the fresh one, on either layout;
3. the device-controlled lockstep (adaptive restart, ratio stop per weight) on the cluster form against the oracle's decisions.

The refusal of two_product_splits has no cell here: tests/test_cluster_planned.py shows that no shape reaches it.

What fails when run_multi_mfma is wrong (three temporary edits, each run against this file on the MI355X):
- the cluster pass taken for a feature call (use_cluster without !two_products): the bitwise comparison of the two layouts fails
  in every cell of part 1, first in cs4-rhs;
- no memset of the candidate block: rows 5000 .. 5055 of the cs8 block (n_pad = 5056) keep what the allocation held, and the
  bitwise comparison of the cs8 cells fails (NaN iterates); cs4 has no padding rows (4096 = 64 x 64) and passes;
- multi.gram_splits (the number of clusters) in place of the recomputed split count: nothing fails, and nothing can - the row
  splits past the panel's rows sum no tile and write zero slabs, which the updates then add: same bits, more work.

The certificate cells (54 tests in 17 s; 46 in 17 s before them) under the four temporary edits of fos_duality_gap that
tests/test_gpu_handle_pairs.py lists: with the row weights also in product 1 the weighted logistic cell fails on both shapes
against fp64 (first cs4-weighted_logistic_gap) and the squared one passes; with dual_scale_kernel skipped all eight tests fail
(first cs4-gap); without + row0 in launch_dual_link, and with nparts not advanced, nothing fails here, and nothing can - both
shapes are a single row panel on 256 CUs, so row0 is 0 and there is one set of partial sums.  The two-panel cells of
tests/test_gpu_handle_pairs.py catch those two.

The resampled calls (include/fos_resample.h) on cs4 and cs8: run_multi_mfma keeps them off the cluster pass by the one term
`!counts` and works the row splits out in a line of its own; fos_gradient_batch_resampled and fos_gram_apply_resampled call
two_product_splits themselves.  Part 1 has a squared path of 5 bootstrap columns, the weighted logistic path of 3 subsamples, the
gradient batch (in-bag and out-of-bag) and the Gram operator on 16 columns; part 2 a "resampled" kind whose fits must also DIFFER
from the plain path's under the same weights and step; part 3 a controlled resampled run.  L is max_i c_ij times the bound of the
whole A, the same on both sides.  66 tests in 24 s on the MI355X at 256 CUs, no skip (54 in 17 s before; the slowest, the
controlled resampled run on cs4, 2.6 s).  No defect was found.  Under the five temporary edits of the resampled host code that
tests/test_gpu_handle_pairs.py lists, each run once:
- use_cluster without `&& !counts`: 6 tests fail - cs4-resampled_path and cs8-resampled_path (first; the bitwise comparison of
  the two layouts, the fits 1.9 apart, before the fp64 check is reached), the "resampled" kind of part 2 on both shapes (at
  "the two layouts": the replanned handle against the cluster-planned one; its "differs from the plain path" condition stands
  last in the test and was not reached - the cluster pass served the call with the row splits of the two-product form, so the
  update summed 8 of the 64 slab sets and the fits were neither the resampled nor the plain ones) and the controlled run on both
  shapes.  The weighted logistic cell passes, and must: row weights make the call a two-product one before `!counts` is asked.
  The gradient and Gram cells pass, and must: they do not go through run_multi_mfma.  Before these cells nothing failed under
  this edit: that was the gap;
- counts or p->row_weight without + row0 in launch_resample_link, and nparts not advanced in gradient_walk: nothing fails here,
  and nothing can - one row panel;
- L.row_weight left set in the resampled branch of run_multi_mfma: the weighted logistic resampled cell fails on both shapes
  against fp64 (relative error 0.44: the weight applied twice); both layouts agree bit for bit."""
import numpy as np
import pytest
import torch

from oracle import fos_oracle as orc
from tests import (_cluster_planned as cp, _coord as cd, _data, _duality as du, _fgroup as fg, _group as gp, _logit as lg,
                   _menu_multi as mm, _multinomial as mn, _resample as rsp, _working_set as ws)

pytestmark = pytest.mark.gpu

ITERS, TOL = cp.ITERS, cp.TOL


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


@pytest.fixture(scope="module", autouse=True)
def _release_the_recipes():
    """The cached designs (0.4 GB of host memory per shape) go when the module is done."""
    yield
    cp.data.cache_clear()
    cp.bounds.cache_clear()
    cp.certificate_case.cache_clear()
    cp.certificate_gradient.cache_clear()
    cp.resample_counts.cache_clear()
    cp.resample_control_case.cache_clear()


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def _leaves(v):
    if isinstance(v, (list, tuple)):
        for e in v:
            yield from _leaves(e)
    else:
        yield v


def assert_same_bits(a, b, where):
    """Every iterate, score, objective and info entry of two results equal bit for bit."""
    la, lb = list(_leaves(a)), list(_leaves(b))
    assert len(la) == len(lb) and any(isinstance(x, torch.Tensor) for x in la), where
    for i, (x, y) in enumerate(zip(la, lb)):
        if isinstance(x, torch.Tensor):
            assert isinstance(y, torch.Tensor) and torch.equal(x, y), (where, i, float((x - y).abs().max()))
        elif isinstance(x, np.ndarray):
            assert np.array_equal(x, y), (where, i, float(np.abs(x - y).max()))
        else:
            assert x == y, (where, i, x, y)


class Ctx:
    """The device matrix of a shape, shared by every problem of its tests, and what the cells bind to it."""

    def __init__(self, fos, name):
        self.fos, self.name, self.d = fos, name, cp.data(name)
        d = self.d
        self.At = torch.from_numpy(d["A32"].copy()).cuda()           # (the recipe's arrays are read-only)
        self.b32, self.y32, self.w32 = (d[k].astype(np.float32) for k in ("b", "y", "w"))
        self.cus = fos.prepare(self.At, self.b32).plan()["cus"]
        self.cs = mm.cluster_size(d["m"], d["n"], self.cus)
        self.L = d["L"]
        self._B = self._classes = None

    @property
    def B(self):
        """Six right-hand sides: (fp32 on the device, the same in fp64)."""
        if self._B is None:
            B32 = cp.targets(self.d, 6)
            self._B = (torch.as_tensor(B32).cuda(), B32.astype(np.float64))
        return self._B

    def classes(self, C):
        if self._classes is None or self._classes[0] != C:
            self._classes = (C, mn.labels(self.d["A"], C, self.d["seed"]))
        return self._classes[1]

    def new(self, build, cluster):
        P = build(self)
        P.replan(cluster=cluster)
        return P


@pytest.fixture(scope="module")
def ctx(request, fos):
    """The shape named by the test's parameter (indirect); one device matrix at a time."""
    c = Ctx(fos, request.param)
    yield c
    del c.At, c._B
    torch.cuda.empty_cache()


def _served(ctx):
    if not ctx.cs:
        pytest.skip(f"no cluster form for {ctx.d['m']} x {ctx.d['n']} on a device of {ctx.cus} CUs")
    if ctx.cus == mm.GPU_CUS:
        assert ctx.cs == cp.EXPECTED_CS[ctx.name]


# ---- 1. every two-product feature on a cluster-planned problem ---------------------------------------------------------------------
def _fold_rows(ctx, K):
    return cp.fold_ids(ctx.d["m"], K, ctx.d["seed"])


def _check_iterates(xs, refs, where):
    for i, ref in refs:
        assert _data.rel(_np(xs[i]), ref) < TOL, (where, i, _data.rel(_np(xs[i]), ref))


class Rhs:
    """fista(A, B) for a 2-D B: six columns, one fos_fista_run_multi_rhs call, no grouping."""
    def build(self, c):
        return c.fos.prepare(c.At, None)

    def call(self, c, P):
        a1, a2 = cp.plain_alphas(c.d)[1]
        return c.fos.fista(P, c.B[0], "elasticnet", a1, a2, max_iter=ITERS, L=c.L)

    def check(self, c, X):
        a1, a2 = cp.plain_alphas(c.d)[1]
        X = _np(X)
        _check_iterates([X[:, j] for j in range(6)],
                        [(j, orc.fista(c.d["A"], c.B[1][:, j], "elasticnet", a1, a2, max_iter=ITERS, L=c.L)) for j in cp.picks(6)], "rhs")


class Multitask:
    """multitask_path: three targets per fit under the group penalty over the lockstep columns, three fits in one call."""
    def build(self, c):
        return c.fos.prepare(c.At, None)

    def weights(self, c):
        return gp.multitask_weights(c.d["A"], c.B[1][:, :3], 3)

    def call(self, c, P):
        return c.fos.multitask_path(P, c.B[0][:, :3].contiguous(), self.weights(c), max_iter=ITERS, L=c.L, return_info=True)

    def check(self, c, out):
        refs = []
        for i, (a1, a2) in enumerate(self.weights(c)):
            X, _ = gp.iterate(gp.MultiTask(c.d["A"], c.B[1][:, :3], a1, a2), c.L, ITERS)
            zero = np.abs(X).sum(axis=1) == 0.0
            assert zero.any() and (~zero).any(), "the group penalty must bite"
            refs.append((i, X))
        _check_iterates(out[0], refs, "multitask")


def _check_cv(c, res, weights, ids, fit, score=None):
    """coefs[:, f, a] against `fit(training rows, a1, a2)` and the held-out score against `score` on the device's own iterate,
    at the first, middle and last (fold, weight) pair."""
    K, La = int(ids.max()) + 1, len(weights)
    pairs = [(f, a) for f in range(K) for a in range(La)]
    coefs = _np(res.coefs)
    for j in cp.picks(len(pairs)):
        f, a = pairs[j]
        assert _data.rel(coefs[:, f, a], fit(ids != f, *weights[a])) < TOL, (f, a)
        if score is not None:
            te = ids == f
            x32 = coefs[:, f, a].astype(np.float32).astype(np.float64)
            want, tol = score(te, x32)
            assert abs(res[1][f, a] * want[1] - want[0]) <= tol, (f, a, res[1][f, a] * want[1], want[0], tol)
    assert res.best == int(np.argmin(res[2]))


class FistaCv:
    """fista_cv: 3 folds x 6 weights as masked columns (two calls), then the refit on all rows in the same call."""
    def build(self, c):
        return c.fos.prepare(c.At, c.b32)

    def call(self, c, P):
        return c.fos.fista_cv(P, None, cp.plain_alphas(c.d), folds=_fold_rows(c, 3), max_iter=ITERS, L=c.L, return_coefs=True)

    def check(self, c, res):
        d, ids = c.d, _fold_rows(c, 3)

        def score(te, x32):
            r = d["A"][te] @ x32 - d["b"][te]
            sse = float(r @ r)
            _, tol = _data.fp32_pass_tolerances_cols(d["A"][te], x32[:, None], d["b"][te], np.zeros((d["n"], 1)), np.array([sse]))
            return (sse, int(te.sum())), float(tol[0])
        _check_cv(c, res, cp.plain_alphas(d), ids,
                  lambda tr, a1, a2: orc.fista(d["A"][tr], d["b"][tr], "elasticnet", a1, a2, max_iter=ITERS, L=c.L), score)
        # the refit alternates with the masked fits inside the one call: it is the plain path at the chosen weight on a fresh
        # cluster-planned problem, bit for bit (one weight: the single-target run on either problem)
        fresh = c.new(self.build, True)
        assert torch.equal(res.x, c.fos.fista_path(fresh, None, [cp.plain_alphas(d)[res.best]], max_iter=ITERS, L=c.L)[0])


class Path:
    """fista_path / logistic_path on a handle with a feature bound: loss, row weights, penalty factors, bounds."""
    def __init__(self, loss, weighted=False, coord=None):
        self.loss, self.weighted, self.coord = loss, weighted, coord          # coord: None, "factors" or "bounds"

    def data(self, c):
        lo = hi = None
        if self.coord == "bounds":
            _, lo, hi = cp.bounds(c.name, self.loss, self.weighted)
        lo, hi = (None if v is None else np.array(v) for v in (lo, hi))         # (writable copies: the recipe's arrays are read-only)
        return dict(p=np.array(c.d["p"]) if self.coord else None, lo=lo, hi=hi, w=c.d["w"] if self.weighted else None,
                    L=cp.L_of(c.d, self.loss, self.weighted), alphas=cp.alphas(c.d, self.loss, self.weighted))

    def build(self, c):
        t32 = c.y32 if self.loss == "logistic" else c.b32
        k = self.data(c)
        if self.coord:
            return c.fos.prepare_penalized(c.At, t32, k["p"], k["lo"], k["hi"], loss=self.loss, sample_weight=c.w32 if self.weighted else None)
        if self.weighted:
            return c.fos.prepare_weighted(c.At, t32, c.w32, loss=self.loss)
        return c.fos.prepare(c.At, t32, loss=self.loss)

    def call(self, c, P):
        k = self.data(c)
        run = c.fos.logistic_path if self.loss == "logistic" else c.fos.fista_path
        return run(P, None, k["alphas"], max_iter=ITERS, L=k["L"], return_info=True)

    def reference(self, c, a1, a2, rows=None):
        k, d = self.data(c), c.d
        A, t, w = d["A"], cp.target(d, self.loss), k["w"]
        if rows is not None:
            A, t, w = A[rows], t[rows], None if w is None else w[rows]
        return cd.run(A, t, a1, a2, k["L"], ITERS, p=k["p"], lo=k["lo"], hi=k["hi"], loss=self.loss, w=w)

    def check(self, c, out):
        k = self.data(c)
        refs = []
        for i, (a1, a2) in enumerate(k["alphas"]):
            ref = self.reference(c, a1, a2)
            assert (ref["x"] == 0).any() and (ref["x"] != 0).any(), "the penalty must bite"
            if self.coord == "bounds":
                pre = cd.preconditions(ref, cp.bounds(c.name, self.loss, self.weighted)[0], k["p"], k["lo"], k["hi"])
                assert min(pre.values()) > 0, pre                # bounds that clamp on either side, an unpenalised coordinate in the model
            refs.append((i, ref["x"]))
        _check_iterates(out[0], refs, (self.loss, self.weighted, self.coord))
        assert out[1] == [(ITERS, 0)] * len(k["alphas"])


class LogisticCv(Path):
    """logistic_cv: 2 folds x 3 weights as masked columns, the held-out log-loss pass, then the refit in the lockstep."""
    def __init__(self):
        super().__init__("logistic")

    def call(self, c, P):
        k = self.data(c)
        return c.fos.logistic_cv(P, None, k["alphas"], folds=_fold_rows(c, 2), max_iter=ITERS, L=k["L"], return_coefs=True)

    def check(self, c, res):
        d, k, ids = c.d, self.data(c), _fold_rows(c, 2)

        def score(te, x32):
            return (float(lg.nll(d["A"][te], x32, d["y"][te])), int(te.sum())), float(lg.nll_tolerance(d["A"][te], x32[:, None])[0])
        _check_cv(c, res, k["alphas"], ids, lambda tr, a1, a2: self.reference(c, a1, a2, tr)["x"], score)
        a1, a2 = k["alphas"][res.best]
        assert _data.rel(_np(res.x), self.reference(c, a1, a2)["x"]) < TOL


class ComposedCv(Path):
    """Penalty factors and bounds with row weights and a fold mask on top: fista_cv on a weighted, penalised handle."""
    def __init__(self):
        super().__init__("squared", True, "bounds")

    def call(self, c, P):
        k = self.data(c)
        return c.fos.fista_cv(P, None, k["alphas"], folds=_fold_rows(c, 2), max_iter=ITERS, L=k["L"], return_coefs=True)

    def check(self, c, res):
        k, ids = self.data(c), _fold_rows(c, 2)
        _check_cv(c, res, k["alphas"], ids, lambda tr, a1, a2: self.reference(c, a1, a2, tr)["x"])
        a1, a2 = k["alphas"][res.best]
        assert _data.rel(_np(res.x), self.reference(c, a1, a2)["x"]) < TOL


class Multinomial:
    """multinomial_path: C = 3 with five weights (five fits in 15 columns, one idle), C = 16 with two (a call each); grouped:
    the group penalty over the classes."""
    def __init__(self, C, count, grouped=False):
        self.C, self.count, self.grouped = C, count, grouped

    def weights(self, c):
        y = c.classes(self.C)
        return (gp.multinomial_weights if self.grouped else mn.weights)(c.d["A"], y, self.C, self.count)

    def build(self, c):
        return c.fos.prepare_multinomial(c.At, c.classes(self.C), self.C, grouped=self.grouped)

    def call(self, c, P):
        return c.fos.multinomial_path(P, None, self.weights(c), max_iter=ITERS, L=cp.L_of(c.d, "multinomial"), return_info=True)

    def check(self, c, out):
        y, L, w = c.classes(self.C), cp.L_of(c.d, "multinomial"), self.weights(c)
        refs = []
        for i in cp.picks(self.count):
            a1, a2 = w[i]
            if self.grouped:
                X, _ = gp.iterate(gp.GroupMultinomial(c.d["A"], y, self.C, a1, a2), L, ITERS)
                zero = np.abs(X).sum(axis=1) == 0.0
                assert zero.any() and (~zero).any(), "the group penalty must bite"
            else:
                X = mn.run(c.d["A"], y, self.C, a1, a2, L, ITERS)
                assert (X == 0).any() and (X != 0).any(), "the penalty must bite"
            refs.append((i, X))
        _check_iterates(out[0], refs, ("multinomial", self.C, self.grouped))


class FeatureGroups:
    """set_feature_groups with fista_path: the group lasso (mu = 0) and the sparse-group lasso (mu = 0.5) on a layout whose groups
    cross the 64-column update blocks."""
    def __init__(self, mu):
        self.mu = mu

    def data(self, c):
        start, gw = cp.group_layout(c.d["n"])
        return start, gw, cp.group_alphas(c.d, start, gw, self.mu)

    def build(self, c):
        start, gw, _ = self.data(c)
        return c.fos.prepare_grouped(c.At, c.b32, np.diff(start), gw, l1_ratio=self.mu)

    def call(self, c, P):
        return c.fos.fista_path(P, None, self.data(c)[2], max_iter=ITERS, L=c.L, return_info=True)

    def check(self, c, out):
        start, gw, alphas = self.data(c)
        refs = []
        for i, (a1, a2) in enumerate(alphas):
            r = fg.run(c.d["A"], c.d["b"], a1, a2, c.L, ITERS, start=start, gw=gw, mu=self.mu)
            zero, _ = fg.zero_groups(r["x"], start)
            assert zero.any() and (~zero).any() and r["closest"] >= fg.CLOSE, (i, r["closest"])
            refs.append((i, r["x"]))
        _check_iterates(out[0], refs, ("fgroup", self.mu))


class WorkingSet:
    """working_set_path on a handle with penalty factors: the KKT scans read fos_gradient_batch on the full problem, and the set
    of the weakest weight outgrows max_fraction, so the group falls back to the full lockstep on the handle itself."""
    def build(self, c):
        return c.fos.prepare_penalized(c.At, c.b32, np.array(c.d["p"]))

    def call(self, c, P):
        return c.fos.working_set_path(P, None, cp.alphas(c.d), max_iter=ITERS, L=c.L, max_rounds=1, return_info=True)

    def check(self, c, out):
        xs, infos = out
        X, info = ws.solve(c.d["A"], c.d["b"], cp.alphas(c.d), ITERS, p=c.d["p"], L=c.L, max_rounds=1)
        assert info["fell_back"] and infos[0].fell_back and infos[0].full_gradients == info["full_gradients"]
        _check_iterates(xs, [(j, X[:, j]) for j in range(3)], "working set")


class Batches:
    """fos_gradient_batch and fos_gram_apply on the problem directly: 16 columns, product 2 into the cluster layout's slabs."""
    def build(self, c):
        return c.fos.prepare(c.At, c.b32)

    def block(self, c):
        rng = np.random.default_rng(900 + c.d["seed"])
        X = rng.standard_normal((c.d["n"], 16)) * (rng.random((c.d["n"], 16)) < 0.1)
        return X.astype(np.float32)

    def call(self, c, P):
        X = torch.as_tensor(self.block(c)).cuda()
        return [P.gradient_batch(X).clone(), P.gram_apply(X).clone()]

    def check(self, c, out):
        d, X = c.d, self.block(c).astype(np.float64)
        AX = d["A"] @ X
        for got, R, b in ((out[0], AX - d["b"][:, None], d["b"]), (out[1], AX, None)):
            G = d["A"].T @ R
            g_tol, _ = _data.fp32_pass_tolerances_cols(d["A"], X, b, G, (R * R).sum(axis=0))
            err = np.linalg.norm(_np(got) - G, axis=0)
            assert (err <= g_tol).all(), (err / g_tol).max()


class Certificate:
    """fos_duality_gap on 16 columns (tests/_cluster_planned.certificate_case): the gradient block by the launches of
    fos_gradient_batch - product 2 into the cluster layout's slabs -, product 1 once more into multi.rbuf16, the row pass per panel
    of multi.panel_rows rows and ws.dual_part sized by the panel count of the plan."""
    def __init__(self, cell):
        self.cell = cell
        self.loss, self.weighted = cp.CERT_CELLS[cell]

    def build(self, c):
        if self.weighted:
            return c.fos.prepare_weighted(c.At, c.y32 if self.loss == "logistic" else c.b32, c.w32, loss=self.loss)
        return c.fos.prepare(c.At, c.y32 if self.loss == "logistic" else c.b32, loss=self.loss)

    def call(self, c, P):
        cs = cp.certificate_case(c.name, self.cell)
        out64, G = P.duality_gap_block(torch.as_tensor(cs["X"]), [a for a, _ in cs["alphas"]], [a for _, a in cs["alphas"]])
        return [out64.clone(), G.clone()]

    def check(self, c, out):
        d, cs = c.d, cp.certificate_case(c.name, self.cell)
        G64, g_tol = cp.certificate_gradient(c.name, self.cell)          # (with the preconditions of the case)
        got, G = out[0].cpu().numpy().reshape(4, 16), out[1].cpu().numpy()
        assert np.isfinite(got).all() and G.shape[0] == 16 and (G[:, d["n"]:] == 0).all()
        G = G[:, :d["n"]]
        ref = du.certificate(self.loss, d["A"], cs["t"], cs["X"], cs["alphas"], None, cs["w"], G=G)     # scale and conjugate from the returned G
        for row, key in enumerate(("primal", "dual", "gap")):
            err = np.abs(got[row] - ref[key]) / ref["mag_" + key]
            assert (err <= du.TOL).all(), (self.cell, key, err.max())
        assert np.abs(got[3] - ref["scale"]).max() <= 1e-12 and np.array_equal(got[2], got[0] - got[1])
        assert ((got[3] > 0) & (got[3] < 1)).any() and (got[3] == 1).any(), got[3]
        err = np.linalg.norm(G.T.astype(np.float64) - G64, axis=0)
        assert (err <= g_tol).all(), (self.cell, (err / g_tol).max())


def _words(P, counts):
    from fastoptsolver_amd import resample
    return resample.pack_counts(torch.from_numpy(np.ascontiguousarray(counts)).to(P.device))


class ResampledPath:
    """resampled_path (fos_fista_run_multi_resampled): every column fits a resample of the rows of its own, and the one term
    `!counts` of run_multi_mfma keeps the call off the one-read cluster pass, which knows no counts."""
    def __init__(self, cell):
        self.cell = cell

    def build(self, c):
        cs = cp.resample_case(c.name, self.cell)
        t32 = c.y32 if cs["loss"] == "logistic" else c.b32
        if cs["weighted"]:
            return c.fos.prepare_weighted(c.At, t32, c.w32, loss=cs["loss"])
        return c.fos.prepare(c.At, t32, loss=cs["loss"])

    def call(self, c, P, **control):
        cs = cp.resample_case(c.name, self.cell)
        res = c.fos.resampled_path(P, cs["alphas"], cs["counts"], ITERS, L=cs["L"], **control)
        return [res.coefs, res.info]

    def check(self, c, out, columns=None):
        cs = cp.resample_case(c.name, self.cell)
        B, La = cs["counts"].shape[1], len(cs["alphas"])
        coefs = _np(out[0])
        assert coefs.shape == (c.d["n"], B, La) and out[1] == [[(ITERS, 0)] * La] * B
        pairs = [(r, a) for r in range(B) for a in range(La)]
        for j in cp.picks(len(pairs)) if columns is None else columns:
            r, a = pairs[j]
            ref = cp.resample_reference(c.name, self.cell, r, a)
            assert (ref == 0).any() and (ref != 0).any(), "the penalty must bite"
            assert _data.rel(coefs[:, r, a], ref) < TOL, (self.cell, r, a, _data.rel(coefs[:, r, a], ref))


class ResampledGradient:
    """fos_gradient_batch_resampled through the C ABI on 16 bootstrap columns: G and the in-bag sums, then the out-of-bag sums with
    G = NULL (product 2 does not run) - gradient_walk calls two_product_splits itself."""
    cell = "resampled_gradient"

    def build(self, c):
        return c.fos.prepare(c.At, c.b32)

    def call(self, c, P):
        from fastoptsolver_amd import _core, _lib
        words = _words(P, cp.resample_counts(c.name, *cp.RESAMPLE_CELLS[self.cell][2:]))
        Xf, nv = P._block16(torch.as_tensor(cp.resample_block(c.d)))
        G = torch.full((nv, P.n_dev), float("nan"), dtype=torch.float32, device=P.device)
        out = [G]
        for oob in (0, 1):
            with P.ctx():
                _lib.check(P.lib.fos_gradient_batch_resampled(_core.ptr(Xf), nv, _core.ptr(words), oob, P.h, None if oob else _core.ptr(G),
                                                              _core.ptr(P.scratch)), "fos_gradient_batch_resampled")
            out.append(P.scratch[:16].clone())
        return out

    def check(self, c, out):
        d, n = c.d, c.d["n"]
        G, inbag, oob = (o.cpu().numpy() for o in out)
        assert G.shape[0] == 16 and np.isfinite(G).all() and (G[:, n:] == 0).all()
        cols = cp.picks(16)
        C = cp.resample_counts(c.name, *cp.RESAMPLE_CELLS[self.cell][2:])[:, cols]
        X = cp.resample_block(d).astype(np.float64)[:, cols]
        W = cp.resample_weights(d, self.cell, C)
        G_ref = rsp.gradient(rsp.SQUARED, d["A"], X, d["b"], W)
        err, g_tol = np.linalg.norm(G[cols, :n].T.astype(np.float64) - G_ref, axis=0), rsp.gradient_tolerance(d["A"], X, d["b"], W, G_ref)
        assert (err <= g_tol).all() and (np.linalg.norm(G_ref, axis=0) > 100.0 * g_tol).all(), (err, g_tol)
        for got, Wk in ((inbag, W), (oob, (C == 0).astype(np.float64))):
            ref, tol = rsp.data_term(rsp.SQUARED, d["A"], X, d["b"], Wk), rsp.loss_tolerance(rsp.SQUARED, d["A"], X, d["b"], Wk)
            assert (np.abs(got[cols] - ref) <= tol).all() and (ref > 100.0 * tol).all(), (got[cols], ref, tol)


class ResampledGram:
    """fos_gram_apply_resampled on the weighted handle, 16 subsamples: A^T ((w * c_j) * (A x_j)), the operator of the power iteration
    per resample - it calls two_product_splits itself."""
    cell = "resampled_gram"

    def build(self, c):
        return c.fos.prepare_weighted(c.At, c.b32, c.w32)

    def call(self, c, P):
        from fastoptsolver_amd import resample
        words = _words(P, cp.resample_counts(c.name, *cp.RESAMPLE_CELLS[self.cell][2:]))
        return [resample._gram_apply(P, torch.as_tensor(cp.resample_block(c.d)), words).clone()]

    def check(self, c, out):
        d, cols = c.d, cp.picks(16)
        got = _np(out[0])
        assert got.shape == (d["n"], 16) and np.isfinite(got).all() and (got[:, 1] == 0).all()         # the zero column of the block
        C = cp.resample_counts(c.name, *cp.RESAMPLE_CELLS[self.cell][2:])[:, cols]
        X = cp.resample_block(d).astype(np.float64)[:, cols]
        W = cp.resample_weights(d, self.cell, C)
        ref = d["A"].T @ (W * (d["A"] @ X))
        err, g_tol = np.linalg.norm(got[:, cols] - ref, axis=0), rsp.gram_tolerance(d["A"], X, W, ref)
        assert (err <= g_tol).all() and (np.linalg.norm(ref, axis=0) > 100.0 * g_tol).all(), (err, g_tol)


CELLS = {
    "rhs": Rhs(), "multitask": Multitask(), "fista_cv": FistaCv(),
    "logistic_path": Path("logistic"), "logistic_cv": LogisticCv(),
    "weighted": Path("squared", True), "weighted_logistic": Path("logistic", True),
    "penalty": Path("squared", False, "bounds"), "penalty_logistic": Path("logistic", False, "bounds"), "penalty_weights_folds": ComposedCv(),
    "grouped_multinomial": Multinomial(3, 3, True),
    "group_lasso": FeatureGroups(0.0), "sparse_group_lasso": FeatureGroups(0.5),
    "multinomial_c3": Multinomial(3, 5), "multinomial_c16": Multinomial(16, 2),
    "working_set": WorkingSet(), "batches": Batches(),
    "gap": Certificate("gap"), "weighted_logistic_gap": Certificate("weighted_logistic_gap"),
    "resampled_path": ResampledPath("resampled_path"), "resampled_weighted_logistic_path": ResampledPath("resampled_weighted_logistic_path"),
    "resampled_gradient": ResampledGradient(), "resampled_gram": ResampledGram(),
}
# cs16: two cells only, to bound the time - the weighted squared loss with penalty factors, and the logistic loss
CS16_CELLS = {"weighted_factors": Path("squared", True, "factors"), "logistic_path": CELLS["logistic_path"]}
ALL_CELLS = dict(CELLS, **CS16_CELLS)
PAIRS = [(name, cell) for name in ("cs4", "cs8") for cell in CELLS] + [("cs16", cell) for cell in CS16_CELLS]
TWO_SHAPES = ["cs4", "cs8"]


@pytest.mark.parametrize("ctx,cell", PAIRS, indirect=["ctx"])
def test_feature_on_a_cluster_planned_problem(ctx, cell):
    """Bitwise equality of the two layouts, per feature, on the MI355X: several right-hand sides, K-fold masks, the logistic loss,
    row weights, penalty factors and bounds, the group penalty, feature groups, the multinomial loss and the working-set gradient
    batch were all bit for bit equal on cs4 and cs8 (row weights with penalty factors and the logistic loss on cs16)."""
    _served(ctx)
    c = ALL_CELLS[cell]
    Pc, Pt = ctx.new(c.build, True), ctx.new(c.build, False)
    rc = c.call(ctx, Pc)
    rt = c.call(ctx, Pt)
    assert Pc.plan()["cluster"] == 1 and Pt.plan()["cluster"] == 0          # the cluster layout was planned under the two-product run
    assert_same_bits(rc, rt, cell)
    c.check(ctx, rc)


# ---- 2. the forms alternate on one problem ------------------------------------------------------------------------------------------
class Attach:
    """A feature bound to and detached from a plain squared-loss handle, and its path call."""
    def __init__(self, kind):
        self.kind = kind
        self.path = {"weights": Path("squared", True), "penalty": Path("squared", False, "bounds"), "groups": FeatureGroups(0.5),
                     "logistic": Path("logistic"), "resampled": ResampledPath(cp.RESAMPLE_PLAIN)}[kind]

    def target32(self, c):
        return c.y32 if self.kind == "logistic" else c.b32           # labels are a squared-loss target as good as any

    def build(self, c):
        return c.fos.prepare(c.At, self.target32(c))

    def plain_alphas(self, c):
        """Six weights (more than four: the matrix-core lockstep), the ladder of test_fista_path_one_read_cluster_pass."""
        lam = float(np.max(np.abs(c.d["A"].T @ cp.target(c.d, "logistic" if self.kind == "logistic" else "squared"))))
        return [(lam * 0.4 * 0.7 ** i, 0.5 if i % 3 == 1 else 0.0) for i in range(6)]

    def plain(self, c, P):
        return c.fos.fista_path(P, None, self.plain_alphas(c), max_iter=ITERS, L=c.L, return_info=True)

    def on(self, c, P):
        from fastoptsolver_amd import _lib
        if self.kind == "weights":
            buf = torch.zeros((c.d["m"] + 3) // 4 * 4, dtype=torch.float32, device=P.device)
            buf[:c.d["m"]] = torch.as_tensor(c.w32)
            P.set_sample_weight(buf[:c.d["m"]])
        elif self.kind == "penalty":
            k = self.path.data(c)
            P.set_penalty(k["p"], k["lo"], k["hi"])
        elif self.kind == "groups":
            start, gw, _ = self.path.data(c)
            P.set_feature_groups(np.diff(start), gw, 0.5)
        elif self.kind == "resampled":
            pass                                                     # a resampled call binds nothing: the counts travel with the call
        else:
            _lib.check(P.lib.fos_problem_set_loss(P.h, _lib.LOSS_LOGISTIC), "fos_problem_set_loss")
            P.loss = "logistic"

    def off(self, c, P):
        from fastoptsolver_amd import _lib
        if self.kind == "weights":
            P.set_sample_weight(None)
        elif self.kind == "penalty":
            P.set_penalty()
        elif self.kind == "groups":
            P.set_feature_groups(None)
        elif self.kind == "resampled":
            pass
        else:
            _lib.check(P.lib.fos_problem_set_loss(P.h, _lib.LOSS_SQUARED), "fos_problem_set_loss")
            P.loss = "squared"

    def feature(self, c, P):
        return self.path.call(c, P)


@pytest.mark.parametrize("ctx", TWO_SHAPES, indirect=True)
@pytest.mark.parametrize("kind", ["weights", "penalty", "groups", "logistic", "resampled"])
def test_forms_alternate_on_one_problem(ctx, kind):
    """Plain path (cluster form), feature (two products), plain path; the feature as the first lockstep call of the problem;
    feature, plain, feature; a replan to the two-product layout in the middle.  The cluster form is bit-reproducible
    (test_fista_path_one_read_cluster_pass) and so is the two-product form: every repeated result is bit for bit the first.
    "resampled": the feature is resampled_path on one 0/1 resample under the plain path's own six weights and step - nothing is
    bound, so only the counts of the call tell the two apart - and every fit of it must differ from the plain path's: a resampled
    call served by the cluster pass, which ignores the counts, would return the plain path's bits on every handle alike and so
    pass every "equal to the fresh one" above."""
    _served(ctx)
    a = Attach(kind)
    plain0 = a.plain(ctx, ctx.new(a.build, True))                   # a fresh cluster-planned problem
    # plain, feature, plain
    P1 = ctx.new(a.build, True)
    before = a.plain(ctx, P1)
    assert P1.plan()["cluster"] == 1
    a.on(ctx, P1)
    f1 = a.feature(ctx, P1)
    a.off(ctx, P1)
    after = a.plain(ctx, P1)
    assert P1.plan()["cluster"] == 1
    assert_same_bits(before, plain0, "plain before the feature")
    assert_same_bits(after, plain0, "plain after the feature")
    # the feature first: plan_multi_mfma is first called from a two-product run
    P2 = ctx.new(a.build, True)
    a.on(ctx, P2)
    f2 = a.feature(ctx, P2)
    assert P2.plan()["cluster"] == 1
    a.off(ctx, P2)
    assert_same_bits(a.plain(ctx, P2), plain0, "plain after a feature that ran first")
    assert_same_bits(f2, f1, "the feature as the first call")
    # feature, plain, feature
    a.on(ctx, P2)
    assert_same_bits(a.feature(ctx, P2), f2, "the feature after a plain path")
    # a replan in the middle: the same handle in the two-product layout is the two-product problem
    P2.replan(cluster=False)
    f4 = a.feature(ctx, P2)
    assert P2.plan()["cluster"] == 0
    Pt = ctx.new(a.build, False)
    a.on(ctx, Pt)
    assert_same_bits(f4, a.feature(ctx, Pt), "the feature after replan(cluster=False)")
    assert_same_bits(f4, f1, "the two layouts")
    t = cp.target(ctx.d, "logistic" if kind == "logistic" else "squared")
    a1, a2 = a.plain_alphas(ctx)[0]
    _check_iterates(plain0[0], [(0, orc.fista(ctx.d["A"], t, "elasticnet", a1, a2, max_iter=ITERS, L=ctx.L))], "plain")
    if kind == "resampled":
        assert cp.resample_case(ctx.name, cp.RESAMPLE_PLAIN)["alphas"] == a.plain_alphas(ctx)
        for i, x in enumerate(plain0[0]):
            assert np.count_nonzero(_np(x)) and not np.array_equal(_np(f1[0][:, 0, i]), _np(x)), ("the resampled fit is the plain path's", i)
        a.path.check(ctx, f1, columns=[0, 5])


class AttachCertificate:
    """A certificate cell on a plain squared-loss handle: what the cell binds goes on before the certificate and off after it."""
    def __init__(self, cell):
        self.cert = Certificate(cell)
        self.plain_form = Attach("logistic" if self.cert.loss == "logistic" else "weights")     # (for its plain path alone)

    def build(self, c):
        return c.fos.prepare(c.At, c.y32 if self.cert.loss == "logistic" else c.b32)

    def plain(self, c, P):
        return self.plain_form.plain(c, P)

    def bind(self, c, P, on):
        from fastoptsolver_amd import _lib
        if self.cert.loss == "logistic":
            _lib.check(P.lib.fos_problem_set_loss(P.h, _lib.LOSS_LOGISTIC if on else _lib.LOSS_SQUARED), "fos_problem_set_loss")
            P.loss = "logistic" if on else "squared"
        if self.cert.weighted:
            buf = None
            if on:
                buf = torch.zeros((c.d["m"] + 3) // 4 * 4, dtype=torch.float32, device=P.device)
                buf[:c.d["m"]] = torch.as_tensor(c.w32)
                buf = buf[:c.d["m"]]
            P.set_sample_weight(buf)

    def certificate(self, c, P):
        self.bind(c, P, True)
        out = self.cert.call(c, P)
        self.bind(c, P, False)
        return out


@pytest.mark.parametrize("ctx", TWO_SHAPES, indirect=True)
@pytest.mark.parametrize("cell", list(cp.CERT_CELLS))
def test_the_certificate_alternates_with_the_plain_path(ctx, cell):
    """Plain path (cluster form), certificate, plain path; certificate, plain path, certificate; then the same handle replanned
    to the two-product layout and back: every plain path is bit for bit that of a fresh cluster-planned problem and every
    certificate (out64 and G) bit for bit that of a fresh one, whichever layout it ran on."""
    _served(ctx)
    a = AttachCertificate(cell)
    plain0 = a.plain(ctx, ctx.new(a.build, True))
    cert0 = a.certificate(ctx, ctx.new(a.build, True))
    a.cert.check(ctx, cert0)
    # plain, certificate, plain
    P1 = ctx.new(a.build, True)
    assert_same_bits(a.plain(ctx, P1), plain0, "plain before the certificate")
    assert_same_bits(a.certificate(ctx, P1), cert0, "the certificate after a plain path")
    assert P1.plan()["cluster"] == 1
    assert_same_bits(a.plain(ctx, P1), plain0, "plain after the certificate")
    # certificate, plain, certificate
    P2 = ctx.new(a.build, True)
    assert_same_bits(a.certificate(ctx, P2), cert0, "the certificate as the first call")
    assert P2.plan()["cluster"] == 1
    assert_same_bits(a.plain(ctx, P2), plain0, "plain after a certificate that ran first")
    assert_same_bits(a.certificate(ctx, P2), cert0, "the certificate again")
    # a replan in the middle, in both orders
    P2.replan(cluster=False)
    assert_same_bits(a.certificate(ctx, P2), cert0, "the certificate after replan(cluster=False)")
    assert P2.plan()["cluster"] == 0
    P2.replan(cluster=True)
    assert_same_bits(a.plain(ctx, P2), plain0, "plain after replan(cluster=True)")
    assert P2.plan()["cluster"] == 1
    assert_same_bits(a.certificate(ctx, P2), cert0, "the certificate after both replans")
    P1.replan(cluster=False)
    P1.replan(cluster=True)
    assert_same_bits(a.certificate(ctx, P1), cert0, "the certificate first after a replan")
    assert_same_bits(a.plain(ctx, P1), plain0, "plain after it")


# ---- 3. the device-controlled lockstep on the cluster form ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctx", TWO_SHAPES, indirect=True)
def test_controlled_lockstep_on_the_cluster_form(ctx):
    """Adaptive restart and the ratio stop per weight, decided on the device every iteration, with the one-read cluster pass as
    the gradient: 16 weights, of which some stop early (masked columns of the cluster pass's candidate block) and some run to the
    end, with genuine restarts - preconditions asserted on the oracle's run, every decision fp32-proof."""
    from fastoptsolver_amd import _core, iterative_solvers as its
    _served(ctx)
    d, fos = ctx.d, ctx.fos
    refs = cp.control_references(ctx.name)
    cp.check_control(refs)
    margin = cp.control_margin(refs)
    print(f"controlled {ctx.name}: smallest decision margin {margin:.3e}, iterations {[r['k'] for r in refs]}")
    assert margin >= cp.MIN_CONTROL_MARGIN, margin
    alphas = cp.control_alphas(d)
    want = [(r["k"], r["stopped"]) for r in refs]

    def build(c):
        return c.fos.prepare(c.At, c.b32)

    def run(P):
        return fos.fista_path(P, None, alphas, max_iter=cp.CONTROL_ITERS, L=ctx.L, return_info=True, **cp.CONTROL)
    Pc, Pt = ctx.new(build, True), ctx.new(build, False)
    xc, info_c = run(Pc)
    xt, info_t = run(Pt)
    assert Pc.plan()["cluster"] == 1 and Pt.plan()["cluster"] == 0
    assert info_c == want and info_t == want, (info_c, info_t, want)
    for i, r in enumerate(refs):
        assert _data.rel(_np(xc[i]), _np(xt[i])) < cp.FORMS_TOL, i
        assert _data.rel(_np(xc[i]), r["x"]) < TOL and _data.rel(_np(xt[i]), r["x"]) < TOL, i
    assert_same_bits(run(Pc), (xc, info_c), "a second controlled run on the cluster form")
    # a stopped weight has not moved after a further call: its column of the candidate block is masked
    fam = its._columns(cp.CONTROL_ITERS, False)
    prms = its._path_params(Pc, alphas, ctx.L, fam, 1.0, None, tol=0.0, tol_ratio=cp.CONTROL["tol_ratio"], grad_rule=True,
                            adaptive_restart=True, restart_threshold=cp.CONTROL["restart_threshold"])
    handles = [its._new_state(Pc, prm) for prm in prms]
    assert _core.run_multi(handles, cp.CONTROL_ITERS)
    first = [st.x_tensor().clone() for st in handles]
    assert_same_bits([x.to(xc[0].dtype) for x in first], list(xc), "the handles of the path call")
    assert _core.run_multi(handles, cp.CONTROL_MORE)
    for i, (st, r) in enumerate(zip(handles, refs)):
        s = st.status()
        if r["stopped"]:
            assert (int(s.k), int(s.stopped)) == want[i] and torch.equal(st.x_tensor(), first[i]), i
        else:                                                # ... and the others went on beside the masked columns as the oracle does
            a1, a2 = alphas[i]
            more = cd.run(d["A"], d["b"], a1, a2, ctx.L, cp.CONTROL_ITERS + cp.CONTROL_MORE, **cp.CONTROL)
            assert cd.fp32_proof(more, cp.CONTROL["restart_threshold"], cp.CONTROL["tol_ratio"]), i
            assert (int(s.k), int(s.stopped)) == (more["k"], more["stopped"]) and more["k"] > cp.CONTROL_ITERS, i
            assert _data.rel(_np(st.x_tensor()), more["x"]) < TOL, i


@pytest.mark.parametrize("ctx", TWO_SHAPES, indirect=True)
def test_controlled_resampled_lockstep_on_a_cluster_planned_problem(ctx):
    """Adaptive restart and the ratio stop per column of a resampled run (two 0/1 resamples under 16 weights: two lockstep groups)
    on a cluster-planned handle: the (resample, weight) cells the fp64 reference decides fp32-proof stop where it stops and end
    within 1e-5 of it, the cluster-planned and the two-product problem agree bit for bit, and a plain controlled path (cluster
    form) before and after is the fresh one."""
    _served(ctx)
    fos = ctx.fos
    C, alphas, kept = cp.resample_control_case(ctx.name)
    cp.check_resample_control(kept)
    print(f"controlled resampled {ctx.name}: {len(kept)} of 32 cells, iterations {sorted({r['k'] for r in kept.values()})}")

    def build(c):
        return c.fos.prepare(c.At, c.b32)

    def run(P):
        res = fos.resampled_path(P, alphas, C, cp.CONTROL_ITERS, L=ctx.L, **cp.RESAMPLE_CONTROL)
        return [res.coefs, res.info]

    def plain(P):
        return fos.fista_path(P, None, alphas, max_iter=cp.CONTROL_ITERS, L=ctx.L, return_info=True, **cp.CONTROL)
    Pc, Pt = ctx.new(build, True), ctx.new(build, False)
    plain0 = plain(ctx.new(build, True))
    before = plain(Pc)                                       # leaves the state machines' device-held momentum behind it
    rc, rt = run(Pc), run(Pt)
    assert Pc.plan()["cluster"] == 1 and Pt.plan()["cluster"] == 0
    assert_same_bits(rc, rt, "the two layouts")
    coefs = _np(rc[0])
    for (r, a), ref in sorted(kept.items()):
        assert rc[1][r][a] == (ref["k"], ref["stopped"]), (r, a, rc[1][r][a], ref["k"], ref["stopped"])
        assert _data.rel(coefs[:, r, a], ref["x"]) < TOL, (r, a, _data.rel(coefs[:, r, a], ref["x"]))
    assert_same_bits(before, plain0, "the controlled plain path before")
    assert_same_bits(plain(Pc), plain0, "the controlled plain path after the resampled run")
    assert_same_bits(run(Pc), rc, "the resampled run again")
