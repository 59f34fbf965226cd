"""GPU: the multinomial (softmax) lockstep against its fp64 reference (tests/_multinomial.py).

The link kernel alone (through fos_residual_batch and through one lockstep iteration from a given X0), multinomial_path at every
shape where the launch geometry changes, the compositions with row weights, penalty factors and bounds, the refusals,
multinomial_cv, multinomial_objective and the guard table of tests/_multinomial_guard.py, executed.  The tolerance is the
project's standing 1e-5 relative against the fp64 reference after 30 iterations (mn.TOL / mn.ITERS)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _multinomial as mn, _multinomial_guard as gd

pytestmark = pytest.mark.gpu

UNSUPPORTED, ARG = -4, -1
CLASSES = (2, 3, 5, 7, 16)          # unused tail columns at 3, 5 and 7, one full segment at 16
ROWS = (257, 1003)                  # more than one workgroup of the link kernel; 1003 is no multiple of 4


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


def _dev(A64, kind="f32"):
    t = torch.as_tensor(np.asarray(A64, dtype=np.float32)).cuda()
    return t.to(torch.bfloat16) if kind == "bf16" else t


def _f32(v):
    return mn.as_np(v).astype(np.float32).astype(np.float64)


def _extreme(m, n, C, seed):
    """The recipe with row 0 replaced so that its logits reach +-80 for the X of `_block`: A[0] = 80 e_0, X[0, j] = +-1."""
    A64, y, _ = mn.recipe(m, n, C, seed)
    A = A64.copy()
    A[0] = 0.0
    A[0, 0] = 80.0
    return A, y


def _block(n, nv, seed):
    X = _f32(0.3 * np.random.default_rng(seed).standard_normal((n, nv)))
    X[0] = np.where(np.arange(nv) % 2 == 0, 1.0, -1.0)
    return X


# ---- the link kernel alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("C_", CLASSES)
def test_link_kernel_loss_through_residual_batch(fos, C_, m):
    """out16[s * C] is the cross-entropy sum of segment s (fp64 on the same fp32 X, within the fp32 bound of nll_tolerance), the
    other entries are exactly 0; logits of +-80 in row 0 neither overflow nor lose the row."""
    n = 68
    A, y = _extreme(m, n, C_, 3)
    P = fos.prepare_multinomial(_dev(A), y, classes=C_)
    for nseg in sorted({1, 16 // C_}):
        nv = nseg * C_
        X = _block(n, nv, 10 * C_ + nseg)
        got = P.residual_batch(torch.as_tensor(X).cuda(), use_b=True)
        assert len(got) == nv and np.isfinite(got).all()
        for s in range(nseg):
            Xs = X[:, s * C_:(s + 1) * C_]
            want = mn.nll(A, Xs, y)
            assert np.abs(A @ Xs)[0].max() == 80.0                                       # row 0 is an extreme one
            assert abs(got[s * C_] - want) <= mn.nll_tolerance(A, Xs), (s, got[s * C_], want)
        assert all(got[j] == 0.0 for j in range(nv) if j % C_)


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("C_", CLASSES)
def test_link_kernel_residual_through_one_lockstep_iteration(fos, C_, m):
    """One iteration from a given X0 without penalties moves every class vector by -tau A^T (softmax(A X0) - onehot(y)): the
    residual block the link kernel leaves for product 2, for every segment of the block (each with its own step), the +-80 row
    included."""
    from fastoptsolver_amd import _core
    n = 68
    A, y = _extreme(m, n, C_, 4)
    P = fos.prepare_multinomial(_dev(A), y, classes=C_)
    nseg = 16 // C_
    X0 = _block(n, nseg * C_, 20 + C_)
    taus = [1e-3 / (s + 1) for s in range(nseg)]
    hs = []
    for s in range(nseg):
        for c in range(C_):
            st = _core.Fista(P)
            st.reset(taus[s], 0.0, 0.0, x0=X0[:, s * C_ + c])
            hs.append(st)
    assert _core.run_multi(hs, 1)
    for s in range(nseg):
        X1 = torch.stack([st.x_tensor() for st in hs[s * C_:(s + 1) * C_]], dim=1).cpu().numpy()
        X0s = X0[:, s * C_:(s + 1) * C_]
        G = A.T @ (mn.softmax(A @ X0s) - mn.onehot(y, C_))
        assert mn.rel((X0s - X1) / taus[s], G) <= mn.TOL, (s, mn.rel((X0s - X1) / taus[s], G))


# ---- multinomial_path parity -------------------------------------------------------------------------------------------
# (m, n, C, weights): 257 x 37 is padded to 68 device columns; 33000 rows take the 128-row tile of product 1 (>= 128 rows per CU);
# 70001 rows are more than one row panel of the plan (256 rows per CU): labels of the second panel are read at an offset.
# Every weight count leaves the last lockstep group partial: floor(16 / C) = 5, 3, 4, 2.
PATH_SHAPES = [(1003, 68, 3, 7), (257, 37, 5, 4), (33000, 68, 4, 5), (70001, 68, 7, 3)]


@pytest.mark.parametrize("delta", [None, 3.0], ids=["fista", "delta"])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("shape", PATH_SHAPES, ids=lambda s: "%dx%d-C%d" % s[:3])
def test_path_matches_the_reference(fos, shape, kind, delta):
    m, n, C_, count = shape
    A64, y, L = mn.recipe(m, n, C_, 3, kind)
    alphas = mn.weights(A64, y, C_, count)
    assert len(alphas) == count and count % (16 // C_) != 0
    xs, info = fos.multinomial_path(_dev(A64, kind), y, alphas, classes=C_, max_iter=mn.ITERS, delta=delta, L=L, return_info=True)
    assert len(xs) == count and info == [(mn.ITERS, 0)] * count
    for (a1, a2), X in zip(alphas, xs):
        ref = mn.reference(m, n, C_, 3, kind, a1, a2, delta)
        assert X.shape == (n, C_) and np.abs(ref).max() > 0
        assert mn.rel(X, ref) <= mn.TOL, (a1, a2, mn.rel(X, ref))


def test_default_step_is_boehnings_bound(fos):
    """L = None: estimate_lipschitz(handle) / 2, one draw from the global NumPy stream; lambda_max(A^T W A) / 2 on a weighted
    handle (not the quarter of the weighted logistic loss)."""
    m, n, C_ = 1003, 68, 3
    A64, y, _ = mn.recipe(m, n, C_, 3)
    w = _f32(np.random.default_rng(5).uniform(0.25, 3.0, size=m))
    a = mn.weights(A64, y, C_, 1)
    for P, ww in ((fos.prepare(_dev(A64), y, loss="multinomial"), None),
                  (fos.prepare_weighted(_dev(A64), y, w, loss="multinomial"), w)):
        assert P.classes == C_ and P.loss == "multinomial"
        np.random.seed(11)
        Ld = fos.estimate_lipschitz(P)
        lam = float(np.linalg.eigvalsh(A64.T @ ((np.ones(m) if ww is None else ww)[:, None] * A64))[-1])
        assert 0.9 * lam <= Ld <= (1 + 1e-5) * lam           # the power iteration approaches lambda_max from below
        np.random.seed(11)
        X = fos.multinomial_path(P, None, a, max_iter=mn.ITERS)[0]
        ref = mn.run(A64, y, C_, a[0][0], a[0][1], Ld / 2.0, w=ww)
        assert mn.rel(X, ref) <= mn.TOL, mn.rel(X, ref)


# ---- composition -------------------------------------------------------------------------------------------------------
def test_zero_one_weights_are_the_fit_on_the_kept_rows(fos):
    m, n, C_ = 1003, 68, 3
    A64, y, L = mn.recipe(m, n, C_, 3)
    keep = np.random.default_rng(2).random(m) < 0.7
    alphas = mn.weights(A64, y, C_, 2)
    P = fos.prepare_weighted(_dev(A64), y, keep.astype(np.float64), loss="multinomial")
    xs = fos.multinomial_path(P, None, alphas, max_iter=mn.ITERS, L=L)
    for (a1, a2), X in zip(alphas, xs):
        ref = mn.run(A64[keep], y[keep], C_, a1, a2, L)
        assert mn.rel(X, ref) <= mn.TOL, mn.rel(X, ref)


def test_fractional_weights_match_the_weighted_reference(fos):
    m, n, C_ = 1003, 68, 5
    A64, y, _ = mn.recipe(m, n, C_, 6)
    w = _f32(np.random.default_rng(8).uniform(0.0, 2.5, size=m))
    L = mn.lipschitz(A64, 6, w)
    alphas = mn.weights(A64, y, C_, 4)                     # two groups: 3 + 1
    P = fos.prepare_multinomial(_dev(A64), y, classes=C_, sample_weight=w)
    xs = fos.multinomial_path(P, None, alphas, max_iter=mn.ITERS, L=L, delta=3.0)
    for (a1, a2), X in zip(alphas, xs):
        ref = mn.run(A64, y, C_, a1, a2, L, w=w, delta=3.0)
        assert mn.rel(X, ref) <= mn.TOL, mn.rel(X, ref)
    # and the weighted objective
    got = fos.multinomial_objective(xs[0], P, None, *alphas[0])
    want = mn.objective(A64, _f32(xs[0]), y, *alphas[0], w=w)
    assert abs(got - want) <= float(w.max()) * mn.nll_tolerance(A64, _f32(xs[0])) + 1e-12 * abs(want)      # every term times w_i <= max w


def test_an_unpenalised_constant_column_is_a_per_class_intercept(fos):
    m, n, C_ = 1003, 67, 3
    A64, y, _ = mn.recipe(m, n, C_, 9)
    y = np.where(np.arange(m) % 4 == 0, 0.0, y)            # unbalanced classes: the intercepts matter
    A1 = np.concatenate([A64, np.ones((m, 1))], axis=1)
    L = mn.lipschitz(A1, 9)
    p = np.r_[np.ones(n), 0.0]
    alphas = mn.weights(A1[:, :n], y, C_, 2)
    P = fos.prepare_penalized(_dev(A1), y, penalty_factor=p, loss="multinomial")
    assert P.classes == C_ and P.penalty_max == 1.0
    xs = fos.multinomial_path(P, None, alphas, max_iter=mn.ITERS, L=L)
    for (a1, a2), X in zip(alphas, xs):
        ref = mn.run(A1, y, C_, a1, a2, L, p=p)
        shrunk = mn.run(A1, y, C_, a1, a2, L)
        assert np.abs(ref[n]).min() > 0 and mn.rel(ref[n], shrunk[n]) > 100 * mn.TOL      # the factor changes the model
        assert mn.rel(X, ref) <= mn.TOL, mn.rel(X, ref)
        got = fos.multinomial_objective(X, P, None, a1, a2)
        want = mn.objective(A1, _f32(X), y, a1, a2, p=p)
        assert abs(got - want) <= mn.nll_tolerance(A1, _f32(X)) + 1e-12 * abs(want)


def test_a_non_negativity_bound(fos):
    m, n, C_ = 1003, 68, 3
    A64, y, L = mn.recipe(m, n, C_, 3)
    a1, a2 = mn.weights(A64, y, C_, 3)[2]
    free = mn.reference(m, n, C_, 3, "f32", a1, a2)
    ref = mn.run(A64, y, C_, a1, a2, L, lo=0.0)
    assert (free < 0).sum() >= 5 and (ref >= 0).all() and (ref > 0).sum() >= 5      # the bound binds on the reference
    P = fos.prepare_multinomial(_dev(A64), y, classes=C_, lower=0.0)
    X = fos.multinomial_path(P, None, [(a1, a2)], max_iter=mn.ITERS, L=L)[0]
    assert (mn.as_np(X) >= 0).all() and mn.rel(X, ref) <= mn.TOL, mn.rel(X, ref)


def test_controlled_and_mixed_groups_are_refused_and_the_handles_stay_usable(fos):
    from fastoptsolver_amd import _core, _lib
    m, n, C_ = 257, 68, 3
    A64, y, L = mn.recipe(m, n, C_, 3)
    (a1, a2), (b1, b2) = mn.weights(A64, y, C_, 2)
    P = fos.prepare(_dev(A64), y, loss="multinomial")
    hs = [_core.Fista(P) for _ in range(2 * C_)]
    ids = _core.fold_ids_tensor(np.arange(m) % 2, P.device)

    def reset(**over):
        for i, st in enumerate(hs):
            q1, q2 = (a1, a2) if i < C_ else (b1, b2)
            st.reset(1.0 / (L + q2), q1, q2, **(over if i == 1 else {}))

    def refused(call):
        assert call() is False
        msg = P.lib.fos_last_error().decode()
        assert all(int(st.status().k) == 0 for st in hs), msg
        return msg

    for over in (dict(tol_ratio=0.1), dict(adaptive_restart=True), dict(tol_step=1e-9)):
        reset(**over)
        assert "plain runs only" in refused(lambda: _core.run_multi(hs, 3))
        assert "plain runs only" in refused(lambda: _core.run_multi_folds(hs, ids, [0] * C_ + [1] * C_, 3))
    reset(tol_grad=1e-3)
    refused(lambda: _core.run_multi(hs, 3))
    reset()
    hs[1].reset(1.0 / (L + a2), 0.5 * a1, a2)                          # a class group with two penalties
    assert "identical" in refused(lambda: _core.run_multi(hs, 3))
    reset()
    assert "one fold" in refused(lambda: _core.run_multi_folds(hs, ids, [0, 0, 1, 1, 1, 1], 3))
    # nv that is no multiple of C: the library's own refusal (the Python wrapper checks before it calls)
    arr = (C.c_void_p * 4)(*[st.h for st in hs[:4]])
    with P.ctx():
        assert P.lib.fos_fista_run_multi(arr, 4, 3) == UNSUPPORTED and "multiple of the classes" in P.lib.fos_last_error().decode()
    X16 = torch.zeros(P.n_dev, 16, device=P.device)
    with P.ctx():
        assert P.lib.fos_residual_batch(P.h, _core.ptr(X16), 4, 1, _core.ptr(P.scratch)) == ARG
        assert P.lib.fos_residual_batch_folds(P.h, _core.ptr(X16), 6, _core.ptr(ids), (C.c_int32 * 6)(0, 0, 1, 1, 1, 1),
                                              _core.ptr(P.scratch)) == ARG
    # the handles are as they were: the plain run is the reference's
    assert _core.run_multi(hs, mn.ITERS)
    for g, (q1, q2) in enumerate(((a1, a2), (b1, b2))):
        X = torch.stack([st.x_tensor() for st in hs[g * C_:(g + 1) * C_]], dim=1).cpu().numpy()
        assert mn.rel(X, mn.reference(m, n, C_, 3, "f32", q1, q2)) <= mn.TOL
    assert _lib.LOSS_MULTINOMIAL == 2


# ---- cross-validation --------------------------------------------------------------------------------------------------
def _cv_reference(A64, y, C_, alphas, ids, K, L, w=None):
    coefs = np.zeros((A64.shape[1], C_, K, len(alphas)))
    score = np.zeros((K, len(alphas)))
    ww = np.ones(A64.shape[0]) if w is None else w
    for f in range(K):
        tr = ids != f
        for a, (a1, a2) in enumerate(alphas):
            coefs[:, :, f, a] = mn.run(A64[tr], y[tr], C_, a1, a2, L, w=None if w is None else w[tr])
            score[f, a] = mn.nll(A64[~tr], coefs[:, :, f, a], y[~tr], ww[~tr]) / ww[~tr].sum()
    return coefs, score


@pytest.mark.parametrize("case", ["int_folds", "fold_ids_weighted"])
def test_cv(fos, case):
    """coefs[:, :, f, a] is multinomial_path on the training rows with the same L, the held-out score is the fp64 mean
    cross-entropy of those coefficients, best is the reference's argmin (on a grid whose reference scores are further apart than
    the tolerance could move them).  K = 4 does not divide m = 1003; 12 (fold, weight) pairs of C = 3 are three groups, 5 + 5 + 2."""
    from fastoptsolver_amd import iterative_solvers as its
    m, n, C_ = 1003, 68, 3
    A64, y, L = mn.recipe(m, n, C_, 3)
    alphas = mn.weights(A64, y, C_, 3)
    if case == "int_folds":
        folds, w = 4, None
        ids = its._cv_folds(4, m)[0].astype(np.int64)
        K = 4
        P = fos.prepare(_dev(A64), y, loss="multinomial")
    else:
        K = 3
        ids = np.random.default_rng(4).integers(0, K, size=m)
        folds = ids
        w = _f32(np.random.default_rng(5).uniform(0.2, 2.0, size=m))
        L = mn.lipschitz(A64, 3, w)
        P = fos.prepare_weighted(_dev(A64), y, w, loss="multinomial")
    ref_coefs, ref_score = _cv_reference(A64, y, C_, alphas, ids, K, L, w)
    ref_mean = ref_score.mean(axis=0)
    gaps = np.abs(np.subtract.outer(ref_mean, ref_mean))[~np.eye(len(alphas), dtype=bool)]
    assert gaps.min() > 1e3 * mn.TOL * ref_mean.max()               # the grid separates the scores: best is decidable
    res = fos.multinomial_cv(P, None, alphas, folds=folds, max_iter=mn.ITERS, L=L, return_coefs=True)
    assert res.coefs.shape == (n, C_, K, len(alphas)) and res.logloss.shape == (K, len(alphas)) and res.x.shape == (n, C_)
    ww = np.ones(m) if w is None else w
    for f in range(K):
        held = ids == f
        for a in range(len(alphas)):
            assert mn.rel(res.coefs[:, :, f, a], ref_coefs[:, :, f, a]) <= mn.TOL, (f, a)
            Xd = _f32(res.coefs[:, :, f, a])
            want = mn.nll(A64[held], Xd, y[held], ww[held]) / ww[held].sum()
            bound = float(ww[held].max()) * mn.nll_tolerance(A64[held], Xd) / ww[held].sum()
            assert abs(res.logloss[f, a] - want) <= bound + 1e-12, (f, a, res.logloss[f, a], want)
            assert res.info[f][a] == (mn.ITERS, 0)
    assert np.allclose(res.mean_logloss, res.logloss.mean(axis=0), rtol=0, atol=1e-15)
    assert res.best == int(np.argmin(ref_mean))
    full = mn.run(A64, y, C_, *alphas[res.best], L, w=w)
    assert mn.rel(res.x, full) <= mn.TOL


# ---- objective ---------------------------------------------------------------------------------------------------------
def test_objective_for_one_and_for_several(fos):
    m, n, C_ = 1003, 68, 3
    A64, y, _ = mn.recipe(m, n, C_, 3)
    P = fos.prepare(_dev(A64), y, loss="multinomial")
    Xs = _f32(0.2 * np.random.default_rng(1).standard_normal((n, C_, 7)))        # 7 members: two passes, 5 + 2
    got = fos.multinomial_objective(Xs, P, None, 0.3, 0.7)
    assert got.shape == (7,) and got.dtype == np.float64
    for k in range(7):
        want = mn.objective(A64, Xs[:, :, k], y, 0.3, 0.7)
        assert abs(got[k] - want) <= mn.nll_tolerance(A64, Xs[:, :, k]) + 1e-12 * abs(want), (k, got[k], want)
    one = fos.multinomial_objective(torch.as_tensor(Xs[:, :, 3]), _dev(A64), y, 0.3, 0.7)
    assert isinstance(one, float) and one == got[3]
    with pytest.raises(ValueError):
        fos.multinomial_objective(Xs[:, :2, 0], P, None, 0.3, 0.7)


# ---- more rows than one row panel ----------------------------------------------------------------------------------------
# 70001 rows are two row panels of the plan (256 rows per CU: the boundary is at row 65536 on 256 CUs).  Labels, weights and fold
# ids are random per row, so a panel that read any of them without its row offset would fit and score other rows' data.
BIG = (70001, 68, 3, 3)              # m, n, C, seed


def _big_weights():
    return _f32(np.random.default_rng(12).uniform(0.0, 2.5, size=BIG[0]))


def test_two_panels_weighted_fit_and_weighted_objective(fos):
    m, n, C_, seed = BIG
    A64, y, _ = mn.recipe(m, n, C_, seed)
    w = _big_weights()
    assert w[65536:].std() > 0.5 and not np.array_equal(w[:m - 65536], w[65536:])
    L = mn.lipschitz(A64, seed, w)
    alphas = mn.weights(A64, y, C_, 2)
    P = fos.prepare_weighted(_dev(A64), y, w, loss="multinomial")
    xs = fos.multinomial_path(P, None, alphas, max_iter=mn.ITERS, L=L)
    for (a1, a2), X in zip(alphas, xs):
        ref = mn.run(A64, y, C_, a1, a2, L, w=w)
        assert np.abs(ref).max() > 0 and mn.rel(X, ref) <= mn.TOL, mn.rel(X, ref)
        got = fos.multinomial_objective(X, P, None, a1, a2)
        want = mn.objective(A64, _f32(X), y, a1, a2, w=w)
        assert abs(got - want) <= float(w.max()) * mn.nll_tolerance(A64, _f32(X)) + 1e-12 * abs(want), (got, want)


def test_two_panels_cross_validation_with_folds_across_the_boundary(fos):
    """run_multi_folds (FOLD_TRAIN) and residual_batch_folds (FOLD_HELD, the partials of both panels folded) on a weighted handle:
    every fold has rows in both panels."""
    m, n, C_, seed = BIG
    A64, y, _ = mn.recipe(m, n, C_, seed)
    w = _big_weights()
    K = 3
    ids = np.random.default_rng(13).integers(0, K, size=m)
    assert all(((ids[:65536] == f).any() and (ids[65536:] == f).any()) for f in range(K))
    L = mn.lipschitz(A64, seed, w)
    alphas = mn.weights(A64, y, C_, 1)
    P = fos.prepare_weighted(_dev(A64), y, w, loss="multinomial")
    ref_coefs, _ = _cv_reference(A64, y, C_, alphas, ids, K, L, w)
    res = fos.multinomial_cv(P, None, alphas, folds=ids, max_iter=mn.ITERS, L=L, refit=False, return_coefs=True)
    assert res.x is None and res.coefs.shape == (n, C_, K, 1)
    for f in range(K):
        held = ids == f
        assert mn.rel(res.coefs[:, :, f, 0], ref_coefs[:, :, f, 0]) <= mn.TOL, f
        Xd = _f32(res.coefs[:, :, f, 0])
        want = mn.nll(A64[held], Xd, y[held], w[held]) / w[held].sum()
        bound = float(w[held].max()) * mn.nll_tolerance(A64[held], Xd) / w[held].sum()
        assert abs(res.logloss[f, 0] - want) <= bound + 1e-12, (f, res.logloss[f, 0], want)


def test_two_panels_objective_for_several(fos):
    """fos_residual_batch on two panels: the loss sums of both panels' workgroups fold into out16[s * C]; 7 members are two
    passes (5 + 2)."""
    m, n, C_, seed = BIG
    A64, y, _ = mn.recipe(m, n, C_, seed)
    P = fos.prepare(_dev(A64), y, loss="multinomial")
    Xs = _f32(0.2 * np.random.default_rng(14).standard_normal((n, C_, 7)))
    got = fos.multinomial_objective(Xs, P, None, 0.3, 0.7)
    for k in range(7):
        want = mn.objective(A64, Xs[:, :, k], y, 0.3, 0.7)
        # the last rows alone carry far more than the tolerance: a second panel that was dropped or misread would show
        assert mn.nll(A64[65536:], Xs[:, :, k], y[65536:]) > 100 * mn.nll_tolerance(A64, Xs[:, :, k])
        assert abs(got[k] - want) <= mn.nll_tolerance(A64, Xs[:, :, k]) + 1e-12 * abs(want), (k, got[k], want)


# ---- the guard table, executed ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup(fos):
    """A multinomial problem with one class group of handles that has run five lockstep iterations."""
    from fastoptsolver_amd import _core
    A64, y, L = mn.recipe(1003, 200, 3, 9)
    a1, a2 = mn.weights(A64, y, 3, 1)[0]
    P = fos.prepare(_dev(A64), y, loss="multinomial")
    hs = []
    for _ in range(3):
        st = _core.Fista(P)
        st.reset(1.0 / (L + a2), a1, a2)
        hs.append(st)
    assert _core.run_multi(hs, 5)
    return P, hs


def _snapshot(hs):
    out = []
    for st in hs:
        s = st.status()
        out.append((st.x_tensor().clone(), tuple(getattr(s, k) for k, _ in s._fields_)))
    return out


def _refusing_calls(P, hs):
    """name -> a call with valid arguments that returns the library's code (a wrapper that raises gives the code in its FosError,
    one that answers None / False stands for FOS_ERR_UNSUPPORTED)."""
    from fastoptsolver_amd import _core, _lib
    lib, st, dev = P.lib, hs[0], P.device
    n, m = P.n_dev, P.m
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)        # noqa: E731
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)        # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)          # noqa: E731
    ptr = _core.ptr
    keep = dict(x=f32(n), xd=f64(n + 4), g=f32(n + 4), gd=f64(n + 4), X16=f32(n, 16), XD=f64(16, n), GD=f64(16, n), B=f32(m, 3),
                rr=f64(16), S=f64(10, n), Y=f64(10, n), work=f64(4096), xh=f64(8, n), h4=f64(8, 4), ls=i32(8), taus=f64(8))
    done, tau = C.c_int32(0), C.c_double(0.0)
    res, res16 = _lib.LbfgsResult(), (_lib.LbfgsResult * 16)()
    nrounds = C.c_int(0)

    def raised(fn):
        def call():
            try:
                fn()
            except _lib.FosError as e:
                assert "code -4" in str(e) and "multinomial" in str(e), str(e)
                return UNSUPPORTED
            return 0
        return call

    def unserved(fn):
        return lambda: UNSUPPORTED if fn() in (None, False) else 0

    def raw(fn):
        def call():
            with P.ctx():
                return fn()
        return call

    return keep, {
        "fos_problem_set_comm": raised(lambda: P.set_comm(None)),
        "fos_problem_set_comm_cols": raw(lambda: lib.fos_problem_set_comm_cols(P.h, C.c_void_p(0x1000))),   # never dereferenced
        "fos_gemv_pair": raised(lambda: P.gemv_pair(keep["x"])),
        "fos_gemv_pair_f64": raw(lambda: lib.fos_gemv_pair_f64(P.h, ptr(keep["xd"]), 0.0, ptr(keep["g"]), None)),
        "fos_gemv_pair_dd": raw(lambda: lib.fos_gemv_pair_dd(P.h, ptr(keep["xd"]), 0.0, ptr(keep["gd"]))),
        "fos_gemv_pair_dd_multi": raw(lambda: lib.fos_gemv_pair_dd_multi(P.h, ptr(keep["XD"]), 3, n, ptr(keep["B"]), 3, 0.0,
                                                                         ptr(keep["GD"]), ptr(keep["rr"]))),
        "fos_residual_objective": raised(lambda: P.residual_objective(keep["x"])),
        "fos_residual_batch_rhs": unserved(lambda: P.residual_batch_rhs(keep["X16"][:, :3], keep["B"])),
        "fos_fista_run_multi_rhs": unserved(lambda: _core.run_multi_rhs(hs, keep["B"], 3)),
        "fos_fista_run": raised(lambda: st.run(3)),
        "fos_fista_run_history": unserved(lambda: st.run_history(3)),
        "fos_fista_run_resident": raw(lambda: lib.fos_fista_run_resident(st.h, 3, 0, 0.5, 1e-2, 0.0, ptr(keep["xh"]), ptr(keep["h4"]),
                                                                         ptr(keep["ls"]), ptr(keep["taus"]), C.byref(done),
                                                                         C.byref(tau))),
        "fos_fista_run_fused": unserved(lambda: st.run_fused(3)),
        "fos_fista_run_chip": unserved(lambda: st.run_chip(3)),
        "fos_fista_grad": raised(lambda: st.grad()),
        "fos_fista_grad_dual": raised(lambda: st.grad(dual=True)),
        "fos_fista_update": raised(lambda: st.update()),
        "fos_fista_trial": raised(lambda: st.trial(0.1)),
        "fos_fista_trial_batch": unserved(lambda: st.trial_batch(0.1, 0.5)),
        "fos_fista_run_backtracking": unserved(lambda: st.run_backtracking(3, 0.5, 1e-2, 1e-6)),
        "fos_fista_run_recorded": unserved(lambda: st.run_recorded(3, False, 0.5, 1e-2, 1e-6)),
        "fos_fista_resume_after_stall": raised(lambda: st.resume_after_stall()),
        "fos_lbfgs_direction_cols": raw(lambda: lib.fos_lbfgs_direction_cols(P.h, ptr(keep["gd"]), ptr(keep["S"]), ptr(keep["Y"]), 0, 0,
                                                                             10, ptr(keep["xd"]), ptr(keep["rr"]), ptr(keep["work"]),
                                                                             4096)),
        "fos_lbfgs_minimize": raw(lambda: lib.fos_lbfgs_minimize(P.h, 1.0, 3, 1e-6, ptr(keep["xd"]), None, None, None, 0,
                                                                 C.byref(res))),
        "fos_lbfgs_minimize_multi": raw(lambda: lib.fos_lbfgs_minimize_multi(P.h, 3, ptr(keep["B"]), 3, 1.0, 3, 1e-6, ptr(keep["XD"]), n,
                                                                             None, None, 0, C.byref(nrounds), res16)),
    }


def test_every_refusing_entry_point_refuses_and_changes_nothing(fos, setup):
    from fastoptsolver_amd import _core
    P, hs = setup
    before = _snapshot(hs)
    keep, calls = _refusing_calls(P, hs)
    assert set(calls) == gd.REFUSES, set(calls) ^ gd.REFUSES
    for name in sorted(calls):
        rc = calls[name]()
        msg = P.lib.fos_last_error().decode()
        assert rc == UNSUPPORTED, (name, rc, msg)
        assert name in msg and "multinomial problem" in msg and "logistic problem" not in msg, (name, msg)
    # fos_residual_batch serves use_b = 1 and refuses use_b = 0
    with pytest.raises(fos.FosError, match="code -4"):
        P.residual_batch(keep["X16"][:, :3], use_b=False)
    assert len(P.residual_batch(keep["X16"][:, :3], use_b=True)) == 3
    torch.cuda.synchronize()
    for (x0, s0), (x1, s1) in zip(before, _snapshot(hs)):
        assert torch.equal(x0, x1) and s0 == s1, (s0, s1)
    assert _core.run_multi(hs, 2) and all(int(st.status().k) == 7 for st in hs)


def test_serving_and_loss_free_entry_points_and_the_public_refusals(fos, setup):
    from fastoptsolver_amd import _lib
    P, _ = setup
    out = C.c_int(-1)
    assert P.lib.fos_problem_get_loss(P.h, C.byref(out)) == 0 and out.value == _lib.LOSS_MULTINOMIAL
    assert P.lib.fos_problem_get_classes(C.byref(out), P.h) == 0 and out.value == 3 == P.classes
    # loss-free entry points keep working
    assert P.power_iter(np.ones(P.n))[0] > 0 and P.plan()["cus"] > 0
    assert P.gram_apply(torch.ones(P.n, 2, device=P.device)).shape == (P.n, 2)
    # a problem without b, or on the LDS-resident plan, cannot become multinomial; the loss can be left again
    bare = fos.prepare(P.A)
    assert P.lib.fos_problem_set_multinomial(3, bare.h) == UNSUPPORTED
    small = fos.prepare(torch.zeros(100, 4, device="cuda"), torch.zeros(100))
    assert P.lib.fos_problem_set_multinomial(3, small.h) == UNSUPPORTED
    assert P.lib.fos_problem_get_loss(small.h, C.byref(out)) == 0 and out.value == _lib.LOSS_SQUARED
    assert P.lib.fos_problem_get_classes(C.byref(out), small.h) == 0 and out.value == 0
    other = fos.prepare(P.A, P.b, loss="multinomial")
    assert P.lib.fos_problem_set_loss(other.h, _lib.LOSS_SQUARED) == 0
    assert P.lib.fos_problem_get_classes(C.byref(out), other.h) == 0 and out.value == 0
    # the other front ends refuse the handle, each way round
    for call in (lambda: fos.fista(P, None, "lasso", 0.1, 0.0, max_iter=3, L=1.0),
                 lambda: fos.fista_delta(P, None, "lasso", 0.1, 0.0, 3.0, max_iter=3, L=1.0),
                 lambda: fos.fista_path(P, None, [(0.1, 0.0)] * 3, max_iter=3, L=1.0),
                 lambda: fos.fista_cv(P, None, [(0.1, 0.0)], folds=2, max_iter=3, L=1.0),
                 lambda: fos.logistic_path(P, None, [(0.1, 0.0)], max_iter=3, L=1.0),
                 lambda: fos.logistic_cv(P, None, [(0.1, 0.0)], folds=2, max_iter=3, L=1.0),
                 lambda: fos.logistic_objective(np.zeros(P.n), P, None, 0.1, 0.0)):
        with pytest.raises(ValueError, match="multinomial"):
            call()
    with pytest.raises(fos.FosError, match="multinomial"):
        fos.LBFGSSolver("ridge", 0.0, 1.0, max_iter=3).fit(P, None)
    logit = fos.prepare(P.A, (P.b > 0).float(), loss="logistic")
    with pytest.raises(ValueError, match="logistic"):
        fos.multinomial_path(logit, None, [(0.1, 0.0)], max_iter=3, L=1.0)
    with pytest.raises(ValueError, match="3 classes"):
        fos.multinomial_path(P, None, [(0.1, 0.0)], classes=4, max_iter=3, L=1.0)
