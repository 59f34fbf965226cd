"""GPU: the group penalty across lockstep columns (fos_fista_params.group; csrc/reduce_update.hpp fista_update_group_kernel)
against its fp64 reference (tests/_group.py).

Grouped multinomial and multi-task fits at the shapes of tests/_menu_coord.shapes where the update's launch geometry changes,
for both prox kinds, FISTA and FISTA-delta, fp32 and bf16 A; the compositions with row weights, penalty factors and fold masks;
the defaults, bit for bit; and the refusals.  The tolerance is the project's standing 1e-5 relative against the fp64 reference
after 30 iterations (gp.TOL / gp.ITERS).  Every reference row that is zero by a margin is exactly 0.0 in every device column."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _data, _group as gp, _multinomial as mn

pytestmark = pytest.mark.gpu

UNSUPPORTED = -4
KINDS = ("f32", "bf16")


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


@pytest.fixture(scope="module")
def cus(fos):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _dev(A64, kind="f32"):
    t = torch.as_tensor(np.asarray(A64, dtype=np.float32)).cuda()
    return t.to(torch.bfloat16) if kind == "bf16" else t


def _f32(v):
    return mn.as_np(v).astype(np.float32).astype(np.float64)


def _direct(P, G, sets, iters=gp.ITERS, *, B=None, group=None, enet=False, delta=None):
    """The fits of `sets` = [(tau, alpha1, alpha2), ...] as handles built through _core, G columns each, floor(16 / G) per
    lockstep call: [X (n x G float64 ndarray), ...].  B: the targets (m x G device tensor) of fos_fista_run_multi_rhs."""
    from fastoptsolver_amd import _core, _lib, multitask
    per, out = 16 // G, []
    for first in range(0, len(sets), per):
        part = sets[first:first + per]
        hs = []
        for tau, a1, a2 in part:
            for _ in range(G):
                st = _core.Fista(P)
                st.reset(tau, a1, a2, mode=_lib.MODE_FISTA if delta is None else _lib.MODE_DELTA, delta=delta or 0.0,
                         prox_kind=_lib.PROX_ENET if enet else _lib.PROX_L1, group=G if group is None else group)
                hs.append(st)
        if B is not None:
            assert _core.run_multi_rhs(hs, multitask.tile_targets(B, len(part)), iters), P.lib.fos_last_error().decode()
        else:
            assert _core.run_multi(hs, iters), P.lib.fos_last_error().decode()
        for i in range(len(part)):
            out.append(torch.stack([st.x_tensor() for st in hs[i * G:(i + 1) * G]], dim=1).cpu().numpy())
            assert all(int(st.status().k) == iters for st in hs[i * G:(i + 1) * G])
    return out


def _check(X, ref, safe, what):
    X = mn.as_np(X)
    assert X.shape == ref.shape and np.abs(ref).max() > 0
    r = mn.rel(X, ref)
    print(what, "rel", r, "safe zero rows", int(safe.sum()))
    assert r <= gp.TOL, (what, r)
    assert np.array_equal(X[safe], np.zeros_like(X[safe])), (what, "a row below the threshold is not exactly zero")


# ---- grouped multinomial against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(gp.VARIANTS))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", gp.MULTINOMIAL_CASES, ids=lambda c: "%s-C%d-x%d" % c)
def test_grouped_multinomial_matches_the_reference(fos, cus, case, kind, variant):
    name, C_, count = case
    enet, delta = gp.VARIANTS[variant]
    m, n = gp.case_shape(name, kind, cus)
    A64, y, L = mn.recipe(m, n, C_, gp.SEED, kind)
    alphas = gp.multinomial_weights(A64, y, C_, count, enet=enet)
    assert count == 1 or C_ > 8 or count % (16 // C_) != 0   # the last lockstep group is partial (C > 8: one fit per call)
    P = fos.prepare_multinomial(_dev(A64, kind), y, classes=C_, grouped=True)
    if enet:
        xs = _direct(P, C_, [(1.0 / (L + a2), a1, a2) for a1, a2 in alphas], enet=True, delta=delta)
    else:
        xs, info = fos.multinomial_path(P, None, alphas, max_iter=gp.ITERS, delta=delta, L=L, return_info=True)
        assert info == [(gp.ITERS, 0)] * count
    for (a1, a2), X in zip(alphas, xs):
        ref, safe = gp.multinomial_reference(m, n, C_, gp.SEED, kind, a1, a2, delta, enet)
        _check(X, ref, safe, (case, kind, variant, a1))


# ---- composition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_tile", "edges"])
def test_grouped_with_row_weights(fos, cus, name):
    m, n = gp.case_shape(name, "f32", cus)
    C_ = 3
    A64, y, _ = mn.recipe(m, n, C_, 6)
    w = _f32(np.random.default_rng(8).uniform(0.0, 2.5, size=m))
    L = mn.lipschitz(A64, 6, w)
    alphas = gp.multinomial_weights(A64, y, C_, 2, w=w)
    P = fos.prepare_multinomial(_dev(A64), y, classes=C_, sample_weight=w, grouped=True)
    xs = fos.multinomial_path(P, None, alphas, max_iter=gp.ITERS, L=L)
    for (a1, a2), X in zip(alphas, xs):
        ref, prob = gp.iterate(gp.GroupMultinomial(A64, y, C_, a1, a2, w=w), L)
        gp.check_recipe(ref, mn.run(A64, y, C_, a1, a2, L, w=w))
        _check(X, ref, gp.safe_zero_rows(prob, ref), (name, "weights", a1))
    got = fos.multinomial_objective(xs[0], P, None, *alphas[0])
    X0 = _f32(xs[0])
    want = mn.nll(A64, X0, y, w) + gp.penalty(X0, *alphas[0])
    assert abs(got - want) <= float(w.max()) * mn.nll_tolerance(A64, X0) + 1e-12 * abs(want)


@pytest.mark.parametrize("name", ["one_tile", "edges"])
def test_grouped_with_penalty_factors_and_an_unpenalised_intercept(fos, cus, name):
    m, n = gp.case_shape(name, "f32", cus)
    C_ = 3
    A64, y, _ = mn.recipe(m, n - 1, C_, 9)
    y = np.where(np.arange(m) % 4 == 0, 0.0, y)            # unbalanced classes: the intercepts matter
    A1 = np.concatenate([A64, np.ones((m, 1))], axis=1)    # the intercept is the last column: the last quad of the last workgroup
    L = mn.lipschitz(A1, 9)
    p = np.r_[_f32(np.random.default_rng(2).uniform(0.5, 2.0, size=n - 1)), 0.0]
    alphas = gp.multinomial_weights(A1[:, :n - 1], y, C_, 2)
    P = fos.prepare_penalized(_dev(A1), y, penalty_factor=p, loss="multinomial")
    P.set_grouped()
    xs = fos.multinomial_path(P, None, alphas, max_iter=gp.ITERS, L=L)
    for (a1, a2), X in zip(alphas, xs):
        ref, prob = gp.iterate(gp.GroupMultinomial(A1, y, C_, a1, a2, p=p), L)
        plain, _ = gp.iterate(gp.GroupMultinomial(A1, y, C_, a1, a2), L)
        gp.check_recipe(ref, mn.run(A1, y, C_, a1, a2, L, p=p))
        assert np.abs(ref[n - 1]).min() > 0 and mn.rel(ref, plain) > 100 * gp.TOL      # the factors change the model
        _check(X, ref, gp.safe_zero_rows(prob, ref), (name, "factors", a1))
        assert np.abs(mn.as_np(X)[n - 1]).min() > 0                                    # the intercept row stays unpenalised
        got = fos.multinomial_objective(X, P, None, a1, a2)
        Xd = _f32(X)
        want = mn.nll(A1, Xd, y) + gp.penalty(Xd, a1, a2, p)
        assert abs(got - want) <= mn.nll_tolerance(A1, Xd) + 1e-12 * abs(want)


@pytest.mark.parametrize("name", ["one_tile", "edges"])
def test_grouped_cv(fos, cus, name):
    """On a grouped handle coefs[:, :, f, a] is multinomial_path on the gathered training rows; logloss the reference's held-out mean."""
    from tests import _menu_cv
    case = _menu_cv.shapes("f32", cus)[name]
    m, n, C_ = case["m"], case["n"], 3
    A64, y, L = mn.recipe(m, n, C_, gp.SEED)
    ids = _menu_cv.fold_ids(case)
    K = int(ids.max()) + 1
    alphas = gp.multinomial_weights(A64, y, C_, 2)
    P = fos.prepare_multinomial(_dev(A64), y, classes=C_, grouped=True)
    res = fos.multinomial_cv(P, None, alphas, folds=ids, max_iter=gp.ITERS, L=L, return_coefs=True)
    assert res.coefs.shape == (n, C_, K, len(alphas)) and res.x.shape == (n, C_)
    some_zero = False
    for f in range(K):
        tr = ids != f
        for a, (a1, a2) in enumerate(alphas):
            ref, prob = gp.iterate(gp.GroupMultinomial(A64[tr], y[tr], C_, a1, a2), L)
            safe = gp.safe_zero_rows(prob, ref)
            some_zero = some_zero or bool(safe.any())
            _check(res.coefs[:, :, f, a], ref, safe, (name, "cv", f, a))
            Xd = _f32(res.coefs[:, :, f, a])
            want = mn.nll(A64[~tr], Xd, y[~tr]) / (~tr).sum()
            assert abs(res.logloss[f, a] - want) <= mn.nll_tolerance(A64[~tr], Xd) / (~tr).sum() + 1e-12, (f, a)
            assert res.info[f][a] == (gp.ITERS, 0)
    assert some_zero
    full, _ = gp.iterate(gp.GroupMultinomial(A64, y, C_, *alphas[res.best]), L)
    assert mn.rel(res.x, full) <= gp.TOL


# ---- multi-task against the reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(gp.VARIANTS))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", gp.MULTITASK_CASES, ids=lambda c: "%s-T%d-x%d" % c)
def test_multitask_matches_the_reference(fos, cus, case, kind, variant):
    name, T, count = case
    enet, delta = gp.VARIANTS[variant]
    m, n = gp.case_shape(name, kind, cus)
    A64, B, L = gp.multitask_recipe(m, n, T, gp.SEED, kind)
    alphas = gp.multitask_weights(A64, B, count, enet=enet)
    assert count == 1 or T > 8 or count % (16 // T) != 0
    Ad, Bd = _dev(A64, kind), torch.as_tensor(B.astype(np.float32)).cuda()
    if enet:
        xs = _direct(fos.prepare(Ad), T, [(1.0 / (L + a2), a1, a2) for a1, a2 in alphas], B=Bd, enet=True, delta=delta)
    else:
        xs, info = fos.multitask_path(Ad, Bd, alphas, max_iter=gp.ITERS, delta=delta, L=L, return_info=True)
        assert info == [(gp.ITERS, 0)] * count
    for (a1, a2), X in zip(alphas, xs):
        ref, safe = gp.multitask_reference(m, n, T, gp.SEED, kind, a1, a2, delta, enet)
        _check(X, ref, safe, (case, kind, variant, a1))
    if variant == "l1-fista":                               # the objective, for one and for several
        Xs = np.stack([_f32(X) for X in xs], axis=2)
        got = fos.multitask_objective(Xs, Ad, Bd, *alphas[0])
        assert got.shape == (count,)
        for k in range(count):
            R = A64 @ Xs[:, :, k] - B
            rr = (R * R).sum(axis=0)
            _, rr_tol = _data.fp32_pass_tolerances_cols(A64, Xs[:, :, k], B, np.zeros((n, T)), rr)
            want = gp.multitask_objective(A64, B, Xs[:, :, k], *alphas[0])
            assert abs(got[k] - want) <= 0.5 * float(rr_tol.sum()) + 1e-12 * abs(want), (k, got[k], want)
        one = fos.multitask_objective(torch.as_tensor(Xs[:, :, 0]), Ad, Bd, *alphas[0])
        # the same device data term; the host's fp64 penalty sums run over arrays of another shape: a few ulp
        assert isinstance(one, float) and abs(one - got[0]) <= 8 * np.finfo(np.float64).eps * abs(one)


def test_multitask_on_a_handle_with_penalty_factors(fos, cus):
    m, n = gp.case_shape("edges", "f32", cus)
    T = 3
    A64, B, L = gp.multitask_recipe(m, n, T, gp.SEED)
    p = _f32(np.random.default_rng(4).uniform(0.0, 2.0, size=n))
    p[-1] = 0.0
    alphas = gp.multitask_weights(A64, B, 2)
    P = fos.prepare_penalized(_dev(A64), B[:, 0], penalty_factor=p)
    Bd = torch.as_tensor(B.astype(np.float32)).cuda()
    xs = fos.multitask_path(P, Bd, alphas, max_iter=gp.ITERS, L=L)
    for (a1, a2), X in zip(alphas, xs):
        ref, prob = gp.iterate(gp.MultiTask(A64, B, a1, a2, p=p), L)
        plain, _ = gp.multitask_reference(m, n, T, gp.SEED, "f32", a1, a2)
        gp.check_recipe(ref, gp.separable_multitask(A64, B, a1, a2, L, p=p))
        assert mn.rel(ref, plain) > 100 * gp.TOL and np.abs(ref[-1]).min() > 0
        _check(X, ref, gp.safe_zero_rows(prob, ref), ("factors", a1))
        Xd = _f32(X)
        R = A64 @ Xd - B
        _, rr_tol = _data.fp32_pass_tolerances_cols(A64, Xd, B, np.zeros((n, T)), (R * R).sum(axis=0))
        want = gp.multitask_objective(A64, B, Xd, a1, a2, p)
        assert abs(fos.multitask_objective(X, P, Bd, a1, a2) - want) <= 0.5 * float(rr_tol.sum()) + 1e-12 * abs(want)
    # bounds on the handle: refused on the host
    P.set_penalty(penalty_factor=p, lower=0.0)
    with pytest.raises(ValueError, match="box bounds"):
        fos.multitask_path(P, Bd, alphas, max_iter=2, L=L)


# ---- defaults unchanged ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_ungrouped_defaults_are_the_group_zero_handles_bit_for_bit(fos, cus, kind):
    m, n = gp.case_shape("edges", kind, cus)
    C_ = 3
    A64, y, L = mn.recipe(m, n, C_, gp.SEED, kind)
    alphas = mn.weights(A64, y, C_, 3)
    P = fos.prepare_multinomial(_dev(A64, kind), y, classes=C_)
    xs = fos.multinomial_path(P, None, alphas, max_iter=gp.ITERS, L=L)
    P.set_grouped()
    P.set_grouped(False)                                    # a handle that was a grouped one for a while
    xg = fos.multinomial_path(P, None, alphas, max_iter=gp.ITERS, L=L)
    raw = _direct(P, C_, [(1.0 / (L + a2), a1, a2) for a1, a2 in alphas], group=0)
    for X, Xg, Xr, (a1, a2) in zip(xs, xg, raw, alphas):
        assert np.array_equal(mn.as_np(X), _f32(Xr)) and np.array_equal(mn.as_np(Xg), _f32(Xr))      # results come back in fp32
        assert mn.rel(X, mn.reference(m, n, C_, gp.SEED, kind, a1, a2)) <= gp.TOL
    # fista(A, B): T independent lassos, the lockstep with group = 0
    A64, B, Lq = gp.multitask_recipe(m, n, 5, gp.SEED, kind)
    a1 = gp.multitask_weights(A64, B, 1)[0][0]
    Ad, Bd = _dev(A64, kind), torch.as_tensor(B.astype(np.float32)).cuda()
    X = fos.fista(Ad, Bd, "lasso", a1, 0.0, max_iter=gp.ITERS, L=Lq)
    Xr = _direct(fos.prepare(Ad), 5, [(1.0 / Lq, a1, 0.0)], B=Bd, group=0)[0]
    assert np.array_equal(mn.as_np(X), _f32(Xr))
    assert mn.rel(Xr, gp.separable_multitask(A64, B, a1, 0.0, Lq)) <= gp.TOL


# ---- guards --------------------------------------------------------------------------------------------------------------------
def _snapshot(hs):
    out = []
    for st in hs:
        s = st.status()
        out.append((st.x_tensor().clone(), int(s.k), int(s.stopped)))
    return out


def _same(a, b):
    return all(torch.equal(x0, x1) and (k0, s0) == (k1, s1) for (x0, k0, s0), (x1, k1, s1) in zip(a, b))


@pytest.fixture(scope="module")
def grouped_handles(fos, cus):
    """A squared-loss problem and three handles with group = 3 that have run five lockstep iterations against three targets."""
    from fastoptsolver_amd import _core
    m, n = gp.case_shape("edges", "f32", cus)
    A64, B, L = gp.multitask_recipe(m, n, 3, gp.SEED)
    a1 = gp.multitask_weights(A64, B, 1)[0][0]
    P = fos.prepare(_dev(A64), B[:, 0].copy())
    Bd = torch.as_tensor(B.astype(np.float32)).cuda()
    hs = []
    for _ in range(3):
        st = _core.Fista(P)
        st.reset(1.0 / L, a1, 0.0, group=3)
        hs.append(st)
    assert _core.run_multi_rhs(hs, Bd, 5)
    return P, hs, Bd, (1.0 / L, a1)


def test_every_single_handle_entry_point_refuses_a_grouped_handle(fos, grouped_handles):
    from fastoptsolver_amd import _core
    P, hs, _, _ = grouped_handles
    lib, st, dev, n = P.lib, hs[0], P.device, P.n_dev
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)        # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)          # noqa: E731
    ptr = _core.ptr
    keep = dict(work=f64(4096), xh=f64(8, n), h4=f64(8, 4), ls=i32(8), taus=f64(8), rr=f64(8))
    done, tau = C.c_int32(0), C.c_double(0.0)
    out8, out128 = (C.c_double * 8)(), (C.c_double * 128)()
    calls = {
        "fos_fista_run": lambda: lib.fos_fista_run(st.h, 3),
        "fos_fista_run_history": lambda: lib.fos_fista_run_history(st.h, 3, ptr(keep["xh"]), ptr(keep["h4"]), ptr(keep["work"])),
        "fos_fista_run_resident": lambda: lib.fos_fista_run_resident(st.h, 3, 0, 0.5, 1e-2, 0.0, ptr(keep["xh"]), ptr(keep["h4"]),
                                                                     ptr(keep["ls"]), ptr(keep["taus"]), C.byref(done), C.byref(tau)),
        "fos_fista_run_fused": lambda: lib.fos_fista_run_fused(st.h, 3),
        "fos_fista_run_chip": lambda: lib.fos_fista_run_chip(st.h, 3),
        "fos_fista_grad": lambda: lib.fos_fista_grad(st.h),
        "fos_fista_grad_dual": lambda: lib.fos_fista_grad_dual(st.h),
        "fos_fista_update": lambda: lib.fos_fista_update(st.h),
        "fos_fista_trial": lambda: lib.fos_fista_trial(st.h, 0.1, 1, out8),
        "fos_fista_trial_batch": lambda: lib.fos_fista_trial_batch(st.h, 0.1, 0.5, 16, out128),
        "fos_fista_run_backtracking": lambda: lib.fos_fista_run_backtracking(st.h, 3, 0.5, 1e-2, 1e-6, ptr(keep["ls"]), ptr(keep["taus"])),
        "fos_fista_run_recorded": lambda: lib.fos_fista_run_recorded(st.h, 3, 0, 0.5, 1e-2, 1e-6, ptr(keep["xh"]), ptr(keep["h4"]),
                                                                     ptr(keep["rr"]), ptr(keep["ls"]), ptr(keep["taus"])),
        "fos_fista_resume_after_stall": lambda: lib.fos_fista_resume_after_stall(st.h, C.byref(tau)),
    }
    from tests.test_group_abi import SINGLE
    assert set(calls) == set(SINGLE)
    before = _snapshot(hs)
    for name in SINGLE:
        with P.ctx():
            rc = calls[name]()
        msg = lib.fos_last_error().decode()
        assert rc == UNSUPPORTED and name in msg and "group penalty" in msg, (name, rc, msg)
    torch.cuda.synchronize()
    assert _same(before, _snapshot(hs))


def test_the_lockstep_refusals_leave_the_state_unchanged(fos, cus, grouped_handles):
    from fastoptsolver_amd import _core
    P, hs, Bd, (tau, a1) = grouped_handles
    before = _snapshot(hs)

    def refused(call, prob=P):
        assert call() is False
        msg = prob.lib.fos_last_error().decode()
        assert "group penalty" in msg, msg
        return msg

    def fresh(prob, count, group=3, **over):
        out = []
        for i in range(count):
            st = _core.Fista(prob)
            st.reset(tau, a1, 0.0, group=group, **(over if i == 1 else {}))
            out.append(st)
        return out

    ids = _core.fold_ids_tensor(np.arange(P.m) % 2, P.device)
    # nv no multiple of G
    assert "multiple" in refused(lambda: _core.run_multi_rhs(hs[:2], Bd[:, :2], 3))
    assert "multiple" in refused(lambda: _core.run_multi(hs[:2], 3))
    # differing parameters inside a segment; differing held folds
    odd = fresh(P, 3)
    odd[1].reset(tau, 0.5 * a1, 0.0, group=3)
    assert "identical" in refused(lambda: _core.run_multi_rhs(odd, Bd, 3))
    assert "identical" in refused(lambda: _core.run_multi_folds(hs, ids, [0, 0, 1], 3))
    # a controlled handle, the gradient-norm rule
    for over in (dict(tol_ratio=0.1), dict(adaptive_restart=True), dict(tol_step=1e-9), dict(tol_grad=1e-3)):
        assert "plain runs only" in refused(lambda: _core.run_multi_rhs(fresh(P, 3, **over), Bd, 3))
    # grouped and ungrouped handles in one call
    mixed = fresh(P, 3) + fresh(P, 3, group=0)
    B6 = Bd.repeat(1, 2).contiguous()
    assert "mix" in refused(lambda: _core.run_multi_rhs(mixed, B6, 3))
    assert "mix" in refused(lambda: _core.run_multi_rhs(mixed[::-1], B6, 3))
    # bound box vectors (factors alone are served: test_multitask_on_a_handle_with_penalty_factors)
    Q = fos.prepare_penalized(P.A, P.b, lower=0.0)
    assert "box bounds" in refused(lambda: _core.run_multi_rhs(fresh(Q, 3), Bd, 3), Q)
    assert "box bounds" in refused(lambda: _core.run_multi(fresh(Q, 3), 3), Q)
    # G != C on a multinomial problem (nv = 12 is a multiple of both)
    m, n = gp.case_shape("one_tile", "f32", cus)
    A64, y, L = mn.recipe(m, n, 4, gp.SEED)
    M = fos.prepare_multinomial(_dev(A64), y, classes=4)
    twelve = fresh(M, 12)
    assert "class count" in refused(lambda: _core.run_multi(twelve, 3), M)
    assert all(int(st.status().k) == 0 for st in twelve + odd + mixed)
    # a right-hand-side block on a logistic problem: the loss guard's own refusal
    Lg = fos.prepare(P.A, (P.b > 0).float(), loss="logistic")
    assert _core.run_multi_rhs(fresh(Lg, 3), Bd, 3) is False and "logistic problem" in Lg.lib.fos_last_error().decode()
    # iters = 0 is served and changes nothing; so did every refusal
    assert _core.run_multi_rhs(hs, Bd, 0) is True
    torch.cuda.synchronize()
    assert _same(before, _snapshot(hs))
    # and the handles still run: eight iterations in all are the reference's eight
    assert _core.run_multi_rhs(hs, Bd, 3) and all(int(st.status().k) == 8 for st in hs)
