"""GPU: every row of tests/_link_guard.py behaves as filed on a Huber and on a squared-hinge problem (fos_problem_set_link_loss).
The refusing entry points return FOS_ERR_UNSUPPORTED with the link losses' own message and leave the handles as they were - an
answer with another loss's quantity on such a handle is the one silent failure the feature could introduce.  The calls are those
of tests/test_gpu_logit_guard.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _link as lk, _link_guard as gd
from tests.test_gpu_logit_guard import UNSUPPORTED, _calls, _snapshot

pytestmark = pytest.mark.gpu
M, N = 1001, 200
CODES = {lk.HUBER: 3, lk.HINGE: 4}


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


@pytest.fixture(scope="module", params=[lk.HUBER, lk.HINGE])
def setup(fos, request):
    """A problem of the loss with three handles that have run five lockstep iterations."""
    from fastoptsolver_amd import _core
    loss = request.param
    if loss == lk.HUBER:
        A64, b, c, L, alphas = lk.huber_recipe(M, N, check=False)
        P = fos.prepare_huber(torch.as_tensor(A64.astype(np.float32)).cuda(), b, c)
    else:
        A64, b, L, alphas = lk.hinge_recipe(M, N, 9, check=False)
        c = None
        P = fos.prepare_hinge(torch.as_tensor(A64.astype(np.float32)).cuda(), b)
    hs = []
    for a1, a2 in alphas:
        st = _core.Fista(P)
        st.reset(1.0 / (L + a2), a1, a2)
        hs.append(st)
    assert _core.run_multi(hs, 5)
    return P, hs, dict(loss=loss, A=A64, b=b, c=c, L=L, alphas=alphas)


def test_every_refusing_entry_point_refuses_and_changes_nothing(fos, setup):
    from fastoptsolver_amd import _core
    P, hs, _ = setup
    before = _snapshot(hs)
    keep, calls = _calls(P, hs)
    assert set(calls) == gd.REFUSES, set(calls) ^ gd.REFUSES
    for name in sorted(calls):
        rc = calls[name]()
        msg = P.lib.fos_last_error().decode()
        assert rc == UNSUPPORTED, (name, rc, msg)
        assert name in msg and "Huber or the squared-hinge loss" in msg and "fos_problem_set_link_loss" in msg, (name, msg)
    # fos_residual_batch serves use_b = 1 and refuses use_b = 0
    with pytest.raises(fos.FosError, match="code -4"):
        P.residual_batch(keep["X16"][:, :3], use_b=False)
    assert "fos_problem_set_link_loss" in P.lib.fos_last_error().decode()
    # refused as on a logistic problem: the group penalty across columns, the gradient-norm rule, the fp64 split gradient
    grouped = [_core.Fista(P) for _ in range(2)]
    for st in grouped:
        st.reset(0.01, 0.1, 0.0, group=2)
    assert _core.run_multi(grouped, 2) is False and "fos_problem_set_link_loss" in P.lib.fos_last_error().decode()
    st = _core.Fista(P)
    st.reset(0.01, 0.1, 0.0, tol_grad=1e-3)
    assert _core.run_multi([st], 3) is False and int(st.status().k) == 0
    st.reset(0.01, 0.1, 0.0)
    st.set_precise(True)
    assert _core.run_multi([st], 3) is False and int(st.status().k) == 0
    # fos_problem_set_loss keeps refusing the two codes, and the getters report the loss
    loss, param, code = C.c_int(-1), C.c_double(-1.0), C.c_int(-1)
    for bad in (3, 4):
        assert P.lib.fos_problem_set_loss(P.h, bad) == -1
    assert P.lib.fos_problem_get_loss(P.h, C.byref(code)) == 0 and code.value == CODES[P.loss]
    assert P.lib.fos_problem_get_link_loss(C.byref(loss), C.byref(param), P.h) == 0
    assert (loss.value, param.value) == (CODES[P.loss], P.threshold or 0.0)
    torch.cuda.synchronize()
    after = _snapshot(hs)
    for (x0, s0), (x1, s1) in zip(before, after):
        assert torch.equal(x0, x1) and s0 == s1, (s0, s1)
    # and the handles still run
    assert _core.run_multi(hs, 2) and all(int(st.status().k) == 7 for st in hs)


def test_serving_and_loss_free_entry_points_answer(fos, setup):
    from fastoptsolver_amd import _core
    P, hs, c = setup
    assert {"fos_fista_run_multi", "fos_fista_run_multi_folds", "fos_residual_batch", "fos_residual_batch_folds", "fos_gradient_batch"} == gd.SERVES
    X = torch.stack([st.x_tensor() for st in hs], dim=1)
    X32 = X.float().double().cpu().numpy()
    got = np.asarray(P.residual_batch(X, use_b=True))
    ref, tol = lk.data_term(c["loss"], c["A"], X32, c["b"], c["c"]), lk.loss_tolerance(c["loss"], c["A"], X32, c["b"], c["c"])
    assert (np.abs(got - ref) <= tol).all(), (got, ref, tol)
    ids = _core.fold_ids_tensor(np.arange(P.m) % 3, P.device)
    assert len(P.residual_batch_folds(X, ids, [0, 1, 2])) == 3
    G, sums = P.gradient_block(X, want_loss=True)
    assert np.allclose(sums, got, rtol=1e-14) and tuple(G.shape) == (3, P.n_dev)
    fresh = []
    for a1, a2 in c["alphas"]:
        st = _core.Fista(P)
        st.reset(1.0 / (c["L"] + a2), a1, a2)
        fresh.append(st)
    assert _core.run_multi_folds(fresh, ids, [0, 1, 2], 3) and all(int(st.status().k) == 3 for st in fresh)
    # loss-free: as before
    assert P.power_iter(np.ones(P.n))[0] > 0 and P.plan()["cus"] > 0
    assert torch.isfinite(P.gram_apply(X[:, :2].float())).all()
    lmax = float(np.linalg.eigvalsh(c["A"].T @ c["A"])[-1])
    assert 0.5 < fos.estimate_lipschitz(P) / lmax <= 1.0 + 1e-5          # ||A^T A v|| of a unit v: from below, to fp32 rounding
    w = torch.ones((P.m + 3) // 4 * 4, device="cuda")
    P.set_sample_weight(w[:P.m])
    assert np.allclose(P.residual_batch(X, use_b=True), got, rtol=1e-14)   # unit weights: the same terms
    P.set_sample_weight(None)
    P.set_penalty(lower=0.0)
    P.set_penalty()
    P.set_feature_groups([100, 100])
    assert P.has_feature_groups and _core.run_multi(fresh, 1)
    P.set_feature_groups(None)
    excess, viol = P.kkt_scan(G, [a1 for a1, _ in c["alphas"]], 0.0, torch.zeros(P.n_dev, dtype=torch.uint8, device="cuda"))
    assert tuple(excess.shape) == (P.n_dev,)
    assert tuple(P.gather_columns(torch.arange(8, device="cuda")).shape) == (P.m, 8)


def test_public_names_behave_as_filed(fos, setup):
    P, _, c = setup
    huber = c["loss"] == lk.HUBER
    x0 = np.zeros(P.n)
    B2 = np.stack([c["b"], c["b"]], axis=1)
    w = [(0.1, 0.0)]
    other = {  # the three functions of the other link loss refuse this handle
        True: dict(hinge_path=lambda: fos.hinge_path(P, None, w, max_iter=2), hinge_cv=lambda: fos.hinge_cv(P, None, w, 3, max_iter=2),
                   hinge_objective=lambda: fos.hinge_objective(x0, P, None, 0.1, 0.0)),
        False: dict(huber_path=lambda: fos.huber_path(P, None, w, max_iter=2), huber_cv=lambda: fos.huber_cv(P, None, w, 3, max_iter=2),
                    huber_objective=lambda: fos.huber_objective(x0, P, None, 0.1, 0.0)),
    }[huber]
    refusing = {
        "ista": lambda: fos.ista(x0, fos.LeastSquares(P), None, fos.L1Prox(0.1), 1.0, max_iter=3),
        "LeastSquares": lambda: fos.LeastSquares(P),
        "fista": lambda: fos.fista(P, None, "lasso", 0.1, 0.0, max_iter=3, L=1.0),
        "fista_delta": lambda: fos.fista_delta(P, None, "lasso", 0.1, 0.0, 3.0, max_iter=3, L=1.0),
        "fista_path": lambda: fos.fista_path(P, None, w, max_iter=2, L=1.0),
        "fista_cv": lambda: fos.fista_cv(P, None, w, 3, max_iter=2, L=1.0),
        "LBFGSSolver": lambda: fos.LBFGSSolver("ridge", 0.0, 1.0, max_iter=3).fit(P, None),
        "compute_objective": lambda: fos.compute_objective(x0, P, None, "lasso", 0.1, 0.0),
        "group_lasso_objective": lambda: fos.group_lasso_objective(x0, P, None, 0.1, 0.0, [100, 100]),
        "logistic_path": lambda: fos.logistic_path(P, None, w, max_iter=2),
        "logistic_cv": lambda: fos.logistic_cv(P, None, w, 3, max_iter=2),
        "logistic_objective": lambda: fos.logistic_objective(x0, P, None, 0.1, 0.0),
        "multinomial_path": lambda: fos.multinomial_path(P, None, w, max_iter=2),
        "multinomial_cv": lambda: fos.multinomial_cv(P, None, w, 3, max_iter=2),
        "multinomial_objective": lambda: fos.multinomial_objective(np.zeros((P.n, 3)), P, None, 0.1, 0.0),
        "multitask_path": lambda: fos.multitask_path(P, B2, w, max_iter=2, L=1.0),
        "multitask_objective": lambda: fos.multitask_objective(np.zeros((P.n, 2)), P, B2, 0.1, 0.0),
        "prepare_weighted": lambda: fos.prepare_weighted(P, None, np.ones(P.m)),
        "prepare_penalized": lambda: fos.prepare_penalized(P, None, lower=0.0),
        "prepare_grouped": lambda: fos.prepare_grouped(P, None, [100, 100]),
        "prepare_multinomial": lambda: fos.prepare_multinomial(P, None),
        "prepare_huber": lambda: fos.prepare_huber(P, None, 1.0),
        "prepare_hinge": lambda: fos.prepare_hinge(P, None),
    }
    assert set(refusing) == {k for k, v in gd.PYTHON.items() if v == "refuses"}
    for name, call in sorted({**refusing, **other}.items()):
        with pytest.raises((fos.FosError, ValueError)):
            call()
        print(name, "refuses")
    for name in ("fista", "fista_delta", "fista_path", "fista_cv", "LBFGSSolver", "compute_objective", "logistic_path", "multinomial_path",
                 "multitask_path"):
        with pytest.raises(ValueError, match="huber_path" if huber else "hinge_path"):     # the message names the right call
            refusing[name]()
    assert fos.prepare(P) is P and fos.alpha_max(P) > 0


def test_the_handle_leaves_the_loss_and_serves_the_squared_forms_again(fos):
    from fastoptsolver_amd import _core, _lib
    A64, b, c, L, alphas = lk.huber_recipe(M, N, check=False)
    At = torch.as_tensor(A64.astype(np.float32)).cuda()
    P = fos.prepare_huber(At, b, c)
    bare = fos.prepare(At, b)
    x = torch.as_tensor(0.1 * np.random.default_rng(4).standard_normal(N)).float().cuda()
    loss, param = C.c_int(-1), C.c_double(-1.0)
    assert P.lib.fos_problem_set_loss(P.h, _lib.LOSS_SQUARED) == 0
    assert P.lib.fos_problem_get_link_loss(C.byref(loss), C.byref(param), P.h) == 0 and (loss.value, param.value) == (0, 0.0)
    assert P.residual_objective(x)[0] == bare.residual_objective(x)[0]
    assert P.residual_batch(x.reshape(-1, 1), use_b=True) == bare.residual_batch(x.reshape(-1, 1), use_b=True)
    # and back: the hinge needs labels, so b = the targets is the caller's mistake to make; Huber with its parameter again
    assert P.lib.fos_problem_set_link_loss(_lib.LOSS_HUBER, c, P.h) == 0
    assert P.lib.fos_problem_set_multinomial(3, P.h) == 0
    assert P.lib.fos_problem_get_link_loss(C.byref(loss), C.byref(param), P.h) == 0 and (loss.value, param.value) == (0, 0.0)
    # what cannot carry the loss
    nob = fos.prepare(At)
    assert P.lib.fos_problem_set_link_loss(_lib.LOSS_HUBER, 1.0, nob.h) == UNSUPPORTED
    small = fos.prepare(torch.zeros(100, 4, device="cuda"), torch.zeros(100))          # the LDS-resident plan
    assert P.lib.fos_problem_set_link_loss(_lib.LOSS_SQUARED_HINGE, 0.0, small.h) == UNSUPPORTED
    assert "fos_problem_set_link_loss" in P.lib.fos_last_error().decode()
