"""GPU: every row of tests/_fgroup_guard.py behaves as filed on a problem with feature groups (fos_feature_groups_bind).  The
refusing entry points return FOS_ERR_UNSUPPORTED with the feature groups' own message and leave the handles as they were - an
answer without the group penalty on such a handle is the one silent failure the feature could introduce.  The calls are those of
tests/test_gpu_logit_guard.py, on a squared-loss problem with feature groups."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _fgroup as fg, _fgroup_guard as gd
from tests.test_gpu_logit_guard import UNSUPPORTED, _calls, _snapshot

pytestmark = pytest.mark.gpu
WORDS = "feature groups"
KEY = ("f32", "squared", 1001, 200, 3203, False, "span150", 0.5)


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


def _labels(start):
    return np.repeat(np.arange(len(start) - 1), np.diff(start))


@pytest.fixture(scope="module")
def setup(fos):
    """A squared-loss problem with feature groups and three handles that have run five lockstep iterations."""
    from fastoptsolver_amd import _core
    c = fg.case(*KEY)
    P = fos.prepare_grouped(torch.as_tensor(c["A"].astype(np.float32)).cuda(), c["b"], _labels(c["start"]), None, 0.5)
    hs = []
    for a1, a2 in c["alphas"][:3]:                   # three: the calls of tests/test_gpu_logit_guard.py hand them a block of three columns
        st = _core.Fista(P)
        st.reset(1.0 / (c["L"] + a2), a1, a2)
        hs.append(st)
    assert _core.run_multi(hs, 5)
    return P, hs, c


def test_every_refusing_entry_point_refuses_and_changes_nothing(fos, setup):
    from fastoptsolver_amd import _core
    P, hs, _ = setup
    before = _snapshot(hs)
    keep, calls = _calls(P, hs)
    assert set(calls) == gd.REFUSES - gd.OWN_CHECK, set(calls) ^ (gd.REFUSES - gd.OWN_CHECK)
    for name in sorted(calls):
        rc = calls[name]()
        msg = P.lib.fos_last_error().decode()
        assert rc == UNSUPPORTED, (name, rc, msg)
        assert name in msg and WORDS in msg and "fos_feature_groups_bind" in msg, (name, msg)     # the groups' own message
    # the two that refuse by a check of their own: neither composes with the group norm
    v = torch.ones(204, device="cuda")
    for name, call in (("fos_coord_bind", lambda: P.lib.fos_coord_bind(_core.ptr(v), None, None, P.h)),
                       ("fos_coord_bind", lambda: P.lib.fos_coord_bind(None, None, _core.ptr(v), P.h)),
                       ("fos_problem_set_multinomial", lambda: P.lib.fos_problem_set_multinomial(3, P.h))):
        assert call() == UNSUPPORTED
        msg = P.lib.fos_last_error().decode()
        assert name in msg and WORDS in msg and "fos_feature_groups_bind" in msg, (name, msg)
    assert P.lib.fos_coord_bind(None, None, None, P.h) == 0                                      # detaching nothing is served
    with pytest.raises(fos.FosError, match="fos_coord_bind"):
        P.set_penalty(lower=0.0)
    assert not P.has_coord and P.has_feature_groups
    # fos_residual_batch serves use_b = 1 and refuses use_b = 0
    with pytest.raises(fos.FosError, match="code -4"):
        P.residual_batch(keep["X16"][:, :3], use_b=False)
    assert WORDS in P.lib.fos_last_error().decode()
    torch.cuda.synchronize()
    after = _snapshot(hs)
    for (x0, s0), (x1, s1) in zip(before, after):
        assert torch.equal(x0, x1) and s0 == s1, (s0, s1)
    # and the handles still run
    assert _core.run_multi(hs, 2) and all(int(st.status().k) == 7 for st in hs)


def test_serving_and_loss_free_entry_points_answer(fos, setup):
    from fastoptsolver_amd import _core, _lib
    P, hs, c = setup
    assert {"fos_fista_run_multi", "fos_fista_run_multi_folds", "fos_residual_batch", "fos_residual_batch_folds"} == gd.SERVES
    X = torch.stack([st.x_tensor() for st in hs], dim=1)
    bare = fos.prepare(P.A, c["b"])                                  # the data term does not depend on the groups
    assert P.residual_batch(X, use_b=True) == bare.residual_batch(X, use_b=True)
    ids = _core.fold_ids_tensor(np.arange(P.m) % 3, P.device)
    assert P.residual_batch_folds(X, ids, [0, 1, 2]) == bare.residual_batch_folds(X, ids, [0, 1, 2])
    fresh = []
    for a1, a2 in c["alphas"]:
        st = _core.Fista(P)
        st.reset(1.0 / (c["L"] + a2), a1, a2)
        fresh.append(st)
    assert _core.run_multi_folds(fresh, ids, [0, 1, 2, 0], 3) and all(int(st.status().k) == 3 for st in fresh)
    # loss-free: as before
    assert P.power_iter(np.ones(P.n))[0] > 0 and P.plan()["cus"] > 0
    out = C.c_int(-1)
    assert P.lib.fos_problem_get_loss(P.h, C.byref(out)) == 0 and out.value == _lib.LOSS_SQUARED
    assert P.lib.fos_problem_get_classes(C.byref(out), P.h) == 0 and out.value == 0
    n, mix = C.c_int32(-1), C.c_double(-1.0)
    assert P.lib.fos_feature_groups_get(C.byref(n), C.byref(mix), P.h) == 0 and (n.value, mix.value) == (len(c["start"]) - 1, 0.5)
    assert torch.equal(P.gram_apply(X[:, :2].float()), bare.gram_apply(X[:, :2].float()))
    assert 0.5 < fos.estimate_lipschitz(P) / c["L"] < 1.0 + 1e-3          # a power iteration from below, its own start vector


def test_public_names_behave_as_filed(fos, setup):
    P, _, c = setup
    x0 = np.zeros(P.n)
    ls = fos.LeastSquares(P)
    B2 = np.stack([c["b"], c["b"]], axis=1)
    refusing = {
        "ista": lambda: fos.ista(x0, ls, ls.grad, fos.L1Prox(0.1), 1.0, max_iter=3),
        "fista": lambda: fos.fista(P, None, "lasso", 0.1, 0.0, max_iter=3, L=1.0),
        "fista_delta": lambda: fos.fista_delta(P, None, "lasso", 0.1, 0.0, 3.0, max_iter=3, L=1.0),
        "LBFGSSolver": lambda: fos.LBFGSSolver("ridge", 0.0, 1.0, max_iter=3).fit(P, None),
        "compute_objective": lambda: fos.compute_objective(x0, P, None, "lasso", 0.1, 0.0),
        "logistic_objective": lambda: fos.logistic_objective(x0, fos.prepare_grouped(P.A, (c["b"] > 0).astype(float), [100, 100], loss="logistic"),
                                                             None, 0.1, 0.0),
        "multinomial_path": lambda: fos.multinomial_path(P, None, [(0.1, 0.0)], max_iter=2),
        "multinomial_cv": lambda: fos.multinomial_cv(P, None, [(0.1, 0.0)], 3, max_iter=2),
        "multinomial_objective": lambda: fos.multinomial_objective(np.zeros((P.n, 3)), P, None, 0.1, 0.0),
        "multitask_path": lambda: fos.multitask_path(P, B2, [(0.1, 0.0)], max_iter=2, L=1.0),
        "multitask_objective": lambda: fos.multitask_objective(np.zeros((P.n, 2)), P, B2, 0.1, 0.0),
        "prepare_weighted": lambda: fos.prepare_weighted(P, None, np.ones(P.m)),
        "prepare_penalized": lambda: fos.prepare_penalized(P, None, lower=0.0),
        "prepare_grouped": lambda: fos.prepare_grouped(P, None, [100, 100]),
        "prepare_multinomial": lambda: fos.prepare_multinomial(P, None),
    }
    assert set(refusing) == {k for k, v in gd.PYTHON.items() if v == "refuses"}
    for name, call in sorted(refusing.items()):
        with pytest.raises((fos.FosError, ValueError)):
            call()
        print(name, "refuses")
    for name in ("ista", "fista", "fista_delta", "LBFGSSolver", "compute_objective"):
        with pytest.raises(fos.FosError, match=WORDS):
            refusing[name]()
    for kw in (dict(tol=1e-3), dict(cols=(0, 4, 8))):
        with pytest.raises(ValueError):
            fos.fista_path(P, None, [(0.1, 0.0)], max_iter=2, L=1.0, **kw)
    assert fos.prepare(P) is P and len(fos.fista_path(P, None, [(0.1, 0.0)], max_iter=2, L=c["L"])) == 1


def test_what_cannot_carry_feature_groups_is_refused(fos, setup):
    """Coordinate data and then groups (the other order is in the first test), a multinomial handle, a sharded problem, a problem
    without b or without the matrix-core pair, a handle under the column-group penalty, a right-hand-side block."""
    from fastoptsolver_amd import _core, _lib
    from fastoptsolver_amd.distributed import Comm
    P, hs, c = setup
    At = P.A
    pen = fos.prepare_penalized(At, c["b"], lower=0.0)
    with pytest.raises(fos.FosError, match="fos_feature_groups_bind"):
        pen.set_feature_groups([100, 100])
    assert "code -4" in str(_fos_error(lambda: pen.set_feature_groups([100, 100]))) and not pen.has_feature_groups and pen.has_coord
    multi = fos.prepare_multinomial(At, np.arange(P.m) % 3)
    assert "code -4" in str(_fos_error(lambda: multi.set_feature_groups([100, 100])))
    with pytest.raises(ValueError):
        fos.prepare_grouped(At, np.arange(P.m) % 3, [100, 100], loss="multinomial")
    sharded = fos.prepare(At, c["b"])
    sharded.set_comm(Comm.solo())
    assert "code -4" in str(_fos_error(lambda: sharded.set_feature_groups([100, 100]))) and "sharded" in sharded.lib.fos_last_error().decode()
    assert "code -4" in str(_fos_error(lambda: fos.prepare(At).set_feature_groups([100, 100])))                 # no b
    small = fos.prepare(torch.zeros(100, 4, device="cuda"), torch.zeros(100))                                 # no matrix-core pair
    assert "code -4" in str(_fos_error(lambda: small.set_feature_groups([2, 2]))) and not small.has_feature_groups
    small.set_feature_groups(None)                                                                            # detaching is always served
    # a handle under the column-group penalty, alone and with a right-hand-side block; an ungrouped block
    grouped = []
    for _ in range(2):
        st = _core.Fista(P)
        st.reset(1.0 / c["L"], c["alphas"][0][0], 0.0, group=2)
        grouped.append(st)
    B = torch.zeros(P.m, 2, device="cuda")
    assert _core.run_multi(grouped, 3) is False and WORDS in P.lib.fos_last_error().decode()
    assert _core.run_multi_rhs(grouped, B, 3) is False and WORDS in P.lib.fos_last_error().decode()
    assert _core.run_multi_rhs(hs[:2], B, 3) is False and WORDS in P.lib.fos_last_error().decode()
    assert all(int(st.status().k) == 0 for st in grouped)
    st = _core.Fista(P)
    st.reset(0.01, 0.1, 0.0, tol_grad=1e-3)                        # the gradient-norm rule: refused as the fold lockstep refuses it
    assert _core.run_multi([st], 3) is False and int(st.status().k) == 0


def _fos_error(call):
    import fastoptsolver_amd as fos
    try:
        call()
    except fos.FosError as e:
        return e
    raise AssertionError("no FosError")
