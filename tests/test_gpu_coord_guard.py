"""GPU: on a problem with penalty factors or bounds (fos_coord_bind) every entry point filed under "refuses" in
tests/_logit_guard.py returns FOS_ERR_UNSUPPORTED with the coordinate message and leaves the handles as they were - an
unconstrained answer on a constrained handle is the one silent failure the feature could introduce.  The calls are those of
tests/test_gpu_logit_guard.py, on a squared-loss problem with coordinate data."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _coord as cd, _logit_guard as gd
from tests.test_gpu_logit_guard import UNSUPPORTED, _calls, _snapshot

pytestmark = pytest.mark.gpu
WORDS = "penalty factors or bounds"


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


@pytest.fixture(scope="module")
def setup(fos):
    """A squared-loss problem with coordinate data and three handles that have run five lockstep iterations."""
    from fastoptsolver_amd import _core
    c = cd.case("f32", "squared", 1001, 200, 9)
    P = fos.prepare_penalized(torch.as_tensor(c["A"].astype(np.float32)).cuda(), c["b"], c["p"], c["lo"], c["hi"])
    hs = []
    for a1, a2 in c["alphas"]:
        st = _core.Fista(P)
        st.reset(1.0 / (c["L"] + a2 * P.penalty_max), a1, a2)
        hs.append(st)
    assert _core.run_multi(hs, 5)
    return P, hs


def test_every_refusing_entry_point_refuses_and_changes_nothing(fos, setup):
    from fastoptsolver_amd import _core
    P, hs = setup
    before = _snapshot(hs)
    keep, calls = _calls(P, hs)
    assert set(calls) == gd.REFUSES, set(calls) ^ gd.REFUSES
    for name in sorted(calls):
        rc = calls[name]()
        msg = P.lib.fos_last_error().decode()
        assert rc == UNSUPPORTED, (name, rc, msg)
        assert name in msg and WORDS in msg and "fos_coord_bind" in msg, (name, msg)     # the coordinate data's own message
    # fos_residual_batch serves use_b = 1 and refuses use_b = 0
    with pytest.raises(fos.FosError, match="code -4"):
        P.residual_batch(keep["X16"][:, :3], use_b=False)
    assert WORDS in P.lib.fos_last_error().decode()
    assert len(P.residual_batch(keep["X16"][:, :3], use_b=True)) == 3
    torch.cuda.synchronize()
    after = _snapshot(hs)
    for (x0, s0), (x1, s1) in zip(before, after):
        assert torch.equal(x0, x1) and s0 == s1, (s0, s1)
    # and the handles still run
    assert _core.run_multi(hs, 2) and all(int(st.status().k) == 7 for st in hs)


def test_public_solvers_fail_with_the_guards_error(fos, setup):
    P, _ = setup
    x0 = np.zeros(P.n)
    ls = fos.LeastSquares(P)
    for call in (lambda: fos.ista(x0, ls, ls.grad, fos.L1Prox(0.1), 1.0, max_iter=3),
                 lambda: fos.fista(P, None, "lasso", 0.1, 0.0, max_iter=3, L=1.0),
                 lambda: fos.fista_delta(P, None, "lasso", 0.1, 0.0, 3.0, max_iter=3, L=1.0),
                 lambda: fos.LBFGSSolver("ridge", 0.0, 1.0, max_iter=3).fit(P, None),
                 lambda: fos.compute_objective(x0, P, None, "lasso", 0.1, 0.0)):
        with pytest.raises(fos.FosError, match=WORDS):
            call()
    for kw in (dict(tol=1e-3), dict(cols=(0, 4, 8))):
        with pytest.raises(ValueError):
            fos.fista_path(P, None, [(0.1, 0.0)], max_iter=2, L=1.0, **kw)


def test_loss_free_entry_points_binding_refusals_and_the_lockstep_refusals(fos, setup):
    from fastoptsolver_amd import _core, _lib
    P, _ = setup
    assert P.power_iter(np.ones(P.n))[0] > 0 and P.plan()["cus"] > 0
    out = C.c_int(-1)
    assert P.lib.fos_problem_get_loss(P.h, C.byref(out)) == 0 and out.value == _lib.LOSS_SQUARED
    got = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
    assert P.lib.fos_coord_get(C.byref(got[0]), C.byref(got[1]), C.byref(got[2]), P.h) == 0
    assert [g.value for g in got] == [t.data_ptr() for t in (P.penalty_factor, P.lower, P.upper)]
    st = _core.Fista(P)
    st.reset(0.01, 0.1, 0.0, tol_grad=1e-3)                        # the gradient-norm rule: refused as the fold lockstep refuses it
    assert _core.run_multi([st], 3) is False and int(st.status().k) == 0
    # what cannot carry coordinate data: no b, the LDS-resident plan; detaching is always served
    v = torch.ones(204, device="cuda")
    bare = fos.prepare(P.A)
    assert P.lib.fos_coord_bind(_core.ptr(v), None, None, bare.h) == UNSUPPORTED
    small = fos.prepare(torch.zeros(100, 4, device="cuda"), torch.zeros(100))
    for args in ((_core.ptr(v), None, None), (None, _core.ptr(v), None), (None, None, _core.ptr(v))):
        assert P.lib.fos_coord_bind(*args, small.h) == UNSUPPORTED
        assert "fos_coord_bind" in P.lib.fos_last_error().decode()
    assert P.lib.fos_coord_get(C.byref(got[0]), C.byref(got[1]), C.byref(got[2]), small.h) == 0
    assert [g.value for g in got] == [None, None, None]
    assert P.lib.fos_coord_bind(None, None, None, small.h) == 0 and P.lib.fos_coord_bind(None, None, None, bare.h) == 0
    with pytest.raises(fos.FosError, match="fos_coord_bind"):
        small.set_penalty(lower=0.0)
    assert not small.has_coord and small.penalty_max == 1.0
