"""GPU: on a problem with row weights every entry point filed under "refuses" in tests/_logit_guard.py returns
FOS_ERR_UNSUPPORTED and leaves the handles as they were - an unweighted answer on a weighted handle is the one silent failure
the feature could introduce.  The calls are those of tests/test_gpu_logit_guard.py, on a weighted squared-loss problem."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _data, _logit_guard as gd, _weighted as wt
from tests.test_gpu_logit_guard import UNSUPPORTED, _calls, _snapshot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


@pytest.fixture(scope="module")
def setup(fos):
    """A weighted squared-loss problem with three handles that have run five lockstep iterations."""
    from fastoptsolver_amd import _core
    A, b, _ = _data.synth(1001, 200, 9)
    A64 = A.astype(np.float32).astype(np.float64)
    w = wt.as_stored(wt.weights("spread", 1001, 9))
    L = wt.lipschitz(A64, w, 9, "squared")
    P = fos.prepare_weighted(torch.as_tensor(A64.astype(np.float32)).cuda(), b, w)
    hs = []
    for a1, a2 in wt.alphas(A64, b, w, "squared"):
        st = _core.Fista(P)
        st.reset(1.0 / (L + a2), a1, a2)
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
        assert name in msg and "row weights" in msg, (name, msg)           # the weights' own message
    # fos_residual_batch serves use_b = 1 and refuses use_b = 0
    with pytest.raises(fos.FosError, match="code -4"):
        P.residual_batch(keep["X16"][:, :3], use_b=False)
    assert "row weights" in P.lib.fos_last_error().decode()
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
        with pytest.raises(fos.FosError, match="row weights"):
            call()


def test_loss_free_entry_points_and_the_lockstep_refusals(fos, setup):
    from fastoptsolver_amd import _core, _lib
    P, _ = setup
    assert P.power_iter(np.ones(P.n))[0] > 0 and P.plan()["cus"] > 0
    out = C.c_int(-1)
    assert P.lib.fos_problem_get_loss(P.h, C.byref(out)) == 0 and out.value == _lib.LOSS_SQUARED
    st = _core.Fista(P)
    st.reset(0.01, 0.1, 0.0, tol_grad=1e-3)                        # the gradient-norm rule: refused as the fold lockstep refuses it
    assert _core.run_multi([st], 3) is False and int(st.status().k) == 0
    # what cannot carry weights: no b, the LDS-resident plan
    w = torch.ones(1004, device="cuda")
    bare = fos.prepare(P.A)
    assert P.lib.fos_row_weights_bind(_core.ptr(w), bare.h) == UNSUPPORTED
    small = fos.prepare(torch.zeros(100, 4, device="cuda"), torch.zeros(100))
    assert P.lib.fos_row_weights_bind(_core.ptr(w), small.h) == UNSUPPORTED
    got = C.c_void_p(1)
    assert P.lib.fos_row_weights_get(C.byref(got), small.h) == 0 and got.value is None
    assert P.lib.fos_row_weights_bind(None, small.h) == 0          # detaching is always served
