"""GPU: on a logistic problem every entry point filed under "refuses" in tests/_logit_guard.py returns FOS_ERR_UNSUPPORTED and
leaves the handles as they were - a squared-loss answer on a logistic problem is the one silent failure the feature could
introduce - and the squared-loss results of an ordinary problem are bitwise those of the commit before the feature
(tests/golden/logit_parent.npz, tests/_logit_golden.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import _data, _logit as lg, _logit_golden as gold, _logit_guard as gd

pytestmark = pytest.mark.gpu

UNSUPPORTED = -4


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


@pytest.fixture(scope="module")
def setup(fos):
    """A logistic problem with three handles that have run five lockstep iterations."""
    from fastoptsolver_amd import _core
    A64, y, _, L = lg.recipe(1001, 200, 9)
    alphas = lg.weights(A64, y)
    P = fos.prepare(torch.as_tensor(A64.astype(np.float32)).cuda(), y, loss="logistic")
    hs = []
    for a1, a2 in alphas:
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


def _calls(P, hs):
    """name -> a call with valid arguments that returns the library's code (through the Python wrapper where one exists: a
    wrapper that raises gives the code in its FosError, one that answers None / False stands for FOS_ERR_UNSUPPORTED)."""
    from fastoptsolver_amd import _core, _lib
    lib, st, dev = P.lib, hs[0], P.device
    n, m = P.n_dev, P.m
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)        # noqa: E731
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)        # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)          # noqa: E731
    ptr = _core.ptr
    keep = dict(x=f32(n), xd=f64(n + 4), g=f32(n + 4), gd=f64(n + 4), X16=f32(n, 16), XD=f64(16, n), GD=f64(16, n), B=f32(m, 3),
                rr=f64(16), S=f64(10, n), Y=f64(10, n), work=f64(4096), hist=f64(64, 4), xh=f64(8, n), h4=f64(8, 4), ls=i32(8),
                taus=f64(8), ms=f32(64), rounds=i32(4))
    done, tau = C.c_int32(0), C.c_double(0.0)
    res, res16 = _lib.LbfgsResult(), (_lib.LbfgsResult * 16)()
    nrounds = C.c_int(0)

    def raised(fn):
        def call():
            try:
                fn()
            except _lib.FosError as e:
                assert "code -4" in str(e) and "logistic" in str(e), str(e)
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
    P, hs = setup
    before = _snapshot(hs)
    keep, calls = _calls(P, hs)
    assert set(calls) == gd.REFUSES, set(calls) ^ gd.REFUSES
    for name in sorted(calls):
        rc = calls[name]()
        assert rc == UNSUPPORTED, (name, rc, P.lib.fos_last_error().decode())
        assert name in P.lib.fos_last_error().decode(), (name, P.lib.fos_last_error().decode())
    # fos_residual_batch serves use_b = 1 and refuses use_b = 0
    with pytest.raises(fos.FosError, match="code -4"):
        P.residual_batch(keep["X16"][:, :3], use_b=False)
    assert len(P.residual_batch(keep["X16"][:, :3], use_b=True)) == 3
    torch.cuda.synchronize()
    after = _snapshot(hs)
    for (x0, s0), (x1, s1) in zip(before, after):
        assert torch.equal(x0, x1) and s0 == s1, (s0, s1)
    # and the handles still run
    from fastoptsolver_amd import _core
    assert _core.run_multi(hs, 2) and all(int(st.status().k) == 7 for st in hs)


def test_public_solvers_fail_with_the_guards_error(fos, setup):
    P, _ = setup
    for call in (lambda: fos.fista(P, None, "lasso", 0.1, 0.0, max_iter=3, L=1.0),
                 lambda: fos.fista_delta(P, None, "lasso", 0.1, 0.0, 3.0, max_iter=3, L=1.0),
                 lambda: fos.LBFGSSolver("ridge", 0.0, 1.0, max_iter=3).fit(P, None)):
        with pytest.raises(fos.FosError, match="logistic"):
            call()


def test_lockstep_refusals_on_a_logistic_problem(fos, setup):
    """The forms the logistic lockstep does not serve are refused as fos_fista_run_multi_folds refuses them; a sharded or
    b-less problem cannot become logistic."""
    from fastoptsolver_amd import _core, _lib
    P, _ = setup
    st = _core.Fista(P)
    st.reset(0.01, 0.1, 0.0, tol_grad=1e-3)                        # the gradient-norm rule
    assert _core.run_multi([st], 3) is False and int(st.status().k) == 0
    bare = fos.prepare(P.A)                                        # no b
    assert P.lib.fos_problem_set_loss(bare.h, _lib.LOSS_LOGISTIC) == UNSUPPORTED
    small = fos.prepare(torch.zeros(100, 4, device="cuda"), torch.zeros(100))          # the LDS-resident plan
    assert P.lib.fos_problem_set_loss(small.h, _lib.LOSS_LOGISTIC) == UNSUPPORTED
    out = C.c_int(-1)
    assert P.lib.fos_problem_get_loss(small.h, C.byref(out)) == 0 and out.value == _lib.LOSS_SQUARED
    assert P.lib.fos_problem_get_loss(P.h, C.byref(out)) == 0 and out.value == _lib.LOSS_LOGISTIC
    assert P.lib.fos_problem_set_loss(small.h, _lib.LOSS_SQUARED) == 0
    # loss-free entry points keep working
    assert P.power_iter(np.ones(P.n))[0] > 0 and P.plan()["cus"] > 0


def test_squared_loss_results_are_bitwise_those_of_the_parent_commit(fos):
    want = np.load(os.path.join(_data.GOLDEN, "logit_parent.npz"))
    got = gold.compute(fos, torch)
    assert sorted(got) == sorted(want.files)
    for k in sorted(got):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, float(np.abs(got[k] - want[k]).max()))
