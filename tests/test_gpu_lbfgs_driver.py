"""GPU: every exit and branch of the two native L-BFGS drivers (fos_lbfgs_minimize, fos_lbfgs_minimize_multi) on the cases of
tests/_lbfgs_cases.py, whose routes the oracle takes whatever the order of summation (tests/test_lbfgs_driver_cases.py) - so
the device run must take them too: the same (nit, nfev, task), iterates to 1e-5, and on the exits that restore the start point
the start point bit for bit.  Through LBFGSSolver.fit and, where the Python layer hides a form (NULL record buffers, a start
point, the extent of what is written), through the raw ABI with NaN guards behind every buffer.

These rows of tests/_menu_lbfgs.py have no entry point of their own and are reached here: stamp_kernel,
lbfgs_first_trial_kernel, lbfgs_store_pair_kernel and the *_multi kernels.

Branches of the drivers that no input found reaches (the oracle searched 400 seeded problems on the CPU - shapes (300, 64),
(200, 33), (60, 80), (40, 12), column scales 1 .. 10^(+-3), a2 in {0, 1e-4, 1e-3, 0.5}, b times 1e-8 .. 1e30 - and met
neither):
  - the memory drop with hist_n > 0 after gd0 >= 0 (L-BFGS-B info = -4): with pairs that all passed the curvature test H is
    positive definite and d = -H g descends; only rounding in an ill-conditioned H could turn g.d non-negative;
  - the rejected curvature pair (s.y <= eps * (-g.d) * stp): on a convex quadratic s.y = s^T (A^T A + a2) s > 0 by the size of
    the step, and the Wolfe condition of an accepted step keeps it far above eps times the slope.
Both stay covered by the CPU comparison of the line search and by reading; they are not executed on the device."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _data, _lbfgs_cases as lc, _menu_lbfgs as ml

pytestmark = pytest.mark.gpu

TOL = 1e-5                    # device run against the oracle (tests/test_gpu_parity.py)
SAME = 1e-9                   # lockstep column against its single fit (tests/test_gpu_lbfgs_multi.py)
NAN = float("nan")
GUARD = 8                     # NaN doubles behind a host record buffer


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def _device_A(A32, kind):
    return torch.as_tensor(A32).to(torch.bfloat16 if kind == "bf16" else torch.float32).cuda()


def _problem(fos, c):
    A32, A64, b32, x0 = lc.data(c)
    prob = fos.prepare(_device_A(A32, c["kind"]), b32, pad=False)
    assert prob.n_dev == c["n"], (c["name"], prob.n_dev)          # the length the driver dispatches on
    return prob, A64, b32, x0


def _solver(c):
    from fastoptsolver_amd.lbfgs import LBFGSSolver
    return LBFGSSolver("ridge", 0.0, c["a2"], max_iter=c["max_iter"], tol=c["tol"])


def _nan_host(count):
    buf = (C.c_double * count)()
    for i in range(count):
        buf[i] = NAN
    return buf


def _raw(prob, c, x0=None, hist=True, iterates=True, fg_ms=True, max_iter=None):
    """fos_lbfgs_minimize through the raw ABI.  hist: 2*max_iter doubles + GUARD NaN; iterates: max_iter*n doubles inside
    NaN guards on the device; both start as NaN.  Returns dict(x, res, hist (list), hist_guard_ok, iterates (tensor view),
    iter_guard_ok)."""
    from fastoptsolver_amd import _core, _lib
    n = c["n"]
    mi = c["max_iter"] if max_iter is None else max_iter
    x = torch.zeros(n, dtype=torch.float64, device="cuda") if x0 is None else torch.as_tensor(x0, dtype=torch.float64).cuda()
    hbuf = _nan_host(2 * mi + GUARD)
    pad = 64
    ibuf = torch.full((pad + mi * n + max(pad, n),), NAN, dtype=torch.float64, device="cuda")    # a stray row lands in the guard
    iview = ibuf[pad: pad + mi * n]
    cap = 21 * max(mi, 1) + 2
    ms = (C.c_float * cap)()
    res = _lib.LbfgsResult()
    with prob.ctx():
        rc = prob.lib.fos_lbfgs_minimize(prob.h, float(c["a2"]), mi, float(c["tol"]), _core.ptr(x),
                                         hbuf if hist else None,
                                         C.c_void_p(ibuf[pad:].data_ptr()) if iterates else None,
                                         ms if fg_ms else None, cap if fg_ms else 0, C.byref(res))
    _lib.check(rc, "fos_lbfgs_minimize")
    torch.cuda.synchronize()
    h = list(hbuf)
    return dict(x=x, res=(res.nit, res.nfev, res.task, res.f, res.gmax), hist=h[: 2 * mi],
                hist_guard_ok=all(v != v for v in h[2 * mi:]), iterates=iview.view(mi, n) if mi else iview,
                iter_guard_ok=bool(torch.isnan(ibuf[:pad]).all() and torch.isnan(ibuf[pad + mi * n:]).all()),
                fg_ms=[ms[i] for i in range(min(res.nfev, cap))])


# ---- every case through LBFGSSolver.fit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in lc.CASES if c["x0"] is None])
def test_fit_takes_the_oracles_route(fos, name):
    c = lc.BY_NAME[name]
    prob, A64, b32, _ = _problem(fos, c)
    ref = lc.oracle(c, A64, b32)
    s = _solver(c).fit(prob, None)
    got = (s.nit_, s.nfev_, lc.TASKS.index(s.task_))
    assert got == (ref["nit"], ref["nfev"], ref["task"]), (name, got, (ref["nit"], ref["nfev"], ref["task"]))
    x = _np(s.x_)
    assert len(s.history_) == s.nit_ and len(s.iterates_) == s.nit_, (name, len(s.history_), len(s.iterates_))
    assert fos.get_metrics()["grad_num_calls"] == s.nfev_
    if ref["task"] == 3:
        # the line search gave up after MAXLS = 20 evaluations with no pair to drop: x is restored from x_old, bit for bit
        assert s.nfev_ <= 21 and not x.any() and np.array_equal(x, np.zeros(c["n"])), name
        return
    assert np.isfinite(x).all() and _data.rel(x, ref["x"]) < TOL, (name, _data.rel(x, ref["x"]))
    for k in range(ref["nit"]):
        assert _data.rel(_np(s.iterates_[k]), ref["iterates"][k]) < TOL, (name, k)
    assert s.final_obj_ == pytest.approx(ref["f"], rel=1e-6, abs=1e-300), name
    if c["max_iter"] <= 1:
        assert got == (1, 3, 2) and len(s.history_) == 1 and len(s.iterates_) == 1, (name, got)   # SciPy's maxiter = 0 and 1
        assert s.history_[0] == pytest.approx(ref["f"], rel=1e-6), name


# ---- what the raw ABI writes, and the NULL forms ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,max_iter", [("div64-iter0", 0), ("div64-iter1", 1), ("n2048-b1e4", 0), ("ragged33-b1e4", 0)])
def test_nothing_is_written_beyond_max_iter_records(fos, name, max_iter):
    """hist holds 2*max_iter doubles and iterates max_iter*n: max_iter = 0 runs one iteration (SciPy's maxiter = 0) and records
    nothing - it used to write hist[0], hist[1] and one row of iterates past buffers of no length."""
    c = lc.BY_NAME[name]
    prob, A64, b32, _ = _problem(fos, c)
    ref = lc.oracle(dict(c, max_iter=max_iter), A64, b32)
    r = _raw(prob, c, max_iter=max_iter)
    assert r["res"][:3] == (ref["nit"], ref["nfev"], ref["task"]) and r["res"][0] == 1 and r["res"][2] == 2, (name, r["res"])
    assert r["hist_guard_ok"], (name, "hist written beyond 2*max_iter doubles")
    assert r["iter_guard_ok"], (name, "iterates written beyond max_iter*n doubles")
    assert _data.rel(_np(r["x"]), ref["x"]) < TOL, name
    if max_iter == 1:
        assert r["hist"][0] == pytest.approx(ref["f"], rel=1e-6) and r["hist"][1] == pytest.approx(float(np.abs(ref["x"]).sum()), rel=1e-6)
        assert torch.equal(r["iterates"][0], r["x"]), name
    other = _raw(prob, c, max_iter=1 - max_iter if max_iter <= 1 else max_iter)       # 0 and 1 are the same run
    assert torch.equal(other["x"], r["x"]) and other["res"] == r["res"], name


@pytest.mark.parametrize("name", ["div64-b1e4", "ragged33-b1e4", "n2048-b1e8", "n2049-b1e4"])
def test_null_record_buffers_change_nothing(fos, name):
    """hist, iterates and fg_ms each NULL in turn: x and the result record are bitwise those of the fully recorded call (and
    the recorded call is LBFGSSolver.fit's).  With fg_ms the evaluations are timed (stamp_kernel or the pass's own stamp)."""
    c = lc.BY_NAME[name]
    prob, A64, b32, _ = _problem(fos, c)
    ref = lc.oracle(c, A64, b32)
    full = _raw(prob, c)
    assert full["res"][:3] == (ref["nit"], ref["nfev"], ref["task"]), (name, full["res"])
    assert full["hist_guard_ok"] and full["iter_guard_ok"], name
    nit = full["res"][0]
    assert np.isfinite(full["hist"][: 2 * nit]).all() and all(v != v for v in full["hist"][2 * nit:]), name
    assert torch.isfinite(full["iterates"][:nit]).all() and torch.isnan(full["iterates"][nit:]).all(), name
    assert torch.equal(full["iterates"][nit - 1], full["x"]), name
    for k in range(nit):
        assert _data.rel(_np(full["iterates"][k]), ref["iterates"][k]) < TOL, (name, k)
    assert len(full["fg_ms"]) == full["res"][1] and all(0.0 <= t < 1e3 for t in full["fg_ms"]), (name, full["fg_ms"])
    for off in ("hist", "iterates", "fg_ms"):
        r = _raw(prob, c, **{off: False})
        assert torch.equal(r["x"], full["x"]) and r["res"] == full["res"], (name, off, r["res"], full["res"])
        assert r["hist_guard_ok"] and r["iter_guard_ok"], (name, off)
        if off == "hist":
            assert all(v != v for v in r["hist"]), name
        if off == "iterates":
            assert torch.isnan(r["iterates"]).all(), name
    s = _solver(c).fit(prob, None)
    assert np.array_equal(_np(s.x_), _np(full["x"].to(s.x_.dtype))), name         # x_ comes back in the caller's type


@pytest.mark.parametrize("name", ["div64-b1e4", "n2048-b1e4", "ragged33-ring"])
def test_a_handle_is_reusable_after_any_fit(fos, name):
    """LbfgsWork is kept on the handle: a second fit, and a fit after one that failed its line search (task 3: from a start
    point of the order of 1e20 the first search takes its 20 evaluations and gives up), are bitwise fits on a fresh handle."""
    c = lc.BY_NAME[name]
    prob, A64, b32, _ = _problem(fos, c)
    fresh = _raw(prob, c)
    again = _raw(prob, c)
    assert torch.equal(again["x"], fresh["x"]) and again["res"] == fresh["res"], name
    assert torch.equal(again["iterates"], fresh["iterates"]) or fresh["res"][0] < c["max_iter"], name
    far = np.random.default_rng(3).standard_normal(c["n"]) * 1e20
    ref = lc.oracle(c, A64, b32, far)
    assert (ref["nit"], ref["nfev"], ref["task"]) == (0, 21, 3)
    failed = _raw(prob, c, x0=far)
    assert failed["res"][:3] == (0, 21, 3), (name, failed["res"])
    assert np.array_equal(_np(failed["x"]), far), (name, "x is not the start point after the failed search")
    assert all(v != v for v in failed["hist"]) and torch.isnan(failed["iterates"]).all(), name
    after = _raw(prob, c)
    assert torch.equal(after["x"], fresh["x"]) and after["res"] == fresh["res"], name
    prob2, _, _, _ = _problem(fos, c)
    other = _raw(prob2, c)
    assert torch.equal(other["x"], fresh["x"]) and other["res"] == fresh["res"], name


def test_start_point(fos):
    c = lc.BY_NAME["div64-start"]
    prob, A64, b32, x0 = _problem(fos, c)
    ref = lc.oracle(c, A64, b32, x0)
    r = _raw(prob, c, x0=x0)
    assert r["res"][:3] == (ref["nit"], ref["nfev"], ref["task"]), r["res"]
    assert _data.rel(_np(r["x"]), ref["x"]) < TOL
    for k in range(ref["nit"]):
        assert _data.rel(_np(r["iterates"][k]), ref["iterates"][k]) < TOL, k
    zero = lc.oracle(c, A64, b32)
    assert _data.rel(ref["iterates"][0], zero["iterates"][0]) > 1e-3          # the start point matters to the run


# ---- the lockstep driver ---------------------------------------------------------------------------------------------------
def _group_solver(max_iter=lc.GROUP_MAX_ITER):
    from fastoptsolver_amd.lbfgs import LBFGSSolver
    return LBFGSSolver("ridge", 0.0, lc.GROUP_A2, max_iter=max_iter, tol=lc.GROUP_TOL)


@pytest.mark.parametrize("name", list(lc.GROUPS))
def test_lockstep_columns_take_their_own_exits(fos, name):
    """One call, columns that stop at once (zero), search for 10+ evaluations (1e8), fail their search (1e20), and ordinary
    ones: each equals its single fit in counts and task and in x to SAME, and the oracle in counts; twins are bitwise equal."""
    gdef = lc.GROUPS[name]
    A32, A64, B, roles = lc.group(**gdef)
    n, nv = gdef["n"], gdef["nv"]
    P = fos.prepare(_device_A(A32, "f32"))
    assert P.n_dev == n and ml.driver_direction(n) == ("chip" if n >= ml.CHIP_MIN_N else 1)
    P.profile(1)
    P.profile_read()
    s = _group_solver().fit(P, B)
    _, launches = P.profile_read()
    P.profile(0)
    rounds = fos.get_metrics()["grad_num_calls"]
    assert launches == 2 * rounds and rounds >= int(np.max(s.nfev_)), (name, launches, rounds)      # the lockstep driver ran
    X = _np(s.x_)
    c = dict(a2=lc.GROUP_A2, max_iter=lc.GROUP_MAX_ITER, tol=lc.GROUP_TOL, n=n)
    for j, role in enumerate(roles):
        ref = lc.oracle(c, A64, B[:, j])
        got = (int(s.nit_[j]), int(s.nfev_[j]), lc.TASKS.index(s.task_[j]))
        assert got == (ref["nit"], ref["nfev"], ref["task"]), (name, j, role, got)
        one = _group_solver().fit(P.sibling(torch.as_tensor(B[:, j].copy()).cuda()), None)
        assert got == (one.nit_, one.nfev_, lc.TASKS.index(one.task_)), (name, j, role)
        if role in ("zero", "1e20"):
            assert not X[:, j].any(), (name, j, role)
            continue
        assert _data.rel(X[:, j], _np(one.x_)) <= SAME, (name, j, role, _data.rel(X[:, j], _np(one.x_)))
        assert _data.rel(X[:, j], ref["x"]) < TOL, (name, j, role)
        assert len(s.history_[j]) == ref["nit"] and np.allclose(s.history_[j], one.history_, rtol=SAME, atol=0), (name, j)
    twins = [j for j, r in enumerate(roles) if r == "twin"]
    if twins:
        a, b = twins
        assert np.array_equal(X[:, a], X[:, b]) and s.history_[a] == s.history_[b], name
    assert len({t for t in s.task_}) >= (3 if nv >= 16 else 2), s.task_


@pytest.mark.parametrize("name", ["group3-n512", "group16-n2052"])
def test_lockstep_max_iter_zero_records_nothing(fos, name):
    from fastoptsolver_amd import _core, _lib
    gdef = lc.GROUPS[name]
    A32, A64, B, roles = lc.group(**gdef)
    n, nv = gdef["n"], gdef["nv"]
    P = fos.prepare(_device_A(A32, "f32"))
    Bd = torch.as_tensor(B).cuda().contiguous()
    out = {}
    for mi in (0, 1):
        X = torch.zeros(nv, n, dtype=torch.float64, device="cuda")
        hbuf = _nan_host(nv * 2 * mi + GUARD)
        res = (_lib.LbfgsResult * nv)()
        rounds = C.c_int(0)
        with P.ctx():
            rc = P.lib.fos_lbfgs_minimize_multi(P.h, nv, _core.ptr(Bd), nv, lc.GROUP_A2, mi, lc.GROUP_TOL, _core.ptr(X), n, hbuf,
                                                None, 0, C.byref(rounds), res)
        _lib.check(rc, "fos_lbfgs_minimize_multi")
        torch.cuda.synchronize()
        h = list(hbuf)
        assert all(v != v for v in h[nv * 2 * mi:]), (name, mi, "hist written beyond nv * 2*max_iter doubles")
        out[mi] = (X, [(r.nit, r.nfev, r.task) for r in res])
        c = dict(a2=lc.GROUP_A2, max_iter=mi, tol=lc.GROUP_TOL, n=n)
        for j in range(nv):
            ref = lc.oracle(c, A64, B[:, j])
            assert out[mi][1][j] == (ref["nit"], ref["nfev"], ref["task"]), (name, mi, j, out[mi][1][j])
            if mi == 1 and ref["nit"] == 1:
                assert h[j * 2] == pytest.approx(ref["f"], rel=1e-6), (name, j)
    assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1], name
