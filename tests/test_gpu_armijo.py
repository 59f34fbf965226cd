"""GPU: every Armijo trial quantity per candidate against the longdouble reference of tests/_armijo.py.

fista(backtracking=True) accepts a step from seven numbers per candidate (gd, dd, nnz, gnorm2, y2, q, rr_y).  fista_trial_kernel,
fista_trial_batch_kernel and fista_trial_batch_bf16_kernel produce them, fold_partials_kernel folds their partials, one pass
over A adds q, and iterative_solvers._armijo_accepts / armijo_decide_kernel apply the same three clauses.  Here each number is
compared on its own, through fos_fista_trial / fos_fista_trial_batch / fos_fista_run_backtracking as they are:

  a  trial_batch for nv in 1, 5, 16 and eta in 0.5, 0.7 with t = ||y|| / ||g||, the gradient the pass left read back and handed
     to the reference: the four sums to their derived bounds, nnz exactly (no coordinate of the reference within 1e-6 of its
     threshold), q to the fp32-pass bound, rr_y == status().rr bit for bit, entry 7 of every row 0.0;
  b  trial at t eta^j against the reference and against row j of trial_batch; without the residual pass q == 0.0 and the
     other six fields are bitwise those of the call with it;
  c  an injected exact gradient (dyadic rationals, fp32 gbuf and fp64 gbuf64): nnz is the count known in advance for all 16
     candidates, with coordinates exactly on their thresholds and one grid step either side;
  d  the device decision: run_backtracking(1) on one handle against decide() on the rows trial_batch gives its twin -
     accept at j = 0, at 0 < j < 16, by nnz = 0, by the noise ball alone, and the stall;
  e  eight device-driven iterations against the host loop on the twin: shrink counts, steps and iterates bitwise.

Every case asserts its route from plan() and that trial_batch / run_backtracking are served exactly where path == 0 and the
plan is not the row-per-thread one.  A is borrowed as it is from a NaN-filled allocation (strided, ragged or compact rows), b
and x0 sit between NaN, so a read outside an operand fails instead of passing.  The largest error / bound per field and
shape is in profiles/armijo/README.md (FOS_ARMIJO_RATIOS=<file> writes the table of a run)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import _armijo as ar
from tests.test_gpu_kernel_menu import _np, _vec

pytestmark = pytest.mark.gpu

PAD = 64                                   # NaN elements before and after A
RATIOS = {}                                # (entry point, shape, field) -> largest error / bound seen


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    yield f
    path = os.environ.get("FOS_ARMIJO_RATIOS")
    if path:
        with open(path, "w") as fh:
            json.dump([dict(entry=k[0], shape=k[1], field=k[2], ratio=v) for k, v in sorted(RATIOS.items())], fh, indent=1)


def _store(A64, dtype, layout):
    """The device view of A inside a NaN-filled allocation: rows of lda = n (compact), n + 2 chunks (strided), n + 1 (ragged)."""
    m, n = A64.shape
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    lda = n + {"compact": 0, "strided": 16 if dtype == "bf16" else 8, "ragged": 1}[layout]
    buf = torch.full((2 * PAD + m * lda,), float("nan"), dtype=tdt, device="cuda")
    view = buf[PAD: PAD + m * lda].view(m, lda)[:, :n]
    view.copy_(torch.as_tensor(np.array(A64)).to(tdt))
    assert torch.equal(view.to(torch.float64).cpu(), torch.as_tensor(np.array(A64)))          # the stored A is the reference's
    return view


def _served(c, plan):
    return plan["path"] == 0 and not (plan["tall"] and c["n"] <= 64)


def _open(fos, shape, prm, source, x0, tau, handles=1):
    """The problem of a shape on its asserted route and `handles` fresh handles at x0."""
    from fastoptsolver_amd import _core, _lib
    c = ar.SHAPES[shape]
    A64, b, _, _ = ar.problem(shape)
    A = _store(A64, c["dtype"], c["layout"])
    prob = fos.prepare(A, _vec(np.array(b)), pad=False)
    assert prob.n_dev == c["n"] and prob.A.data_ptr() == A.data_ptr()                # borrowed as it is
    plan = prob.plan()
    assert {k: plan[k] for k in c["route"]} == c["route"], (shape, plan)
    assert _served(c, plan) == c["batch"], (shape, plan)
    hs = []
    for _ in range(handles):
        f = _core.Fista(prob)
        f.reset(tau, prm["alpha1"], prm["alpha2"], prox_kind=_lib.PROX_ENET if prm["prox"] == "enet" else _lib.PROX_L1,
                x0=_vec(np.array(x0), torch.float64))
        if source == "f64":
            f.set_precise(True, own_buffer=True)
        hs.append(f)
    return prob, hs


def _gradient(f, source):
    """The gradient the last grad() left, as the trial kernels read it."""
    n = f.prob.n_dev
    return _np(f.gbuf64[:n]) if source == "f64" else _np(f.prob.gbuf[:n])


def _inject(f, source, g):
    n = f.prob.n_dev
    if source == "f64":
        f.gbuf64[:n] = torch.as_tensor(g, dtype=torch.float64)
    else:
        f.prob.gbuf[:n] = torch.as_tensor(g, dtype=torch.float32)
    torch.cuda.synchronize()
    assert np.array_equal(_gradient(f, source), g)


def _at_state(f, state, source):
    """Bring a fresh handle to `state` and run the gradient pass there: (x_cur, x_prev, beta, g, rr)."""
    xs = [_np(f.x_tensor())]
    if state == "three":
        for _ in range(3):
            f.grad()
            f.update()
            xs.append(_np(f.x_tensor()))
    x_cur, x_prev = xs[-1], xs[-2] if len(xs) > 1 else xs[-1]
    beta = float(f.status().beta)
    if state == "three":
        assert beta > 0.0 and not np.array_equal(x_cur, x_prev)
    f.grad()
    st = f.status()
    assert float(st.beta) == beta
    return x_cur, x_prev, beta, _gradient(f, source), float(st.rr)


def _batch(f, t, eta, nv):
    """fos_fista_trial_batch as it answers: [dict of the seven fields] (entry 7 of every row checked), or None."""
    from fastoptsolver_amd import _lib
    out = (C.c_double * (8 * nv))(*([float("nan")] * (8 * nv)))
    with f.prob.ctx():
        rc = f.lib.fos_fista_trial_batch(f.h, float(t), float(eta), int(nv), out)
    if not _lib.served(rc, "fos_fista_trial_batch"):
        return None
    a = np.array(out).reshape(nv, 8)
    assert np.array_equal(a[:, 7], np.zeros(nv)) and not np.signbit(a[:, 7]).any(), a[:, 7]
    return [dict(zip(ar.FIELDS, (float(v) for v in a[j, :7]))) for j in range(nv)]


def _note(entry, shape, field, ratio):
    key = (entry, shape, field)
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(ratio))


def _compare(entry, shape, where, got, ref, bnd, qb, j, rr, with_q=True):
    """One row of a trial call against candidate j of the reference."""
    want = ref["rows"][j]
    assert all(np.isfinite(got[k]) for k in ar.FIELDS), (where, j, got)
    for k in ar.SUMS:
        err = abs(float(ar.LD(got[k]) - want[k]))
        _note(entry, shape, k, err / bnd[j][k])
        print(f"armijo {entry} {where} j={j} {k}: got {got[k]!r} err {err:.3e} bound {bnd[j][k]:.3e}")
        assert err <= bnd[j][k], (where, j, k, got[k], float(want[k]), err, bnd[j][k])
    assert got["nnz"] == want["nnz"], (where, j, got["nnz"], want["nnz"])
    if with_q:
        err = abs(got["q"] - want["q"])
        _note(entry, shape, "q", err / qb[j])
        print(f"armijo {entry} {where} j={j} q: got {got['q']!r} err {err:.3e} bound {qb[j]:.3e}")
        assert err <= qb[j], (where, j, "q", got["q"], want["q"], err, qb[j])
    assert got["rr_y"] == rr, (where, j, got["rr_y"], rr)                           # bit for bit what the pass left


def _reference(shape, state, prm, t, eta):
    """(ref, bounds, q bounds) of 16 candidates; the thresholds separate the coordinates and none sits within NEAR of one."""
    A64 = ar.problem(shape)[0]
    x_cur, x_prev, beta, g, _ = state
    ref = ar.reference(A64, x_cur, x_prev, beta, g, prm, t, eta, ar.NV)
    if prm["alpha1"] > 0:
        near = ar.near_threshold(ref, prm)
        assert sum(r[0] for r in near) >= 1 and sum(r[1] for r in near) >= 1, (shape, near)
        assert min(r[2] for r in near) > ar.NEAR, (shape, near)
    return ref, ar.bounds(ref, x_cur, x_prev, beta, prm), ar.q_bounds(A64, ref)


def _cell(fos, cell):
    shape, prox, state, source = cell
    prm = ar.params(shape, prox)
    prob, (f,) = _open(fos, shape, prm, source, ar.problem(shape)[2], ar.step_for(shape, prm))
    st = _at_state(f, state, source)
    y = st[0] + st[2] * (st[0] - st[1])
    t = float(np.linalg.norm(y) / np.linalg.norm(st[3]))
    return prob, f, prm, st, t


_CELL_IDS = ["-".join(c) for c in ar.cells()]


# ---- a. trial_batch against the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ar.cells(), ids=_CELL_IDS)
def test_trial_batch_against_the_reference(fos, cell):
    shape = cell[0]
    prob, f, prm, st, t = _cell(fos, cell)
    if not ar.SHAPES[shape]["batch"]:
        assert _batch(f, t, 0.5, ar.NV) is None and f.run_backtracking(1, 0.5, ar.ARMIJO_C, ar.GRAD_EPS[cell[3]]) is None
        return
    for eta in ar.ETAS:
        ref, bnd, qb = _reference(shape, st, prm, t, eta)
        for nv in ar.NVS:
            rows = _batch(f, t, eta, nv)
            assert rows is not None and len(rows) == nv, cell
            for j in range(nv):
                _compare("trial_batch", shape, (cell, eta, nv), rows[j], ref, bnd, qb, j, st[4])
            assert float(f.status().rr) == st[4]
    torch.cuda.synchronize()


# ---- b. trial against the reference and against trial_batch ---------------------------------------------------------------
@pytest.mark.parametrize("cell", ar.cells(), ids=_CELL_IDS)
def test_trial_against_the_reference_and_the_batch(fos, cell):
    shape = cell[0]
    prob, f, prm, st, t = _cell(fos, cell)
    for eta in ar.ETAS:
        ref, bnd, qb = _reference(shape, st, prm, t, eta)
        rows = _batch(f, t, eta, ar.NV)
        assert (rows is not None) == ar.SHAPES[shape]["batch"], cell
        for j in (0, 3, 15):
            tj = ref["t"][j]
            one = f.trial(tj, with_residual=True)
            _compare("trial", shape, (cell, eta), one, ref, bnd, qb, j, st[4])
            bare = f.trial(tj, with_residual=False)
            assert bare["q"] == 0.0 and not np.signbit(bare["q"]), (cell, j, bare)
            assert all(np.float64(bare[k]).tobytes() == np.float64(one[k]).tobytes() for k in ar.FIELDS if k != "q"), (cell, j, bare, one)
            if rows is not None:
                for k in ar.SUMS:
                    assert abs(one[k] - rows[j][k]) <= 2.0 * bnd[j][k], (cell, eta, j, k, one[k], rows[j][k])
                assert abs(one["q"] - rows[j]["q"]) <= 2.0 * qb[j], (cell, eta, j, one["q"], rows[j]["q"])
                assert one["nnz"] == rows[j]["nnz"] and one["rr_y"] == rows[j]["rr_y"]
    torch.cuda.synchronize()


# ---- c. injected exact gradient -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ar.SOURCES)
@pytest.mark.parametrize("prox", list(ar.EXACT_PROX))
@pytest.mark.parametrize("shape", ar.DECISION_SHAPES)
def test_injected_exact_gradient(fos, shape, prox, source):
    c = ar.SHAPES[shape]
    A64 = ar.problem(shape)[0]
    y, g, prm, classes = ar.exact_inputs(c["n"], prox)
    counts = ar.exact_counts(y, g, prm)
    prob, (f,) = _open(fos, shape, prm, source, y, 1.0)
    f.grad()
    rr = float(f.status().rr)
    _inject(f, source, g)
    ref = ar.reference(A64, y, y, 0.0, g, prm, ar.EXACT_T, ar.EXACT_ETA, ar.NV)
    assert [r["nnz"] for r in ref["rows"]] == counts
    bnd, qb = ar.bounds(ref, y, y, 0.0, prm), ar.q_bounds(A64, ref)
    assert float(f.status().beta) == 0.0 and np.array_equal(_np(f.x_tensor()), y)
    # entries at 2^-20 of the largest entry of every candidate (bf16 storage: the three-term split has to keep them)
    D = np.abs(ref["D32"])
    assert (D[classes["above"]].max(axis=0) <= 2.0 ** -20 * D.max(axis=0)).all() and (D[classes["above"]] > 0).all()
    rows = _batch(f, ar.EXACT_T, ar.EXACT_ETA, ar.NV)
    assert (rows is not None) == c["batch"]
    for j in range(ar.NV):
        if rows is not None:
            assert rows[j]["nnz"] == counts[j], (shape, prox, source, j, rows[j]["nnz"], counts[j])
            _compare("trial_batch", shape, (shape, prox, source, "exact"), rows[j], ref, bnd, qb, j, rr)
        if rows is None or j in (0, ar.EXACT_TIE_AT, 15):
            one = f.trial(ref["t"][j])
            assert one["nnz"] == counts[j], (shape, prox, source, j, one["nnz"], counts[j])
            _compare("trial", shape, (shape, prox, source, "exact"), one, ref, bnd, qb, j, rr)
    torch.cuda.synchronize()


# ---- d. the device decision -----------------------------------------------------------------------------------------------
def _decide_on_device(f, iters, eta, grad_eps):
    """fos_fista_run_backtracking into sentinel-filled outputs: (ls, tau_hist) as host arrays, or None."""
    from fastoptsolver_amd import _core, _lib
    ls = torch.full((iters,), -7, dtype=torch.int32, device="cuda")
    taus = torch.full((iters,), float("nan"), dtype=torch.float64, device="cuda")
    with f.prob.ctx():
        rc = f.lib.fos_fista_run_backtracking(f.h, iters, float(eta), ar.ARMIJO_C, float(grad_eps), _core.ptr(ls), _core.ptr(taus))
    if not _lib.served(rc, "fos_fista_run_backtracking"):
        return None
    torch.cuda.synchronize()
    return ls.cpu().numpy(), taus.cpu().numpy()


DECISIONS = {      # name -> (prox, eta, tau L, what decide() has to say about handle 1's rows)
    "first": ("l1_ridge", 0.5, 1.0, lambda j, clause: j == 0 and clause == "excess"),
    "shrunk": ("l1_ridge", 0.7, 32.0, lambda j, clause: j is not None and 0 < j < 16 and clause == "excess"),
    "nnz": ("l1", 0.5, 2.0 ** 20, lambda j, clause: j == 0 and clause == "nnz"),
    "stall": ("l1_ridge", 0.7, 2.0 ** 24, lambda j, clause: j is None and clause == "stall"),
    "ball": ("l1", 0.5, None, lambda j, clause: j == 0 and clause == "ball"),
}


@pytest.mark.parametrize("source", ar.SOURCES)
@pytest.mark.parametrize("case", list(DECISIONS))
@pytest.mark.parametrize("shape", ar.DECISION_SHAPES)
def test_device_decision(fos, shape, case, source):
    from fastoptsolver_amd import _lib
    prox, eta, tau_l, expected = DECISIONS[case]
    A64, b, x0, L = ar.problem(shape)
    n, grad_eps = A64.shape[1], ar.GRAD_EPS[source]
    prm = dict(ar.params(shape, prox))
    tau = ar.ball_tau(L, source) if case == "ball" else tau_l / L
    if case in ("nnz", "ball"):
        x0 = np.zeros(n)
        prm["alpha1"] = 1.01 * float(np.max(np.abs(A64.T @ b.astype(np.float64))))
    if case == "ball":                   # alpha1 a few ulps below max |g| of the gradient the device itself leaves
        _, (probe,) = _open(fos, shape, prm, source, x0, tau)
        probe.grad()
        prm["alpha1"] = ar.ball_alpha1(_gradient(probe, source), source)
        del probe
    prob, (h1, h2) = _open(fos, shape, prm, source, x0, tau, handles=2)
    a2s = ar.smooth_a2(prm)
    h1.grad()
    rows = _batch(h1, tau, eta, ar.NV)
    j, tj, clause = ar.decide(rows, tau, eta, a2s, ar.ARMIJO_C, grad_eps)
    assert expected(j, clause), (shape, case, source, j, clause, rows)
    if case == "ball":                   # the only true clause of the accepted row
        assert rows[0]["nnz"] == 1.0 and ar.clauses(rows[0], tau, a2s, ar.ARMIJO_C, grad_eps) == dict(nnz=False, excess=False, ball=True)
    if case == "nnz":
        assert rows[0]["dd"] == 0.0 and rows[0]["q"] == 0.0
    k0 = int(h2.status().k)
    out = _decide_on_device(h2, 1, eta, grad_eps)
    assert out is not None
    ls, taus = out
    s2 = h2.status()
    if case == "stall":
        assert s2.stopped == _lib.STOP_LS_STALL and int(s2.k) == k0 == 0
        assert float(s2.tau) == tj == ar.steps(tau, eta, ar.NV + 1)[ar.NV]
        assert ls[0] == -7 and np.isnan(taus[0])
        assert np.array_equal(_np(h2.x_tensor()), x0)
        return
    assert s2.stopped == _lib.STOP_NONE and int(s2.k) == k0 + 1
    assert ls[0] == j and taus[0] == tj and float(s2.tau) == tj, (shape, case, source, ls, taus, float(s2.tau), j, tj)
    h1.set_tau(tj)
    h1.update()
    x1, x2 = h1.x_tensor(), h2.x_tensor()
    assert torch.equal(x1, x2), (shape, case, source, float((x1 - x2).abs().max()))
    if case == "ball":
        assert int(torch.count_nonzero(x2)) == 1
    if case == "nnz":
        assert int(torch.count_nonzero(x2)) == 0


# ---- e. eight iterations --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ar.SOURCES)
@pytest.mark.parametrize("shape", ar.EIGHT_SHAPES)
def test_eight_device_driven_iterations_equal_the_host_loop(fos, shape, source):
    from fastoptsolver_amd import _lib
    iters, eta, grad_eps = 8, 0.5, ar.GRAD_EPS[source]
    A64, b, x0, L = ar.problem(shape)
    prm = ar.params(shape, "l1_ridge")
    tau = 8.0 / L
    prob, (h1, h2) = _open(fos, shape, prm, source, x0, tau, handles=2)
    a2s = ar.smooth_a2(prm)
    ls_host, taus_host, t = [], [], tau
    for _ in range(iters):
        h1.grad()
        rows = _batch(h1, t, eta, ar.NV)
        j, t, clause = ar.decide(rows, t, eta, a2s, ar.ARMIJO_C, grad_eps)
        assert j is not None, (shape, source, clause)
        h1.set_tau(t)
        h1.update()
        ls_host.append(j)
        taus_host.append(t)
    assert ls_host[0] > 0                                                        # the search did shrink
    ls, taus = _decide_on_device(h2, iters, eta, grad_eps)
    s2 = h2.status()
    assert s2.stopped == _lib.STOP_NONE and int(s2.k) == iters
    assert ls.tolist() == ls_host, (shape, source, ls.tolist(), ls_host)
    assert taus.tolist() == taus_host and float(s2.tau) == taus_host[-1], (shape, source, taus.tolist(), taus_host)
    assert torch.equal(h1.x_tensor(), h2.x_tensor()), (shape, source)
