"""GPU: every launchable cell of the multi-vector kernels (tests/_menu_multi.py) against the fp64 oracle on the stored A.

One test per cell (table, dtype, geometry, variant).  The cases are built for the CU count of the device (the row
thresholds of the dispatchers scale with it) and sit at the edges: widths at a tile multiple / the capacity, one chunk
short of it, one chunk past the previous one; one row, fewer rows than a row tile, 1 mod 64, a partial last row split, a
second panel of a few rows; 1..16 vectors.  A is borrowed as it is (pad=False) from a NaN-filled allocation (strided
rows, a column block, compact), the X and B blocks have NaN between and around their columns, so a kernel that reads
outside an operand and masks the value by multiplying with zero fails instead of passing.

What is compared:
  resid cells   ||A X_j - b_j||^2 of residual_batch / residual_batch_rhs / trial_batch per column, to the rr bound of
                _data.fp32_pass_tolerances for that column (column 0 fits its right-hand side to 1e-3: there the absolute
                term of the bound is the one that matters)
  lockstep      ONE iteration of nv handles from x0 with alpha1 = alpha2 = 0 and a step tau_j per handle: x_prev starts equal
                to x0 (fos_fista_reset), so the extrapolation point is x0 and (x0_j - x1_j) / tau_j is the gradient the pass
                produced for column j.  The update (fista_update_body) is carried in fp64 on the fp64 state, so the bound
                is the gradient bound of fp32_pass_tolerances for that column plus a few eps64 (|x0| + |x1|) / tau - no
                fp32 rounding of the update enters.  A second run with alpha1 > 0 (cases marked prox) checks zero pattern,
                signs and values of the prox step away from the threshold.
  dd cells      fos_gemv_pair_dd_multi: gradient and ||r||^2 to 1e-12 relative, and against the single fp64 pass.
Every case asserts the route: the cell is in the set the table's route function gives for (m, n, nv, storage type, CUs),
plan() (path, tall, cluster, geometry, workgroups) and the A-pass launches of profile_read() (one per lockstep iteration
and per residual batch, two per panel of the fp64 pair)."""
import numpy as np
import pytest
import torch

from oracle import fos_oracle as orc
from tests import _data, _menu_multi as mm
from tests.test_gpu_kernel_menu import _matrix, _np, _seed, _vec

pytestmark = pytest.mark.gpu

EPS64 = float(np.finfo(np.float64).eps)
PAD = 64                                   # NaN elements before and after every block


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    yield f
    _matrix.cache_clear()


@pytest.fixture(scope="module")
def cus(fos):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _block(M, ld, dtype=torch.float32):
    """(view of the rows x k block M with row stride ld inside a NaN-filled allocation, the allocation)."""
    rows, k = M.shape
    assert ld >= k
    buf = torch.full((2 * PAD + rows * ld,), float("nan"), dtype=dtype, device="cuda")
    view = buf[PAD: PAD + rows * ld].view(rows, ld)[:, :k]
    view.copy_(torch.as_tensor(np.ascontiguousarray(M), dtype=dtype))
    return view, buf


def _problem(fos, row, c, b=None):
    A, A64 = _matrix(row["dtype"], c["m"], c["n"], c["layout"])
    prob = fos.prepare(A, None if b is None else _vec(b), pad=False)
    assert prob.n_dev == c["n"] and prob.A.data_ptr() == A.data_ptr()            # borrowed as it is
    return prob, A64


def _cell(row):
    return (row["table"], row["dtype"], row["geometry"], row["variant"])


def _profiled(prob, fn):
    prob.profile(1)
    prob.profile_read()
    out = fn()
    launches = prob.profile_read()[1]
    prob.profile(0)
    return out, launches


def _fit_column(A64, x, rng):
    """A right-hand side that x fits to 1e-3 per row (fp32)."""
    return (A64 @ x.astype(np.float64) + 1e-3 * rng.standard_normal(A64.shape[0])).astype(np.float32)


# ---- product 1 alone -----------------------------------------------------------------------------------------------------
def _check_resid(fos, row, c, cus, trial):
    from fastoptsolver_amd import _core, _lib
    dtype, m, n, nv, rhs = row["dtype"], c["m"], c["n"], c["nv"], c["rhs"]
    where = (mm.row_id(row), c)
    assert _cell(row) in mm.resid_cells(dtype, m, cus, rhs), (where, cus)
    rng = np.random.default_rng(_seed("resid", m, n, nv, rhs))
    X = (rng.standard_normal((n, nv)) * np.logspace(0, -6, nv)).astype(np.float32)     # candidates shrink like t * eta^j
    X64 = X.astype(np.float64)
    A64 = _matrix(dtype, m, n, c["layout"])[1]
    b = _fit_column(A64, X[:, 0], rng) if rhs == "b" else None
    prob, A64 = _problem(fos, row, c, b)
    plan = prob.plan()
    assert (plan["path"], plan["colblock"], plan["resident"], plan["cus"]) == (0, 0, 0, cus), (where, plan)
    Xd, _ = _block(X, mm.NV_MAX)                                                       # NaN in the slots from nv on
    lib = prob.lib

    def compare(got, Bref, what):
        R = A64 @ X64 - (0.0 if Bref is None else Bref if Bref.ndim == 2 else Bref[:, None])
        rr_ref = (R * R).sum(axis=0)
        _, rr_tol = _data.fp32_pass_tolerances_cols(A64, X64, Bref, np.zeros((n, nv)), rr_ref)
        err = np.abs(np.asarray(got) - rr_ref)
        assert np.isfinite(got).all() and (err <= rr_tol).all(), (where, what, got, rr_ref, float(np.max(err / rr_tol)))

    if rhs == "B":
        Bm = rng.standard_normal((m, nv)).astype(np.float32)
        Bm[:, 0] = _fit_column(A64, X[:, 0], rng)
        Bd, _ = _block(Bm, nv + 3)
        with prob.ctx():
            rc, launches = _profiled(prob, lambda: lib.fos_residual_batch_rhs(prob.h, _core.ptr(Xd), nv, _core.ptr(Bd), int(Bd.stride(0)),
                                                                              _core.ptr(prob.scratch)))
        _lib.check(rc, "fos_residual_batch_rhs")
        assert launches == 1, (where, launches)
        compare(prob.scratch[:nv].cpu().numpy(), Bm.astype(np.float64), "rhs")
    else:
        for use_b in (1, 0):
            with prob.ctx():
                rc, launches = _profiled(prob, lambda: lib.fos_residual_batch(prob.h, _core.ptr(Xd), nv, use_b, _core.ptr(prob.scratch)))
            _lib.check(rc, "fos_residual_batch")
            assert launches == 1, (where, launches)
            compare(prob.scratch[:nv].cpu().numpy(), b.astype(np.float64) if (use_b and b is not None) else None, ("use_b", use_b))
    if trial and rhs == "b":
        # the line-search candidates of one handle: dlt_j = (y - t eta^j g) - y from the pass's own gradient, q_j = ||A dlt_j||^2
        x0 = rng.standard_normal(n).astype(np.float32)
        f = _core.Fista(prob)
        f.reset(1.0, 0.0, 0.0, x0=x0)
        f.grad()
        g = _np(prob.gbuf[:n])
        t, eta = float(np.linalg.norm(x0) / np.linalg.norm(g)), 0.5
        got = f.trial_batch(t, eta, nv)
        assert got is not None, where
        y = x0.astype(np.float64)
        D = np.stack([((y - t * eta ** j * g) - y).astype(np.float32) for j in range(nv)], axis=1).astype(np.float64)
        q_ref = ((A64 @ D) ** 2).sum(axis=0)
        _, q_tol = _data.fp32_pass_tolerances_cols(A64, D, None, np.zeros((n, nv)), q_ref)
        q = np.array([o["q"] for o in got])
        assert np.isfinite(q).all() and (np.abs(q - q_ref) <= q_tol).all(), (where, "trial_batch", q, q_ref)
    del prob
    torch.cuda.synchronize()


# ---- one lockstep iteration ----------------------------------------------------------------------------------------------
def _lockstep_inputs(A64, c, prox):
    """x0 (n x nv, representable in fp32), the right-hand sides, the scale of every column."""
    m, n, nv, rhs = c["m"], c["n"], c["nv"], c["rhs"]
    rng = np.random.default_rng(_seed("lockstep", m, n, nv, rhs, prox))
    if prox:       # magnitudes in [1, 2) or [0.01, 0.02): nothing near the threshold 0.5 before or after a step of a tenth
        u = rng.random((n, nv))
        X0 = np.sign(rng.standard_normal((n, nv))) * np.where(rng.random((n, nv)) < 0.5, 1.0 + u, 0.01 * (1.0 + u))
    else:
        X0 = rng.standard_normal((n, nv))
    # one b for all columns: x0 of very different scales, as the candidates of a line search have
    scale = np.array([1.0 if (rhs == "B" or j % 2 == 0) else 1e-6 for j in range(nv)])
    X0 = (X0 * scale).astype(np.float32)
    b, Bm, zero = None, None, None
    if rhs == "b":
        b = rng.standard_normal(m).astype(np.float32)
    elif rhs == "B":
        Bm = rng.standard_normal((m, nv)).astype(np.float32)
        if nv >= 2:                      # a column that must not see its neighbours: x0 = 0, b = 0
            zero = nv // 2
            X0[:, zero] = 0.0
            Bm[:, zero] = 0.0
    return X0, b, Bm, scale, zero


def _run_lockstep(prob, X0, tau, a1, Bd, where):
    from fastoptsolver_amd import _core
    nv = X0.shape[1]
    hs = [_core.Fista(prob) for _ in range(nv)]
    for j, h in enumerate(hs):
        h.reset(float(tau[j]), float(a1[j]), 0.0, x0=X0[:, j])
    run = (lambda: _core.run_multi(hs, 1)) if Bd is None else (lambda: _core.run_multi_rhs(hs, Bd, 1))
    ok, launches = _profiled(prob, run)
    assert ok is True, (where, "the lockstep run was refused")       # any other return code (a cluster member that never arrived) raises
    assert launches == 1, (where, launches)
    xs = [h.x_tensor() for h in hs]
    torch.cuda.synchronize()
    return xs


def _check_lockstep(fos, row, c, cus):
    dtype, m, n, nv, rhs = row["dtype"], c["m"], c["n"], c["nv"], c["rhs"]
    where = (mm.row_id(row), c)
    cluster = row["table"] == "cluster"
    assert _cell(row) in mm.lockstep_cells(dtype, m, n, nv, cus, rhs, cluster), (where, cus)
    A64 = _matrix(dtype, m, n, c["layout"])[1]
    for prox in (False, True) if c["prox"] else (False,):
        X0, b, Bm, scale, zero = _lockstep_inputs(A64, c, prox)
        prob, _ = _problem(fos, row, c, b)
        if row["table"] == "valu":
            th, k, r = c["tune"]
            prob.replan(no_resident=True)
            prob.tune(th, k, r, c["wg"])
            plan = prob.plan()
            assert (plan["path"], plan["tall"], plan["colblock"], plan["resident"]) == (0, 0, 0, 0), (where, plan)
            assert (plan["threads"], plan["chunks"], plan["rows"]) == (th, k, r), (where, plan)
            if c["tail"]:
                assert plan["workgroups"] == c["wg"], (where, plan)
        else:
            if cluster:
                prob.replan(cluster=True)
            plan = prob.plan()
            assert (plan["path"], plan["tall"], plan["colblock"], plan["resident"]) == (0, int(mm.is_tall(dtype, n)), 0, 0), (where, plan)
        assert plan["cus"] == cus, (where, plan)
        Bd = None if Bm is None else _block(Bm, nv + 3)[0]
        X64 = X0.astype(np.float64)
        Bref = None if rhs is None else b.astype(np.float64) if rhs == "b" else Bm.astype(np.float64)
        R = A64 @ X64 - (0.0 if Bref is None else Bref if Bref.ndim == 2 else Bref[:, None])
        G_ref, rr_ref = A64.T @ R, (R * R).sum(axis=0)
        for j in (0, nv - 1):            # the block form is the oracle's gradient, column by column
            gj, rj = orc.gram_gradient(A64, X64[:, j], None if Bref is None else Bref if Bref.ndim == 1 else Bref[:, j])
            assert _data.rel(G_ref[:, j], gj) < 1e-12 and rr_ref[j] == pytest.approx(rj, rel=1e-12)
        g_tol, _ = _data.fp32_pass_tolerances_cols(A64, X64, Bref, G_ref, rr_ref)
        xn, gn = np.linalg.norm(X64, axis=0), np.linalg.norm(G_ref, axis=0)
        live = (xn > 0) & (gn > 0)
        # tau_j ||g_j|| of the order of ||x0_j|| (a tenth of it in the prox run), different for every handle
        tau = np.where(live, xn / np.where(live, gn, 1.0), 1.0) * (0.1 if prox else 1.0) * (1.0 + 0.02 * np.arange(nv))
        thr = 0.5 * scale
        a1 = thr / tau if prox else np.zeros(nv)
        xs = _run_lockstep(prob, X0, tau, a1, Bd, where)
        if cluster:
            assert prob.plan()["cluster"] == 1, (where, prob.plan())
            again = _run_lockstep(prob, X0, tau, a1, Bd, where)            # the flag epochs: a second launch, bitwise equal
            assert all(torch.equal(x, y) for x, y in zip(xs, again)), where
        else:
            assert prob.plan()["cluster"] == 0, (where, prob.plan())
        for j in range(nv):
            x1 = _np(xs[j])
            assert np.isfinite(x1).all(), (where, j)
            if j == zero:
                assert not x1.any(), (where, j, "the zero column moved")
                continue
            slack = 8.0 * EPS64 * float(np.linalg.norm(X64[:, j]) + np.linalg.norm(x1)) / tau[j]
            if not prox:
                err = float(np.linalg.norm((X64[:, j] - x1) / tau[j] - G_ref[:, j]))
                assert err <= g_tol[j] + slack, (where, j, err, float(g_tol[j]), float(gn[j]))
                continue
            v = X64[:, j] - tau[j] * G_ref[:, j]
            margin = tau[j] * (g_tol[j] + slack)
            sure = np.abs(np.abs(v) - thr[j]) > margin
            assert 1.0 - sure.mean() <= 0.01, (where, j, float(1.0 - sure.mean()))
            want = orc.prox_l1(v, thr[j])
            assert 0.2 < np.mean(want == 0.0) < 0.8, (where, j)                       # the threshold separates the two groups
            assert np.array_equal(x1[sure] == 0.0, want[sure] == 0.0), (where, j, "zero pattern")
            assert np.array_equal(np.sign(x1[sure]), np.sign(want[sure])), (where, j, "signs")
            assert float(np.linalg.norm((x1 - want)[sure])) <= margin, (where, j)
        del prob
    torch.cuda.synchronize()


# ---- the fp64 pair -------------------------------------------------------------------------------------------------------
def _check_dd(fos, row, c, cus, with_single):
    from fastoptsolver_amd import _core, _lib
    dtype, m, n, nv = row["dtype"], c["m"], c["n"], c["nv"]
    where = (mm.row_id(row), c)
    assert _cell(row) in mm.dd_cells(dtype, m, cus), (where, cus)
    prob, A64 = _problem(fos, row, c)
    plan = prob.plan()
    assert (plan["path"], plan["colblock"], plan["resident"], plan["cus"]) == (0, 0, 0, cus), (where, plan)
    rng = np.random.default_rng(_seed("dd", m, n, nv))
    X = rng.standard_normal((nv, n)) * (1.0 + 1e-9 * rng.standard_normal((nv, n)))         # not representable in fp32
    Bm = rng.standard_normal((m, nv)).astype(np.float32)
    a2, ldx = 0.7, n + 3
    Xd, _ = _block(X, ldx, torch.float64)
    Bd, _ = _block(Bm, nv + 2)
    Gd, gbuf = _block(np.full((nv, n), np.nan), ldx, torch.float64)
    rbuf = torch.full((2 * PAD + nv,), float("nan"), dtype=torch.float64, device="cuda")
    with prob.ctx():
        rc, launches = _profiled(prob, lambda: prob.lib.fos_gemv_pair_dd_multi(
            prob.h, _core.ptr(Xd), nv, ldx, _core.ptr(Bd), int(Bd.stride(0)), a2, _core.ptr(Gd), _core.ptr(rbuf[PAD:])))
    _lib.check(rc, "fos_gemv_pair_dd_multi")
    torch.cuda.synchronize()
    assert launches == 2 * len(mm.panels(m, cus)), (where, launches)                        # both products of every panel
    full = gbuf[PAD: PAD + nv * ldx].view(nv, ldx)
    assert torch.isnan(gbuf[:PAD]).all() and torch.isnan(gbuf[PAD + nv * ldx:]).all() and torch.isnan(full[:, n:]).all(), where
    assert torch.isnan(rbuf[:PAD]).all() and torch.isnan(rbuf[PAD + nv:]).all(), where
    G, rr = full[:, :n].cpu().numpy(), rbuf[PAD: PAD + nv].cpu().numpy()
    assert np.isfinite(G).all() and np.isfinite(rr).all(), where
    for j in range(nv):
        g_ref, rr_ref = orc.gram_gradient(A64, X[j], Bm[:, j].astype(np.float64), a2)
        assert _data.rel(G[j], g_ref) < 1e-12, (where, j, _data.rel(G[j], g_ref))
        assert rr[j] == pytest.approx(rr_ref, rel=1e-12), (where, j)
    for j in range(min(nv, 2) if with_single else 0):          # the single fp64 pass on the same column
        sib = prob.sibling(torch.as_tensor(Bm[:, j].copy()).cuda())
        out = torch.empty(n + 1, dtype=torch.float64, device="cuda")
        with sib.ctx():
            _lib.check(sib.lib.fos_gemv_pair_dd(sib.h, _core.ptr(torch.as_tensor(X[j]).cuda()), a2, _core.ptr(out)), "fos_gemv_pair_dd")
        ref = out.cpu().numpy()
        assert _data.rel(G[j], ref[:n]) < 1e-12 and abs(rr[j] - ref[n]) <= 1e-12 * ref[n], (where, j)
    del prob
    torch.cuda.synchronize()


@pytest.mark.parametrize("rid", [mm.row_id(r) for r in mm.ROWS])
def test_cell(fos, cus, rid):
    row = {mm.row_id(r): r for r in mm.build(cus)}[rid]
    if row["unreachable"]:
        pytest.skip(row["unreachable"])                       # a device whose CU count shuts the cell out (not an MI355X)
    for i, c in enumerate(row["cases"]):
        assert mm.case_bytes(row, c) <= mm.cap_bytes(row), (rid, c)
        if row["how"] == "resid":
            _check_resid(fos, row, c, cus, trial=i == 0)
        elif row["how"] == "dd":
            _check_dd(fos, row, c, cus, with_single=i == 0)
        else:
            _check_lockstep(fos, row, c, cus)
    if row["table"] == "cluster":
        _matrix.cache_clear()                                  # 128 MiB matrices: not kept for the next cell


@pytest.mark.parametrize("dtype,n", [("bf16", 512), ("f32", 8196), ("f32", 128)])
def test_one_handle_is_the_single_run_and_two_without_a_valu_kernel_are_refused(fos, cus, dtype, n):
    from fastoptsolver_amd import _core
    m = 97
    row = dict(dtype=dtype)
    c = dict(m=m, n=n, layout="strided")
    rng = np.random.default_rng(_seed("refused", dtype, n))
    b = rng.standard_normal(m).astype(np.float32)
    prob, A64 = _problem(fos, row, c, b)
    x0 = rng.standard_normal((n, 2)).astype(np.float32)
    tau = 1.0 / float(np.sum(A64 * A64))
    Bd, _ = _block(rng.standard_normal((m, 2)).astype(np.float32), 5)

    def handles(k):
        hs = [_core.Fista(prob) for _ in range(k)]
        for j, h in enumerate(hs):
            h.reset(tau, 0.0, 0.0, x0=x0[:, j])
        return hs
    assert mm.lockstep_form(dtype, n, 2, "b") == mm.lockstep_form(dtype, n, 2, "B") == "refused"
    assert _core.run_multi(handles(2), 1) is False and _core.run_multi_rhs(handles(2), Bd, 1) is False
    assert _core.run_multi_rhs(handles(1), Bd[:, :1], 1) is False
    one, ref = handles(1), handles(1)
    assert _core.run_multi(one, 3) is True
    ref[0].run(3)
    assert torch.equal(one[0].x_tensor(), ref[0].x_tensor())
