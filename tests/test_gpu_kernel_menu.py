"""GPU: every launchable cell of the single-pass kernel menus (tests/_menu.py) against the fp64 oracle on the stored A.

One test per cell (table, dtype, geometry, variant); its cases sit at the edges where a kernel goes wrong - widths at the
capacity, one chunk short of it, one chunk above the previous capacity; one row; a last workgroup that ends inside a
row step; b = None.  Everything around the operands is NaN (the padding columns of strided rows, the columns around a
column block, the elements around y, b and x), so a kernel that reads outside them and masks the value by multiplying
with zero fails instead of passing.  Every case asserts the route the planner took (plan()), DUAL cases count the
A-pass launches (one for the DUAL kernel, two for the fallback)."""
import functools
import zlib

import numpy as np
import pytest
import torch

from oracle import fos_oracle as orc
from tests import _data, _menu

pytestmark = pytest.mark.gpu

ALPHA2 = 0.37
WIDE_GEO = {"f32": (512, 16, 1), "bf16": (512, 8, 1)}           # gemv_wide.hpp: WD_THREADS, WD_K (bf16: WD_K / 2)


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    yield f
    _matrix.cache_clear()


@pytest.fixture(scope="module")
def comm(fos):
    from fastoptsolver_amd import distributed as fd
    return fd.Comm.solo()


def _seed(*key):
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=16)
def _matrix(dtype, m, n, layout):
    """(device view of A in `layout`, NaN everywhere around it; the stored A in fp64)."""
    rng = np.random.default_rng(_seed(dtype, m, n, layout))
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    A = torch.as_tensor(rng.standard_normal((m, n)).astype(np.float32)).to(tdt)
    A64 = A.to(torch.float64).numpy()
    e = _menu.EPC[dtype]
    if layout == "compact":
        view = A.cuda()
    elif layout == "misaligned":
        flat = torch.full((m * n + 2,), float("nan"), dtype=tdt, device="cuda")
        flat[1:1 + m * n] = A.reshape(-1).cuda()
        view = flat[1:1 + m * n].view(m, n)
    else:
        pad, lo = {"strided": (2 * e, 0), "ragged": (1, 0), "cbview": (2 * e, e)}[layout]
        full = torch.full((m, n + pad), float("nan"), dtype=tdt, device="cuda")
        full[:, lo:lo + n] = A.cuda()
        view = full[:, lo:lo + n]
    return view, A64


def _vec(v, dtype=torch.float32):
    """v on the device as a 16-byte aligned view inside a NaN-filled buffer."""
    off = 16 // torch.tensor([], dtype=dtype).element_size()
    buf = torch.full((len(v) + 2 * off,), float("nan"), dtype=dtype, device="cuda")
    buf[off:off + len(v)] = torch.as_tensor(np.asarray(v), dtype=dtype)
    return buf[off:off + len(v)]


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)


def _problem(fos, row, c):
    dtype, m, n = row["dtype"], c["m"], c["n"]
    A, A64 = _matrix(dtype, m, n, c["layout"])
    b = np.random.default_rng(_seed("b", m)).standard_normal(m).astype(np.float32) if c["b"] else None
    prob = fos.prepare(A, None if b is None else _vec(b), pad=False)
    assert prob.n_dev == n and prob.A.data_ptr() == A.data_ptr()           # borrowed as it is
    return prob, A64, b


def _route(fos, row, c, prob, comm=None):
    """Force the row's cell and assert the plan that results."""
    dtype, m, n, table = row["dtype"], c["m"], c["n"], row["table"]
    where = (_menu.row_id(row), c)
    if row["variant"] == "cb":
        prob.set_comm_cols(comm)
        plan = prob.plan()
        assert (plan["path"], plan["colblock"], plan["tall"]) == (0, 1, 0), (where, plan)
        assert (plan["threads"], plan["chunks"], plan["rows"]) == row["tune"], (where, plan)
        return plan
    if table in ("wide", "fallback"):
        plan = prob.plan()
        if table == "wide":
            assert (plan["path"], plan["tall"], plan["colblock"]) == (0, 0, 0), (where, plan)
            assert (plan["threads"], plan["chunks"], plan["rows"]) == WIDE_GEO[dtype], (where, plan)
        else:
            assert plan["path"] == 1, (where, plan)
        return plan
    prob.replan(no_resident=True, no_tall=c["no_tall"], interleave=c["il"])
    if table == "kMenu":
        th, k, r = row["tune"]
        prob.tune(th, k, r, c["wg"])
        plan = prob.plan()
        assert (plan["path"], plan["tall"], plan["colblock"], plan["resident"]) == (0, 0, 0, 0), (where, plan)
        assert (plan["threads"], plan["chunks"], plan["rows"]) == (th, k, r), (where, plan)
        assert plan["interleave"] == int(c["il"]), (where, plan)
        if c["tail"]:
            # plan_fused clamps the hint to at least 2 R rows per workgroup: the tail is checked, not assumed
            assert plan["workgroups"] == plan["slabs"] == c["wg"], (where, plan)
            rpw = -(-m // c["wg"])
            last = m - (c["wg"] - 1) * rpw
            assert 0 < last < rpw and (r == 1 or (rpw % r and last % r)), (where, plan, rpw, last)
        return plan
    if table == "kDdMenu":
        from fastoptsolver_amd import _lib
        if c["wg"]:
            _lib.check(prob.lib.fos_problem_tune_dd(prob.h, c["wg"]), "fos_problem_tune_dd")
        plan = prob.plan()
        assert (plan["path"], plan["tall"], plan["colblock"], plan["resident"]) == (0, 0, 0, 0), (where, plan)
        e = _menu.MENU[_menu.first_fit(_menu.MENU, dtype, n)]         # the fp32 pass's geometry; fp64 by capacity
        assert (plan["threads"], plan["chunks"], plan["rows"]) == e[1:4], (where, plan)
        return plan
    # tall tables: the load form follows from the layout (tests/test_kernel_menu.py checks that on the CPU)
    if c["wg"]:
        prob.tune(0, 0, 0, c["wg"])
    plan = prob.plan()
    assert (plan["path"], plan["tall"], plan["resident"], plan["colblock"]) == (0, 1, 0, 0), (where, plan)
    assert (plan["threads"], plan["chunks"], plan["rows"]) == (256, row["lanes"], 0), (where, plan)
    if c["wg"]:
        rpw = (-(-m // c["wg"]) + 3) // 4 * 4
        assert plan["workgroups"] == -(-m // rpw), (where, plan)
    return plan


def _check_pass(prob, A64, b, c, where, with_g=True, resid=True):
    n = c["n"]
    y = np.random.default_rng(_seed("y", n)).standard_normal(n).astype(np.float32)
    yd = _vec(y)
    y64 = y.astype(np.float64)
    g_ref, rr_ref = orc.gram_gradient(A64, y64, None if b is None else b.astype(np.float64), ALPHA2)
    g_tol, rr_tol = _data.fp32_pass_tolerances(A64, y, b, g_ref, rr_ref)
    if with_g:
        rr = torch.zeros(1, dtype=torch.float64, device="cuda")
        g = _np(prob.gemv_pair(yd, alpha2=ALPHA2, rr_out=rr))
        rr = float(rr.cpu())
        assert np.isfinite(g).all() and np.isfinite(rr), where
        assert np.linalg.norm(g - g_ref) <= g_tol, (where, np.linalg.norm(g - g_ref), g_tol)
        assert abs(rr - rr_ref) <= rr_tol, (where, rr, rr_ref)
    if resid:
        r2, x2, x1 = prob.residual_objective(yd)
        assert np.isfinite(r2) and abs(r2 - rr_ref) <= rr_tol, (where, r2, rr_ref)
        assert x2 == pytest.approx(float(y64 @ y64), rel=1e-6) and x1 == pytest.approx(float(np.abs(y64).sum()), rel=1e-6)


def _check_dual(fos, prob, A64, b, c, where, launches_expected):
    """Gradient at y_k and ||A x_k - b||^2 in one pass: the gradient equals the plain pass's, rr_x the fp64 residual of
    x_k; the profiled A-pass launches tell the DUAL kernel (one) from the two-pass fallback (two)."""
    from fastoptsolver_amd import _core
    b64 = np.zeros(c["m"]) if b is None else b.astype(np.float64)
    L = float(np.sum(A64 * A64))                   # ||A||_F^2 >= ||A||_2^2: a valid step
    a1 = 0.05 * float(np.max(np.abs(A64.T @ b64))) if b is not None else 0.0
    x0 = np.random.default_rng(_seed("x0", c["n"])).standard_normal(c["n"])
    # a tenth of the step keeps x_k away from the solution: at m <= 2 rows (or one column) three full steps solve the
    # problem and the gradient left is fp32 cancellation noise that no two summation orders agree on
    f = _core.Fista(prob)
    f.reset(0.1 / (L + ALPHA2), a1, ALPHA2, x0=x0)
    f.run(3)
    f.grad()
    g0 = _np(prob.gbuf[: c["n"]])
    prob.profile(1)
    prob.profile_read()
    f.grad(dual=True)
    launches = prob.profile_read()[1]
    prob.profile(0)
    g1 = _np(prob.gbuf[: c["n"]])
    assert np.isfinite(g1).all(), where
    assert _data.rel(g1, g0) < 1e-6, (where, _data.rel(g1, g0))
    x = _np(f.x_tensor())
    r = A64 @ x - b64
    rr_x = float(f.status().rr_x)
    assert rr_x == pytest.approx(float(r @ r), rel=1e-5), (where, rr_x, float(r @ r))
    assert launches == launches_expected, (where, launches)


def _check_dd(prob, A64, b, c, where):
    from fastoptsolver_amd import _core, _lib
    n = c["n"]
    rng = np.random.default_rng(_seed("x", n))
    x = rng.standard_normal(n) * (1.0 + 1e-9 * rng.standard_normal(n))        # not representable in fp32
    out = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
    _lib.check(prob.lib.fos_gemv_pair_dd(prob.h, _core.ptr(_vec(x, torch.float64)), ALPHA2, _core.ptr(out)), "fos_gemv_pair_dd")
    g_ref, rr_ref = orc.gram_gradient(A64, x, None if b is None else b.astype(np.float64), ALPHA2)
    got = out.cpu().numpy()
    assert np.isfinite(got).all(), where
    assert _data.rel(got[:n], g_ref) < 1e-12, (where, _data.rel(got[:n], g_ref))
    assert got[n] == pytest.approx(rr_ref, rel=1e-12), where


def _check_cb_solver(fos, prob, comm, A64, b, c, where):
    n = c["n"]
    b64 = b.astype(np.float64)
    L = float(np.sum(A64 * A64))
    a1 = 0.1 * float(np.max(np.abs(A64.T @ b64)))
    x = fos.fista(prob, None, "elasticnet", a1, 0.5, comm=comm, cols=(0, n, n), L=L, max_iter=10)
    x_ref = orc.fista(A64, b64, "elasticnet", a1, 0.5, L=L, max_iter=10)
    assert _data.rel(_np(x), x_ref) < 1e-5, (where, _data.rel(_np(x), x_ref))
    x, h = fos.fista(prob, None, "elasticnet", a1, 0.5, comm=comm, cols=(0, n, n), L=L, max_iter=10, return_history=True)
    x_ref, h_ref = orc.fista(A64, b64, "elasticnet", a1, 0.5, L=L, max_iter=10, return_history=True)
    assert _data.rel(_np(x), x_ref) < 1e-5, where
    assert len(h["obj"]) == len(h_ref["obj"]) and np.allclose([float(o) for o in h["obj"]], h_ref["obj"], rtol=1e-5), where


def _run_row(fos, row, comm=None, launches_expected=None):
    v = row["variant"]
    for i, c in enumerate(row["cases"]):
        where = (_menu.row_id(row), i, c)
        prob, A64, b = _problem(fos, row, c)
        _route(fos, row, c, prob, comm)
        if v in ("dual", "dual_il"):
            _check_dual(fos, prob, A64, b, c, where, launches_expected)
        elif v in ("dd", "dd_il"):
            _check_dd(prob, A64, b, c, where)
        elif v == "cb":
            _check_pass(prob, A64, b, c, where)
            if b is not None:
                _check_cb_solver(fos, prob, comm, A64, b, c, where)
        elif row["table"] in ("wide", "fallback"):
            _check_pass(prob, A64, b, c, where)
        else:
            _check_pass(prob, A64, b, c, where, with_g=v.startswith("with_g"), resid=v.startswith("resid"))
        del prob
    torch.cuda.synchronize()


@pytest.mark.parametrize("row", _menu.reachable() + _menu.EXTRA, ids=_menu.row_id)
def test_cell(fos, comm, row):
    _run_row(fos, row, comm if row["variant"] == "cb" else None, launches_expected=1)


@pytest.mark.parametrize("row", _menu.dual_fallback(), ids=lambda r: _menu.row_id(r) + "-fallback")
def test_dual_fallback_on_entries_without_dual(fos, row):
    """Entries without a DUAL instantiation: fos_fista_grad_dual runs a residual pass at x_k and then the gradient."""
    _run_row(fos, row, launches_expected=2)
