"""GPU: every launchable instantiation of the L-BFGS kernels that has an entry point of its own (tests/_menu_lbfgs.py, the
rows whose check is not a driver) against a NumPy fp64 restatement of the same operation, math.fsum for the sums.

Every operand is a view inside a larger NaN-filled device allocation and every output starts as NaN inside NaN guards that
must be unchanged afterwards: a read outside an operand that is masked by a zero weight turns the result into NaN, a write
outside an output leaves a number in a guard.  The ring slots of S and Y outside the live window [head, head + hist) are NaN
as well, so a wrong slot index is visible."""
import math

import numpy as np
import pytest
import torch

from oracle import fos_oracle as orc
from tests import _data, _menu_lbfgs as ml
from tests.test_gpu_kernel_menu import _seed

pytestmark = pytest.mark.gpu

TOL = 1e-5                                  # fp32 two-loop recursion: the north-star tolerance of tests/test_gpu_parity.py
EPS32 = float(np.finfo(np.float32).eps)
PAD = 64                                    # NaN elements before and after every operand (512 bytes of doubles: alignment kept)
NAN = float("nan")
TDT = {"float": torch.float32, "double": torch.float64}
NDT = {"float": np.float32, "double": np.float64}


@pytest.fixture(scope="module")
def lib():
    import fastoptsolver_amd  # noqa: F401
    from fastoptsolver_amd import _lib
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return _lib.load()


def _ptr(t):
    from fastoptsolver_amd import _core
    return _core.ptr(t)


def _stream():
    from fastoptsolver_amd import _core
    return _core.stream_ptr()


class Guarded:
    """`count` elements at element offset `off` behind PAD NaN guards inside one allocation; data=None leaves them NaN."""

    def __init__(self, count, dtype, data=None, off=0):
        self.lo, self.count = PAD + off, count
        self.buf = torch.full((2 * PAD + off + count,), NAN, dtype=dtype, device="cuda")
        self.view = self.buf[self.lo: self.lo + count]
        if data is not None:
            self.view.copy_(torch.as_tensor(np.ascontiguousarray(data).reshape(-1), dtype=dtype))

    def guards_intact(self):
        return bool(torch.isnan(self.buf[: self.lo]).all() and torch.isnan(self.buf[self.lo + self.count:]).all())

    def numpy(self):
        return self.view.cpu().numpy().astype(np.float64)


def _ring(pool, cap, hist, head, n, dtype, off):
    """[cap][n] ring holding pool[(head + i) % cap] in the live slots and NaN in the dead ones (None when cap = 0)."""
    if cap == 0:
        return None, []
    order = [(head + i) % cap for i in range(hist)]
    M = np.full((cap, n), np.nan)
    M[order] = pool[order]
    return Guarded(cap * n, dtype, M, off), order


def _pools(vt, n, cap, key):
    rng = np.random.default_rng(_seed(key, vt, n))
    S = rng.standard_normal((cap, n)).astype(NDT[vt]).astype(np.float64)
    Y = (S + 0.3 * rng.standard_normal((cap, n))).astype(NDT[vt]).astype(np.float64)      # s.y > 0
    g = rng.standard_normal(n).astype(NDT[vt]).astype(np.float64)
    return S, Y, g


def _two_loop_f32(g, S, Y):
    """The recursion with q held in float32 (rounded after every update, as lbfgs_two_loop_kernel<float> keeps it) and every
    dot product in fp64: what is left of the error when the kernel is right."""
    f32 = lambda v: v.astype(np.float32).astype(np.float64)      # noqa: E731
    q, k = f32(g), len(S)
    rho, coef = [0.0] * k, [0.0] * k
    for i in range(k - 1, -1, -1):
        rho[i] = 1.0 / float(Y[i] @ S[i])
        coef[i] = rho[i] * float(S[i] @ q)
        q = f32(q - coef[i] * Y[i])
    if k:
        q = f32(q * (float(S[-1] @ Y[-1]) / float(Y[-1] @ Y[-1])))
    for i in range(k):
        q = f32(q + S[i] * (coef[i] - rho[i] * float(Y[i] @ q)))
    return -q


# ---- two-loop recursion ------------------------------------------------------------------------------------------------
def _check_two_loop(lib, row, c):
    vt, nq = row["targs"][0], int(row["targs"][1])
    n, off = c["n"], c["off"]
    fn = lib.fos_lbfgs_two_loop if vt == "float" else lib.fos_lbfgs_two_loop_dd
    S, Y, g = _pools(vt, n, max(cap for _, cap, _ in c["cfgs"]) or 1, "two_loop")
    gd = Guarded(n, TDT[vt], g, off)
    for hist, cap, head in c["cfgs"]:
        where = (ml.row_id(row), n, off, hist, cap, head)
        Sd, order = _ring(S, cap, hist, head, n, TDT[vt], off)
        Yd, _ = _ring(Y, cap, hist, head, n, TDT[vt], off)
        out = Guarded(n, TDT[vt], None, off)
        ptrs = [gd.view.data_ptr(), out.view.data_ptr()] + ([Sd.view.data_ptr(), Yd.view.data_ptr()] if Sd else [])
        aligned = all(p % ml.ALIGN[vt] == 0 for p in ptrs)
        assert aligned == (off == 0), (where, "an offset of one element must break the alignment, none must keep it")
        assert ml.two_loop_nq(n, aligned) == nq, where                              # the case reaches the row's instantiation
        rc = fn(_ptr(gd.view), _ptr(Sd.view) if Sd else None, _ptr(Yd.view) if Yd else None, hist, head, cap, n,
                _ptr(out.view), _stream())
        assert rc == 0, (where, rc)
        torch.cuda.synchronize()
        ref = orc.two_loop_direction(g, [S[i] for i in order], [Y[i] for i in order])
        got = out.numpy()
        assert np.isfinite(got).all(), (where, "NaN: a dead slot or a guard was read")
        assert out.guards_intact() and gd.guards_intact() and (Sd is None or (Sd.guards_intact() and Yd.guards_intact())), where
        err = _data.rel(got, ref)
        if vt == "double":
            assert err < 1e-12, (where, err)
            continue
        bound = TOL
        if hist == ml.LB_MAXHIST:
            # 64 pairs round q to fp32 128 times.  The float32 restatement above differs from the fp64 recursion by 2.8e-7 ..
            # 2.9e-7 relative on these inputs (measured on the CPU for every 64-pair case of the table, n = 4092 .. 70001);
            # 4x that, 1.2e-6, is allowed where it exceeds TOL - it does not, so TOL = 1e-5 stands for 64 pairs as well.
            restated = _data.rel(_two_loop_f32(g, [S[i] for i in order], [Y[i] for i in order]), ref)
            bound = max(TOL, 4.0 * restated)
        assert err < bound, (where, err, bound)


# ---- whole-chip direction ------------------------------------------------------------------------------------------------
def _check_direction(lib, row, c):
    n = c["n"]
    S, Y, g = _pools("double", n, max(cap for _, cap, _ in c["cfgs"]), "direction")
    gdev = Guarded(n, torch.float64, g)
    nwork = int(lib.fos_lbfgs_direction_work(n))
    assert nwork == ml.direction_work(n), (n, nwork)
    for hist, cap, head in c["cfgs"]:
        where = (ml.row_id(row), n, hist, cap, head, c["gd"], c["tail"])
        Sd, order = _ring(S, cap, hist, head, n, torch.float64, 0)
        Yd, _ = _ring(Y, cap, hist, head, n, torch.float64, 0)
        sp, yp = (_ptr(Sd.view), _ptr(Yd.view)) if Sd else (None, None)
        d_tl = Guarded(n, torch.float64)
        assert lib.fos_lbfgs_two_loop_dd(_ptr(gdev.view), sp, yp, hist, head, cap, n, _ptr(d_tl.view), _stream()) == 0, where
        d = Guarded(n, torch.float64)
        gd = Guarded(2, torch.float64)
        work = Guarded(nwork + c["tail"], torch.float64)
        rc = lib.fos_lbfgs_direction_dd(_ptr(gdev.view), sp, yp, hist, head, cap, n, _ptr(d.view),
                                        _ptr(gd.view) if c["gd"] else None, _ptr(work.view), nwork + c["tail"], _stream())
        assert rc == 0, (where, rc)
        torch.cuda.synchronize()
        ref = orc.two_loop_direction(g, [S[i] for i in order], [Y[i] for i in order])
        got = d.numpy()
        assert np.isfinite(got).all(), (where, "NaN: a dead slot, a guard or an unwritten partial was read")
        assert d.guards_intact() and gd.guards_intact() and work.guards_intact() and gdev.guards_intact(), where
        assert bool(torch.isnan(work.view[nwork:]).all()), (where, "write behind fos_lbfgs_direction_work(n) doubles")
        assert Sd is None or (Sd.guards_intact() and Yd.guards_intact()), where
        assert _data.rel(got, ref) < 1e-12, (where, _data.rel(got, ref))
        assert _data.rel(got, d_tl.numpy()) < 1e-12, (where, _data.rel(got, d_tl.numpy()))
        if c["gd"]:
            gdn = gd.numpy()
            assert gdn[0] == pytest.approx(float(g @ ref), rel=1e-11), where
            assert gdn[1] == pytest.approx(float(ref @ ref), rel=1e-11), where
            # ... and against the two-loop kernel's direction
            tl = d_tl.numpy()
            assert gdn[0] == pytest.approx(float(g @ tl), rel=1e-11) and gdn[1] == pytest.approx(float(tl @ tl), rel=1e-11), where
        else:
            assert bool(torch.isnan(gd.view).all()), where


# ---- statistics ------------------------------------------------------------------------------------------------------------
def _stats_ref(x, g, d):
    z = np.zeros_like(g if g is not None else x if x is not None else d)
    x, g, d = (z if v is None else v for v in (x, g, d))
    sums = [math.fsum(x * x), math.fsum(g * d), math.fsum(d * d), float(np.max(np.abs(g))), math.fsum(np.abs(x))]
    scale = [math.fsum(x * x), math.fsum(np.abs(g * d)), math.fsum(d * d), 0.0, math.fsum(np.abs(x))]
    return sums, scale


def _check_stats(lib, row, c):
    xt, gt = row["targs"]
    fn = getattr(lib, row["entry"])
    n = c["n"]
    rng = np.random.default_rng(_seed("stats", xt, gt, n))
    x = (rng.standard_normal(n) * (1.0 + 1e-9 * rng.standard_normal(n))).astype(NDT[xt]).astype(np.float64)
    g = rng.standard_normal(n)
    g[-1] = -(np.max(np.abs(g)) + 1.5)                       # the largest |g|: negative, in the last position
    g = g.astype(NDT[gt]).astype(np.float64)
    d = rng.standard_normal(n).astype(NDT[gt]).astype(np.float64)
    dev = dict(x=Guarded(n, TDT[xt], x), g=Guarded(n, TDT[gt], g), d=Guarded(n, TDT[gt], d))
    host = dict(x=x, g=g, d=d)

    def run(present, spoil=None):
        ops = {}
        for k in "xgd":
            if k not in present:
                ops[k] = None
            elif k == spoil:
                v = host[k].copy()
                v[(3 * n) // 7] = np.nan
                ops[k] = Guarded(n, TDT[xt if k == "x" else gt], v)
            else:
                ops[k] = dev[k]
        out = Guarded(5, torch.float64)
        rc = fn(*[_ptr(ops[k].view) if ops[k] else None for k in "xgd"], n, _ptr(out.view), _stream())
        assert rc == 0, (ml.row_id(row), n, present, rc)
        torch.cuda.synchronize()
        assert out.guards_intact() and all(o is None or o.guards_intact() for o in ops.values()), (ml.row_id(row), n, present)
        return out.numpy()

    for present in ("xgd", "gd", "xd", "xg"):
        where = (ml.row_id(row), n, present)
        got = run(present)
        ref, scale = _stats_ref(*[host[k] if k in present else None for k in "xgd"])
        assert np.isfinite(got).all(), (where, got)
        for i in (0, 1, 2, 4):
            assert abs(got[i] - ref[i]) <= 1e-13 * scale[i], (where, i, got[i], ref[i])
        assert got[3] == ref[3], (where, got[3], ref[3])                       # max|g|: exact
    # a NaN anywhere in g must reach max|g| (fmax dropped it: an all-NaN gradient "converged"); in x or d, the sums
    got = run("xgd", spoil="g")
    assert math.isnan(got[3]) and math.isnan(got[1]) and np.isfinite(got[[0, 2, 4]]).all(), (ml.row_id(row), n, "NaN in g", got)
    got = run("xgd", spoil="x")
    assert math.isnan(got[0]) and math.isnan(got[4]) and np.isfinite(got[[1, 2, 3]]).all(), (ml.row_id(row), n, "NaN in x", got)
    got = run("xgd", spoil="d")
    assert math.isnan(got[1]) and math.isnan(got[2]) and np.isfinite(got[[0, 3, 4]]).all(), (ml.row_id(row), n, "NaN in d", got)
    all_nan = Guarded(n, TDT[gt], np.full(n, np.nan))
    out = Guarded(5, torch.float64)
    assert fn(None, _ptr(all_nan.view), None, n, _ptr(out.view), _stream()) == 0
    torch.cuda.synchronize()
    assert math.isnan(out.numpy()[3]), (ml.row_id(row), n, "all-NaN g", out.numpy())


# ---- axpby -------------------------------------------------------------------------------------------------------------------
def _check_axpby(lib, row, c):
    fn = getattr(lib, row["entry"])
    n = c["n"]
    f64 = row["kernel"] == "vec_axpby_f64_kernel"
    ytype = row["targs"][0] if f64 else "float"
    a, x, b, y = ml.axpby_inputs(n, _seed("axpby", n), ytype)
    if not f64:
        # the fp32 entry point takes a and b as doubles and rounds them to float: representable values keep the bound below
        # about the kernel (one rounded product, one fma) and not about that conversion
        a, b, x = 0.75, -1.375, x.astype(np.float32).astype(np.float64)
    xdt = torch.float64 if f64 else torch.float32
    ydt = TDT[ytype] if f64 else torch.float32
    xd, yd = Guarded(n, xdt, x), Guarded(n, ydt, y)
    for bb, yy in ((b, yd), (0.0, None), (0.0, yd)):
        where = (ml.row_id(row), n, bb, yy is not None)
        out = Guarded(n, xdt)
        rc = fn(a, _ptr(xd.view), bb, _ptr(yy.view) if yy else None, _ptr(out.view), n, _stream())
        assert rc == 0, (where, rc)
        torch.cuda.synchronize()
        assert out.guards_intact() and xd.guards_intact() and yd.guards_intact(), where
        got = out.numpy()
        if f64:
            want = bb * y + a * x if bb != 0.0 else a * x                     # NumPy: every product and the sum rounded once
            assert np.array_equal(got, want), (where, int(np.sum(got != want)), "elements differ in their bits")
        else:
            exact = a * x + bb * y
            tol = EPS32 * (np.abs(a * x) + np.abs(bb * y))
            assert np.isfinite(got).all() and (np.abs(got - exact) <= tol).all(), (where, float(np.max(np.abs(got - exact) / np.maximum(tol, 1e-300))))
    if row["entry"] == "fos_vec_axpby_dd":
        # a y that is given takes part even with b = 0: NumPy's 0 * inf + x is NaN (a line-search step of 0 along an
        # infinite direction), and the drivers rely on it
        yi = y.copy()
        yi[n // 2] = np.inf
        yinf, out = Guarded(n, ydt, yi), Guarded(n, xdt)
        assert fn(a, _ptr(xd.view), 0.0, _ptr(yinf.view), _ptr(out.view), n, _stream()) == 0
        torch.cuda.synchronize()
        got = out.numpy()
        with np.errstate(invalid="ignore"):
            want = 0.0 * yi + a * x
        assert np.array_equal(got, want, equal_nan=True) and math.isnan(got[n // 2]), (ml.row_id(row), n, "0 * inf")
    # argument errors: FOS_ERR_ARG and nothing launched (the output keeps its NaN)
    out = Guarded(n, xdt)
    for args in ((a, None, b, _ptr(yd.view), _ptr(out.view), n), (a, _ptr(xd.view), b, _ptr(yd.view), None, n),
                 (a, _ptr(xd.view), b, None, _ptr(out.view), n), (a, _ptr(xd.view), b, _ptr(yd.view), _ptr(out.view), 0),
                 (a, _ptr(xd.view), b, _ptr(yd.view), _ptr(out.view), -5)):
        assert fn(*args, _stream()) == -1, (ml.row_id(row), n, args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.buf).all()), (ml.row_id(row), n, "a refused call wrote")


# ---- the kernels of this header that the A passes launch --------------------------------------------------------------------
def _check_pass(lib, row, c):
    import fastoptsolver_amd as fos
    from fastoptsolver_amd import _core, _lib
    m, n = c["m"], c["n"]
    where = (ml.row_id(row), m, n)
    rng = np.random.default_rng(_seed("pass", m, n))
    A = rng.standard_normal((m, n)).astype(np.float32)
    b = rng.standard_normal(m).astype(np.float32)
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    prob = fos.prepare(torch.as_tensor(A).cuda(), b, pad=False)
    prob.replan(no_resident=True)
    assert prob.plan()["resident"] == 0 and prob.n_dev == n, (where, prob.plan())
    a2 = 0.375
    if row["kernel"] == "add_l2_kernel":
        dbl = row["targs"][0] == "double"
        y = rng.standard_normal(n) * (1.0 + 1e-9 * rng.standard_normal(n))
        if not dbl:
            y = y.astype(np.float32).astype(np.float64)
        yd = Guarded(n, torch.float64 if dbl else torch.float32, y)
        out, rr = Guarded(n, torch.float32), Guarded(1, torch.float64)
        fn = lib.fos_gemv_pair_f64 if dbl else lib.fos_gemv_pair
        with prob.ctx():
            _lib.check(fn(prob.h, _core.ptr(yd.view), a2, _core.ptr(out.view), _core.ptr(rr.view)), row["entry"])
        torch.cuda.synchronize()
        assert out.guards_intact() and rr.guards_intact() and yd.guards_intact(), where
        raw = prob.gbuf[:n].cpu().numpy().astype(np.float64)                  # A^T r as the pass left it
        want = (raw + a2 * y).astype(np.float32)                              # the kernel's own arithmetic: one fp64 sum, rounded
        got = out.view.cpu().numpy()
        assert np.array_equal(got, want), (where, int(np.sum(got != want)))
        g_ref, rr_ref = orc.gram_gradient(A64, y, b64, a2)
        g_tol, rr_tol = _data.fp32_pass_tolerances(A64, y, b64, g_ref, rr_ref)
        assert float(np.linalg.norm(got - g_ref)) <= g_tol + 2 * EPS32 * float(np.linalg.norm(g_ref)), where
        assert abs(float(rr.numpy()[0]) - rr_ref) <= rr_tol, where
        # alpha2 = 0 copies the raw gradient
        out0 = Guarded(n, torch.float32)
        with prob.ctx():
            _lib.check(fn(prob.h, _core.ptr(yd.view), 0.0, _core.ptr(out0.view), None), row["entry"])
        torch.cuda.synchronize()
        assert out0.guards_intact() and np.array_equal(out0.view.cpu().numpy(), prob.gbuf[:n].cpu().numpy()), where
    elif row["kernel"] == "vec_norms_kernel":
        x = rng.standard_normal(n).astype(np.float32)
        x[-1] = -3.0
        xd = Guarded(n, torch.float32, x)
        with prob.ctx():
            _lib.check(lib.fos_residual_objective(prob.h, _core.ptr(xd.view), _core.ptr(prob.scratch)), row["entry"])
        got = prob.scratch[:3].cpu().numpy()
        x64 = x.astype(np.float64)
        assert got[1] == pytest.approx(math.fsum(x64 * x64), rel=1e-13) and got[2] == pytest.approx(math.fsum(np.abs(x64)), rel=1e-13), where
        r = A64 @ x64 - b64
        _, rr_tol = _data.fp32_pass_tolerances(A64, x64, b64, np.zeros(n), float(r @ r))
        assert abs(got[0] - float(r @ r)) <= rr_tol and xd.guards_intact(), where
    else:                                                     # cast_f64_f32_kernel: x_k rounded to fp32 for the residual pass
        x0 = rng.standard_normal(n) * (1.0 + 1e-9 * rng.standard_normal(n))
        x0[[0, n // 2, n - 1]] = 3.0 * (1.0 + 2.0 ** -30)
        f = _core.Fista(prob)
        f.reset(1e-3, 0.0, 0.0, x0=x0)
        f.set_precise(True)
        f.grad(dual=True)
        rr_x = float(f.status().rr_x)
        x32 = x0.astype(np.float32).astype(np.float64)
        r = A64 @ x32 - b64
        _, rr_tol = _data.fp32_pass_tolerances(A64, x32, b64, np.zeros(n), float(r @ r))
        assert abs(rr_x - float(r @ r)) <= rr_tol, (where, rr_x, float(r @ r))
        # every element took part: dropping any single x_i moves ||r||^2 by more than the bound
        drop = np.array([float(np.sum((r - A64[:, i] * x32[i]) ** 2)) for i in (0, n // 2, n - 1)])
        assert (np.abs(drop - float(r @ r)) > 2 * rr_tol).all(), (where, drop, rr_tol)
    del prob
    torch.cuda.synchronize()


CHECKS = {"two_loop": _check_two_loop, "direction": _check_direction, "stats": _check_stats, "axpby": _check_axpby,
          "pass": _check_pass}


@pytest.mark.parametrize("rid", [ml.row_id(r) for r in ml.ROWS if r["check"] in CHECKS])
def test_cell(lib, rid):
    row = {ml.row_id(r): r for r in ml.ROWS}[rid]
    assert row["cases"], rid
    for c in row["cases"]:
        CHECKS[row["check"]](lib, row, c)


def test_direction_refuses_what_it_cannot_serve(lib):
    """More than VL_MAXH pairs are the one-workgroup kernel's job; too little scratch, a head outside the ring and a NULL
    history with pairs are argument errors.  Nothing is launched: d keeps its NaN."""
    n = 300
    S, Y, g = _pools("double", n, ml.VL_MAXH + 1, "refuse")
    gd, Sd, Yd = Guarded(n, torch.float64, g), Guarded(S.size, torch.float64, S), Guarded(Y.size, torch.float64, Y)
    d, work = Guarded(n, torch.float64), Guarded(ml.direction_work(n), torch.float64)
    nw = ml.direction_work(n)
    call = lambda hist, head, cap, w, s=Sd: lib.fos_lbfgs_direction_dd(                       # noqa: E731
        _ptr(gd.view), _ptr(s.view) if s else None, _ptr(Yd.view), hist, head, cap, n, _ptr(d.view), None, _ptr(work.view), w, _stream())
    assert call(ml.VL_MAXH + 1, 0, ml.VL_MAXH + 1, nw) == -4
    assert call(3, 0, 4, nw - 1) == -1 and call(3, 4, 4, nw) == -1 and call(3, 0, 2, nw) == -1 and call(3, 0, 4, nw, None) == -1
    for fn, dt in ((lib.fos_lbfgs_two_loop, torch.float32), (lib.fos_lbfgs_two_loop_dd, torch.float64)):
        o = Guarded(n, dt)
        gg, ss = Guarded(n, dt, g), Guarded(S.size, dt, S)
        assert fn(_ptr(gg.view), _ptr(ss.view), _ptr(ss.view), ml.LB_MAXHIST + 1, 0, ml.LB_MAXHIST + 1, n, _ptr(o.view), _stream()) == -1
        assert fn(_ptr(gg.view), _ptr(ss.view), _ptr(ss.view), 3, 5, 5, n, _ptr(o.view), _stream()) == -1
        torch.cuda.synchronize()
        assert bool(torch.isnan(o.buf).all())
    torch.cuda.synchronize()
    assert bool(torch.isnan(d.buf).all()) and bool(torch.isnan(work.buf).all())
