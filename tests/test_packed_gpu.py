"""The gradient pass from the 28-bit packed copy of fp32 A (csrc/gemv_packed.hpp), forced onto small shapes with
FOS_PLAN_PACK: one gradient and whole FISTA runs against the fp64 oracle, and the life cycle of the copy."""
import numpy as np
import pytest
import torch

from oracle import fos_oracle as orc
from tests import _data

pytestmark = pytest.mark.gpu

TOL = 1e-5            # tests/test_gpu_parity.py::test_gemv_pair


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device="cuda")


# 515 rows: no multiple of the grid or of the two register tiles, tail steps, clamped prefetch rows; 16368 and 4112 columns:
# dead threads and a partly filled last plane (4112 = 257 of 512 threads); 3 rows: fewer rows than workgroups
SHAPES = [(515, 16384), (515, 8192), (37, 16368), (260, 4112), (3, 16384)]
_cache = {}


def _case(m, n):
    """A with out-of-window elements planted in the first, the last (next to the dead threads where there are any) and an inner
    column, in the first and the last row; b, y and the fp64 gradients with and without b.  Built once per shape."""
    if (m, n) not in _cache:
        rng = np.random.default_rng(m * 31 + n)
        A = rng.standard_normal((m, n)).astype(np.float32)
        A[0, 0], A[0, n - 1], A[0, n // 2] = 0.0, 300.0, 1e-30
        A[m - 1, 0], A[m - 1, n - 1], A[m - 1, 17] = -5000.0, 1e-40, -0.0
        A[m // 2, n - 1], A[m // 2, 0] = -1e-30, 777.0
        b = rng.standard_normal(m).astype(np.float32)
        y = rng.standard_normal(n).astype(np.float32)
        A64, y64 = A.astype(np.float64), y.astype(np.float64)
        _cache[(m, n)] = (A, b, y, orc.gram_gradient(A64, y64, b.astype(np.float64), 0.3), orc.gram_gradient(A64, y64, None, 0.3))
    return _cache[(m, n)]


@pytest.mark.parametrize("m,n", SHAPES)
@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("interleave", [False, True])
def test_packed_gradient(fos, m, n, with_b, interleave):
    A, b, y, ref_b, ref_0 = _case(m, n)
    g_ref, rr_ref = ref_b if with_b else ref_0
    prob = fos.prepare(A, b if with_b else None)
    prob.replan(no_resident=True, interleave=interleave, pack=True)
    assert prob.plan()["packed"] == 0                       # nothing is packed before the first gradient
    rr = torch.zeros(1, dtype=torch.float64, device="cuda")
    g = prob.gemv_pair(_dev(y), alpha2=0.3, rr_out=rr).cpu().numpy().astype(np.float64)
    plan = prob.plan()
    assert plan["packed"] == 1 and plan["interleave"] == int(interleave), plan
    assert _data.rel(g, g_ref) < TOL, plan
    assert float(rr.cpu()) == pytest.approx(rr_ref, rel=TOL)
    g2 = prob.gemv_pair(_dev(y), alpha2=0.3).cpu().numpy().astype(np.float64)
    assert (g2 == g).all()                                  # fixed summation order: the same bits every time


@pytest.fixture(scope="module")
def full_run():
    rng = np.random.default_rng(11)
    m, n = 2048, 16384
    A = rng.standard_normal((m, n)).astype(np.float32)
    A[5, 9], A[m - 1, n - 1], A[0, 0] = 0.0, 400.0, 1e-30
    x_true = np.zeros(n)
    x_true[rng.choice(n, 50, replace=False)] = rng.standard_normal(50)
    A64 = A.astype(np.float64)
    b = (A64 @ x_true + 0.1 * rng.standard_normal(m)).astype(np.float32)
    v = rng.standard_normal(n)
    for _ in range(30):                                     # an upper estimate of ||A||_2^2 is all the step needs
        v = A64.T @ (A64 @ v)
        v /= np.linalg.norm(v)
    L = 1.05 * float(np.linalg.norm(A64 @ v) ** 2)
    lam = 0.1 * float(np.abs(A64.T @ b.astype(np.float64)).max())
    x_ref = orc.fista(A64, b.astype(np.float64), "elasticnet", lam, 0.5, max_iter=40, L=L)
    return A, b, L, lam, x_ref


def test_packed_full_run_against_oracle_and_raw_plan(fos, full_run):
    A, b, L, lam, x_ref = full_run
    prob = fos.prepare(A, b)
    assert prob.plan()["packed"] == 0
    x_raw = _np(fos.fista(prob, None, "elasticnet", lam, 0.5, max_iter=40, L=L)).astype(np.float64)
    assert prob.plan()["packed"] == 0                       # 128 MiB: below the planner's size threshold, not forced
    prob.replan(pack=True)
    x_pk = _np(fos.fista(prob, None, "elasticnet", lam, 0.5, max_iter=40, L=L)).astype(np.float64)
    assert prob.plan()["packed"] == 1
    d_raw, d_pk, d = _data.rel(x_raw, x_ref), _data.rel(x_pk, x_ref), _data.rel(x_pk, x_raw)
    print(f"raw vs oracle {d_raw:.3e}  packed vs oracle {d_pk:.3e}  packed vs raw {d:.3e}")
    assert d_raw < TOL and d_pk < TOL
    # the packed pass re-associates fp32 sums of the same terms: a perturbation of the size of the raw pass's own rounding,
    # which is what raw vs fp64 measures; twice that (two passes that are each that far from exact) bounds their distance
    assert d <= 2.0 * d_raw


def test_packed_copy_life_cycle(fos, full_run):
    A, b, L, lam, x_ref = full_run
    prob = fos.prepare(A[:512], b[:512])
    prob.replan(pack=True)
    x1 = _np(fos.fista(prob, None, "elasticnet", lam, 0.5, max_iter=5, L=L))
    assert prob.plan()["packed"] == 1
    prob.tune(1024, 4, 1)                                   # an invalidating call drops the copy ...
    assert prob.plan()["packed"] == 0
    x2 = _np(fos.fista(prob, None, "elasticnet", lam, 0.5, max_iter=5, L=L))
    assert prob.plan()["packed"] == 1                       # ... and the next run packs again
    assert (x1 == x2).all()
    prob.replan(pack=True)                                  # a replan repacks
    assert prob.plan()["packed"] == 0
    x3 = _np(fos.fista(prob, None, "elasticnet", lam, 0.5, max_iter=5, L=L))
    assert prob.plan()["packed"] == 1 and (x3 == x1).all()
    prob.replan(pack=False)                                 # FOS_PLAN_NO_PACK
    x4 = _np(fos.fista(prob, None, "elasticnet", lam, 0.5, max_iter=5, L=L))
    assert prob.plan()["packed"] == 0
    assert _data.rel(x4.astype(np.float64), x1.astype(np.float64)) < TOL


def test_refused_matrices_keep_the_raw_plan(fos):
    rng = np.random.default_rng(12)
    m, n = 300, 8192
    b = rng.standard_normal(m).astype(np.float32)
    y = rng.standard_normal(n).astype(np.float32)
    sparse01 = (rng.random((m, n)) < 0.05).astype(np.float32)           # above the exception cap
    with_inf = rng.standard_normal((m, n)).astype(np.float32)
    with_inf[7, 100] = np.inf
    with_nan, with_ninf = with_inf.copy(), with_inf.copy()             # the other two refusals of tests/test_packed_format.py
    with_nan[7, 100], with_ninf[7, 100] = np.nan, -np.inf
    for A in (sparse01, with_inf, with_nan, with_ninf):
        prob = fos.prepare(A, b)
        prob.replan(no_resident=True, pack=True)
        g = prob.gemv_pair(_dev(y)).cpu().numpy()
        assert prob.plan()["packed"] == 0
        if np.isfinite(A).all():
            g_ref, _ = orc.gram_gradient(A.astype(np.float64), y.astype(np.float64), b.astype(np.float64), 0.0)
            assert _data.rel(g.astype(np.float64), g_ref) < TOL
