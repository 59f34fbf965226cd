"""GPU: several targets - fista(A, B) / fista_delta(A, B) with a 2-D B (m x k).  Column j must equal the oracle's
fista(A, B[:, j]) (1e-5 relative, on the bf16-rounded A for bf16 storage) and the GPU's single-target solve (1e-6: same
arithmetic, other summation order) on every dispatch branch: the multi-vector VALU pass (2..4 columns, fp32), the two
matrix-core products (5..16), groups plus a remainder, and the column-by-column fallbacks."""
import numpy as np
import pytest
import torch

from oracle import fos_oracle as orc
from tests import _data

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def _case(kind, m, n, k, seed, zero_col=1):
    """Device A (fp32 / bf16), its fp64 value as stored, and B (m x k fp32, column `zero_col` all zeros)."""
    rng = np.random.default_rng(seed)
    A, _, _ = _data.synth(m, n, seed)
    At = torch.as_tensor(A.astype(np.float32)).to(torch.bfloat16 if kind == "bf16" else torch.float32).cuda()
    A64 = At.to(torch.float64).cpu().numpy()
    X = np.zeros((n, k))
    for j in range(k):
        idx = rng.choice(n, max(1, n // 20), replace=False)
        X[idx, j] = rng.standard_normal(idx.size) * (1.0 + j % 3)
    B = (A64 @ X + 0.1 * rng.standard_normal((m, k))).astype(np.float32)
    if zero_col is not None and zero_col < k:
        B[:, zero_col] = 0.0
    return At, A64, B


def _L(A64):
    return float(np.linalg.norm(A64, 2) ** 2)


CASES = [("f32", 3000, 512, 2), ("f32", 3000, 512, 3), ("f32", 2048, 1024, 4),     # multi-vector VALU pass
         ("bf16", 2000, 256, 2),                                                    # no VALU form in bf16: one by one
         ("f32", 1000, 200, 5), ("f32", 4096, 512, 16),                            # matrix cores
         ("f32", 2000, 256, 17), ("f32", 1500, 384, 40),                           # groups + remainder
         ("bf16", 2000, 1024, 16),                                                  # bf16 storage on the matrix cores
         ("f32", 1200, 1030, 6),                                                    # ragged n: padded device A
         ("f32", 70000, 128, 9),                                                    # several row panels
         ("f32", 500, 16, 3)]                                                       # n <= 64: one by one


@pytest.mark.parametrize("kind,m,n,k", CASES)
def test_fista_multi_target_per_column(fos, kind, m, n, k):
    At, A64, B = _case(kind, m, n, k, 11 + n + k)
    L = _L(A64)
    a1 = 0.1 * float(np.max(np.abs(A64.T @ B[:, 0])))
    a2 = 0.5
    X = fos.fista(At, B, "elasticnet", a1, a2, max_iter=30, L=L)
    assert tuple(X.shape) == (n, k)
    X = _np(X)
    assert np.all(X[:, 1] == 0.0), "a zero target must give exactly zero"
    for j in range(k):
        x_ref = orc.fista(A64, B[:, j].astype(np.float64), "elasticnet", a1, a2, max_iter=30, L=L)
        assert _data.rel(X[:, j], x_ref) < TOL, (j, _data.rel(X[:, j], x_ref))
        if j != 1 and (k <= 17 or j in (0, 15, 16, 31, 32, k - 1)):
            x_one = _np(fos.fista(At, B[:, j].copy(), "elasticnet", a1, a2, max_iter=30, L=L))
            assert _data.rel(X[:, j], x_one) < 1e-6, (j, _data.rel(X[:, j], x_one))


@pytest.mark.parametrize("kind,m,n,k", [("f32", 3000, 512, 3), ("f32", 4096, 512, 16), ("bf16", 2000, 1024, 5),
                                        ("f32", 2000, 256, 17), ("f32", 500, 16, 2)])
def test_fista_delta_multi_target_per_column(fos, kind, m, n, k):
    At, A64, B = _case(kind, m, n, k, 5 + n + k)
    L = _L(A64)
    a1 = 0.1 * float(np.max(np.abs(A64.T @ B[:, 0])))
    X = _np(fos.fista_delta(At, B, "elasticnet", a1, 0.3, 3.0, max_iter=30, L=L))
    assert X.shape == (n, k) and np.all(X[:, 1] == 0.0)
    for j in range(k):
        x_ref = orc.fista_delta(A64, B[:, j].astype(np.float64), "elasticnet", a1, 0.3, 3.0, max_iter=30, L=L)
        assert _data.rel(X[:, j], x_ref) < TOL, j
    x_one = _np(fos.fista_delta(At, B[:, k - 1].copy(), "elasticnet", a1, 0.3, 3.0, max_iter=30, L=L))
    assert _data.rel(X[:, k - 1], x_one) < 1e-6


@pytest.mark.parametrize("kind,m,n,k", [("f32", 3000, 512, 8), ("bf16", 1500, 1024, 5), ("f32", 900, 2048, 16)])
def test_lockstep_keeps_per_column_control(fos, kind, m, n, k):
    """Adaptive restart and the ratio stop decided per column inside the lockstep: columns of different scales stop at
    different iterations, each at the oracle's iteration with the oracle's iterate."""
    At, A64, B = _case(kind, m, n, k, 71 + n, zero_col=None)
    B = B * np.array([0.05 * 4.0 ** (j % 5) for j in range(k)], dtype=np.float32)
    L = _L(A64)
    a1 = 0.05 * float(np.max(np.abs(A64.T @ B[:, 2])))
    kw = dict(adaptive_restart=True, restart_threshold=0.9, tol_ratio=0.5)
    X = _np(fos.fista(At, B, "elasticnet", a1, 0.0, max_iter=60, L=L, **kw))
    stops = []
    for j in range(k):
        x_ref, h_ref = orc.fista(A64, B[:, j].astype(np.float64), "elasticnet", a1, 0.0, max_iter=60, L=L,
                                 return_history=True, **kw)
        stops.append(len(h_ref["obj"]))
        assert _data.rel(X[:, j], x_ref) < TOL, (j, stops[-1])
    assert len(set(stops)) > 1, stops


@pytest.mark.parametrize("n,k", [(512, 16), (512, 4)])
def test_one_read_of_A_per_iteration_per_group(fos, n, k):
    At, A64, B = _case("f32", 4096, n, k, 3)
    P = fos.prepare(At)
    P.profile(1)
    P.profile_read()
    fos.fista(P, B, "lasso", 0.05 * float(np.max(np.abs(A64.T @ B[:, 0]))), 0.0, max_iter=20, L=_L(A64))
    _, launches = P.profile_read()
    P.profile(0)
    assert launches == 20, launches
    m = fos.get_metrics()
    assert m["grad_num_calls"] == 20


def test_lipschitz_estimated_once(fos):
    At, A64, B = _case("f32", 2000, 256, 5, 9)
    np.random.seed(123)
    x0 = _np(fos.fista(At, B[:, 0].copy(), "lasso", 1.0, 0.0, max_iter=10))
    one_call = np.random.get_state()[1].copy()
    np.random.seed(123)
    X = _np(fos.fista(At, B, "lasso", 1.0, 0.0, max_iter=10))
    assert np.array_equal(np.random.get_state()[1], one_call)
    assert _data.rel(X[:, 0], x0) < 1e-6


def test_types_shapes_and_unchanged_paths(fos):
    At, A64, B = _case("f32", 1500, 256, 3, 21)
    L = _L(A64)
    A32 = At.cpu().numpy()
    X = fos.fista(A32, B, "lasso", 1.0, 0.0, max_iter=15, L=L)
    assert isinstance(X, np.ndarray) and X.dtype == np.float64 and X.shape == (256, 3)
    Xt = fos.fista(At, torch.as_tensor(B).cuda(), "lasso", 1.0, 0.0, max_iter=15, L=L)
    assert isinstance(Xt, torch.Tensor) and Xt.is_cuda and tuple(Xt.shape) == (256, 3)
    assert _data.rel(_np(Xt), X) < 1e-6
    # a vector, in any orientation, stays a single-target call with a 1-D result
    b = B[:, 0].copy()
    x1 = fos.fista(A32, b, "lasso", 1.0, 0.0, max_iter=15, L=L)
    x2 = fos.fista(A32, b[:, None], "lasso", 1.0, 0.0, max_iter=15, L=L)
    assert x1.shape == (256,) and x2.shape == (256,) and np.array_equal(x1, x2)
    # a Problem with its own b: that b is used, the argument ignored (as before)
    P = fos.prepare(A32, b)
    assert np.array_equal(fos.fista(P, B, "lasso", 1.0, 0.0, max_iter=15, L=L), x1)
    for kw in (dict(return_history=True), dict(comm=object()), dict(cols=(0, 256, 256))):
        with pytest.raises(ValueError):
            fos.fista(A32, B, "lasso", 1.0, 0.0, max_iter=5, L=L, **kw)


@pytest.mark.parametrize("kind,n,k", [("f32", 512, 16), ("f32", 512, 3), ("bf16", 1024, 16), ("f32", 16, 3)])
def test_compute_objective_sums_the_columns(fos, kind, n, k):
    At, A64, B = _case(kind, 2000, n, k, 41 + k)
    X = _np(fos.fista(At, B, "elasticnet", 1.0, 0.5, max_iter=10, L=_L(A64)))
    X32 = X.astype(np.float32).astype(np.float64)          # the pass over A reads x in fp32
    for reg in ("lasso", "ridge", "elasticnet"):
        ref = sum(orc.compute_objective(X32[:, j], A64, B[:, j].astype(np.float64), reg, 1.0, 0.5) for j in range(k))
        got = fos.compute_objective(X, At, B, reg, 1.0, 0.5)
        assert got == pytest.approx(ref, rel=1e-6), (reg, got, ref)
