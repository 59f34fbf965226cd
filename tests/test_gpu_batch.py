"""GPU: batches of small independent problems - fista(A, b) / fista_delta(A, b) with a 3-D A or a sequence of matrices, one
workgroup per problem in one launch (fos_fista_run_batch).  Every member must equal its own single call (same kernel body,
same arithmetic: 1e-12 and the same iteration count) and the fp64 oracle (1e-5 relative, on the bf16-rounded A for bf16
storage); the global NumPy stream, the metric lists and the histories must be those of P single calls."""
import numpy as np
import pytest
import torch

from oracle import fos_oracle as orc
from tests import _data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def _batch(P, m, n, seed, kind="f32", scales=None):
    """(A as handed in, its fp64 value as stored, b (P x m fp32))."""
    rng = np.random.default_rng(seed)
    A = np.stack([_data.synth(m, n, seed + i)[0] for i in range(P)]).astype(np.float32)
    if kind == "bf16":
        At = torch.as_tensor(A).to(torch.bfloat16)
        A64 = At.to(torch.float64).numpy()
    else:
        At, A64 = A, A.astype(np.float64)
    X = np.zeros((P, n))
    for i in range(P):
        idx = rng.choice(n, max(1, n // 5), replace=False)
        X[i, idx] = rng.standard_normal(idx.size)
    b = np.einsum("pmn,pn->pm", A64, X) + 0.1 * rng.standard_normal((P, m))
    if scales is not None:
        b = b * np.asarray(scales)[:, None]
    return At, A64, b.astype(np.float32)


def _rel(a, b):
    return float(np.linalg.norm(_np(a) - _np(b)) / max(np.linalg.norm(_np(b)), 1e-30))


def _a1(A64, b):
    return [0.1 * float(np.max(np.abs(A64[i].T @ b[i].astype(np.float64)))) for i in range(len(b))]


CASES = [(7, 1000, 5, "f32"), (33, 600, 12, "f32"), (5, 200, 40, "bf16")]


@pytest.mark.parametrize("P,m,n,kind", CASES)
@pytest.mark.parametrize("solver", ["fista", "fista_delta"])
@pytest.mark.parametrize("reg", ["lasso", "elasticnet"])
def test_uniform_batch_matches_single_calls_and_oracle(fos, P, m, n, kind, solver, reg):
    At, A64, b = _batch(P, m, n, 11 + n, kind=kind)
    a1 = float(np.median(_a1(A64, b)))
    a2 = 0.05 if reg == "elasticnet" else 0.0
    Ls = [float(np.linalg.norm(A64[i], 2) ** 2) for i in range(P)]
    extra = (3.0,) if solver == "fista_delta" else ()
    dt = dict(dtype="bf16") if kind == "bf16" else {}
    fn, ofn = getattr(fos, solver), getattr(orc, solver)
    X = fn(At, b, reg, a1, a2, *extra, max_iter=150, L=Ls, **dt)
    assert tuple(X.shape) == (P, n)
    assert isinstance(X, torch.Tensor) if kind == "bf16" else (isinstance(X, np.ndarray) and X.dtype == np.float64)
    for i in range(P):
        x1 = _np(fn(At[i], b[i], reg, a1, a2, *extra, max_iter=150, L=Ls[i], **dt))
        assert np.max(np.abs(_np(X[i]) - x1)) <= 1e-12 * max(1.0, np.max(np.abs(x1))), i
        xo = ofn(A64[i], b[i].astype(np.float64), reg, a1, a2, *extra, max_iter=150, L=Ls[i])
        assert _rel(X[i], xo) < 1e-5, (i, _rel(X[i], xo))


def test_own_L_keeps_the_rng_stream(fos):
    P, m, n = 6, 400, 7
    At, A64, b = _batch(P, m, n, 3)
    a1 = float(np.median(_a1(A64, b)))
    np.random.seed(5)
    X = fos.fista(At, b, "lasso", a1, 0.0, max_iter=80)
    state_batch = np.random.get_state()
    np.random.seed(5)
    singles = [fos.fista(At[i], b[i], "lasso", a1, 0.0, max_iter=80) for i in range(P)]
    state_single = np.random.get_state()
    assert state_batch[0] == state_single[0] and np.array_equal(state_batch[1], state_single[1])
    assert state_batch[2:] == state_single[2:]
    for i in range(P):
        assert np.max(np.abs(X[i] - singles[i])) <= 1e-12 * max(1.0, np.max(np.abs(singles[i])))
    np.random.seed(9)
    Lb = fos.estimate_lipschitz(At)
    np.random.seed(9)
    Ls = [fos.estimate_lipschitz(At[i]) for i in range(P)]
    assert Lb.dtype == np.float64 and Lb.shape == (P,)
    assert list(Lb) == Ls
    np.random.seed(9)
    Lq = fos.estimate_lipschitz([At[i] for i in range(P)])
    assert list(Lq) == Ls


@pytest.mark.parametrize("solver", ["fista", "fista_delta"])
def test_per_problem_control_matches_oracle(fos, solver):
    """b scaled per problem so the runs stop at different iterations; backtracking at t_init 2.0, tol, tol_ratio and
    adaptive restart decided per problem; the metric lists are the sums of the oracle's per-problem metrics."""
    P, m, n = 6, 500, 6
    scales = [1.0, 0.3, 3.0, 0.05, 10.0, 1.0]
    At, A64, b = _batch(P, m, n, 21, scales=scales)
    a1 = float(np.median(_a1(A64, b)))
    Ls = [float(np.linalg.norm(A64[i], 2) ** 2) for i in range(P)]
    kw = dict(backtracking=True, t_init_factor=2.0, max_iter=400, tol=1e-6, tol_ratio=0.0)
    if solver == "fista":
        kw.update(adaptive_restart=True)
    extra = (3.0,) if solver == "fista_delta" else ()
    X, H = getattr(fos, solver)(At, b, "lasso", a1, 0.0, *extra, L=Ls, return_history=True, **kw)
    met = fos.get_metrics()
    keys = ("grad_num_calls", "ls_num_calls", "ls_iters_total")
    tot, tot1 = dict.fromkeys(keys, 0), dict.fromkeys(keys, 0)
    stops = set()
    for i in range(P):
        (xo, ho), mo = getattr(orc, solver)(A64[i], b[i].astype(np.float64), "lasso", a1, 0.0, *extra, L=Ls[i],
                                             return_history=True, return_metrics=True, **kw)
        x1, h1 = getattr(fos, solver)(At[i], b[i], "lasso", a1, 0.0, *extra, L=Ls[i], return_history=True, **kw)
        m1 = fos.get_metrics()
        assert len(H[i]["obj"]) == len(ho["obj"]) == len(h1["obj"]), i      # the stop iteration
        stops.add(len(ho["obj"]))
        assert _rel(X[i], xo) < 1e-5, i
        assert np.max(np.abs(X[i] - x1)) <= 1e-12 * max(1.0, np.max(np.abs(x1))), i
        for key in keys:
            tot[key] += mo[key]
            tot1[key] += m1[key]
    assert len(stops) > 1, "the scaled problems should stop at different iterations"
    for key in keys:
        assert met[key] == tot1[key], (key, met[key], tot1[key])          # P single calls, exactly
    # the oracle's counts: searches and gradients exactly; the shrinks of a search can differ where the fp64 comparison
    # g(x_tmp) <= g(y) + C*grad.dlt is a near tie in another summation order (as for the single call)
    assert met["grad_num_calls"] == tot["grad_num_calls"] and met["ls_num_calls"] == tot["ls_num_calls"]
    assert abs(met["ls_iters_total"] - tot["ls_iters_total"]) <= max(2, 0.05 * tot["ls_iters_total"])
    # tol_ratio per problem, plain runs
    kw2 = dict(max_iter=300, tol_ratio=0.999)
    X2 = getattr(fos, solver)(At, b, "lasso", a1, 0.0, *extra, L=Ls, **kw2)
    for i in range(P):
        x1 = getattr(fos, solver)(At[i], b[i], "lasso", a1, 0.0, *extra, L=Ls[i], **kw2)
        assert np.max(np.abs(X2[i] - x1)) <= 1e-12 * max(1.0, np.max(np.abs(x1)))


@pytest.mark.parametrize("solver", ["fista", "fista_delta"])
def test_history_matches_single_calls(fos, solver):
    P, m, n = 4, 300, 9
    At, A64, b = _batch(P, m, n, 31)
    a1 = float(np.median(_a1(A64, b)))
    Ls = [float(np.linalg.norm(A64[i], 2) ** 2) for i in range(P)]
    extra = (3.0,) if solver == "fista_delta" else ()
    fn = getattr(fos, solver)
    X, H = fn(At, b, "elasticnet", a1, 0.05, *extra, max_iter=60, tol=1e-7, L=Ls, return_history=True)
    assert isinstance(H, list) and len(H) == P
    for i in range(P):
        x1, h1 = fn(At[i], b[i], "elasticnet", a1, 0.05, *extra, max_iter=60, tol=1e-7, L=Ls[i], return_history=True)
        assert len(H[i]["x"]) == len(h1["x"]) and len(H[i]["obj"]) == len(h1["obj"])
        for u, v in zip(H[i]["x"], h1["x"]):
            assert np.max(np.abs(u - v)) <= 1e-12 * max(1.0, np.max(np.abs(v)))
        np.testing.assert_allclose(H[i]["obj"], h1["obj"], rtol=1e-9)


def test_ragged_sequence_with_fallback(fos):
    """n <= 8 and n > 8 (both register classes) in one call, plus a member beyond the LDS limits that falls back."""
    shapes = [(300, 5), (400, 20), (2500, 3), (120, 64), (1500, 40), (50, 8)]     # (1500, 40): not resident
    mats, vecs = [], []
    for j, (m, n) in enumerate(shapes):
        A, _, _ = _data.synth(m, n, 40 + j)
        A = A.astype(np.float32)
        mats.append(A)
        vecs.append((A.astype(np.float64) @ np.linspace(-1, 1, n) + 0.1).astype(np.float32))
    a1 = 0.5
    for bt in (False, True):
        np.random.seed(2)
        xs = fos.fista(mats, vecs, "lasso", a1, 0.0, max_iter=120, backtracking=bt, tol=1e-7)
        met = fos.get_metrics()
        state = np.random.get_state()
        assert isinstance(xs, list) and len(xs) == len(shapes)
        np.random.seed(2)
        tot = {"grad_num_calls": 0, "ls_iters_total": 0}
        for i, (A, b) in enumerate(zip(mats, vecs)):
            x1 = fos.fista(A, b, "lasso", a1, 0.0, max_iter=120, backtracking=bt, tol=1e-7)
            m1 = fos.get_metrics()
            for key in tot:
                tot[key] += m1[key]
            assert xs[i].shape == (shapes[i][1],)
            assert np.max(np.abs(xs[i] - x1)) <= 1e-12 * max(1.0, np.max(np.abs(x1))), i
        assert np.array_equal(np.random.get_state()[1], state[1])
        for key in tot:
            assert met[key] == tot[key], key


def test_edge_cases_and_types(fos):
    At, A64, b = _batch(3, 100, 4, 51)
    L = float(max(np.linalg.norm(A64[i], 2) ** 2 for i in range(3)))
    assert fos.fista(np.zeros((0, 10, 4), np.float32), np.zeros((0, 10), np.float32), "lasso", 0.1, 0.0).shape == (0, 4)
    assert fos.fista([], [], "lasso", 0.1, 0.0) == []
    X0 = fos.fista(At, b, "lasso", 0.1, 0.0, max_iter=0, L=[1.0, 2.0, 3.0])
    assert X0.shape == (3, 4) and not X0.any()
    X0h, H0 = fos.fista(At, b, "lasso", 0.1, 0.0, max_iter=0, L=2.0, return_history=True)
    assert all(len(h["x"]) == 1 and h["obj"] == [] for h in H0)
    Xt = fos.fista(torch.as_tensor(At).cuda(), torch.as_tensor(b).cuda(), "lasso", 0.1, 0.0, max_iter=50, L=L)
    assert isinstance(Xt, torch.Tensor) and Xt.shape == (3, 4) and Xt.is_cuda
    x1 = fos.fista(torch.as_tensor(At[1]).cuda(), torch.as_tensor(b[1]).cuda(), "lasso", 0.1, 0.0, max_iter=50, L=L)
    assert Xt.dtype == x1.dtype and torch.equal(Xt[1], x1)
    Xn = fos.fista(At, b, "lasso", 0.1, 0.0, max_iter=50, L=L)
    assert isinstance(Xn, np.ndarray) and np.max(np.abs(Xn[1] - _np(x1))) < 1e-6


@pytest.mark.parametrize("kw", [dict(backtracking=True, t_init_factor=2.0), dict(tol=1e-6), dict(tol_ratio=0.999)])
def test_several_targets_on_a_resident_A_run_as_one_batch(fos, kw):
    m, n, k = 1000, 5, 16
    A, _, _ = _data.synth(m, n, 61)
    A = A.astype(np.float32)
    rng = np.random.default_rng(1)
    B = (A.astype(np.float64) @ rng.standard_normal((n, k)) + 0.1 * rng.standard_normal((m, k))).astype(np.float32)
    L = float(np.linalg.norm(A.astype(np.float64), 2) ** 2)
    X = fos.fista(A, B, "lasso", 0.5, 0.0, max_iter=200, L=L, **kw)
    met = fos.get_metrics()
    assert X.shape == (n, k)
    tot = 0
    for j in range(k):
        x1 = fos.fista(A, B[:, j], "lasso", 0.5, 0.0, max_iter=200, L=L, **kw)
        tot += fos.get_metrics()["grad_num_calls"]
        assert np.all(np.isfinite(x1)) and np.max(np.abs(X[:, j] - x1)) <= 1e-12 * max(1.0, np.max(np.abs(x1))), j
    assert met["grad_num_calls"] == tot
