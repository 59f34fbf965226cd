"""GPU: K-fold cross-validation in lockstep - fista_cv, fos_fista_run_multi_folds, fos_residual_batch_folds.

Every (fold, weight) fit must equal the fp64 oracle's fista / fista_delta on the GATHERED training rows with the same L
(1e-5 relative, on the bf16-rounded A for bf16 storage); L comes from the oracle's power iteration on the whole A and is
passed to both sides.  The held-out squared error is compared against fp64 NumPy on the kernel's OWN x rounded to fp32,
within tests/_data.fp32_pass_tolerances_cols for that column: this isolates the mask from solver drift.  The shapes are the
rows of tests/_menu_cv.py (the smallest at which the mask can go wrong), built for the CU count Problem.plan() reports."""
import numpy as np
import pytest
import torch

from oracle import fos_oracle as orc
from tests import _data, _menu_cv as mc

pytestmark = pytest.mark.gpu

TOL = 1e-5
ITERS = 30


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


@pytest.fixture(scope="module")
def cus(fos):
    return int(fos.prepare(torch.zeros(8, 68, device="cuda")).plan()["cus"])


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def _problem(kind, m, n, seed):
    """Device A (fp32 / bf16), its fp64 value as stored, b (fp32-representable, as the device keeps it) and L of the whole A."""
    A, b, _ = _data.synth(m, n, seed)
    At = torch.as_tensor(A.astype(np.float32)).to(torch.bfloat16 if kind == "bf16" else torch.float32).cuda()
    A64 = At.to(torch.float64).cpu().numpy()
    b = b.astype(np.float32).astype(np.float64)
    L = float(orc.estimate_lipschitz(A64, v0=np.random.default_rng(seed + 1).standard_normal(n)))
    return At, A64, b, L


def _alphas(A64, b, count):
    """A cross-validation grid below alpha_max = max |A^T b| (above it every fit is zero): lasso and elastic-net weights."""
    amax = float(np.max(np.abs(A64.T @ b)))
    return [(0.3 * amax, 0.0), (0.1 * amax, 0.5), (0.03 * amax, 0.0)][:count]


def _served(m, n, kind):
    """Whether the device copy of A has aligned rows (as given, or zero-padded by Problem from 2^20 elements on): the shapes
    the masked lockstep serves; the others take fista_cv's fold-by-fold path."""
    return n % (8 if kind == "bf16" else 4) == 0 or m * n >= (1 << 20)


def _check(fos, res, A64, b, ids, alphas, L, iters=ITERS, delta=None, **kw):
    """Every column against the oracle on the gathered rows; every held-out error against fp64 on the kernel's own x."""
    K, La = int(ids.max()) + 1, len(alphas)
    coefs = _np(res.coefs)
    assert coefs.shape == (A64.shape[1], K, La) and res.mse.shape == (K, La) and res.mse.dtype == np.float64
    for f in range(K):
        tr, te = ids != f, ids == f
        for a, (a1, a2) in enumerate(alphas):
            if delta is None:
                x_ref = orc.fista(A64[tr], b[tr], "elasticnet", a1, a2, max_iter=iters, L=L, **kw)
            else:
                x_ref = orc.fista_delta(A64[tr], b[tr], "elasticnet", a1, a2, delta, max_iter=iters, L=L, **kw)
            assert _data.rel(coefs[:, f, a], x_ref) < TOL, (f, a, _data.rel(coefs[:, f, a], x_ref))
        X32 = coefs[:, f, :].astype(np.float32).astype(np.float64)          # the pass over A reads x in fp32
        R = A64[te] @ X32 - b[te][:, None]
        sse_ref = (R * R).sum(axis=0)
        _, tol = _data.fp32_pass_tolerances_cols(A64[te], X32, b[te], np.zeros_like(X32), sse_ref)
        got = res.mse[f] * int(te.sum())
        print(f"fold {f}: sse {got} ref {sse_ref} err/tol {np.abs(got - sse_ref) / tol}")
        assert np.isfinite(got).all() and (np.abs(got - sse_ref) <= tol).all(), (f, got, sse_ref, tol)
    assert np.allclose(res.mean_mse, res.mse.mean(axis=0), rtol=1e-14) and res.best == int(np.argmin(res.mean_mse))


def _cv_cases():
    out = []
    for name in ("one_tile", "edges", "rb2", "panels"):
        out += [(name, "f32", None), (name, "bf16", None)]
        if name != "edges":
            out.append((name, "bf16", 68))       # the fp32 width on bf16 storage: ragged rows (fold by fold, or zero-padded)
    return out


@pytest.mark.parametrize("name,kind,width", _cv_cases())
def test_fista_cv_matches_the_oracle_on_gathered_rows(fos, cus, name, kind, width):
    c = mc.shapes(kind, cus)[name]
    m, n, nalpha = c["m"], width or c["n"], c["nalpha"]
    ids = mc.fold_ids(c, seed=m)
    K = c["folds"][1]
    At, A64, b, L = _problem(kind, m, n, 3 * m + n)
    alphas = _alphas(A64, b, nalpha)
    P = fos.prepare(At, b)
    P.profile(1)
    P.profile_read()
    folds = K if c["folds"][0] == "contiguous" else ids
    res = fos.fista_cv(P, None, alphas, folds, max_iter=ITERS, L=L, refit=False, return_coefs=True)
    _, launches = P.profile_read()
    P.profile(0)
    groups = -(-K * nalpha // 16)
    if _served(m, n, kind):
        # the masked lockstep on the one bound A: one bracketed pass per iteration per group, one for the held-out errors
        assert launches == groups * (ITERS + 1), (launches, groups)
        assert fos.get_metrics()["grad_num_calls"] == groups * ITERS
    else:
        assert launches == 0, launches               # fold by fold on gathered copies: nothing ran on P
    assert res.x is None and all(i == (ITERS, 0) for row in res.info for i in row), res.info
    _check(fos, res, A64, b, ids, alphas, L)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_fista_delta_cv(fos, cus, kind):
    c = mc.shapes(kind, cus)["edges"]
    At, A64, b, L = _problem(kind, c["m"], c["n"], 77)
    alphas = _alphas(A64, b, 3)
    res = fos.fista_cv(At, b, alphas, 5, max_iter=ITERS, L=L, delta=3.0, refit=False, return_coefs=True)
    assert isinstance(res.coefs, torch.Tensor) and res.coefs.is_cuda
    _check(fos, res, A64, b, mc.fold_ids(c), alphas, L, delta=3.0)


@pytest.mark.parametrize("kind,kw", [("f32", dict(adaptive_restart=True, tol_ratio=1e-3)),
                                     ("bf16", dict(adaptive_restart=True, tol_ratio=1e-3)),
                                     ("f32", dict(adaptive_restart=True, restart_threshold=0.9, tol_ratio=0.5))],
                         ids=["f32", "bf16", "f32-early-stops"])
def test_controlled_run_keeps_per_column_control(fos, kind, kw):
    """18 columns -> two groups, the second of 2: restarts and the ratio stop per column inside the masked lockstep; every
    column runs the oracle's number of iterations and ends on the oracle's iterate, whatever its neighbours did."""
    m, n, K, iters = 1001, 200, 6, 60
    At, A64, b, L = _problem(kind, m, n, 501)
    alphas = _alphas(A64, b, 3)
    res = fos.fista_cv(At, b, alphas, K, max_iter=iters, L=L, refit=False, return_coefs=True, **kw)
    ids = mc.fold_ids(dict(m=m, folds=("contiguous", K)))
    stops = np.zeros((K, 3), dtype=int)
    for f in range(K):
        for a, (a1, a2) in enumerate(alphas):
            _, h = orc.fista(A64[ids != f], b[ids != f], "elasticnet", a1, a2, max_iter=iters, L=L, return_history=True, **kw)
            stops[f, a] = len(h["obj"])
    got = np.array([[i[0] for i in row] for row in res.info])
    print("iterations", got.tolist(), "oracle", stops.tolist())
    assert np.array_equal(got, stops), (got, stops)
    assert all(i[1] != 0 for row in res.info for i in row if i[0] < iters), res.info       # fewer iterations: a stop code
    if kw["tol_ratio"] == 0.5:
        assert len(set(stops.ravel().tolist())) > 1 and stops.min() < iters, stops      # columns did stop at different iterations
        assert fos.get_metrics()["grad_num_calls"] == int(stops.ravel()[:16].max() + stops.ravel()[16:].max())
    _check(fos, res, A64, b, ids, alphas, L, iters=iters, **kw)


def _handles(fos, P, alphas, L, count):
    from fastoptsolver_amd import _core
    hs = []
    for j in range(count):
        a1, a2 = alphas[j % len(alphas)]
        st = _core.Fista(P)
        st.reset(1.0 / (L + a2), a1, a2)
        hs.append(st)
    return hs


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_c_level_entry_points(fos, cus, kind):
    from fastoptsolver_amd import _core
    c = mc.shapes(kind, cus)["edges"]
    m, n = c["m"], c["n"]
    ids = mc.fold_ids(c)
    At, A64, b, L = _problem(kind, m, n, 909)
    alphas = _alphas(A64, b, 3)
    P = fos.prepare(At, b)
    ids_dev = _core.fold_ids_tensor(ids, P.device)
    assert ids_dev.numel() == 1004 and ids_dev.data_ptr() % 4 == 0
    # held = -1 everywhere: every column keeps every row - the unmasked lockstep on handles of the same parameters
    masked, plain = _handles(fos, P, alphas, L, 15), _handles(fos, P, alphas, L, 15)
    assert _core.run_multi_folds(masked, ids_dev, [-1] * 15, ITERS)
    assert _core.run_multi(plain, ITERS)
    for j, (u, v) in enumerate(zip(masked, plain)):
        assert _data.rel(_np(u.x_tensor()), _np(v.x_tensor())) < 1e-6, j
    # one state machine is served (the alternative is a copy of the rows)
    one = _handles(fos, P, alphas[1:], L, 1)
    assert _core.run_multi_folds(one, ids_dev, [2], ITERS)
    a1, a2 = alphas[1]
    x_ref = orc.fista(A64[ids != 2], b[ids != 2], "elasticnet", a1, a2, max_iter=ITERS, L=L)
    assert _data.rel(_np(one[0].x_tensor()), x_ref) < TOL
    # the held-out pass: -1 holds no row, a fold id its rows
    X = torch.stack([st.x_tensor() for st in masked[:5]], dim=1)
    assert P.residual_batch_folds(X, ids_dev, [-1] * 5) == [0.0] * 5
    got = np.array(P.residual_batch_folds(X, ids_dev, [0, 4, -1, 2, 2]))
    X32 = _np(X).astype(np.float32).astype(np.float64)
    assert got[2] == 0.0
    for j, f in ((0, 0), (1, 4), (3, 2), (4, 2)):
        te = ids == f
        r = A64[te] @ X32[:, j] - b[te]
        ref = float(r @ r)
        _, tol = _data.fp32_pass_tolerances_cols(A64[te], X32[:, j:j + 1], b[te], np.zeros((n, 1)), np.array([ref]))
        assert abs(got[j] - ref) <= tol[0], (j, f, got[j], ref, tol[0])


def test_unserved_configurations_are_refused_not_run(fos):
    """FOS_ERR_UNSUPPORTED (False here), nothing run: a problem without b, the resident plan, a handle with the gradient-norm rule."""
    from fastoptsolver_amd import _core
    At, A64, b, L = _problem("f32", 1001, 200, 31)
    ids = np.arange(1001) % 3
    for P, tol_grad in ((fos.prepare(At), 0.0), (fos.prepare(At[:, :4].contiguous(), b), 0.0), (fos.prepare(At, b), 1e-3)):
        ids_dev = _core.fold_ids_tensor(ids, P.device)
        hs = [_core.Fista(P) for _ in range(3)]
        for st in hs:
            st.reset(1.0 / L, 1.0, 0.0, tol_grad=tol_grad)
        assert _core.run_multi_folds(hs, ids_dev, [0, 1, 2], 5) is False
        assert all(int(st.status().k) == 0 for st in hs)
        if tol_grad == 0.0:
            assert P.residual_batch_folds(torch.zeros(P.n, 3, device="cuda"), ids_dev, [0, 1, 2]) is None


def test_fallback_on_the_resident_plan_equals_the_oracle(fos):
    m, n, K = 1000, 5, 4
    At, A64, b, L = _problem("f32", m, n, 12)
    P = fos.prepare(At, b)
    assert P.plan()["resident"] == 1
    amax = float(np.max(np.abs(A64.T @ b)))
    alphas = [(0.5 * amax, 0.0), (0.05 * amax, 0.1), (0.001 * amax, 0.0)]
    ids = np.random.default_rng(4).permutation(m) % K
    res = fos.fista_cv(P, None, alphas, ids, max_iter=50, L=L, return_coefs=True)
    _check(fos, res, A64, b, ids, alphas, L, iters=50)
    mse_ref = np.zeros((K, 3))
    for f in range(K):
        for a, (a1, a2) in enumerate(alphas):
            x = orc.fista(A64[ids != f], b[ids != f], "elasticnet", a1, a2, max_iter=50, L=L)
            r = A64[ids == f] @ x - b[ids == f]
            mse_ref[f, a] = float(r @ r) / int((ids == f).sum())
    assert res.best == int(np.argmin(mse_ref.mean(axis=0)))
    assert np.allclose(res.mse, mse_ref, rtol=1e-4)
    assert _data.rel(_np(res.x), orc.fista(A64, b, "elasticnet", *alphas[res.best], max_iter=50, L=L)) < TOL


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_refit_is_the_all_rows_fit_at_the_best_weight(fos, cus, kind):
    c = mc.shapes(kind, cus)["edges"]
    At, A64, b, L = _problem(kind, c["m"], c["n"], 2024)
    alphas = _alphas(A64, b, 3)
    A_in = At.cpu().numpy() if kind == "f32" else At               # results come back as the kind that went in
    res = fos.fista_cv(A_in, b, alphas, 5, max_iter=ITERS, L=L)
    assert res.coefs is None and res.alphas == [tuple(map(float, a)) for a in alphas]
    x_path = fos.fista_path(A_in, b, [alphas[res.best]], max_iter=ITERS, L=L)[0]
    assert type(res.x) is (np.ndarray if kind == "f32" else torch.Tensor)
    assert np.array_equal(_np(res.x), _np(x_path))
    assert _data.rel(_np(res.x), orc.fista(A64, b, "elasticnet", *alphas[res.best], max_iter=ITERS, L=L)) < TOL


def test_lipschitz_is_estimated_once_on_the_whole_matrix(fos, cus):
    c = mc.shapes("f32", cus)["edges"]
    At, A64, b, _ = _problem("f32", c["m"], c["n"], 5)
    np.random.seed(123)
    fos.fista_path(At, b, [(1.0, 0.0)], max_iter=3)
    one_call = np.random.get_state()[1].copy()
    np.random.seed(123)
    L = float(orc.estimate_lipschitz(A64))
    np.random.seed(123)
    res = fos.fista_cv(At, b, [(1.0, 0.0), (0.5, 0.0)], 5, max_iter=ITERS, return_coefs=True)
    assert np.array_equal(np.random.get_state()[1], one_call)
    x_ref = orc.fista(A64[201:], b[201:], "lasso", 1.0, 0.0, max_iter=ITERS, L=L)
    assert _data.rel(_np(res.coefs)[:, 0, 0], x_ref) < 1e-4          # L itself is an fp32 power iteration here
