"""GPU: sparse logistic regression in the lockstep - logistic_path, logistic_cv, logistic_objective.

Every fit must equal the fp64 reference of tests/_logit.py (the oracle's FistaProblem with the logistic gradient: the same
momentum, restart and stop rules) within 1e-5 relative, on the bf16-rounded A for bf16 storage; L = lambda_max(A^T A) / 4
comes from the oracle's power iteration and is passed to both sides.  Log-loss sums are compared against fp64 on the kernel's
OWN x rounded to fp32 within tests/_logit.nll_tolerance, which isolates the epilogue from solver drift.  The shapes are those of
tests/_menu_cv.py (imported through tests/_menu_logit.py), built for the CU count Problem.plan() reports."""
import functools

import numpy as np
import pytest
import torch

from oracle import fos_oracle as orc
from tests import _data, _logit as lg, _menu_logit as ml

pytestmark = pytest.mark.gpu

TOL, ITERS = lg.TOL, lg.ITERS
NAMES = ("one_tile", "edges", "rb2", "panels")
KINDS = ("f32", "bf16")


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


def _bf16(A32):
    return torch.as_tensor(A32).to(torch.bfloat16).to(torch.float64).numpy()


@functools.lru_cache(maxsize=None)
def _recipe(kind, m, n, seed):
    """(A as the device stores it in fp64, labels, L, the three weights): computed once per shape, never modified."""
    A64, y, _, L = lg.recipe(m, n, seed, _bf16 if kind == "bf16" else None)
    for a in (A64, y):
        a.setflags(write=False)
    return A64, y, L, tuple(lg.weights(A64, y))


def _device(kind, A64):
    return torch.as_tensor(A64.astype(np.float32)).to(torch.bfloat16 if kind == "bf16" else torch.float32).cuda()


@functools.lru_cache(maxsize=None)
def _ref(kind, m, n, seed, a1, a2, iters, delta, rows=None, **kw):
    """(x, iterations) of the reference; rows: a fold id and K as (f, K, kind of split) -> the fit on the other rows."""
    A64, y, L, _ = _recipe(kind, m, n, seed)
    if rows is not None:
        keep = _ids(m, rows[1], rows[2], seed) != rows[0]
        A64, y = A64[keep], y[keep]
    x, k = lg.run(A64, y, a1, a2, L, iters, delta=delta, **kw)
    x.setflags(write=False)
    return x, k


@functools.lru_cache(maxsize=None)
def _ids(m, K, split, seed):
    ids = ml.fold_ids(dict(m=m, folds=(split, K)), seed=seed)
    ids.setflags(write=False)
    return ids


def _case(kind, cus, name):
    c = ml.shapes(kind, cus)[name]
    return c, 3 * c["m"] + c["n"]


# ---- logistic_path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [None, 3.0], ids=["fista", "delta"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_logistic_path_matches_the_reference(fos, cus, name, kind, delta):
    c, seed = _case(kind, cus, name)
    m, n = c["m"], c["n"]
    A64, y, L, alphas = _recipe(kind, m, n, seed)
    P = fos.prepare(_device(kind, A64), y, loss="logistic")
    xs, info = fos.logistic_path(P, None, alphas, max_iter=ITERS, L=L, delta=delta, return_info=True)
    assert len(xs) == 3 and info == [(ITERS, 0)] * 3, info
    assert fos.get_metrics()["grad_num_calls"] == ITERS
    for (a1, a2), x in zip(alphas, xs):
        x_ref, _ = _ref(kind, m, n, seed, a1, a2, ITERS, delta)
        err = _data.rel(_np(x), x_ref)
        print(f"{name} {kind} delta={delta} alpha=({a1:.3g}, {a2}) rel err {err:.3e} nnz {int(np.count_nonzero(x_ref))}")
        assert np.linalg.norm(x_ref) > 0 and err < TOL, (a1, a2, err)


@functools.lru_cache(maxsize=None)
def _many_weights(kind, m, n, seed):
    _, _, _, alphas = _recipe(kind, m, n, seed)
    return tuple((a1 * 0.93 ** (j // 3), a2) for j in range(18) for a1, a2 in [alphas[j % 3]])


@pytest.fixture(scope="module")
def alone(fos, cus):
    """Every one of the 18 weights run alone (a one-column lockstep), once per storage type."""
    out = {}

    def get(kind):
        if kind not in out:
            c, seed = _case(kind, cus, "edges")
            A64, y, L, _ = _recipe(kind, c["m"], c["n"], seed)
            P = fos.prepare(_device(kind, A64), y, loss="logistic")
            out[kind] = [_np(fos.logistic_path(P, None, [w], max_iter=ITERS, L=L)[0])
                         for w in _many_weights(kind, c["m"], c["n"], seed)]
        return out[kind]
    return get


@pytest.mark.parametrize("count", [1, 3, 16, 18])
@pytest.mark.parametrize("kind", KINDS)
def test_group_sizes_all_go_through_the_lockstep(fos, cus, alone, kind, count):
    c, seed = _case(kind, cus, "edges")
    m, n = c["m"], c["n"]
    A64, y, L, _ = _recipe(kind, m, n, seed)
    ws = list(_many_weights(kind, m, n, seed))[:count]
    P = fos.prepare(_device(kind, A64), y, loss="logistic")
    P.profile(1)
    P.profile_read()
    xs = fos.logistic_path(P, None, ws, max_iter=ITERS, L=L)
    _, launches = P.profile_read()
    P.profile(0)
    groups = -(-count // 16)
    assert launches == groups * ITERS, (launches, groups)          # one bracketed two-product pass per iteration per group
    assert fos.get_metrics()["grad_num_calls"] == groups * ITERS
    single = alone(kind)
    for j, x in enumerate(xs):
        assert _data.rel(_np(x), single[j]) < 1e-6, (j, _data.rel(_np(x), single[j]))
    x_ref, _ = _ref(kind, m, n, seed, ws[-1][0], ws[-1][1], ITERS, None)
    assert _data.rel(_np(xs[-1]), x_ref) < TOL


# ---- device control ----------------------------------------------------------------------------------------------------
CTRL = dict(adaptive_restart=True, restart_threshold=0.9, tol_ratio=0.5)


@pytest.mark.parametrize("kind", KINDS)
def test_device_control_per_column(fos, kind):
    """18 masked columns in two groups, 60 iterations: restarts and the ratio stop per column.  The reference stops the
    heaviest weight early in every fold and runs the others to the end; every column must run the reference's number of
    iterations, end with its stop code and on its iterate."""
    m, n, K, iters, seed = 1001, 200, 6, 60, 501
    A64, y, L, alphas = _recipe(kind, m, n, seed)
    ids = _ids(m, K, "contiguous", seed)
    want = np.zeros((K, 3), dtype=int)
    refs = {}
    for f in range(K):
        for a, (a1, a2) in enumerate(alphas):
            refs[f, a], want[f, a] = _ref(kind, m, n, seed, a1, a2, iters, None, rows=(f, K, "contiguous"), **CTRL)
    print("reference iterations", want.tolist())
    assert want.min() < iters and want.max() == iters, want          # both early and full-length columns: not vacuous
    res = fos.logistic_cv(_device(kind, A64), y, alphas, K, max_iter=iters, L=L, refit=False, return_coefs=True, **CTRL)
    got = np.array([[i[0] for i in row] for row in res.info])
    codes = np.array([[i[1] for i in row] for row in res.info])
    print("device iterations", got.tolist(), "codes", codes.tolist())
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(codes, np.where(want < iters, 2, 0)), codes       # FOS_STOP_RATIO where the reference stopped
    coefs = _np(res.coefs)
    for (f, a), x_ref in refs.items():
        assert _data.rel(coefs[:, f, a], x_ref) < TOL, (f, a, _data.rel(coefs[:, f, a], x_ref))
    # the unmasked lockstep under the same control
    xs, info = fos.logistic_path(_device(kind, A64), y, alphas, max_iter=iters, L=L, return_info=True, **CTRL)
    for (a1, a2), x, (k, code) in zip(alphas, xs, info):
        x_ref, k_ref = _ref(kind, m, n, seed, a1, a2, iters, None, **CTRL)
        assert (k, code) == (k_ref, 2 if k_ref < iters else 0) and _data.rel(_np(x), x_ref) < TOL, (a1, k, k_ref, code)


# ---- logistic_cv -------------------------------------------------------------------------------------------------------
def _check_cv(res, kind, m, n, seed, ids, split, alphas, iters=ITERS):
    A64, y, L, _ = _recipe(kind, m, n, seed)
    K, La = int(ids.max()) + 1, len(alphas)
    coefs = _np(res.coefs)
    assert coefs.shape == (n, K, La) and res.logloss.shape == (K, La) and res.logloss.dtype == np.float64
    for f in range(K):
        te = ids == f
        for a, (a1, a2) in enumerate(alphas):
            x_ref, _ = _ref(kind, m, n, seed, a1, a2, iters, None, rows=(f, K, split))
            err = _data.rel(coefs[:, f, a], x_ref)
            assert err < TOL, (f, a, err)
        X32 = coefs[:, f, :].astype(np.float32).astype(np.float64)          # the pass over A reads x in fp32
        ref = lg.nll(A64[te], X32, y[te])
        tol = lg.nll_tolerance(A64[te], X32)
        got = res.logloss[f] * int(te.sum())
        print(f"fold {f}: log-loss {got} ref {ref} err/tol {np.abs(got - ref) / tol}")
        assert np.isfinite(got).all() and (np.abs(got - ref) <= tol).all(), (f, got, ref, tol)
    assert np.allclose(res.mean_logloss, res.logloss.mean(axis=0), rtol=1e-14) and res.best == int(np.argmin(res.mean_logloss))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_logistic_cv_matches_the_reference_on_gathered_rows(fos, cus, name, kind):
    c, seed = _case(kind, cus, name)
    m, n, nalpha = c["m"], c["n"], c["nalpha"]
    split, K = c["folds"]
    ids = _ids(m, K, split, seed)
    A64, y, L, alphas = _recipe(kind, m, n, seed)
    alphas = alphas[:nalpha]
    P = fos.prepare(_device(kind, A64), y, loss="logistic")
    P.profile(1)
    P.profile_read()
    res = fos.logistic_cv(P, None, alphas, K if split == "contiguous" else ids, max_iter=ITERS, L=L, refit=False,
                          return_coefs=True)
    _, launches = P.profile_read()
    P.profile(0)
    groups = -(-K * nalpha // 16)
    assert launches == groups * (ITERS + 1), (launches, groups)       # per group: the iterations and one held-out pass
    assert fos.get_metrics()["grad_num_calls"] == groups * ITERS
    assert res.x is None and all(i == (ITERS, 0) for row in res.info for i in row), res.info
    assert isinstance(res, fos.LogisticCVResult) and res.alphas == [tuple(map(float, a)) for a in alphas]
    _check_cv(res, kind, m, n, seed, ids, split, alphas)


@pytest.mark.parametrize("kind", KINDS)
def test_refit_is_the_path_at_the_best_weight(fos, cus, kind):
    c, seed = _case(kind, cus, "edges")
    A64, y, L, alphas = _recipe(kind, c["m"], c["n"], seed)
    A_in = A64.astype(np.float32) if kind == "f32" else _device(kind, A64)       # results come back as the kind that went in
    res = fos.logistic_cv(A_in, y, alphas, 5, max_iter=ITERS, L=L)
    assert res.coefs is None and type(res.x) is (np.ndarray if kind == "f32" else torch.Tensor)
    x_path = fos.logistic_path(A_in, y, [alphas[res.best]], max_iter=ITERS, L=L)[0]
    assert np.array_equal(_np(res.x), _np(x_path))
    a1, a2 = alphas[res.best]
    assert _data.rel(_np(res.x), _ref(kind, c["m"], c["n"], seed, a1, a2, ITERS, None)[0]) < TOL


def test_default_lipschitz_is_a_quarter_of_one_power_iteration(fos, cus):
    c, seed = _case("f32", cus, "edges")
    A64, y, _, alphas = _recipe("f32", c["m"], c["n"], seed)
    At = _device("f32", A64)
    np.random.seed(123)
    fos.estimate_lipschitz(At)
    one_call = np.random.get_state()[1].copy()
    np.random.seed(123)
    L = float(orc.estimate_lipschitz(A64)) / 4.0
    np.random.seed(123)
    x = fos.logistic_path(At, y, [alphas[1]], max_iter=ITERS)[0]
    assert np.array_equal(np.random.get_state()[1], one_call)             # one draw, as fista_path
    x_ref, _ = lg.run(A64, y, alphas[1][0], alphas[1][1], L, ITERS)
    assert _data.rel(_np(x), x_ref) < 1e-4                               # L itself is an fp32 power iteration here


# ---- logistic_objective ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_logistic_objective(fos, cus, name, kind):
    c, seed = _case(kind, cus, name)
    m, n = c["m"], c["n"]
    A64, y, L, alphas = _recipe(kind, m, n, seed)
    P = fos.prepare(_device(kind, A64), y, loss="logistic")
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 16)) * (rng.random((n, 16)) < 0.2) * np.logspace(-2, 0.5, 16)   # |z| from ~0.01 to ~10
    a1, a2 = 0.7, 0.3
    X32 = X.astype(np.float32).astype(np.float64)
    ref = lg.nll(A64, X32, y) + a1 * np.abs(X).sum(axis=0) + 0.5 * a2 * (X * X).sum(axis=0)
    tol = lg.nll_tolerance(A64, X32) + 1e-14 * np.abs(ref)
    got = fos.logistic_objective(X, P, None, a1, a2)
    print(f"{name} {kind} block err/tol {np.abs(got - ref) / tol}")
    assert got.shape == (16,) and (np.abs(got - ref) <= tol).all(), (got, ref, tol)
    one = fos.logistic_objective(torch.as_tensor(X[:, 5]), P, None, a1, a2)
    assert isinstance(one, float) and abs(one - ref[5]) <= tol[5]
    assert abs(fos.logistic_objective(np.zeros(n), P, None, a1, a2) - m * np.log(2.0)) <= 4 * np.finfo(np.float32).eps * m


# ---- continuation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctrl", [False, True], ids=["plain", "controlled"])
@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_of_15_equal_one_of_30_bitwise(fos, cus, kind, ctrl):
    from fastoptsolver_amd import _core
    c, seed = _case(kind, cus, "edges")
    A64, y, L, alphas = _recipe(kind, c["m"], c["n"], seed)
    P = fos.prepare(_device(kind, A64), y, loss="logistic")
    kw = dict(adaptive_restart=True, restart_threshold=0.9, tol_ratio=1e-3) if ctrl else {}

    def handles():
        hs = []
        for a1, a2 in alphas:
            st = _core.Fista(P)
            st.reset(1.0 / (L + a2), a1, a2, **kw)
            hs.append(st)
        return hs
    split, whole = handles(), handles()
    assert _core.run_multi(split, 15) and _core.run_multi(split, 15) and _core.run_multi(whole, 30)
    for u, v in zip(split, whole):
        assert int(u.status().k) == int(v.status().k) and torch.equal(u.x_tensor(), v.x_tensor())
    a1, a2 = alphas[0]
    x_ref, k_ref = _ref(kind, c["m"], c["n"], seed, a1, a2, 30, None, **({k: v for k, v in kw.items()}))
    assert int(whole[0].status().k) == k_ref and _data.rel(_np(whole[0].x_tensor()), x_ref) < TOL


# ---- padding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["boston", "ragged"])
def test_padded_shapes_match_the_reference(fos, shape, kind):
    if shape == "boston":                               # 1000 x 5: the LDS-resident plan for the squared loss
        A, b, _ = orc.boston_like_data()
        y = (b > np.median(b)).astype(np.float64)
    else:                                               # 300 x 131: ragged rows below the automatic padding of the squared loss
        A, _, xt = _data.synth(300, 131, 77)
        y = lg.labels(A, xt, 77)
    A32 = A.astype(np.float32)
    A64 = _bf16(A32) if kind == "bf16" else A32.astype(np.float64)
    m, n = A64.shape
    L = lg.lipschitz(A64, 5)
    alphas = lg.weights(A64, y)
    P = fos.prepare(A32, y, dtype="bf16" if kind == "bf16" else None, loss="logistic")
    gran = 8 if kind == "bf16" else 4
    assert P.n == n and P.n_dev == max(-(-n // gran) * gran, (72 if kind == "bf16" else 68) if n <= 64 else 0)
    xs = fos.logistic_path(A32, y, alphas, max_iter=ITERS, L=L, dtype="bf16" if kind == "bf16" else None)
    for (a1, a2), x in zip(alphas, xs):
        assert isinstance(x, np.ndarray) and x.shape == (n,)                  # the padding never shows
        x_ref, _ = lg.run(A64, y, a1, a2, L, ITERS)
        err = _data.rel(x, x_ref)
        print(f"{shape} {kind} alpha=({a1:.3g}, {a2}) rel err {err:.3e}")
        assert np.linalg.norm(x_ref) > 0 and err < TOL, (a1, a2, err)
    res = fos.logistic_cv(P, None, alphas, 4, max_iter=ITERS, L=L, return_coefs=True)
    assert res.coefs.shape == (n, 4, 3) and res.x.shape == (n,)
    assert fos.logistic_objective(np.zeros((n, 2)), P, None, 1.0, 1.0).shape == (2,)


def test_prepare_refuses_what_the_lockstep_cannot_serve(fos):
    A = np.ones((8, 68), dtype=np.float32)
    for bad in ([0.0, 1.0, 2.0, 0, 0, 0, 0, 0], [0.0, -0.1, 1, 1, 1, 1, 1, 1], [np.nan] + [0.0] * 7, [np.inf] + [1.0] * 7):
        with pytest.raises(ValueError, match="labels"):
            fos.prepare(A, np.array(bad), loss="logistic")
    with pytest.raises(ValueError, match="labels"):
        fos.prepare(A, None, loss="logistic")
    with pytest.raises(ValueError, match="16384"):
        fos.prepare(np.zeros((2, 16388), dtype=np.float32), np.zeros(2), loss="logistic")
    with pytest.raises(ValueError, match="squared"):
        fos.logistic_path(fos.prepare(A, np.zeros(8)), None, [(0.1, 0.0)], max_iter=2, L=1.0)
    P = fos.prepare(A, np.array([0.0, 1.0, 0.25, 0.75, 1, 0, 1, 0]), loss="logistic")         # soft labels are labels
    assert P.loss == "logistic" and P.sibling(np.zeros(8)).loss == "logistic"
    assert fos.prepare(P) is P and fos.prepare(P, loss="logistic") is P
