"""GPU: per-row sample weights in the lockstep - fista_path / fista_cv / logistic_path / logistic_cv / logistic_objective on a
prepare_weighted handle, fos_gram_apply and the weighted estimate_lipschitz.

Every fit must equal the fp64 reference of tests/_weighted.py (the unmodified oracle on (sqrt(w) A, sqrt(w) b) for the squared
loss, the logistic reference with the weighted gradient for the log-loss: the same momentum, restart and stop rules) within 1e-5
relative, on the bf16-rounded A for bf16 storage and on the weights as the device stores them (fp32); L = lambda_max(A^T W A)
(a quarter of it for the log-loss) comes from the reference's power iteration and is passed to both sides.  Weighted sums are
compared against fp64 on the kernel's OWN x rounded to fp32, which isolates the epilogue from solver drift.  With 0/1 weights the
weighted kernels must reproduce the fold-masked ones bit for bit.  The shapes are those of tests/_menu_cv.py (imported through
tests/_menu_weighted.py), built for the CU count Problem.plan() reports."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _data, _logit as lg, _menu_weighted as mw, _weighted as wt

pytestmark = pytest.mark.gpu

TOL, ITERS = lg.TOL, lg.ITERS
NAMES = ("one_tile", "edges", "rb2", "panels")
KINDS = ("f32", "bf16")
LOSSES = ("squared", "logistic")
# every recipe on some case; the second panel ("panels") and the fold edges inside a lane's 4 rows ("edges") get weights that
# differ in every row
RECIPE = {"one_tile": "counts", "edges": "spread", "rb2": "binary", "panels": "spread"}


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
def _recipe(kind, loss, m, n, seed, wkind):
    """(A as the device stores it in fp64, b or the labels, the weights as the device stores them, L of the weighted data term,
    the three penalty pairs): computed once per shape, never modified."""
    A64, y, _, _ = lg.recipe(m, n, seed, _bf16 if kind == "bf16" else None)
    b = y if loss == "logistic" else _data.synth(m, n, seed)[1].astype(np.float32).astype(np.float64)
    w = wt.as_stored(wt.weights(wkind, m, seed))
    for a in (A64, b, w):
        a.setflags(write=False)
    return A64, b, w, wt.lipschitz(A64, w, seed, loss), tuple(wt.alphas(A64, b, w, loss))


def _device(kind, A64):
    return torch.as_tensor(A64.astype(np.float32)).to(torch.bfloat16 if kind == "bf16" else torch.float32).cuda()


@functools.lru_cache(maxsize=None)
def _ids(m, K, split, seed):
    ids = mw.fold_ids(dict(m=m, folds=(split, K)), seed=seed)
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def _ref(kind, loss, m, n, seed, wkind, a1, a2, iters, delta, rows=None, **kw):
    """(x, iterations) of the reference; rows: a fold id and K as (f, K, kind of split) -> the fit on the other rows."""
    A64, b, w, L, _ = _recipe(kind, loss, m, n, seed, wkind)
    if rows is not None:
        keep = _ids(m, rows[1], rows[2], seed) != rows[0]
        A64, b, w = A64[keep], b[keep], w[keep]
    x, k = wt.run(A64, b, w, a1, a2, L, iters, loss=loss, delta=delta, **kw)
    x.setflags(write=False)
    return x, k


def _case(kind, cus, name):
    c = mw.shapes(kind, cus)[name]
    return c, 3 * c["m"] + c["n"], RECIPE[name]


def _handle(fos, kind, loss, A64, b, w):
    P = fos.prepare_weighted(_device(kind, A64), b, w, loss=loss)
    assert P.sample_weight.dtype == torch.float32 and P.sample_weight.data_ptr() % 16 == 0 and P.loss == loss
    return P


def _path(fos, loss):
    return fos.logistic_path if loss == "logistic" else fos.fista_path


# ---- the path ------------------------------------------------------------------------------------------------------------
MODES = {"plain": {}, "controlled": dict(adaptive_restart=True, restart_threshold=0.9, tol_ratio=0.5), "delta": dict(delta=3.0)}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_path_matches_the_reference(fos, cus, name, kind, loss, mode):
    c, seed, wkind = _case(kind, cus, name)
    m, n = c["m"], c["n"]
    A64, b, w, L, alphas = _recipe(kind, loss, m, n, seed, wkind)
    P = _handle(fos, kind, loss, A64, b, w)
    kw = dict(MODES[mode])
    delta = kw.pop("delta", None)
    xs, info = _path(fos, loss)(P, None, alphas, max_iter=ITERS, L=L, delta=delta, return_info=True, **kw)
    assert len(xs) == 3
    for (a1, a2), x, (k, code) in zip(alphas, xs, info):
        x_ref, k_ref = _ref(kind, loss, m, n, seed, wkind, a1, a2, ITERS, delta, **kw)
        err = _data.rel(_np(x), x_ref)
        print(f"{name} {kind} {loss} {mode} alpha=({a1:.3g}, {a2}) rel err {err:.3e} iterations {k} / {k_ref} "
              f"nnz {int(np.count_nonzero(x_ref))}")
        assert (k, code) == (k_ref, 2 if k_ref < ITERS else 0), (a1, k, k_ref, code)
        assert np.linalg.norm(x_ref) > 0 and err < TOL, (a1, a2, err)


@pytest.mark.parametrize("loss", LOSSES)
def test_one_weight_and_seventeen_go_through_the_lockstep(fos, cus, loss):
    c, seed, wkind = _case("f32", cus, "edges")
    A64, b, w, L, alphas = _recipe("f32", loss, c["m"], c["n"], seed, wkind)
    P = _handle(fos, "f32", loss, A64, b, w)
    many = [(alphas[0][0] * 0.9 ** j, 0.0) for j in range(17)]
    for ws, groups in (([alphas[1]], 1), (many, 2)):
        P.profile(1)
        P.profile_read()
        xs = _path(fos, loss)(P, None, ws, max_iter=ITERS, L=L)
        _, launches = P.profile_read()
        P.profile(0)
        assert launches == groups * ITERS, (launches, groups)       # one bracketed two-product pass per iteration per group
        x_ref, _ = _ref("f32", loss, c["m"], c["n"], seed, wkind, ws[-1][0], ws[-1][1], ITERS, None)
        assert _data.rel(_np(xs[-1]), x_ref) < TOL
    with pytest.raises(ValueError):
        fos.fista_path(P, None, [alphas[0]], max_iter=2, L=L, tol=1e-3)
    with pytest.raises(ValueError):
        fos.fista_path(P, None, [alphas[0]], max_iter=2, L=L, cols=(0, 4, 8))


# ---- cross-validation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_cv_matches_the_reference_on_gathered_rows(fos, cus, name, kind, loss):
    c, seed, wkind = _case(kind, cus, name)
    m, n, nalpha = c["m"], c["n"], c["nalpha"]
    split, K = c["folds"]
    ids = _ids(m, K, split, seed)
    A64, b, w, L, alphas = _recipe(kind, loss, m, n, seed, wkind)
    alphas = alphas[:nalpha]
    P = _handle(fos, kind, loss, A64, b, w)
    cv = fos.logistic_cv if loss == "logistic" else fos.fista_cv
    P.profile(1)
    P.profile_read()
    res = cv(P, None, alphas, K if split == "contiguous" else ids, max_iter=ITERS, L=L, refit=False, return_coefs=True)
    _, launches = P.profile_read()
    P.profile(0)
    groups = -(-K * nalpha // 16)
    assert launches == groups * (ITERS + 1), (launches, groups)       # per group: the iterations and one held-out pass
    assert res.x is None and all(i == (ITERS, 0) for row in res.info for i in row), res.info
    coefs = _np(res.coefs)
    score = res.logloss if loss == "logistic" else res.mse
    assert coefs.shape == (n, K, nalpha) and score.shape == (K, nalpha) and score.dtype == np.float64
    ref_score, bound = np.zeros((K, nalpha)), np.zeros((K, nalpha))
    for f in range(K):
        te = ids == f
        wsum = float(w[te].sum())
        for a, (a1, a2) in enumerate(alphas):
            x_ref, _ = _ref(kind, loss, m, n, seed, wkind, a1, a2, ITERS, None, rows=(f, K, split))
            err = _data.rel(coefs[:, f, a], x_ref)
            assert err < TOL, (f, a, err)
        X32 = coefs[:, f, :].astype(np.float32).astype(np.float64)          # the pass over A reads x in fp32
        if loss == "logistic":
            ref = wt.wnll(A64[te], X32, b[te], w[te])
            tol = wt.wnll_tolerance(A64[te], X32, w[te])
        else:                                                               # the bounds of the unweighted pass on (sqrt(w) A, sqrt(w) b)
            sw = np.sqrt(w[te])
            ref = wt.wsse(A64[te], X32, b[te], w[te])
            _, tol = _data.fp32_pass_tolerances_cols(sw[:, None] * A64[te], X32, sw * b[te], np.zeros_like(X32), ref)
        got = score[f] * wsum
        print(f"fold {f}: weighted sum {got} ref {ref} err/tol {np.abs(got - ref) / tol}")
        assert np.isfinite(got).all() and (np.abs(got - ref) <= tol).all(), (f, got, ref, tol)
        ref_score[f], bound[f] = ref / wsum, tol / wsum
    mean = res.mean_logloss if loss == "logistic" else res.mean_mse
    assert np.allclose(mean, score.mean(axis=0), rtol=1e-14) and res.best == int(np.argmin(mean))
    ref_mean, slack = ref_score.mean(axis=0), bound.mean(axis=0)
    order = np.argsort(ref_mean)
    if nalpha > 1 and ref_mean[order[1]] - ref_mean[order[0]] > slack[order[1]] + slack[order[0]]:
        assert res.best == int(order[0]), (res.best, ref_mean, slack)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("kind", KINDS)
def test_refit_is_the_lockstep_path_at_the_best_weight(fos, cus, kind, loss):
    c, seed, wkind = _case(kind, cus, "edges")
    A64, b, w, L, alphas = _recipe(kind, loss, c["m"], c["n"], seed, wkind)
    P = _handle(fos, kind, loss, A64, b, w)
    cv = fos.logistic_cv if loss == "logistic" else fos.fista_cv
    res = cv(P, None, alphas, 5, max_iter=ITERS, L=L)
    x_path = _path(fos, loss)(P, None, [alphas[res.best]], max_iter=ITERS, L=L)[0]
    assert res.coefs is None and np.array_equal(_np(res.x), _np(x_path))
    a1, a2 = alphas[res.best]
    assert _data.rel(_np(res.x), _ref(kind, loss, c["m"], c["n"], seed, wkind, a1, a2, ITERS, None)[0]) < TOL
    # a fold without weight cannot be scored: refused before any solver launch
    ids = np.arange(c["m"]) % 3
    wz = np.array(w)
    wz[ids == 1] = 0.0
    Pz = _handle(fos, kind, loss, A64, b, wz)
    Pz.profile(1)
    Pz.profile_read()
    with pytest.raises(ValueError, match="fold 1"):
        cv(Pz, None, alphas, ids, max_iter=ITERS, L=L)
    assert Pz.profile_read()[1] == 0


# ---- the weighted sums -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_weighted_sums_of_sixteen_points(fos, cus, name, kind, loss):
    c, seed, wkind = _case(kind, cus, name)
    m, n = c["m"], c["n"]
    A64, b, w, L, alphas = _recipe(kind, loss, m, n, seed, wkind)
    P = _handle(fos, kind, loss, A64, b, w)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 16)) * (rng.random((n, 16)) < 0.2) * np.logspace(-2, 0.5, 16)
    X32 = X.astype(np.float32).astype(np.float64)
    if loss == "logistic":
        a1, a2 = 0.7, 0.3
        ref = wt.wnll(A64, X32, b, w) + a1 * np.abs(X).sum(axis=0) + 0.5 * a2 * (X * X).sum(axis=0)
        tol = wt.wnll_tolerance(A64, X32, w) + 1e-14 * np.abs(ref)
        got = fos.logistic_objective(X, P, None, a1, a2)
        zero = fos.logistic_objective(np.zeros(n), P, None, a1, a2)
        assert abs(zero - w.sum() * np.log(2.0)) <= 4 * np.finfo(np.float32).eps * w.sum()
    else:
        sw = np.sqrt(w)
        ref = wt.wsse(A64, X32, b, w)
        _, tol = _data.fp32_pass_tolerances_cols(sw[:, None] * A64, X32, sw * b, np.zeros_like(X32), ref)
        got = np.asarray(P.residual_batch(torch.as_tensor(X32), use_b=True))
    print(f"{name} {kind} {loss} err/tol {np.abs(got - ref) / tol}")
    assert got.shape == (16,) and (np.abs(got - ref) <= tol).all(), (got, ref, tol)


# ---- 0 / 1 weights are a fold mask, bit for bit ------------------------------------------------------------------------------
def _states(P, alphas, L, **kw):
    from fastoptsolver_amd import _core
    hs = []
    for a1, a2 in alphas:
        st = _core.Fista(P)
        st.reset(1.0 / (L + a2), a1, a2, **kw)
        hs.append(st)
    return hs


@pytest.mark.parametrize("ctrl", [False, True], ids=["plain", "controlled"])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["edges", "panels"])
def test_binary_weights_are_the_fold_mask_bitwise(fos, cus, name, kind, loss, ctrl):
    from fastoptsolver_amd import _core
    c, seed, _ = _case(kind, cus, name)
    m, n = c["m"], c["n"]
    A64, b, w, L, alphas = _recipe(kind, loss, m, n, seed, "binary")
    assert 0 < int((w == 0).sum()) < m and set(w[-4:].tolist()) <= {0.0, 1.0}
    At = _device(kind, A64)
    kw = dict(adaptive_restart=True, restart_threshold=0.9, tol_ratio=1e-3) if ctrl else {}
    Pw = fos.prepare_weighted(At, b, w, loss=loss)
    Pu = fos.prepare(At, b, loss=loss)
    ids_dev = _core.fold_ids_tensor((w == 0).astype(np.uint8), Pu.device)          # fold 1: the rows without weight
    weighted, masked = _states(Pw, alphas, L, **kw), _states(Pu, alphas, L, **kw)
    assert _core.run_multi(weighted, ITERS) and _core.run_multi_folds(masked, ids_dev, [1] * 3, ITERS)
    for u, v in zip(weighted, masked):
        assert int(u.status().k) == int(v.status().k) and torch.equal(u.x_tensor(), v.x_tensor())
    assert torch.count_nonzero(weighted[0].x_tensor()) > 0
    X = torch.stack([st.x_tensor() for st in weighted], dim=1)
    assert Pw.residual_batch(X, use_b=True) == Pu.residual_batch_folds(X, ids_dev, [0] * 3)
    # weights and a fold mask together: column j holds out fold j of the rows, on both sides with the weightless rows out
    ids3 = np.where(w == 0, 3, np.arange(m) % 3).astype(np.uint8)
    both = _states(Pw, alphas, L, **kw)
    ids3_w, ids4_u = _core.fold_ids_tensor(np.arange(m) % 3, Pw.device), _core.fold_ids_tensor(ids3, Pu.device)
    assert _core.run_multi_folds(both, ids3_w, [0, 1, 2], 5)
    Xb = torch.stack([st.x_tensor() for st in both], dim=1)
    assert Pw.residual_batch_folds(Xb, ids3_w, [0, 1, 2]) == Pu.residual_batch_folds(Xb, ids4_u, [0, 1, 2])
    # all-ones weights: the unweighted lockstep with nothing held out
    P1 = fos.prepare_weighted(At, b, np.ones(m), loss=loss)
    ones, plain = _states(P1, alphas, L, **kw), _states(Pu, alphas, L, **kw)
    assert _core.run_multi(ones, ITERS) and _core.run_multi_folds(plain, ids_dev, [-1] * 3, ITERS)
    for u, v in zip(ones, plain):
        assert int(u.status().k) == int(v.status().k) and torch.equal(u.x_tensor(), v.x_tensor())


# ---- fos_gram_apply and the step size ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [1, 3, 16])
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "identity"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["edges", "panels"])
def test_gram_apply(fos, cus, name, kind, weighted, nv):
    c, seed, wkind = _case(kind, cus, name)
    m, n = c["m"], c["n"]
    A64, b, w, _, _ = _recipe(kind, "logistic", m, n, seed, wkind)
    # neither b nor the loss enters: a logistic handle serves it
    P = _handle(fos, kind, "logistic", A64, b, w) if weighted else fos.prepare(_device(kind, A64), b, loss="logistic")
    w_eff = w if weighted else np.ones(m)
    X32 = np.random.default_rng(seed + nv).standard_normal((n, nv)).astype(np.float32).astype(np.float64)
    got = _np(P.gram_apply(torch.as_tensor(X32)))
    ref = wt.gram(A64, w_eff, X32)
    sw = np.sqrt(w_eff)
    As = sw[:, None] * A64
    g_tol, _ = _data.fp32_pass_tolerances_cols(As, X32, None, ref, ((As @ X32) ** 2).sum(axis=0))
    err = np.linalg.norm(got - ref, axis=0)
    print(f"{name} {kind} weighted={weighted} nv={nv} err/tol {err / g_tol}")
    assert got.shape == (n, nv) and (err <= g_tol).all(), (err, g_tol)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("kind", KINDS)
def test_estimate_lipschitz_is_the_power_iteration_on_the_weighted_gram(fos, cus, kind, loss):
    c, seed, wkind = _case(kind, cus, "edges")
    m, n = c["m"], c["n"]
    A64, b, w, _, alphas = _recipe(kind, loss, m, n, seed, wkind)
    P = _handle(fos, kind, loss, A64, b, w)
    np.random.seed(11)
    L = fos.estimate_lipschitz(P)
    after = np.random.randn()
    np.random.seed(11)
    v0 = np.random.randn(n)
    assert after == np.random.randn()                                      # one draw of n normals, as ref:50
    L_ref = wt.estimate_lipschitz(A64, w, v0)
    top = float(np.linalg.eigvalsh(A64.T @ (w[:, None] * A64))[-1])
    print(f"{kind} {loss} L {L} reference {L_ref} top eigenvalue {top} max(w) lambda_max(A^T A) "
          f"{w.max() * np.linalg.eigvalsh(A64.T @ A64)[-1]}")
    assert L == pytest.approx(L_ref, rel=TOL)
    # the default step of the path is that estimate (a quarter of it for the log-loss)
    np.random.seed(11)
    x = _path(fos, loss)(P, None, [alphas[1]], max_iter=ITERS)[0]
    x_ref, _ = wt.run(A64, b, w, alphas[1][0], alphas[1][1], L_ref / (4.0 if loss == "logistic" else 1.0), ITERS, loss=loss)
    assert _data.rel(_np(x), x_ref) < 1e-4                                 # L itself is an fp32 power iteration here


# ---- handle hygiene and padding ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_detached_weights_leave_an_unweighted_handle(fos, cus, kind):
    c, seed, wkind = _case(kind, cus, "edges")
    A64, b, w, L, alphas = _recipe(kind, "squared", c["m"], c["n"], seed, wkind)
    At = _device(kind, A64)
    P = fos.prepare_weighted(At, b, w)
    fos.fista_path(P, None, alphas, max_iter=ITERS, L=L)
    ones = np.ones(c["m"])                                                 # the penalties and the step of the unweighted problem
    L, alphas = wt.lipschitz(A64, ones, seed, "squared"), wt.alphas(A64, b, ones, "squared")
    out = C.c_void_p(1)
    assert P.lib.fos_row_weights_get(C.byref(out), P.h) == 0 and out.value == P.sample_weight.data_ptr()
    P.set_sample_weight(None)                                              # fos_row_weights_bind(NULL, p)
    assert P.lib.fos_row_weights_get(C.byref(out), P.h) == 0 and out.value is None and P.sample_weight is None
    xs = fos.fista_path(P, None, alphas, max_iter=ITERS, L=L)
    fresh = fos.fista_path(fos.prepare(At, b), None, alphas, max_iter=ITERS, L=L)
    for x, y in zip(xs, fresh):
        assert torch.equal(x, y) and torch.count_nonzero(x) > 0
    assert len(P.residual_batch(torch.zeros(c["n"], 2), use_b=False)) == 2   # served again: the guard follows the binding


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("kind", KINDS)
def test_padded_shapes_match_the_reference(fos, kind, loss):
    from oracle import fos_oracle as orc
    A, b, _ = orc.boston_like_data()                        # 1000 x 5: the LDS-resident plan of an unweighted problem
    if loss == "logistic":
        b = (b > np.median(b)).astype(np.float64)
    A32 = A.astype(np.float32)
    A64 = _bf16(A32) if kind == "bf16" else A32.astype(np.float64)
    b = b.astype(np.float32).astype(np.float64)
    m, n = A64.shape
    w = wt.as_stored(wt.weights("spread", m, 5))
    L = wt.lipschitz(A64, w, 5, loss)
    alphas = wt.alphas(A64, b, w, loss)
    P = fos.prepare_weighted(A32, b, w, dtype="bf16" if kind == "bf16" else None, loss=loss)
    assert P.n == n and P.n_dev == (72 if kind == "bf16" else 68)
    xs = _path(fos, loss)(P, None, alphas, max_iter=ITERS, L=L)
    for (a1, a2), x in zip(alphas, xs):
        assert isinstance(x, np.ndarray) and x.shape == (n,)                  # the padding never shows
        x_ref, _ = wt.run(A64, b, w, a1, a2, L, ITERS, loss=loss)
        err = _data.rel(x, x_ref)
        print(f"boston {kind} {loss} alpha=({a1:.3g}, {a2}) rel err {err:.3e}")
        assert np.linalg.norm(x_ref) > 0 and err < TOL, (a1, a2, err)
    with pytest.raises(ValueError, match="16384"):
        fos.prepare_weighted(np.zeros((2, 16388), dtype=np.float32), np.zeros(2), np.ones(2))
