"""CPU: the fp64 reference of the weighted lockstep (tests/_weighted.py) is the weighted problem - integer weights equal
physically repeated rows, 0/1 weights equal the gathered rows, for both losses - and its power iteration finds the top
eigenvalue of A^T W A."""
import numpy as np
import pytest

from tests import _data, _logit as lg, _weighted as wt

M, N, SEED = 40, 12, 3


def _case(loss):
    A, b, xt = _data.synth(M, N, SEED)
    if loss == "logistic":
        b = lg.labels(A, xt, SEED)
    return A, b


@pytest.mark.parametrize("delta", [None, 3.0], ids=["fista", "delta"])
@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_count_weights_equal_repeated_rows(loss, delta):
    A, b = _case(loss)
    w = wt.weights("counts", M, SEED)
    assert set(w.tolist()) >= {0.0, 1.0, 2.0, 3.0}
    rep = np.repeat(np.arange(M), w.astype(int))
    L = wt.lipschitz(A, w, SEED, loss)
    for a1, a2 in wt.alphas(A, b, w, loss):
        x_w, k_w = wt.run(A, b, w, a1, a2, L, loss=loss, delta=delta)
        x_r, k_r = wt.run(A[rep], b[rep], np.ones(len(rep)), a1, a2, L, loss=loss, delta=delta)
        assert k_w == k_r == lg.ITERS and np.linalg.norm(x_r) > 0
        assert _data.rel(x_w, x_r) < 1e-12, (a1, a2, _data.rel(x_w, x_r))


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_binary_weights_equal_the_gathered_rows(loss):
    A, b = _case(loss)
    w = wt.weights("binary", M, SEED)
    keep = w > 0
    assert 0 < keep.sum() < M
    L = wt.lipschitz(A, w, SEED, loss)
    for a1, a2 in wt.alphas(A, b, w, loss):
        x_w, _ = wt.run(A, b, w, a1, a2, L, loss=loss, adaptive_restart=True)
        if loss == "squared":
            from oracle import fos_oracle as orc
            x_g = orc.fista(A[keep], b[keep], "elasticnet", a1, a2, max_iter=lg.ITERS, L=L, adaptive_restart=True)
        else:
            x_g, _ = lg.run(A[keep], b[keep], a1, a2, L, adaptive_restart=True)
        assert np.linalg.norm(x_g) > 0 and _data.rel(x_w, x_g) < 1e-12, (a1, a2, _data.rel(x_w, x_g))


@pytest.mark.parametrize("kind", wt.RECIPES)
def test_power_iteration_finds_the_top_eigenvalue(kind):
    A, _ = _case("squared")
    w = wt.weights(kind, M, SEED)
    tol = 1e-9
    L = wt.estimate_lipschitz(A, w, np.random.default_rng(SEED + 1).standard_normal(N), n_iter=5000, tol=tol)
    top = float(np.linalg.eigvalsh(A.T @ (w[:, None] * A))[-1])
    # the iteration stops when two successive estimates differ by less than tol; the estimates rise monotonically to the top
    # eigenvalue at the rate (lambda_2 / lambda_1)^2 per step, so the remainder is below tol / (1 - that rate)
    ev = np.linalg.eigvalsh(A.T @ (w[:, None] * A))
    rate = float((ev[-2] / ev[-1]) ** 2)
    assert 0.0 <= top - L <= tol / (1.0 - rate) + 1e-12 * top, (L, top, rate)
    assert wt.lipschitz(A, w, SEED, "logistic") == wt.lipschitz(A, w, SEED, "squared") / 4.0


def test_gram_is_the_weighted_normal_operator():
    A, _ = _case("squared")
    w = wt.weights("spread", M, SEED)
    X = np.random.default_rng(5).standard_normal((N, 3))
    assert np.allclose(wt.gram(A, w, X), A.T @ np.diag(w) @ A @ X, rtol=1e-12, atol=0)
    assert np.allclose(wt.gram(A, w, X[:, 0]), (A.T @ np.diag(w) @ A @ X)[:, 0], rtol=1e-12, atol=0)
    assert np.allclose(wt.wsse(A, X, A @ X[:, 0], w)[0], 0.0) and (wt.wnll_tolerance(A, X, w) > 0).all()
