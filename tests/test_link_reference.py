"""CPU: the fp64 reference of the Huber and squared-hinge lockstep (tests/_link.py) is the gradient of its own objective, reaches
the KKT conditions, reduces to the oracle's squared run for a threshold no residual reaches, and its recipes mix both branches of
either loss."""
import numpy as np
import pytest

from oracle import fos_oracle as orc
from tests import _data, _link as lk

SHAPES = ((257, 37), (1003, 68))


def _problem(kind, m, n):
    if kind == lk.HUBER:
        A, b, c, L, alphas = lk.huber_recipe(m, n)
        return A, b, c, L, alphas
    A, y, L, alphas = lk.hinge_recipe(m, n, 3 * m + n)
    return A, y, None, L, alphas


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("kind", [lk.HUBER, lk.HINGE])
def test_gradient_is_the_derivative_of_the_objective(kind, weighted):
    m, n = SHAPES[0]
    A, b, c, _, _ = _problem(kind, m, n)
    rng = np.random.default_rng(5)
    w = rng.uniform(0.2, 2.0, m) if weighted else None
    x = 0.3 * rng.standard_normal(n)
    g = lk.gradient(kind, A, x, b, c, w)
    # central differences of a C^1 function with a piecewise-constant second derivative: O(h) off at the few rows a kink falls
    # into, O(h^2) elsewhere; h = 1e-6 against gradients of order |A^T 1|
    h = 1e-6
    for j in range(n):
        e = np.zeros(n)
        e[j] = h
        fd = (lk.data_term(kind, A, x + e, b, c, w) - lk.data_term(kind, A, x - e, b, c, w)) / (2 * h)
        assert abs(fd - g[j]) <= 1e-6 * (1.0 + abs(g[j])), (j, fd, g[j])
    X = np.stack([x, -x, np.zeros(n)], axis=1)                       # a block answers per column
    assert np.allclose(lk.gradient(kind, A, X, b, c, w)[:, 0], g, rtol=1e-13, atol=1e-13)
    assert np.allclose(lk.data_term(kind, A, X, b, c, w)[0], lk.data_term(kind, A, x, b, c, w), rtol=1e-14)


@pytest.mark.parametrize("kind", [lk.HUBER, lk.HINGE])
def test_a_long_run_reaches_the_kkt_conditions(kind):
    m, n = SHAPES[0]
    A, b, c, L, alphas = _problem(kind, m, n)
    a1, a2 = alphas[0][0], 0.0
    x, k = lk.run(kind, A, b, a1, a2, L, 3000, c=c)
    assert k == 3000 and np.count_nonzero(x) > 0
    g = lk.gradient(kind, A, x, b, c)
    on = x != 0
    assert np.all(np.abs(g[~on]) <= a1 * (1 + 1e-6))
    assert np.allclose(g[on], -a1 * np.sign(x[on]), rtol=0, atol=1e-6 * a1)


def test_huber_with_an_unreachable_threshold_is_the_squared_run():
    m, n = SHAPES[1]
    A, b, _, L, alphas = lk.huber_recipe(m, n, check=False)
    for (a1, a2), delta in zip(alphas, (None, 3.0, None)):
        x, _ = lk.run(lk.HUBER, A, b, a1, a2, L, c=1e30, delta=delta)
        prob = orc.FistaProblem(A, b, a1, a2)
        st = prob.init_state(L)
        for _ in range(lk.ITERS):
            prob.step(st) if delta is None else prob.step_delta(st, delta)
        assert np.array_equal(x, st.x), (a1, a2, _data.rel(x, st.x))


@pytest.mark.parametrize("m,n", SHAPES)
def test_recipes_mix_both_branches(m, n):
    A, b, c, L, alphas = lk.huber_recipe(m, n)                       # asserts the clipped share at x = 0 and at the final iterates
    assert abs(lk.clipped_share(A, np.zeros(n), b, c) - 0.5) < 0.01 and len(alphas) == 3
    A, y, L, alphas = lk.hinge_recipe(m, n, 3 * m + n)               # asserts the active share at the final iterates
    assert set(np.unique(y)) == {-1.0, 1.0} and lk.active_share(A, np.zeros(n), y) == 1.0


def test_loss_tolerance_is_small_and_positive():
    m, n = SHAPES[0]
    for kind in (lk.HUBER, lk.HINGE):
        A, b, c, L, alphas = _problem(kind, m, n)
        x, _ = lk.run(kind, A, b, *alphas[2], L, c=c)
        tol = lk.loss_tolerance(kind, A, x[:, None], b, c)
        val = lk.data_term(kind, A, x, b, c)
        assert tol.shape == (1,) and 0 < tol[0] < 1e-4 * val, (tol, val)
