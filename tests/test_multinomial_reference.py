"""CPU: the fp64 reference of the multinomial lockstep (tests/_multinomial.py) is the model it claims to be - its gradient is
the derivative of its objective, its iterates reach the optimality conditions of the L1 problem, two classes are the logistic
model, and Boehning's constant gives a descent step."""
import numpy as np
import pytest

from tests import _logit as lg, _multinomial as mn


def _case(m=200, n=30, C=3, seed=5):
    A64, y, L = mn.recipe(m, n, C, seed)
    return A64, y, L, mn.weights(A64, y, C)


@pytest.mark.parametrize("C", [2, 3, 5, 16])
@pytest.mark.parametrize("weighted", [False, True])
def test_gradient_against_central_differences(C, weighted):
    A64, y, _ = mn.recipe(120, 12, C, 3)
    rng = np.random.default_rng(C)
    w = rng.uniform(0.0, 2.0, size=120) if weighted else None
    p = rng.uniform(0.5, 2.0, size=12)
    prob = mn.MultinomialProblem(A64, y, C, 0.0, 0.7, w=w, p=p)          # the smooth part: data term + ridge
    x = 0.3 * rng.standard_normal(12 * C)
    g = prob.gradient(x)
    h = 1e-6
    for i in rng.choice(12 * C, 12, replace=False):
        e = np.zeros_like(x)
        e[i] = h
        fd = (prob.value(x + e) - prob.value(x - e)) / (2 * h)
        # central differences: O(h^2 f''') truncation plus eps64 |f| / h rounding, both far below 1e-6 of the scale here
        assert abs(fd - g[i]) <= 1e-6 * max(1.0, np.abs(g).max()), (i, fd, g[i])


KKT_ITERS = 300          # measured on this case: the violation is 3e-7 a1 after 100 iterations and 2e-13 a1 after 300
KKT_TOL = 1e-9           # relative to alpha1


def test_reference_meets_the_kkt_conditions_of_the_l1_problem():
    A64, y, L, alphas = _case()
    a1 = alphas[0][0]
    X = mn.run(A64, y, 3, a1, 0.0, L, KKT_ITERS)
    G = mn.MultinomialProblem(A64, y, 3, a1, 0.0).gradient(X.reshape(-1)).reshape(X.shape)
    nz = X != 0
    assert nz.sum() >= 4 and (~nz).sum() >= 4
    assert np.abs(G + a1 * np.sign(X))[nz].max() <= KKT_TOL * a1          # stationarity on the support
    assert (np.abs(G[~nz]) <= a1 * (1 + KKT_TOL)).all()                  # the subgradient condition off it


def test_two_classes_are_the_logistic_model():
    """R of C = 2 is [1 - sigma(z1 - z0), sigma(z1 - z0)] - onehot."""
    A64, y, _ = mn.recipe(150, 10, 2, 7)
    x = np.random.default_rng(1).standard_normal(20)
    R = mn.MultinomialProblem(A64, y, 2, 0.0, 0.0).residual(x)
    Z = A64 @ x.reshape(10, 2)
    s = lg.sigmoid(Z[:, 1] - Z[:, 0])
    want = np.stack([1.0 - s, s], axis=1) - mn.onehot(y, 2)
    assert np.abs(R - want).max() <= 1e-14
    assert abs(mn.nll(A64, x.reshape(10, 2), y) - float(lg.nll(A64, x.reshape(10, 2)[:, 1] - x.reshape(10, 2)[:, 0], y))) <= 1e-10


def test_softmax_and_nll_are_stable_at_both_ends():
    Z = np.array([[800.0, -800.0, 0.0], [-800.0, -800.0, -800.0]])
    assert np.allclose(mn.softmax(Z), [[1.0, 0.0, 0.0], [1 / 3, 1 / 3, 1 / 3]])
    A = np.array([[1.0], [1.0]])
    t = mn.nll_terms(A, Z[:1], np.array([0, 1]))
    assert np.allclose(t, [0.0, 1600.0])


def test_half_of_lambda_max_gives_monotone_descent():
    """300 iterations at t_init_factor = 1 with the momentum switched off (restart_threshold = 0 restarts every iteration: the
    proximal gradient method) never increase the objective: the step 1 / (lambda_max / 2 + alpha2) is short enough (Boehning:
    the softmax Hessian is <= 1/2 I (x) A^T A)."""
    A64, y, L, alphas = _case(67, 68, 4, 11)
    for a1, a2 in alphas:
        objs = []
        mn.run(A64, y, 4, a1, a2, L, 300, adaptive_restart=True, restart_threshold=0.0, objectives=objs)
        d = np.diff(objs)
        assert len(objs) == 300 and (d <= 1e-12 * np.abs(objs[0])).all(), float(d.max())
        assert objs[-1] < mn.objective(A64, np.zeros((68, 4)), y, a1, a2)


def test_recipe_labels_cover_every_class_and_logits_stay_moderate():
    for C in (2, 3, 5, 7, 16):
        A64, y, L = mn.recipe(257, 37, C, 2)
        assert set(y.astype(int).tolist()) == set(range(C)) and L > 0
