"""CPU: the fp64 reference of the logistic lockstep (tests/_logit.py) is itself right - its gradient is the derivative of its
negative log-likelihood, and lambda_max(A^T A) / 4 is a valid Lipschitz constant of it."""
import numpy as np

from tests import _logit as lg


def test_gradient_against_central_differences():
    A64, y, xt, L = lg.recipe(67, 68, 11)
    rng = np.random.default_rng(3)
    for a2 in (0.0, 0.5):
        prob = lg.LogisticProblem(A64, y, 0.1, a2)
        x = 0.3 * rng.standard_normal(68)
        g = prob.gradient(x)
        h = 1e-5
        fd = np.empty(68)
        for j in range(68):
            e = np.zeros(68)
            e[j] = h
            fd[j] = (lg.objective(A64, x + e, y, 0.0, a2) - lg.objective(A64, x - e, y, 0.0, a2)) / (2 * h)
        assert np.linalg.norm(g - fd) <= 1e-6 * np.linalg.norm(fd), np.linalg.norm(g - fd) / np.linalg.norm(fd)


def test_reference_only_replaces_the_gradient():
    assert [k for k in vars(lg.LogisticProblem) if not k.startswith("__")] == ["gradient"]


def test_nll_is_stable_at_both_ends():
    A = np.array([[1000.0], [-1000.0], [0.0]])
    t = lg.nll_terms(A, np.array([1.0]), np.array([1.0, 0.0, 0.5]))
    assert np.allclose(t, [0.0, 0.0, np.log(2.0)]) and np.isfinite(lg.nll(A, np.array([-1.0]), np.array([1.0, 0.0, 0.5])))
    assert np.allclose(lg.sigmoid([-800.0, 0.0, 800.0]), [0.0, 0.5, 1.0])


def test_quarter_of_lambda_max_gives_monotone_descent():
    """300 iterations at t_init_factor = 1 with the momentum switched off (restart_threshold = 0 restarts every iteration: the
    proximal gradient method) never increase the objective: the step 1 / (lambda_max / 4 + alpha2) is short enough
    (sigma' <= 1/4 bounds the Hessian A^T diag(sigma') A by A^T A / 4)."""
    A64, y, xt, L = lg.recipe(67, 68, 11)
    for a1, a2 in lg.weights(A64, y):
        objs = []
        lg.run(A64, y, a1, a2, L, 300, adaptive_restart=True, restart_threshold=0.0, objectives=objs)
        assert len(objs) == 300
        d = np.diff(objs)
        assert (d <= 1e-12 * np.abs(objs[0])).all(), float(d.max())
        assert objs[-1] < lg.objective(A64, np.zeros(68), y, a1, a2)
