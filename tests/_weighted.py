"""The fp64 reference of the weighted lockstep and the weight recipes its tests share (a helper: no tests in here).

Squared loss: sum_i w_i 0.5 (a_i.x - b_i)^2 = 0.5 ||sqrt(w) * (A x - b)||^2, so the reference is the UNMODIFIED oracle
FistaProblem on (sqrt(w) * A, sqrt(w) * b).  Logistic loss: the weight multiplies the loss and not the row, so the reference is
tests/_logit.LogisticProblem with ONE method replaced: gradient(y) = A^T (w * (sigma(A y) - b)) (+ alpha2 y).  Momentum,
restarts and stops are the oracle's own in both."""
import numpy as np

from oracle import fos_oracle as orc
from tests import _logit as lg

RECIPES = ("binary", "counts", "spread")


def weights(kind, m, seed):
    """m weights by seeded generator.  binary: 0 / 1, a fold mask; counts: integers 0..3, frequency weights; spread:
    log-uniform over 1e-3..1e3 - every row differs, also within a lane's 4 rows.  Never all zero."""
    rng = np.random.default_rng(7000 + seed)
    if kind == "binary":
        w = (rng.random(m) < 0.7).astype(np.float64)
    elif kind == "counts":
        w = rng.integers(0, 4, size=m).astype(np.float64)
    elif kind == "spread":
        w = 10.0 ** rng.uniform(-3.0, 3.0, size=m)
    else:
        raise ValueError(kind)
    w[0] = 1.0
    return w


def as_stored(w):
    """The weights as the device keeps them (fp32), in fp64."""
    return np.asarray(w, dtype=np.float32).astype(np.float64)


class WeightedLogisticProblem(lg.LogisticProblem):
    def __init__(self, A, b, w, alpha1, alpha2):
        super().__init__(A, b, alpha1, alpha2)
        self.w = np.asarray(w, dtype=np.float64)

    def gradient(self, y):
        g = self.A.T @ (self.w * (lg.sigmoid(self.A @ y) - self.b))
        return g + self.a2 * y if self.a2 > 0 else g


def problem(A, b, w, alpha1, alpha2, loss):
    w = np.asarray(w, dtype=np.float64)
    if loss == "squared":
        sw = np.sqrt(w)
        return orc.FistaProblem(sw[:, None] * np.asarray(A, dtype=np.float64), sw * np.asarray(b, dtype=np.float64), alpha1, alpha2)
    return WeightedLogisticProblem(A, b, w, alpha1, alpha2)


def run(A, b, w, alpha1, alpha2, L, max_iter=lg.ITERS, *, loss="squared", delta=None, t_init_factor=1.0, tol_ratio=0.0,
        adaptive_restart=False, restart_threshold=1.0):
    """(x, iterations run) of FISTA (FISTA-delta with `delta`) on the weighted objective from x0 = 0; L is the constant of the
    weighted data term."""
    prob = problem(A, b, w, alpha1, alpha2, loss)
    st = prob.init_state(L, t_init_factor)
    for _ in range(max_iter):
        if delta is None:
            prob.step(st, tol_ratio=tol_ratio, adaptive_restart=adaptive_restart, restart_threshold=restart_threshold)
        else:
            prob.step_delta(st, delta, tol_ratio=tol_ratio)
        if st.stopped:
            break
    return st.x, st.k


def gram(A, w, X):
    """A^T (w * (A X)) in fp64."""
    A = np.asarray(A, dtype=np.float64)
    AX = A @ np.asarray(X, dtype=np.float64)
    return A.T @ (np.asarray(w, dtype=np.float64).reshape((-1,) + (1,) * (AX.ndim - 1)) * AX)


def estimate_lipschitz(A, w, v0, n_iter=100, tol=1e-6):
    """lambda_max(A^T W A): the oracle's power iteration (same start vector handling, same stopping rule) on sqrt(w) * A."""
    return float(orc.estimate_lipschitz(np.sqrt(np.asarray(w, dtype=np.float64))[:, None] * np.asarray(A, dtype=np.float64),
                                        n_iter=n_iter, tol=tol, v0=v0))


def lipschitz(A64, w, seed, loss):
    """The constant of the weighted data term passed to both sides: lambda_max(A^T W A), a quarter of it for the log-loss."""
    L = estimate_lipschitz(A64, w, np.random.default_rng(seed + 1).standard_normal(A64.shape[1]))
    return L / 4.0 if loss == "logistic" else L


def alphas(A64, b, w, loss, count=3):
    """Below alpha_max of the weighted problem (above it x = 0 is the solution): lasso and elastic-net weights."""
    g0 = A64.T @ (w * ((b - 0.5) if loss == "logistic" else b))
    amax = float(np.max(np.abs(g0)))
    return [(0.3 * amax, 0.0), (0.1 * amax, 0.5), (0.03 * amax, 0.0)][:count]


def wsse(A, X, b, w):
    """sum_i w_i (a_i.X_j - b_i)^2 per column (fp64)."""
    R = np.asarray(A, dtype=np.float64) @ np.asarray(X, dtype=np.float64) - np.asarray(b, dtype=np.float64)[:, None]
    return (np.asarray(w, dtype=np.float64)[:, None] * R * R).sum(axis=0)


def wnll(A, X, y, w):
    """sum_i w_i (log(1 + e^{z_ij}) - y_i z_ij) per column (fp64)."""
    return (np.asarray(w, dtype=np.float64)[:, None] * lg.nll_terms(A, X, y)).sum(axis=0)


def wnll_tolerance(A, X, w):
    """tests/_logit.nll_tolerance with each row's term scaled by w_i, plus one eps32 per term for the product with w."""
    A = np.asarray(A, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)[:, None]
    eps32 = float(np.finfo(np.float32).eps)
    z = A @ X
    terms = np.abs(z) + np.log(2.0)                # 0 <= l_ij <= |z_ij| + log 2 for labels in [0, 1]
    return 4.0 * eps32 * ((w * (np.abs(A) @ np.abs(X))).sum(axis=0) + (w * (np.abs(z) + 1.0)).sum(axis=0)) + \
        eps32 * (w * terms).sum(axis=0)
