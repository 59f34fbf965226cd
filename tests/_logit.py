"""The fp64 reference of the logistic lockstep and the data recipe its tests share (a helper: no tests in here).

LogisticProblem is the oracle's FistaProblem with ONE method replaced: gradient(y) = A^T (sigma(A y) - b) (+ alpha2 y).  init_state,
prox, step and step_delta - momentum, restarts, stops - are the oracle's own, so a logistic run follows the reference's loop
exactly as a squared-loss run does."""
import numpy as np

from oracle import fos_oracle as orc
from tests import _data

ITERS = 30
TOL = 1e-5                                # the project's standing tolerance of the lockstep against the fp64 oracle


def sigmoid(z):
    return 0.5 * (1.0 + np.tanh(0.5 * np.asarray(z, dtype=np.float64)))


def nll_terms(A, x, y):
    """log(1 + e^z) - y z per row, z = A x, without overflow at either end (fp64)."""
    z = np.asarray(A, dtype=np.float64) @ np.asarray(x, dtype=np.float64)
    yy = np.asarray(y, dtype=np.float64)
    yy = yy.reshape(yy.shape + (1,) * (z.ndim - 1))
    return np.maximum(z, 0.0) - yy * z + np.log1p(np.exp(-np.abs(z)))


def nll(A, x, y):
    """sum_i log(1 + e^{z_i}) - y_i z_i for a vector x, or per column of an n x k block."""
    return nll_terms(A, x, y).sum(axis=0)


def objective(A, x, y, alpha1, alpha2):
    x = np.asarray(x, dtype=np.float64)
    return nll(A, x, y) + alpha1 * np.abs(x).sum(axis=0) + 0.5 * alpha2 * (x * x).sum(axis=0)


class LogisticProblem(orc.FistaProblem):
    def gradient(self, y):
        g = self.A.T @ (sigmoid(self.A @ y) - self.b)
        return g + self.a2 * y if self.a2 > 0 else g


def run(A, y, alpha1, alpha2, L, max_iter=ITERS, *, delta=None, t_init_factor=1.0, tol_ratio=0.0, adaptive_restart=False,
        restart_threshold=1.0, objectives=None):
    """(x, iterations run) of FISTA (FISTA-delta with `delta`) on the logistic objective from x0 = 0, L the constant of the data
    term.  objectives: a list that receives the objective after every iteration."""
    prob = LogisticProblem(A, y, alpha1, alpha2)
    st = prob.init_state(L, t_init_factor)
    for _ in range(max_iter):
        if delta is None:
            prob.step(st, tol_ratio=tol_ratio, adaptive_restart=adaptive_restart, restart_threshold=restart_threshold)
        else:
            prob.step_delta(st, delta, tol_ratio=tol_ratio)
        if objectives is not None:
            objectives.append(float(objective(prob.A, st.x, prob.b, alpha1, alpha2)))
        if st.stopped:
            break
    return st.x, st.k


def labels(A, xt, seed):
    """Bernoulli labels of the planted model: P(y_i = 1) = sigma(2 a_i . xt)."""
    return (np.random.default_rng(seed + 7).random(A.shape[0]) < sigmoid(2.0 * (A @ xt))).astype(np.float64)


def lipschitz(A64, seed):
    """lambda_max(A^T A) / 4 from the oracle's power iteration, passed to both sides."""
    return float(orc.estimate_lipschitz(A64, v0=np.random.default_rng(seed + 1).standard_normal(A64.shape[1]))) / 4.0


def weights(A64, y, count=3):
    """Below alpha_max = max |A^T (y - 1/2)| (above it x = 0 is the solution): lasso and elastic-net weights."""
    amax = float(np.max(np.abs(A64.T @ (y - 0.5))))
    return [(0.3 * amax, 0.0), (0.1 * amax, 0.5), (0.03 * amax, 0.0)][:count]


def recipe(m, n, seed, round_a=None):
    """(A fp64 as the device stores it, y, xt, L).  round_a: a function float32 ndarray -> the stored values as fp64 (bf16
    storage rounds A; the comparison is against the rounded matrix)."""
    A, _, xt = _data.synth(m, n, seed)
    A64 = A.astype(np.float32).astype(np.float64) if round_a is None else round_a(A.astype(np.float32))
    return A64, labels(A, xt, seed), xt, lipschitz(A64, seed)


def nll_tolerance(A, X, y=None):
    """Bound of an fp32 log-loss sum against fp64 on the same fp32 x, per column: the log-loss is 1-Lipschitz in z, z carries
    the 4 eps32 |A_i| . |x| of _data.fp32_pass_tolerances, each term's own fp32 rounding is a few ulp of |z| + 1."""
    A = np.asarray(A, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    eps32 = float(np.finfo(np.float32).eps)
    return 4.0 * eps32 * ((np.abs(A) @ np.abs(X)).sum(axis=0) + (np.abs(A @ X) + 1.0).sum(axis=0))
