"""The fp64 reference of the multinomial (softmax) lockstep and the data recipes its tests share (a helper: no tests in here).

MultinomialProblem is the oracle's FistaProblem on the stacked unknown vec(X), X n x C (row-major: x.reshape(n, C)), with the
gradient replaced: A^T (w * (softmax(A X) - onehot(y))) (+ alpha2 p * X).  step and step_delta - momentum and the update order -
are the oracle's own, so a multinomial run follows the reference's loop exactly as a squared-loss run does.  init_state sizes the
stacked zeros (tau = t / (L + alpha2 max p), the oracle's rule with the factor of tests/_coord.py) and prox is the oracle's
soft threshold per coordinate, scaled by the penalty factor and clipped to the box when a test binds them; both reduce to the
oracle's own without factors and bounds."""
import functools

import numpy as np

from oracle import fos_oracle as orc
from tests import _data, _forms

ITERS = 30
TOL = 1e-5                                # the project's standing tolerance of the lockstep against the fp64 oracle (_logit.TOL)


def softmax(Z):
    Z = np.asarray(Z, dtype=np.float64)
    E = np.exp(Z - Z.max(axis=-1, keepdims=True))
    return E / E.sum(axis=-1, keepdims=True)


def onehot(y, C):
    y = np.asarray(y).astype(np.int64)
    out = np.zeros((y.shape[0], C))
    out[np.arange(y.shape[0]), y] = 1.0
    return out


def nll_terms(A, X, y):
    """logsumexp(z_i) - z_{i, y_i} per row, Z = A X (fp64, no overflow)."""
    Z = np.asarray(A, dtype=np.float64) @ np.asarray(X, dtype=np.float64)
    mx = Z.max(axis=1)
    lse = np.log(np.exp(Z - mx[:, None]).sum(axis=1)) + mx
    return lse - Z[np.arange(Z.shape[0]), np.asarray(y).astype(np.int64)]


def nll(A, X, y, w=None):
    t = nll_terms(A, X, y)
    return float(t.sum() if w is None else (np.asarray(w, dtype=np.float64) * t).sum())


def objective(A, X, y, alpha1, alpha2, w=None, p=None):
    X = np.asarray(X, dtype=np.float64)
    pp = np.ones(X.shape[0]) if p is None else np.asarray(p, dtype=np.float64)
    return nll(A, X, y, w) + alpha1 * (pp[:, None] * np.abs(X)).sum() + 0.5 * alpha2 * (pp[:, None] * X * X).sum()


class MultinomialProblem(orc.FistaProblem):
    def __init__(self, A, y, C, alpha1, alpha2, w=None, p=None, lo=None, hi=None):
        super().__init__(A, y, alpha1, alpha2)
        n = self.A.shape[1]
        self.C = int(C)
        self.T = onehot(y, self.C)
        self.w = np.ones(self.A.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
        self.p = np.ones(n) if p is None else np.asarray(p, dtype=np.float64)
        self.lo = np.full(n, -np.inf) if lo is None else np.broadcast_to(np.asarray(lo, dtype=np.float64), (n,))
        self.hi = np.full(n, np.inf) if hi is None else np.broadcast_to(np.asarray(hi, dtype=np.float64), (n,))

    def residual(self, y):
        return self.w[:, None] * (softmax(self.A @ y.reshape(-1, self.C)) - self.T)

    def gradient(self, y):
        G = self.A.T @ self.residual(y)
        if self.a2 > 0:
            G = G + (self.a2 * self.p)[:, None] * y.reshape(-1, self.C)
        return G.reshape(-1)

    def prox(self, v, step):
        x = orc.prox_l1(v, step * self.a1 * np.repeat(self.p, self.C)) if self.a1 > 0 else v
        return np.clip(x, np.repeat(self.lo, self.C), np.repeat(self.hi, self.C))

    def init_state(self, L, t_init_factor=1.0):
        if self.a2 > 0:
            L = L + self.a2 * float(self.p.max())
        z = np.zeros(self.A.shape[1] * self.C)
        return orc.FistaState(x=z.copy(), x_old=z.copy(), y=z.copy(), t=1.0, tau=t_init_factor / L)

    def value(self, x):
        return objective(self.A, x.reshape(-1, self.C), self.b, self.a1, self.a2, self.w, self.p)


def run(A, y, C, alpha1, alpha2, L, max_iter=ITERS, *, delta=None, t_init_factor=1.0, w=None, p=None, lo=None, hi=None,
        objectives=None, adaptive_restart=False, restart_threshold=1.0):
    """X (n x C) of FISTA (FISTA-delta with `delta`) on the multinomial objective from X0 = 0 after exactly max_iter iterations,
    L the constant of the data term.  objectives: a list that receives the objective after every iteration.  adaptive_restart / restart_threshold: the oracle's
    momentum restart (threshold 0 restarts every iteration: the proximal gradient method) - the reference only, the device has no
    such multinomial run."""
    prob = MultinomialProblem(A, y, C, alpha1, alpha2, w, p, lo, hi)
    st = prob.init_state(L, t_init_factor)
    for _ in range(max_iter):
        if delta is None:
            prob.step(st, adaptive_restart=adaptive_restart, restart_threshold=restart_threshold)
        else:
            prob.step_delta(st, delta)
        if objectives is not None:
            objectives.append(prob.value(st.x))
    return st.x.reshape(-1, C)


def lipschitz(A64, seed, w=None):
    """Boehning's bound lambda_max(A^T W A) / 2 from the oracle's power iteration, passed to both sides."""
    B = A64 if w is None else np.sqrt(np.asarray(w, dtype=np.float64))[:, None] * A64
    return float(orc.estimate_lipschitz(B, v0=np.random.default_rng(seed + 1).standard_normal(A64.shape[1]))) / 2.0


def labels(A, C, seed):
    """Class labels drawn from the softmax of a sparse planted model scaled so that every logit stays within +-10; every class
    occurs (asserted)."""
    rng = np.random.default_rng(seed + 11)
    n = A.shape[1]
    XT = np.zeros((n, C))
    nz = max(3, n // 10)
    for c in range(C):
        XT[rng.choice(n, nz, replace=False), c] = rng.standard_normal(nz)
    Z = A @ XT
    Z = Z * (3.0 / Z.std())
    Z = Z * min(1.0, 10.0 / np.abs(Z).max())
    y = np.argmax(Z + rng.gumbel(size=Z.shape), axis=1)
    assert set(y.tolist()) == set(range(C)), "a class does not occur"
    assert np.abs(Z).max() <= 10.0 + 1e-9
    return y.astype(np.float64)


def weights(A64, y, C, count=3):
    """Below alpha_max = max |A^T (onehot(y) - 1/C)| (above it X = 0 is the solution): lasso and elastic-net weights."""
    amax = float(np.max(np.abs(A64.T @ (onehot(y, C) - 1.0 / C))))
    fr = [(0.3, 0.0), (0.1, 0.5), (0.03, 0.0), (0.2, 0.0), (0.06, 0.25), (0.15, 0.0), (0.05, 0.0), (0.08, 1.0), (0.25, 0.1)]
    return [(f * amax, a2) for f, a2 in fr[:count]]


@functools.lru_cache(maxsize=None)
def recipe(m, n, C, seed, kind="f32"):
    """(A fp64 as the device stores it, y, L), computed once and never modified.  kind "bf16": A rounded to bf16."""
    A, _, _ = _data.synth(m, n, seed)
    A32 = A.astype(np.float32)
    A64 = _forms.bf16_round_np(A32).astype(np.float64) if kind == "bf16" else A32.astype(np.float64)
    y = labels(A, C, seed)
    A64.setflags(write=False)
    y.setflags(write=False)
    return A64, y, lipschitz(A64, seed)


@functools.lru_cache(maxsize=None)
def reference(m, n, C, seed, kind, a1, a2, delta=None, iters=ITERS):
    A64, y, L = recipe(m, n, C, seed, kind)
    X = run(A64, y, C, a1, a2, L, iters, delta=delta)
    X.setflags(write=False)
    return X


def nll_tolerance(A, X):
    """Bound of an fp32 cross-entropy sum against fp64 on the same fp32 X: logsumexp - z_y is 2-Lipschitz in the logits (sup
    norm), a logit carries the 4 eps32 |A_i| . |x_c| of _data.fp32_pass_tolerances, each term's own fp32 rounding (max,
    exponentials, C-term sum, log, the two additions) is a few ulp of |z| + log C + 1."""
    A = np.asarray(A, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    eps32 = float(np.finfo(np.float32).eps)
    zerr = (np.abs(A) @ np.abs(X)).max(axis=1)
    return 4.0 * eps32 * float((2.0 * zerr).sum() + (2.0 * np.abs(A @ X).max(axis=1) + np.log(X.shape[1]) + 1.0).sum())


def as_np(v):
    """A result as a float64 ndarray (the solvers answer a device tensor with a tensor on that device)."""
    return v.detach().to("cpu").double().numpy() if hasattr(v, "detach") else np.asarray(v, dtype=np.float64)


def rel(a, b):
    return _data.rel(as_np(a).reshape(-1), as_np(b).reshape(-1))
