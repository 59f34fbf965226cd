"""The fp64 reference of the group penalty across lockstep columns and the data recipes its tests share (a helper: no tests in
here).

    data term(X) + alpha1 sum_j p_j ||X[j,:]||_2 + 0.5 alpha2 sum_j p_j ||X[j,:]||_2^2 ,   X n x G

GroupMultinomial is tests/_multinomial.MultinomialProblem with `prox` replaced by the row-group threshold; MultiTask is the
oracle's FistaProblem on the stacked unknown vec(X) (row-major) with the gradient A^T (A X - B) (+ alpha2 p X).  Momentum and
update order stay the oracle's step / step_delta.  enet=True is the device's PROX_ENET form: the ridge term leaves the gradient
and the thresholded row is divided by 1 + step alpha2 p_j.  Every prox call records the row norms ||v_j|| and thresholds it saw,
so a test knows which zero rows of the last iteration are zero by a margin."""
import functools

import numpy as np

from oracle import fos_oracle as orc
from tests import _data, _forms, _menu_coord, _multinomial as mn

ITERS, TOL = mn.ITERS, mn.TOL


# (shape name of tests/_menu_coord.shapes, columns G of a fit, weight pairs) - every count but the single-pair ones leaves the
# last lockstep group partial: floor(16 / G) = 8, 5, 3, 1.
MULTINOMIAL_CASES = [("one_tile", 2, 9), ("edges", 3, 7), ("edges", 5, 4), ("rb2", 16, 1), ("panels", 5, 2), ("whole_wgs", 3, 6),
                     ("whole_wgs", 16, 2)]
MULTITASK_CASES = [("one_tile", 2, 9), ("edges", 3, 6), ("edges", 5, 4), ("panels", 16, 1), ("panels", 3, 2), ("one_tile", 16, 2)]
VARIANTS = {"l1-fista": (False, None), "l1-delta": (False, 3.0), "enet-fista": (True, None), "enet-delta": (True, 3.0)}   # (enet, delta)
SEED = 3


def case_shape(name, kind, cus=256):
    c = _menu_coord.shapes(kind, cus)[name]
    return c["m"], c["n"]


def group_prox(V, step, alpha1, alpha2_prox, p, record=None):
    """Row j of V (n x G) scaled by max(0, 1 - step alpha1 p_j / ||V[j]||), exactly 0.0 where the norm is at most the threshold,
    then divided by 1 + step alpha2_prox p_j."""
    V = np.asarray(V, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    nrm = np.sqrt((V * V).sum(axis=1))
    thr = step * alpha1 * p
    if alpha1 > 0:
        s = np.where(nrm <= thr, 0.0, 1.0 - thr / np.where(nrm > 0, nrm, 1.0))
    else:
        s = np.ones_like(nrm)
    X = s[:, None] * V
    X[s == 0.0] = 0.0
    if alpha2_prox > 0:
        X = X / (1.0 + step * alpha2_prox * p)[:, None]
    if record is not None:
        record.last_vnorm, record.last_thr = nrm, thr
    return X


def penalty(X, alpha1, alpha2, p=None):
    X = np.asarray(X, dtype=np.float64)
    pp = np.ones(X.shape[0]) if p is None else np.asarray(p, dtype=np.float64)
    row2 = (X * X).sum(axis=1)
    return alpha1 * float((pp * np.sqrt(row2)).sum()) + 0.5 * alpha2 * float((pp * row2).sum())


class GroupMultinomial(mn.MultinomialProblem):
    def __init__(self, A, y, C, alpha1, alpha2, w=None, p=None, enet=False):
        super().__init__(A, y, C, alpha1, alpha2, w, p)
        self.enet = bool(enet)

    def gradient(self, y):
        G = self.A.T @ self.residual(y)
        if self.a2 > 0 and not self.enet:
            G = G + (self.a2 * self.p)[:, None] * y.reshape(-1, self.C)
        return G.reshape(-1)

    def prox(self, v, step):
        return group_prox(v.reshape(-1, self.C), step, self.a1, self.a2 if self.enet else 0.0, self.p, self).reshape(-1)

    def smooth_gradient(self, X):
        """The gradient of the data term alone (the KKT conditions carry both penalty terms themselves)."""
        return self.A.T @ self.residual(np.asarray(X).reshape(-1))

    def value(self, x):
        X = x.reshape(-1, self.C)
        return mn.nll(self.A, X, self.b, self.w) + penalty(X, self.a1, self.a2, self.p)


class MultiTask(orc.FistaProblem):
    def __init__(self, A, B, alpha1, alpha2, p=None, enet=False):
        super().__init__(A, B, alpha1, alpha2)
        self.C = self.b.shape[1]
        self.p = np.ones(self.A.shape[1]) if p is None else np.asarray(p, dtype=np.float64)
        self.enet = bool(enet)

    def smooth_gradient(self, X):
        X = np.asarray(X).reshape(-1, self.C)
        return self.A.T @ (self.A @ X - self.b)

    def gradient(self, y):
        G = self.smooth_gradient(y)
        if self.a2 > 0 and not self.enet:
            G = G + (self.a2 * self.p)[:, None] * y.reshape(-1, self.C)
        return G.reshape(-1)

    def prox(self, v, step):
        return group_prox(v.reshape(-1, self.C), step, self.a1, self.a2 if self.enet else 0.0, self.p, self).reshape(-1)

    def init_state(self, L, t_init_factor=1.0):
        if self.a2 > 0:
            L = L + self.a2 * float(self.p.max())
        z = np.zeros(self.A.shape[1] * self.C)
        return orc.FistaState(x=z.copy(), x_old=z.copy(), y=z.copy(), t=1.0, tau=t_init_factor / L)

    def value(self, x):
        X = x.reshape(-1, self.C)
        R = self.A @ X - self.b
        return 0.5 * float((R * R).sum()) + penalty(X, self.a1, self.a2, self.p)


def iterate(prob, L, max_iter=ITERS, *, delta=None, objectives=None, adaptive_restart=False, restart_threshold=1.0,
            move_tol=0.0):
    """(X n x G, the problem) after max_iter iterations of the oracle's loop from X0 = 0 (sooner once an iterate moves by less
    than move_tol)."""
    st = prob.init_state(L)
    for _ in range(max_iter):
        if delta is None:
            out = prob.step(st, adaptive_restart=adaptive_restart, restart_threshold=restart_threshold)
        else:
            out = prob.step_delta(st, delta)
        if objectives is not None:
            objectives.append(prob.value(st.x))
        if move_tol > 0.0 and out["move"] < move_tol:
            break
    return st.x.reshape(-1, prob.C), prob


def kkt_violation(prob, X):
    """Largest violation of the group KKT conditions at X: ||g_j|| - alpha1 p_j (if positive) on zero rows, || g_j + alpha1 p_j
    x_j / ||x_j|| + alpha2 p_j x_j || on the others; g the gradient of the data term."""
    G = prob.smooth_gradient(X)
    nrm = np.sqrt((X * X).sum(axis=1))
    zero = nrm == 0.0
    worst = 0.0
    if zero.any():
        worst = max(worst, float(np.max(np.sqrt((G[zero] ** 2).sum(axis=1)) - prob.a1 * prob.p[zero])))
    if (~zero).any():
        Xn, pn = X[~zero], prob.p[~zero]
        res = G[~zero] + (prob.a1 * pn / nrm[~zero])[:, None] * Xn + (prob.a2 * pn)[:, None] * Xn
        worst = max(worst, float(np.sqrt((res ** 2).sum(axis=1)).max()))
    return worst


def safe_zero_rows(prob, X):
    """Rows of the reference that are zero after the last iteration with ||v_j|| < (1 - 1e-3) tau alpha1 p_j: the device, which
    is TOL-close before the threshold, must have them exactly 0.0 in every column."""
    return (np.abs(X).sum(axis=1) == 0.0) & (prob.last_vnorm < (1.0 - 1e-3) * prob.last_thr)


def check_recipe(X, X_sep):
    """What every GPU recipe must show on the reference, so that a GPU test cannot pass vacuously: an all-zero row, a non-zero
    row, and more than 100 TOL of relative distance from the separable reference at the same weights."""
    zero = np.abs(X).sum(axis=1) == 0.0
    assert zero.any(), "no all-zero row"
    assert (~zero).any(), "no non-zero row"
    assert mn.rel(X, X_sep) > 100 * TOL, mn.rel(X, X_sep)


# ---- grouped multinomial recipes -----------------------------------------------------------------------------------------
FRACTIONS = [(0.3, 0.0), (0.1, 0.5), (0.03, 0.0), (0.2, 0.0), (0.06, 0.25), (0.15, 0.0), (0.05, 0.0), (0.08, 1.0), (0.25, 0.1)]


def multinomial_weights(A64, y, C, count=3, w=None, enet=False):
    """Below the group alpha_max = max_j ||(A^T W (onehot(y) - 1/C))_j||_2 (above it X = 0 solves the problem).  enet: every
    pair has alpha2 > 0."""
    ww = np.ones(A64.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    G0 = A64.T @ (ww[:, None] * (mn.onehot(y, C) - 1.0 / C))
    gmax = float(np.sqrt((G0 * G0).sum(axis=1)).max())
    return [(f * gmax, (a2 if a2 > 0 else 0.5) if enet else a2) for f, a2 in FRACTIONS[:count]]


@functools.lru_cache(maxsize=None)
def multinomial_reference(m, n, C, seed, kind, a1, a2, delta=None, enet=False):
    """(X, safe zero rows) of the grouped reference on mn.recipe after ITERS iterations; the recipe is checked here."""
    A64, y, L = mn.recipe(m, n, C, seed, kind)
    X, prob = iterate(GroupMultinomial(A64, y, C, a1, a2, enet=enet), L, delta=delta)
    check_recipe(X, mn.run(A64, y, C, a1, a2, L, delta=delta))
    safe = safe_zero_rows(prob, X)
    X.setflags(write=False)
    return X, safe


# ---- multi-task recipes --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def multitask_recipe(m, n, T, seed, kind="f32"):
    """(A fp64 as the device stores it, B fp64 of the fp32 targets, L): B = A X* + noise with X* supported on max(3, n / 10)
    shared rows.  Computed once and never modified."""
    A, _, _ = _data.synth(m, n, seed)
    A32 = A.astype(np.float32)
    A64 = _forms.bf16_round_np(A32).astype(np.float64) if kind == "bf16" else A32.astype(np.float64)
    rng = np.random.default_rng(seed + 23)
    XT = np.zeros((n, T))
    rows = rng.choice(n, max(3, n // 10), replace=False)
    XT[rows] = rng.standard_normal((rows.size, T))
    B = (A @ XT + 0.1 * rng.standard_normal((m, T))).astype(np.float32).astype(np.float64)
    L = 2.0 * mn.lipschitz(A64, seed)
    A64.setflags(write=False)
    B.setflags(write=False)
    return A64, B, L


def multitask_weights(A64, B, count=3, enet=False):
    G0 = A64.T @ B
    gmax = float(np.sqrt((G0 * G0).sum(axis=1)).max())
    return [(f * gmax, (a2 if a2 > 0 else 0.5) if enet else a2) for f, a2 in FRACTIONS[:count]]


def separable_multitask(A64, B, a1, a2, L, delta=None, p=None):
    """T independent lassos (the oracle's own soft threshold on the stacked unknown) at the same weights."""
    prob = MultiTask(A64, B, a1, a2, p)
    pp = np.repeat(prob.p, prob.C)
    prob.prox = lambda v, step: orc.prox_l1(v, step * a1 * pp) if a1 > 0 else v
    return iterate(prob, L, delta=delta)[0]


@functools.lru_cache(maxsize=None)
def multitask_reference(m, n, T, seed, kind, a1, a2, delta=None, enet=False):
    A64, B, L = multitask_recipe(m, n, T, seed, kind)
    X, prob = iterate(MultiTask(A64, B, a1, a2, enet=enet), L, delta=delta)
    check_recipe(X, separable_multitask(A64, B, a1, a2, L, delta))
    safe = safe_zero_rows(prob, X)
    X.setflags(write=False)
    return X, safe


def multitask_objective(A64, B, X, a1, a2, p=None):
    R = A64 @ np.asarray(X, dtype=np.float64) - B
    return 0.5 * float((R * R).sum()) + penalty(X, a1, a2, p)
