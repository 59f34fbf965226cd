"""The fp64 reference of the duality-gap certificate (include/fos_duality.h, fastoptsolver_amd/duality.py) and the seeded cases
its tests share (a helper: no tests in here).

For one column - a point x with the weights (alpha1, alpha2) - with z = A x, row weights w (or 1), penalty factors p (or 1),
tau = alpha1 p, rho = alpha2 p, psi = df/dz and G = A^T (w psi):

    P = sum_i w_i f(z_i, b_i) + sum_k (tau_k |x_k| + rho_k x_k^2 / 2)
    s = min(1, min over {k : rho_k = 0 and G_k != 0} of tau_k / |G_k|)
    D = sum_i w_i d(z_i, b_i; s) - sum over {k : rho_k > 0} of max(s |G_k| - tau_k, 0)^2 / (2 rho_k)

The loss functions are those of tests/_link.py (Huber, squared hinge) and tests/_logit.py (sigmoid, log-loss terms); the FISTA
iterates come from tests/_coord.problem, the oracle's loop with the per-coordinate penalty, for the squared and the logistic loss
and from tests/_link.LinkProblem / CoordLinkProblem for the other two.  tests/test_duality_reference.py validates this file on its own, on the CPU;
tests/test_gpu_duality.py compares the device with it."""
import functools

import numpy as np

from tests import _coord as cd, _forms, _link as lk, _logit as lg

SQUARED, LOGISTIC, HUBER, HINGE = "squared", "logistic", lk.HUBER, lk.HINGE
LOSSES = (SQUARED, LOGISTIC, HUBER, HINGE)
FORMS = ("plain", "weighted", "penalised")
TOL = 1e-5                               # the project's fp32 parity bound


def _col(v, z):
    return np.asarray(v, dtype=np.float64).reshape((-1,) + (1,) * (np.ndim(z) - 1))


def psi(loss, z, b, c=None):
    """df/dz per element, unweighted (fp64); z (m) or (m x k), b (m)."""
    z = np.asarray(z, dtype=np.float64)
    if loss in (HUBER, HINGE):
        return lk.psi(loss, z, b, c)
    return (lg.sigmoid(z) if loss == LOGISTIC else z) - _col(b, z)


def loss_terms(loss, z, b, c=None):
    """f per element: (z - b)^2 / 2 with its half, the log-loss, the Huber loss, the squared hinge with its half."""
    z = np.asarray(z, dtype=np.float64)
    if loss in (HUBER, HINGE):
        return lk.loss_terms(loss, z, b, c)
    bb = _col(b, z)
    if loss == LOGISTIC:
        return np.maximum(z, 0.0) - bb * z + np.log1p(np.exp(-np.abs(z)))          # tests/_logit.nll_terms on a given z
    return 0.5 * (z - bb) ** 2


def _xlogx(q):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(q > 0.0, q * np.log(np.where(q > 0.0, q, 1.0)), 0.0)


def dual_terms(loss, z, b, s, c=None):
    """d per element: minus the conjugate of the loss at the scaled derivative s psi.  s: a scalar, or one value per column of z."""
    z = np.asarray(z, dtype=np.float64)
    bb = _col(b, z)
    s = np.asarray(s, dtype=np.float64)
    if loss == HINGE:
        h = np.maximum(0.0, 1.0 - bb * z)
        return s * h - 0.5 * (s * h) ** 2
    if loss == LOGISTIC:
        q = bb + s * (lg.sigmoid(z) - bb)
        return -(_xlogx(q) + _xlogx(1.0 - q))
    v = psi(loss, z, b, c)
    return -s * v * bb - 0.5 * (s * v) ** 2


def gradient(loss, A, X, b, c=None, w=None):
    """G = A^T (w psi(A X)) in fp64: n x k."""
    A = np.asarray(A, dtype=np.float64)
    Z = A @ np.asarray(X, dtype=np.float64)
    R = psi(loss, Z, b, c)
    if w is not None:
        R = _col(w, Z) * R
    return A.T @ R


def _tau_rho(n, p, alphas):
    p = np.ones(n) if p is None else np.asarray(p, dtype=np.float32).astype(np.float64)      # (double)p_k of the stored factor
    a1 = np.asarray([a for a, _ in alphas], dtype=np.float64)[:, None]
    a2 = np.asarray([a for _, a in alphas], dtype=np.float64)[:, None]
    return a1 * p[None, :], a2 * p[None, :]


def scale_of(G, p, alphas):
    """dual_scale_kernel's scale, restated: per column j, min(1, min over {k : rho_jk = 0 and G_jk != 0} of tau_jk / (double)|G_jk|)
    with tau_jk = alpha1_j * (double)p_k, all in fp64 on the given G (nv x n; float32 as the device returns it, or float64)."""
    G = np.asarray(G)
    a = np.abs(G).astype(np.float64)
    tau, rho = _tau_rho(G.shape[1], p, alphas)
    on = (rho == 0.0) & (a != 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(on, tau / np.where(on, a, 1.0), np.inf)
    return np.minimum(1.0, ratio.min(axis=1))


def certificate(loss, A, b, X, alphas, c=None, w=None, p=None, G=None):
    """The certificate of the columns of X (n x nv) in fp64: a dict of per-column arrays - primal, dual, gap, scale, and the
    magnitudes the comparisons are normalised by: mag_primal = sum |w f| + penalty, mag_dual = sum |w d| + conjugate, mag_gap their
    sum.  G (nv x n): the gradient block the scale and the conjugate are formed from; None takes the fp64 gradient."""
    A, X = np.asarray(A, dtype=np.float64), np.asarray(X, dtype=np.float64)
    n, nv = X.shape
    assert len(alphas) == nv
    Z = A @ X
    ww = np.ones((A.shape[0], 1)) if w is None else np.asarray(w, dtype=np.float64)[:, None]
    G = gradient(loss, A, X, b, c, w).T if G is None else np.asarray(G)[:, :n]
    tau, rho = _tau_rho(n, p, alphas)
    s = scale_of(G, p, alphas)
    f = ww * loss_terms(loss, Z, b, c)
    d = ww * dual_terms(loss, Z, b, s[None, :], c)
    pen = (tau * np.abs(X.T) + 0.5 * rho * X.T ** 2).sum(axis=1)
    excess = np.maximum(s[:, None] * np.abs(G).astype(np.float64) - tau, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        conj = np.where(rho > 0.0, excess ** 2 / np.where(rho > 0.0, 2.0 * rho, 1.0), 0.0).sum(axis=1)
    primal, dual = f.sum(axis=0) + pen, d.sum(axis=0) - conj
    mag_p, mag_d = np.abs(f).sum(axis=0) + pen, np.abs(d).sum(axis=0) + conj
    return dict(primal=primal, dual=dual, gap=primal - dual, scale=s, mag_primal=mag_p, mag_dual=mag_d, mag_gap=mag_p + mag_d)


# ---- FISTA iterates of the reference ------------------------------------------------------------------------------------------
def lipschitz(loss, A, w=None):
    """The exact constant of the data term: lambda_max(A^T W A), a quarter of it for the log-loss."""
    A = np.asarray(A, dtype=np.float64)
    if w is not None:
        A = np.sqrt(np.asarray(w, dtype=np.float64))[:, None] * A
    L = float(np.linalg.norm(A, 2) ** 2)
    return L / 4.0 if loss == LOGISTIC else L


def iterates(loss, A, b, a1, a2, L, counts, c=None, w=None, p=None):
    """The FISTA iterates x_k of the reference's loop from x = 0 at the iteration counts `counts` (increasing): n x len(counts)."""
    if loss in (HUBER, HINGE):
        if p is None:
            prob = lk.LinkProblem(loss, A, b, a1, a2, c, w)
        else:
            assert a2 == 0.0             # tests/_link.CoordLinkProblem: the factors on the lasso penalty
            prob = lk.CoordLinkProblem(loss, A, b, a1, 0.0, c, w).bind(pf=p)
    else:
        prob = cd.problem(A, b, a1, a2, p, loss=loss, w=w)
    st = prob.init_state(L)
    out, k = [], 0
    for count in counts:
        for _ in range(count - k):
            prob.step(st)
        k = count
        out.append(st.x.copy())
    return np.stack(out, axis=1)


# ---- the cases of the end-to-end tests ----------------------------------------------------------------------------------------
SHAPES = {"one_tile": (257, 37), "edges": (1003, 68), "panels": (70001, 68)}          # tests/test_gpu_link.py's
COUNTS = (1, 3, 6, 12, 300)              # iterations: four points on the way (some gap / P(0) in [1e-4, 1e-1]) and a converged one
# The tall shape is so well conditioned that one full step all but solves it: its iterates take half the step (a valid,
# conservative constant), so that its points on the way are on the way.  Both were chosen on the CPU, on this file alone;
# tests/test_duality_reference.py asserts what they are chosen for.
STEP_DIVISOR = {"one_tile": 1.0, "edges": 1.0, "panels": 2.0}


def stored(A, kind):
    A32 = np.asarray(A, dtype=np.float32)
    return (_forms.bf16_round_np(A32) if kind == "bf16" else A32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(loss, form, shape, kind="f32"):
    """One end-to-end case, computed once and never modified: dict(A (fp64, as stored), b, c, w, p, alpha (a1, a2), L, X64 - the
    iterates at COUNTS, n x 5 -, X - the same rounded to fp32, what the device is given -, pre - the fp64 certificate of X64 under
    the case's weights, which the preconditions are asserted on -, p0 - P(0)).  The weight sits at a tenth of alpha_max; the
    weighted form has zeros among its weights; the penalised form has factors in [0.5, 2]; the iterates are those of the elastic
    net with alpha2 = alpha1 / 10, of the lasso on a penalised Huber or squared-hinge problem."""
    m, n = SHAPES[shape]
    rng = np.random.default_rng(7000 + 13 * m + n)
    A = stored(rng.standard_normal((m, n)) / np.sqrt(m), kind)
    xt = np.zeros(n)
    xt[rng.choice(n, size=6, replace=False)] = rng.choice([-1.0, 1.0], size=6) * rng.uniform(1.0, 2.0, size=6)
    c = None
    if loss == LOGISTIC:
        b = (rng.random(m) < lg.sigmoid(4.0 * (A @ xt))).astype(np.float64)
    elif loss == HINGE:
        b = np.sign(A @ xt + 0.05 * rng.standard_normal(m))
        b[b == 0] = 1.0
    else:
        b = (A @ xt + 0.05 * rng.standard_normal(m)).astype(np.float32).astype(np.float64)
        if loss == HUBER:
            b[rng.choice(m, size=m // 10, replace=False)] += 1.0
            b = b.astype(np.float32).astype(np.float64)
            c = float(np.float32(np.median(np.abs(b))))
    w = p = None
    if form == "weighted":
        w = rng.uniform(0.25, 4.0, m).astype(np.float32).astype(np.float64)
        w[rng.choice(m, size=m // 20, replace=False)] = 0.0
    if form == "penalised":
        p = rng.uniform(0.5, 2.0, n).astype(np.float32).astype(np.float64)
    g0 = np.abs(gradient(loss, A, np.zeros((n, 1)), b, c, w)[:, 0])
    a1 = 0.1 * float((g0 / (1.0 if p is None else p)).max())
    a2 = a1 / 10.0 if (form != "penalised" or loss in (SQUARED, LOGISTIC)) else 0.0
    L = STEP_DIVISOR[shape] * lipschitz(loss, A, w)
    X64 = iterates(loss, A, b, a1, a2, L, COUNTS, c, w, p)
    pre = certificate(loss, A, b, X64, [(a1, a2)] * len(COUNTS), c, w, p)
    p0 = certificate(loss, A, b, np.zeros((n, 1)), [(a1, a2)], c, w, p)["primal"][0]
    out = dict(A=A, b=b, c=c, w=w, p=p, alpha=(a1, a2), L=L, X64=X64, X=X64.astype(np.float32).astype(np.float64), pre=pre, p0=float(p0))
    for v in list(out.values()) + list(pre.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- certified_path on the planted-support recipe of tests/_working_set.py (300 x 256, 16 weights) ------------------------------
GAP_TOL = 1e-4                           # certified_path's default; the fp64 working-set reference ends far below it within the
PATH_ITERS, PATH_ROUNDS = 500, 20        # budget (tests/test_duality_reference.py), and 1e-4 P(0) is above the device's resolution
