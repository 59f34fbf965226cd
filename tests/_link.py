"""The fp64 reference of the Huber and squared-hinge lockstep and the data recipes its tests share (a helper: no tests in here).

LinkProblem is the oracle's FistaProblem with ONE method replaced: gradient(y) = A^T (w * psi(A y, b)) (+ alpha2 y) with psi =
clip(z - b, -c, c) (Huber) or -b max(0, 1 - b z) (squared hinge).  init_state, prox, step and step_delta - momentum, restarts,
stops - are the oracle's own, so such a run follows the reference's loop exactly as a squared-loss run does.

The recipes assert the branch mix on the fp64 reference alone, so that no test passes on one branch of a loss only: the clipped
share of a Huber problem lies in [0.05, 0.95] at x = 0 and at the final iterate, both branches of the hinge hold at least 10 % of
the rows at the final iterate."""
import numpy as np

from oracle import fos_oracle as orc
from tests import _data

ITERS = 30
TOL = 1e-5                                # the project's standing tolerance of the lockstep against the fp64 oracle
HUBER, HINGE = "huber", "squared_hinge"
HUBER_FRACTIONS = ((0.3, 0.0), (0.1, 0.5), (0.03, 0.0))
HINGE_FRACTIONS = ((0.1, 0.5), (0.03, 0.0), (0.01, 0.0))


def psi(kind, z, b, c=None):
    """dl/dz per element (fp64); z (m) or (m x k), b (m)."""
    z = np.asarray(z, dtype=np.float64)
    bb = np.asarray(b, dtype=np.float64).reshape((-1,) + (1,) * (z.ndim - 1))
    if kind == HUBER:
        return np.clip(z - bb, -c, c)
    return -bb * np.maximum(0.0, 1.0 - bb * z)


def loss_terms(kind, z, b, c=None):
    """l per element (fp64), its 1/2 included."""
    z = np.asarray(z, dtype=np.float64)
    bb = np.asarray(b, dtype=np.float64).reshape((-1,) + (1,) * (z.ndim - 1))
    if kind == HUBER:
        r = np.abs(z - bb)
        return np.where(r <= c, 0.5 * r * r, c * r - 0.5 * c * c)
    u = np.maximum(0.0, 1.0 - bb * z)
    return 0.5 * u * u


def _w(w, z):
    return 1.0 if w is None else np.asarray(w, dtype=np.float64).reshape((-1,) + (1,) * (np.ndim(z) - 1))


def data_term(kind, A, x, b, c=None, w=None):
    """sum_i w_i l_i for a vector x, or per column of an n x k block."""
    z = np.asarray(A, dtype=np.float64) @ np.asarray(x, dtype=np.float64)
    return (_w(w, z) * loss_terms(kind, z, b, c)).sum(axis=0)


def gradient(kind, A, x, b, c=None, w=None):
    A = np.asarray(A, dtype=np.float64)
    z = A @ np.asarray(x, dtype=np.float64)
    return A.T @ (_w(w, z) * psi(kind, z, b, c))


def objective(kind, A, x, b, alpha1, alpha2, c=None, w=None):
    x = np.asarray(x, dtype=np.float64)
    return data_term(kind, A, x, b, c, w) + alpha1 * np.abs(x).sum(axis=0) + 0.5 * alpha2 * (x * x).sum(axis=0)


class LinkProblem(orc.FistaProblem):
    def __init__(self, kind, A, b, alpha1, alpha2, c=None, w=None):
        super().__init__(A, b, alpha1, alpha2)
        self.kind, self.c, self.w = kind, c, None if w is None else np.asarray(w, dtype=np.float64)

    def gradient(self, y):
        g = gradient(self.kind, self.A, y, self.b, self.c, self.w)
        return g + self.a2 * y if self.a2 > 0 else g


class CoordLinkProblem(LinkProblem):
    """Penalty factors pf >= 0 and a box [lo, hi] around 0 on the lasso penalty (alpha2 = 0): the exact prox is the soft
    threshold by step * alpha1 * pf_j followed by the clamp."""
    pf = lo = hi = None

    def bind(self, pf=None, lo=None, hi=None):
        assert self.a2 == 0.0
        self.pf, self.lo, self.hi = pf, lo, hi
        return self

    def prox(self, v, step):
        thr = step * self.a1 * (1.0 if self.pf is None else np.asarray(self.pf, dtype=np.float64))
        x = np.sign(v) * np.maximum(np.abs(v) - thr, 0.0)
        return np.clip(x, -np.inf if self.lo is None else self.lo, np.inf if self.hi is None else self.hi)


def run(kind, A, b, alpha1, alpha2, L, max_iter=ITERS, *, c=None, w=None, delta=None, t_init_factor=1.0, tol_ratio=0.0,
        adaptive_restart=False, restart_threshold=1.0, prob=None, trace=None):
    """(x, iterations run) of FISTA (FISTA-delta with `delta`) on the objective from x0 = 0, L the constant of the data term.
    prob: a problem built by the caller (another prox on the same gradient) in place of LinkProblem(kind, A, b, ...).
    trace: a dict that receives x, ratios and moves, the record tests/_coord.fp32_proof judges a controlled run by."""
    prob = LinkProblem(kind, A, b, alpha1, alpha2, c, w) if prob is None else prob
    st = prob.init_state(L, t_init_factor)
    for _ in range(max_iter):
        if delta is None:
            info = prob.step(st, tol_ratio=tol_ratio, adaptive_restart=adaptive_restart, restart_threshold=restart_threshold)
        else:
            info = prob.step_delta(st, delta, tol_ratio=tol_ratio)
        if trace is not None:
            trace.setdefault("ratios", []).append(info["ratio"])
            trace.setdefault("moves", []).append(info["move"])
        if st.stopped:
            break
    if trace is not None:
        trace["x"] = st.x
    return st.x, st.k


def lipschitz(A64, seed, w=None):
    """lambda_max(A^T W A) from the oracle's power iteration, passed to both sides."""
    Aw = A64 if w is None else A64 * np.sqrt(np.asarray(w, dtype=np.float64))[:, None]
    return float(orc.estimate_lipschitz(Aw, v0=np.random.default_rng(seed + 1).standard_normal(A64.shape[1])))


def clipped_share(A, x, b, c):
    return float(np.mean(np.abs(np.asarray(A) @ x - b) > c))


def active_share(A, x, y):
    return float(np.mean(1.0 - y * (np.asarray(A) @ x) > 0.0))


def huber_recipe(m, n, seed=3, round_a=None, check=True):
    """(A fp64 as the device stores it, b with 10 % gross outliers, c = median |b|, L, the three weights).  round_a: a function
    float32 ndarray -> the stored values as fp64 (bf16 storage)."""
    A, b, _ = _data.synth(m, n, seed)
    A64 = A.astype(np.float32).astype(np.float64) if round_a is None else round_a(A.astype(np.float32))
    rng = np.random.default_rng(20)
    out = rng.choice(m, size=max(1, m // 10), replace=False)
    b = b.copy()
    b[out] += rng.choice([-1.0, 1.0], size=out.size) * 10.0 * np.std(b)
    b = b.astype(np.float32).astype(np.float64)
    c = float(np.float32(np.median(np.abs(b))))
    L = lipschitz(A64, seed)
    amax = float(np.max(np.abs(A64.T @ psi(HUBER, np.zeros(m), b, c))))
    alphas = tuple((f * amax, a2) for f, a2 in HUBER_FRACTIONS)
    if check:
        x0 = np.zeros(A64.shape[1])
        shares = [clipped_share(A64, x0, b, c)] + [clipped_share(A64, run(HUBER, A64, b, a1, a2, L, c=c)[0], b, c) for a1, a2 in alphas]
        assert all(0.05 <= s <= 0.95 for s in shares), shares
    return A64, b, c, L, alphas


def hinge_recipe(m, n, seed, round_a=None, check=True):
    """(A fp64 as the device stores it, labels -1 / +1 of a noisy planted model, L, the three weights)."""
    A, _, xt = _data.synth(m, n, seed)
    A64 = A.astype(np.float32).astype(np.float64) if round_a is None else round_a(A.astype(np.float32))
    s = A @ xt
    y = np.sign(s + 0.5 * np.std(s) * np.random.default_rng(seed + 7).standard_normal(m))
    y[y == 0] = 1.0
    L = lipschitz(A64, seed)
    amax = float(np.max(np.abs(A64.T @ y)))
    alphas = tuple((f * amax, a2) for f, a2 in HINGE_FRACTIONS)
    if check:
        shares = [active_share(A64, run(HINGE, A64, y, a1, a2, L)[0], y) for a1, a2 in alphas]
        assert all(0.1 <= s <= 0.9 for s in shares), shares
    return A64, y, L, alphas


def loss_tolerance(kind, A, X, b, c=None, w=None):
    """Bound of an fp32 loss sum against fp64 on the same fp32 x, per column.  rho_c is min(|r|, c)-Lipschitz in z and the squared
    hinge max(0, 1 - t)-Lipschitz; z = a_i . x carries the 4 eps32 (|A_i| . |x| + |b_i|) of _data.fp32_pass_tolerances; forming
    the term from z (a subtraction, two products, the weight) is a few ulp of the term itself: 4 eps32 l."""
    A = np.asarray(A, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    eps32 = float(np.finfo(np.float32).eps)
    z = A @ X
    bb = np.asarray(b, dtype=np.float64)[:, None]
    dz = 4.0 * eps32 * (np.abs(A) @ np.abs(X) + np.abs(bb))
    # the Lipschitz factor at the far end of the interval z +- dz
    slope = np.minimum(np.abs(z - bb) + dz, c) if kind == HUBER else np.maximum(0.0, 1.0 - bb * z) + dz
    ww = _w(w, z)
    return (ww * (slope * dz + 4.0 * eps32 * loss_terms(kind, z, b, c))).sum(axis=0)
