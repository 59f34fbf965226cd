"""The fp64 reference of the working-set solve (fastoptsolver_amd/working_set.py) and the seeded cases its tests share (a helper:
no tests in here).

`scan` restates fos_kkt_scan in the arithmetic include/fos_working_set.h states, `gradient` the data-term gradient of
fos_gradient_batch, `solve` the outer loop of working_set_path on top of the existing references: the inner solver of a round is
tests/_coord.problem - the oracle's FistaProblem, tests/_logit.LogisticProblem or tests/_weighted's weighted forms with the
per-coordinate penalty - stepped by the oracle's own `step` from the warm start.  tests/test_working_set_reference.py validates this
file on its own, on the CPU; tests/test_gpu_working_set.py compares the device with it."""
import functools

import numpy as np

from tests import _coord as cd, _forms, _logit as lg

PAD_COLUMNS, MIN_COLUMNS = 64, 128
EPS32 = float(np.finfo(np.float32).eps)


def scan(G, alpha1, slack, in_ws, p=None):
    """(excess as float32, violators as int32 in increasing order) of fos_kkt_scan.  G: nv x n float32 (the device block)."""
    G = np.asarray(G, dtype=np.float32)
    nv, n = G.shape
    p = np.ones(n) if p is None else np.asarray(p, dtype=np.float32).astype(np.float64)
    out = np.asarray(in_ws) == 0
    a = np.abs(G).astype(np.float64)                                     # (double)|G_ij|
    d = np.asarray(alpha1, dtype=np.float64)[:, None] * p[None, :]       # alpha1[j] * (double)p_i
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(d > 0.0, a / np.where(d > 0.0, d, 1.0), np.where(a > 0.0, np.inf, 0.0))
    excess = np.where(out, e.max(axis=0), 0.0).astype(np.float32)
    viol = out & (a > d * (1.0 + float(slack))).any(axis=0)
    return excess, np.nonzero(viol)[0].astype(np.int32)


def gradient(A, b, X, loss="squared", w=None):
    """The gradient of the data term at the columns of X (n x nv) in fp64: A^T W (A X - b) or A^T W (sigma(A X) - b); n x nv."""
    A, X = np.asarray(A, dtype=np.float64), np.asarray(X, dtype=np.float64)
    Z = A @ X
    R = (lg.sigmoid(Z) if loss == "logistic" else Z) - np.asarray(b, dtype=np.float64)[:, None]
    if w is not None:
        R = np.asarray(w, dtype=np.float64)[:, None] * R
    return A.T @ R


def data_term(A, b, X, loss="squared", w=None):
    """What fos_residual_batch(use_b = 1) gives per column: sum_i w_i r_i^2, or the weighted log-loss sum."""
    A, X = np.asarray(A, dtype=np.float64), np.asarray(X, dtype=np.float64)
    w = np.ones(A.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    if loss == "logistic":
        return (w[:, None] * lg.nll_terms(A, X, b)).sum(axis=0)
    R = A @ X - np.asarray(b, dtype=np.float64)[:, None]
    return (w[:, None] * R * R).sum(axis=0)


def lipschitz(A, loss="squared", w=None):
    """The exact constant of the data term: lambda_max(A^T W A), a quarter of it for the log-loss."""
    A = np.asarray(A, dtype=np.float64)
    if w is not None:
        A = np.sqrt(np.asarray(w, dtype=np.float64))[:, None] * A
    L = float(np.linalg.norm(A, 2) ** 2)
    return L / 4.0 if loss == "logistic" else L


def inner(A, b, alpha1, alpha2, L, iters, *, p=None, loss="squared", w=None, x0=None):
    """`iters` FISTA iterations of tests/_coord's problem from x0 (t = 1, y = x0: what fos_fista_reset makes of an x0)."""
    prob = cd.problem(A, b, alpha1, alpha2, p, loss=loss, w=w)
    st = prob.init_state(L)
    if x0 is not None:
        x0 = np.asarray(x0, dtype=np.float64)
        st.x, st.x_old, st.y = x0.copy(), x0.copy(), x0.copy()
    for _ in range(iters):
        prob.step(st)
    return st.x


def full(A, b, alphas, iters, *, p=None, loss="squared", w=None, L=None):
    """The full-problem reference: every weight on all columns from zero; n x nv."""
    L = lipschitz(A, loss, w) if L is None else L
    return np.stack([inner(A, b, a1, a2, L, iters, p=p, loss=loss, w=w) for a1, a2 in alphas], axis=1)


def kkt_violation(A, b, X, alphas, *, p=None, loss="squared", w=None):
    """Per weight, the largest violation of the full problem's optimality conditions at column j of X, relative to alpha1_j:
    |g + a2 p x + a1 p sign(x)| on the support, max(|g| - a1 p, 0) off it (g: the data-term gradient)."""
    n = A.shape[1]
    p = np.ones(n) if p is None else np.asarray(p, dtype=np.float64)
    G = gradient(A, b, X, loss, w)
    out = []
    for j, (a1, a2) in enumerate(alphas):
        x, g = X[:, j], G[:, j] + a2 * p * X[:, j]
        v = np.where(x != 0.0, np.abs(g + a1 * p * np.sign(x)), np.maximum(np.abs(g) - a1 * p, 0.0))
        out.append(float(v.max()) / a1)
    return np.asarray(out)


def solve(A, b, alphas, iters, *, p=None, loss="squared", w=None, L=None, kkt_tol=1e-4, max_rounds=20, grow=2.0, max_fraction=0.5,
          initial=None):
    """The outer loop of working_set_path for ONE group of up to 16 weights, in fp64: (X n x nv, info dict with rounds, sizes,
    full_gradients, worst_excess, fell_back).  L: None takes every sub-problem's own exact constant."""
    A = np.asarray(A, dtype=np.float64)
    n, nv = A.shape[1], len(alphas)
    assert nv <= 16
    a1s = [a1 for a1, _ in alphas]
    pf = np.ones(n) if p is None else np.asarray(p, dtype=np.float64)
    X = np.zeros((n, nv))
    grads, sizes, fell_back = 0, [], False

    def check(slack, in_ws):
        return scan(gradient(A, b, X, loss, w).T.astype(np.float32), a1s, slack, in_ws, pf)

    if initial is not None:
        mask = np.zeros(n, dtype=np.uint8)
        mask[np.asarray(initial)] = 1
        worst = float("nan")
    else:
        mask = (pf == 0).astype(np.uint8)
        excess, viol = check(0.0, mask)
        grads += 1
        mask[viol] = 1
        worst = float(excess.max())
    while True:
        idx = np.nonzero(mask)[0]
        if idx.size == 0:
            break
        if idx.size > max_fraction * n or len(sizes) == max_rounds:
            fell_back = True
            break
        sizes.append(int(idx.size))
        A_ws = A[:, idx]
        L_ws = lipschitz(A_ws, loss, w) if L is None else L
        for j, (a1, a2) in enumerate(alphas):
            X[idx, j] = inner(A_ws, b, a1, a2, L_ws, iters, p=None if p is None else pf[idx], loss=loss, w=w, x0=X[idx, j])
        excess, viol = check(kkt_tol, mask)
        grads += 1
        worst = float(excess.max())
        if viol.size == 0:
            break
        mask[viol] = 1
        want = int((grow - 1.0) * idx.size)
        if viol.size < want:
            order = np.argsort(-excess.astype(np.float64), kind="stable")[:want]
            mask[order[excess[order] > 0]] = 1
    if fell_back:
        Lf = lipschitz(A, loss, w) if L is None else L
        for j, (a1, a2) in enumerate(alphas):
            X[:, j] = inner(A, b, a1, a2, Lf, iters, p=p, loss=loss, w=w, x0=X[:, j])
        excess, _ = check(kkt_tol, (X != 0).any(axis=1).astype(np.uint8))
        grads += 1
        worst = float(excess.max())
    return X, dict(rounds=len(sizes), sizes=sizes, full_gradients=grads, worst_excess=worst, fell_back=fell_back)


# ---- the cases of the end-to-end tests: 300 x 256, a planted support of 8, 16 weights --------------------------------------------
M, N, SUPPORT, WEIGHTS = 300, 256, 8, 16
FRACTIONS = (0.9, 0.35)                  # the weights, as fractions of alpha_max: geometric from the first to the second
ITERS = 500                              # lockstep iterations per round; twice as many take the fp64 references to 1e-14 of alpha1
# The planted growth case: neighbouring columns correlate (AR(1), 0.5) and the weights reach further down, so coordinates whose
# gradient at X = 0 lies below every weight enter the model once their neighbours are fitted - round 1 (20 columns) leaves
# violators, the set doubles (the top-k branch of the growth step) and round 2 (40 columns) certifies.  Found by a seed search on
# the reference alone; tests/test_working_set_reference.py asserts that it still does what this comment says.
GROWTH = dict(seed=14, corr=0.5, fractions=(0.9, 0.25))
FALLBACK_FRACTION = 0.02                 # max_fraction * 256 = 5 columns: below the first set of every case


def stored(A, kind):
    """A as the device stores it (fp32, or bf16 for kind "bf16"), in fp64."""
    A32 = np.asarray(A, dtype=np.float32)
    return (_forms.bf16_round_np(A32) if kind == "bf16" else A32).astype(np.float64)


def alpha_max(A, b, p=None, loss="squared", w=None):
    g0 = np.abs(gradient(A, b, np.zeros((A.shape[1], 1)), loss, w)[:, 0])
    p = np.ones(A.shape[1]) if p is None else np.asarray(p, dtype=np.float64)
    return float((g0[p > 0] / p[p > 0]).max())


@functools.lru_cache(maxsize=None)
def case(loss, weighted, penalized, kind, seed=11, corr=0.0, m=M, n=N, fractions=FRACTIONS, enet=True):
    """One end-to-end case, computed once and never modified: dict(A (fp64, as stored), b, w, p, alphas, L (of the full data
    term), support).  corr: the correlation of neighbouring columns (an AR(1) design).  The weights alternate lasso and elastic net
    (alpha2 = alpha1 / 10) when `enet`."""
    rng = np.random.default_rng(4200 + seed)
    Z = rng.standard_normal((m, n))
    if corr:
        for c in range(1, n):
            Z[:, c] = corr * Z[:, c - 1] + np.sqrt(1.0 - corr * corr) * Z[:, c]
    A = stored(Z, kind)
    support = np.sort(rng.choice(n, size=SUPPORT, replace=False))
    xt = np.zeros(n)
    xt[support] = rng.choice([-1.0, 1.0], size=SUPPORT) * rng.uniform(1.0, 2.0, size=SUPPORT)
    if loss == "logistic":
        b = (rng.random(m) < lg.sigmoid(A @ xt)).astype(np.float64)
    else:
        b = (A @ xt + 0.1 * rng.standard_normal(m)).astype(np.float32).astype(np.float64)
    w = rng.integers(1, 4, size=m).astype(np.float64) if weighted else None
    p = None
    if penalized:                        # factors over half a decade, two unpenalised coordinates (one on the support)
        p = (10.0 ** rng.uniform(-0.25, 0.25, size=n)).astype(np.float32).astype(np.float64)
        p[[support[0], (support[0] + 1) % n]] = 0.0
    amax = alpha_max(A, b, p, loss, w)
    a1 = amax * np.geomspace(fractions[0], fractions[1], WEIGHTS)
    alphas = tuple((float(a), float(a) / 10.0 if (enet and i % 2) else 0.0) for i, a in enumerate(a1))
    out = dict(A=A, b=b, w=w, p=p, alphas=alphas, L=lipschitz(A, loss, w), support=support, amax=amax)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
