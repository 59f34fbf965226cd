"""The references and recipes of the resampled lockstep (fastoptsolver_amd/resample.py, include/fos_resample.h) - a helper: no
tests in here.

Column j of a resampled pass fits the problem with the row weights w * c_j, so its fp64 reference is the existing weighted
reference: tests/_weighted.problem for the squared and the logistic loss, tests/_link.LinkProblem(w=) for Huber and the squared
hinge, driven by the loop of tests/_link.run (the oracle's own step, momentum, restarts and stops).  `run` below only picks the
problem and can hand back the prox input of the last step, which the stability test needs to tell a decided zero from one that
fp32 rounding may flip."""
import functools

import numpy as np

from tests import _data, _link as lk, _logit as lg, _weighted as wt

SQUARED, LOGISTIC, HUBER, HINGE = "squared", "logistic", lk.HUBER, lk.HINGE
LOSSES = (SQUARED, LOGISTIC, HUBER, HINGE)
SHAPES = {"one_tile": (257, 37), "edges": (1003, 68), "panels": (70001, 68)}       # tests/test_gpu_link.py
NVS = (1, 5, 16)
RECIPES = ("ones", "binary", "bootstrap")
TOL, ITERS = lk.TOL, lk.ITERS
MAX_COUNT = 15
F32 = np.float32


# ---- the multiplicities ---------------------------------------------------------------------------------------------------------
def pack_np(counts):
    """The layout of include/fos_resample.h restated: word i = sum_j counts[i, j] << 4 j (uint64)."""
    counts = np.asarray(counts)
    words = np.zeros(counts.shape[0], dtype=np.uint64)
    for j in range(counts.shape[1]):
        words |= counts[:, j].astype(np.uint64) << np.uint64(4 * j)
    return words


@functools.lru_cache(maxsize=None)
def counts(recipe, m, nv, seed=0):
    """m x nv int64 multiplicities.  ones: every row once; binary: a random half (0 / 1); bootstrap: m draws of m rows with
    replacement per column, and one planted row per column at 15 (with a row at 0 beside it).  Never a column of zeros."""
    rng = np.random.default_rng(9100 + 31 * seed + nv)
    if recipe == "ones":
        c = np.ones((m, nv), dtype=np.int64)
    elif recipe == "binary":
        c = (rng.random((m, nv)) < 0.5).astype(np.int64)
        c[0] = 1
    elif recipe == "bootstrap":
        c = np.stack([np.bincount(rng.integers(0, m, size=m), minlength=m) for _ in range(nv)], axis=1).astype(np.int64)
        for j in range(nv):
            c[(7 + 3 * j) % m, j] = MAX_COUNT
            c[(8 + 3 * j) % m, j] = 0
    else:
        raise ValueError(recipe)
    assert c.min() >= 0 and c.max() <= MAX_COUNT and (c.sum(axis=0) > 0).all()
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def row_weights(m, seed=0):
    """Sample weights as the device stores them: fp32 values in 0.25 .. 4 with a twentieth of exact zeros."""
    rng = np.random.default_rng(77 + seed)
    w = rng.uniform(0.25, 4.0, m).astype(F32).astype(np.float64)
    w[rng.choice(m, m // 20, replace=False)] = 0.0
    w.setflags(write=False)
    return w


def effective(w, c):
    """The weights of the reference of one column: w * c_j (w None: c_j)."""
    c = np.asarray(c, dtype=np.float64)
    return c if w is None else np.asarray(w, dtype=np.float64) * c


# ---- data -----------------------------------------------------------------------------------------------------------------------
def bf16_round(A32):
    import torch
    return torch.as_tensor(A32).to(torch.bfloat16).to(torch.float64).numpy()


@functools.lru_cache(maxsize=None)
def recipe(loss, kind, m, n):
    """(A in fp64 as the device stores it, b or the labels, the Huber threshold or None, lambda_max(A^T A) of the whole A, three
    weights below alpha_max): once per cell, never modified."""
    rnd = bf16_round if kind == "bf16" else None
    if loss == HUBER:
        A64, b, c, L, alphas = lk.huber_recipe(m, n, round_a=rnd, check=False)
    elif loss == HINGE:
        A64, b, L, alphas = lk.hinge_recipe(m, n, 3 * m + n, round_a=rnd, check=False)
        c = None
    else:
        A, b, xt = _data.synth(m, n, 3)
        A64 = A.astype(F32).astype(np.float64) if rnd is None else rnd(A.astype(F32))
        c = None
        if loss == LOGISTIC:
            b = lg.labels(A, xt, 3)
        else:
            b = b.astype(F32).astype(np.float64)
        L = lk.lipschitz(A64, 3)
        alphas = tuple(wt.alphas(A64, b, np.ones(m), loss))
    for a in (A64, b):
        a.setflags(write=False)
    return A64, b, c, float(L), tuple(alphas)


def divisor(loss):
    return 4.0 if loss == LOGISTIC else 1.0


def lipschitz(A64, w, v0):
    """lambda_max(A^T diag(w) A) from the oracle's power iteration at the start vector v0 (tests/_weighted.estimate_lipschitz)."""
    return wt.estimate_lipschitz(A64, w, v0)


# ---- the reference --------------------------------------------------------------------------------------------------------------
def problem(loss, A64, b, w, alpha1, alpha2, c=None):
    if loss in (SQUARED, LOGISTIC):
        return wt.problem(A64, b, w, alpha1, alpha2, loss)
    return lk.LinkProblem(loss, A64, b, alpha1, alpha2, c, w)


def run(loss, A64, b, w, alpha1, alpha2, L, max_iter=ITERS, *, c=None, prob=None, want_u=False, trace=None, **kw):
    """(x, iterations) of the reference on the problem with the row weights w; L is the constant of ITS data term (the divisor of
    the logistic loss applied by the caller).  prob: another prox on the same gradient (tests/_link.CoordLinkProblem, the
    feature-group class).  want_u: also the prox input y - tau grad(y) and the step tau of the last iteration run."""
    prob = problem(loss, A64, b, w, alpha1, alpha2, c) if prob is None else prob
    if not want_u:
        return lk.run(loss, A64, b, alpha1, alpha2, L, max_iter, prob=prob, trace=trace, **kw)
    assert not kw                                   # the plain loop of tests/_link.run, stopped one step early to read u
    st = prob.init_state(L)
    for _ in range(max_iter - 1):
        prob.step(st)
    u = st.y - st.tau * prob.gradient(st.y)
    prob.step(st)
    return st.x, st.k, u, st.tau


def psi(loss, z, b, c=None):
    if loss in (HUBER, HINGE):
        return lk.psi(loss, z, b, c)
    bb = np.asarray(b, dtype=np.float64).reshape((-1,) + (1,) * (np.ndim(z) - 1))
    return (lg.sigmoid(z) if loss == LOGISTIC else np.asarray(z, dtype=np.float64)) - bb


def loss_terms(loss, A64, X, b, c=None):
    """l per (row, column) in fp64: the squared loss with its 1/2."""
    if loss in (HUBER, HINGE):
        return lk.loss_terms(loss, np.asarray(A64) @ np.asarray(X, dtype=np.float64), b, c)
    if loss == LOGISTIC:
        return lg.nll_terms(A64, X, b)
    r = np.asarray(A64) @ np.asarray(X, dtype=np.float64) - np.asarray(b, dtype=np.float64)[:, None]
    return 0.5 * r * r


def gradient(loss, A64, X, b, W, c=None):
    """A^T (W * psi(A X, b)) with W the m x k weights of the columns."""
    return np.asarray(A64).T @ (W * psi(loss, np.asarray(A64) @ np.asarray(X, dtype=np.float64), b, c))


def data_term(loss, A64, X, b, W, c=None):
    return (W * loss_terms(loss, A64, X, b, c)).sum(axis=0)


def loss_tolerance(loss, A64, X, b, W, c=None):
    """The bound of an fp32 loss sum against fp64 on the same fp32 X, per column, from the existing checks: tests/_link
    .loss_tolerance (Huber, hinge), tests/_weighted.wnll_tolerance (logistic), and for the squared loss half the ||r||^2 bound of
    tests/_data.fp32_pass_tolerances_cols on the rows scaled by sqrt(W) plus the 4 eps32 l of forming r^2 / 2 in fp32, as
    tests/_link.loss_tolerance counts it.  Every column has weights of its own."""
    k = X.shape[1]
    out = np.zeros(k)
    for j in range(k):
        wj, Xj = W[:, j], X[:, j:j + 1]
        if loss in (HUBER, HINGE):
            out[j] = lk.loss_tolerance(loss, A64, Xj, b, c, wj)[0]
        elif loss == LOGISTIC:
            out[j] = wt.wnll_tolerance(A64, Xj, wj)[0]
        else:
            sw = np.sqrt(wj)
            ref = data_term(loss, A64, Xj, b, wj[:, None])
            _, rr = _data.fp32_pass_tolerances_cols(sw[:, None] * A64, Xj, sw * b, np.zeros_like(Xj), 2.0 * ref)
            out[j] = 0.5 * rr[0] + 4.0 * float(np.finfo(F32).eps) * ref[0]
    return out


def gradient_tolerance(A64, X, b, W, G_ref):
    """psi is 1-Lipschitz in z for all four losses: the residual bound of the squared pass on the rows scaled by sqrt(W), as
    tests/test_gpu_link.py judges its gradient.  Per column."""
    k = X.shape[1]
    out = np.zeros(k)
    for j in range(k):
        sw = np.sqrt(W[:, j])
        out[j] = _data.fp32_pass_tolerances_cols(sw[:, None] * A64, X[:, j:j + 1], sw * np.abs(b), G_ref[:, j:j + 1], np.ones(1))[0][0]
    return out


def gram_tolerance(A64, X, W, G_ref):
    """tests/test_gpu_weighted.test_gram_apply's bound, per column."""
    k = X.shape[1]
    out = np.zeros(k)
    for j in range(k):
        As = np.sqrt(W[:, j])[:, None] * A64
        Xj = X[:, j:j + 1]
        out[j] = _data.fp32_pass_tolerances_cols(As, Xj, None, G_ref[:, j:j + 1], ((As @ Xj) ** 2).sum(axis=0))[0][0]
    return out


# ---- the link per element, in numpy fp32 ------------------------------------------------------------------------------------------
def link32(loss, Z, b, w, C, oob, c):
    """The kernel's per-element expressions in numpy fp32, in its order: (R, l) of the in-bag form - the weight first, the count
    second - or (None, l) of the out-of-bag form.  loss "gram": R = z."""
    Z = Z.astype(F32)
    bb = None if b is None else b.astype(F32)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        if loss == "gram":
            v, l = Z, np.zeros_like(Z)
        elif loss == SQUARED:
            r = Z - bb
            v, l = r, (F32(0.5) * r) * r
        elif loss == LOGISTIC:
            e = np.exp(-np.abs(Z))
            p = np.where(Z >= 0, F32(1) / (F32(1) + e), e / (F32(1) + e))
            v = p - bb
            l = (np.maximum(Z, F32(0)) - bb * Z) + np.log1p(e)
        elif loss == HUBER:
            r = Z - bb
            v = np.minimum(np.maximum(r, F32(-c)), F32(c))
            l = np.where(np.abs(r) <= F32(c), (F32(0.5) * r) * r, F32(c) * np.abs(r) - (F32(0.5) * F32(c)) * F32(c))
        else:
            u = np.maximum(F32(0), F32(1) - bb * Z)
            v, l = -bb * u, (F32(0.5) * u) * u
        assert v.dtype == F32 and l.dtype == F32
        if w is not None:
            v, l = v * w.astype(F32)[:, None], l * w.astype(F32)[:, None]
        if oob:
            return None, np.where(C == 0, l, F32(0)).astype(F32)
        cf = C.astype(F32)
        return (v * cf).astype(F32), (l * cf).astype(F32)


# ---- stability selection end to end ---------------------------------------------------------------------------------------------
ST_SHAPE, ST_SUPPORT, ST_NOISE, ST_PAIRS, ST_ITERS = (1003, 68), 6, 0.5, 16, 200
ST_FRACTIONS = (0.3, 0.1, 0.03, 0.01)
ST_NEAR, ST_LEFT_OUT = 1e-5, 0.005


@functools.lru_cache(maxsize=None)
def stability_case():
    """A (fp32 values), b = A xt + 0.5 noise with a planted support of 6, the four weights as fractions of alpha_max of the whole
    data, lambda_max(A^T A) of the whole A (valid for every subsample) and the 32 complementary subsamples of seed 0."""
    from fastoptsolver_amd import resample as rs
    m, n = ST_SHAPE
    rng = np.random.default_rng(2024)
    A64 = rng.standard_normal((m, n)).astype(F32).astype(np.float64)
    support = np.sort(rng.choice(n, ST_SUPPORT, replace=False))
    xt = np.zeros(n)
    xt[support] = rng.choice([-1.0, 1.0], ST_SUPPORT) * rng.uniform(1.0, 2.0, ST_SUPPORT)
    b = (A64 @ xt + ST_NOISE * rng.standard_normal(m)).astype(F32).astype(np.float64)
    amax = float(np.abs(A64.T @ b).max())
    alphas = tuple((f * amax, 0.0) for f in ST_FRACTIONS)
    L = lk.lipschitz(A64, 5)
    C = rs.subsample_counts(m, 2 * ST_PAIRS, 0.5, seed=0)
    for a in (A64, b, C):
        a.setflags(write=False)
    return dict(A=A64, b=b, support=support, alphas=alphas, L=L, counts=C)


@functools.lru_cache(maxsize=None)
def stability_reference():
    """(nonzero - B x L x n bool, the fp64 reference fits' selections -, near - the cells whose prox input lies within 1e-5
    (relative to the larger of ||u||_inf and tau alpha1) of the threshold tau alpha1: fp32 rounding may decide them either way)."""
    d = stability_case()
    B, La, n = d["counts"].shape[1], len(d["alphas"]), d["A"].shape[1]
    nonzero, near = np.zeros((B, La, n), dtype=bool), np.zeros((B, La, n), dtype=bool)
    for r in range(B):
        w = d["counts"][:, r].astype(np.float64)
        for a, (a1, a2) in enumerate(d["alphas"]):
            x, _, u, tau = run(SQUARED, d["A"], d["b"], w, a1, a2, d["L"], ST_ITERS, want_u=True)
            thr = tau * a1
            nonzero[r, a] = x != 0
            near[r, a] = np.abs(np.abs(u) - thr) <= ST_NEAR * max(float(np.abs(u).max()), thr)
    return nonzero, near


# ---- controlled runs ------------------------------------------------------------------------------------------------------------
CONTROL_MENU = (dict(adaptive_restart=True, restart_threshold=1.0, tol_ratio=0.1), dict(adaptive_restart=True, restart_threshold=0.9, tol_ratio=0.2),
                dict(adaptive_restart=True, restart_threshold=1.0, tol_ratio=0.3))
CONTROL_ITERS = 60


@functools.lru_cache(maxsize=None)
def controlled_case(loss, kind):
    """(control, counts - m x B 0/1 -, the (resample, weight) cells kept, their reference (x, iterations)) of the controlled check
    on 1003 x 68, as tests/test_gpu_link._controlled chooses it: the first entry of CONTROL_MENU under which at least three of the
    nine cells (three subsamples x three weights) have fp32-proof restart and stop decisions on the reference
    (tests/_coord.fp32_proof), some stopping early and not all at the same iteration.  Decided on the reference alone; L is that of
    the whole A, valid for 0/1 counts."""
    from tests import _coord as cd
    m, n = SHAPES["edges"]
    A64, b, c, L, alphas = recipe(loss, kind, m, n)
    C = counts("binary", m, 3, seed=4)
    for ctl in CONTROL_MENU:
        keep, refs = [], []
        for r in range(3):
            for a, (a1, a2) in enumerate(alphas):
                tr = {}
                x, k = run(loss, A64, b, C[:, r].astype(np.float64), a1, a2, L / divisor(loss), CONTROL_ITERS, c=c, trace=tr, **ctl)
                if cd.fp32_proof(tr, ctl["restart_threshold"], ctl["tol_ratio"]):
                    keep.append((r, a))
                    refs.append((x, k))
        ks = [k for _, k in refs]
        if len(keep) >= 3 and min(ks) < CONTROL_ITERS and len(set(ks)) >= 2:
            return ctl, C, tuple(keep), tuple(refs)
    raise AssertionError("no entry of CONTROL_MENU gives three controlled runs with fp32-proof decisions")
