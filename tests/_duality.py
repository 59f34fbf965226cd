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

from tests import _coord as cd, _forms, _link as lk, _logit as lg, _working_set as wk

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


def _round(loss, A, b, a1, a2, L, iters, x0, c=None, w=None, p=None):
    """`iters` FISTA iterations of the loss's reference problem from x0 (t = 1, y = x0: what fos_fista_reset makes of an x0)."""
    if loss not in (HUBER, HINGE):
        return wk.inner(A, b, a1, a2, L, iters, p=p, loss=loss, w=w, x0=x0)
    assert p is None                     # (tests/_link.CoordLinkProblem carries the factors on the lasso penalty only)
    prob = lk.LinkProblem(loss, A, b, a1, a2, c, w)
    st = prob.init_state(L)
    st.x, st.x_old, st.y = x0.copy(), x0.copy(), x0.copy()
    for _ in range(iters):
        prob.step(st)
    return st.x


def certified(loss, A, b, alphas, gap_tol, iters, *, c=None, w=None, p=None, L=None, max_rounds=20, grow=2.0, max_fraction=0.5):
    """The loop of fastoptsolver_amd.duality._certified_group for ONE group of up to 16 weights, restated in fp64 on the building
    blocks of tests/_working_set.solve: the certificate at 0, the first set from the scan with slack 0 plus the unpenalised
    coordinates, rounds of `iters` iterations warm-started on the set, one certificate per round, the stop gap_j <= gap_tol P_j(0)
    for every column, working_set_path's growth rule, a round without a violator on the same set again, and the three ways to
    fall back (an empty set, a set beyond max_fraction * n, max_rounds rounds).  L: None takes every sub-problem's own exact
    constant.  A sub-problem of the device is padded with zero columns of factor 1, which its step t / (L + alpha2 max p) sees:
    with factors, so does the round here.

    (X n x nv, info): rounds, sizes, certificates, fell_back, certified, primal, dual, gap, scale, mag_gap of the last certificate,
    and what every decision had to spare - stop_margins (|gap_j - bound_j| / mag_gap_j per column at every test of the stop rule),
    scan_margins (the distance of the closest excess value outside the set from 1 at every scan) and growth_gaps (the last excess
    value the growth step takes minus the first it leaves), as tests/_handle_pairs.WorkingSet records them."""
    A = np.asarray(A, dtype=np.float64)
    n, nv = A.shape[1], len(alphas)
    assert nv <= 16
    a1s = [a1 for a1, _ in alphas]
    pf = np.ones(n) if p is None else np.asarray(p, dtype=np.float64)
    X = np.zeros((n, nv))
    stop_margins, scan_margins, growth_gaps = [], [], []

    def certify():
        G = gradient(loss, A, X, b, c, w).T
        return certificate(loss, A, b, X, alphas, c, w, p, G=G), G.astype(np.float32)

    def scan(G32, in_ws, want=None):
        excess, viol = wk.scan(G32, a1s, 0.0, in_ws, pf)
        out = np.asarray(in_ws) == 0
        e = np.asarray(excess, dtype=np.float64)[out]
        scan_margins.append(float(np.abs(e - 1.0).min()) if out.any() else np.inf)
        top = np.sort(e[e > 0])[::-1]
        if want is not None and 0 < viol.size < want < top.size:      # the growth step takes the `want` largest
            growth_gaps.append(float(top[want - 1] - top[want]))
        return excess, viol

    def met(cert):
        stop_margins.append(np.abs(cert["gap"] - bound) / cert["mag_gap"])
        return bool((cert["gap"] <= bound).all())

    cert, G32 = certify()
    certificates = 1
    bound = gap_tol * cert["primal"]
    free = (pf == 0).astype(np.uint8)
    _, viol = scan(G32, free)
    mask = free.copy()
    mask[viol] = 1
    limit = max_fraction * n
    sizes, fell_back, idx = [], False, None
    while not met(cert):
        if idx is None:
            idx = np.nonzero(mask)[0]
        if idx.size == 0 or idx.size > limit or len(sizes) == max_rounds:
            fell_back = True
            break
        sizes.append(int(idx.size))
        A_ws, p_ws = A[:, idx], None
        if p is not None:
            p_ws = pf[idx]
            if idx.size < max(wk.MIN_COLUMNS, -(-idx.size // wk.PAD_COLUMNS) * wk.PAD_COLUMNS):       # a padding column: zero, factor 1
                A_ws, p_ws = np.concatenate([A_ws, np.zeros((A.shape[0], 1))], axis=1), np.concatenate([p_ws, [1.0]])
        L_ws = lipschitz(loss, A_ws, w) if L is None else L
        for j, (a1, a2) in enumerate(alphas):
            x0 = np.zeros(A_ws.shape[1])
            x0[:idx.size] = X[idx, j]
            X[idx, j] = _round(loss, A_ws, b, a1, a2, L_ws, iters, x0, c, w, p_ws)[:idx.size]
        cert, G32 = certify()
        certificates += 1
        want = int((grow - 1.0) * idx.size)
        excess, viol = scan(G32, mask, want)
        if viol.size == 0:               # the zeros are right and the gap is not there yet: the same set again
            continue
        mask[viol] = 1
        if viol.size < want:
            order = np.argsort(-excess.astype(np.float64), kind="stable")[:want]
            mask[order[excess[order] > 0]] = 1
        idx = None
    if fell_back:
        Lf = lipschitz(loss, A, w) if L is None else L
        for j, (a1, a2) in enumerate(alphas):
            X[:, j] = _round(loss, A, b, a1, a2, Lf, iters, X[:, j].copy(), c, w, p)
        cert, _ = certify()
        certificates += 1
        met(cert)                        # GapInfo.certified of a group that fell back: the stop rule once more, per column
    info = dict(rounds=len(sizes), sizes=sizes, certificates=certificates, fell_back=fell_back, certified=cert["gap"] <= bound,
                bound=bound, stop_margins=np.array(stop_margins), scan_margins=np.array(scan_margins), growth_gaps=np.array(growth_gaps))
    info.update({k: cert[k] for k in ("primal", "dual", "gap", "scale", "mag_gap")})
    return X, info


PATH_LOSS = {"squared_weighted": SQUARED, "huber": HUBER, "hinge_weighted": HINGE, "logistic_factors": LOGISTIC}


@functools.lru_cache(maxsize=None)
def path_case(name, kind="f32", seed=11, corr=0.0, fractions=wk.FRACTIONS):
    """A case of the certified path on tests/_working_set.case's recipe (300 x 256, a planted support of 8, 16 weights from
    fractions[0] to fractions[1] of alpha_max, every other one an elastic net): dict(loss, A, b, c, w, p, alphas, L - of the full
    data term).  squared_weighted: integer row weights 1 .. 3.  huber: a tenth of the rows of b shifted by 1, the threshold the
    median of |b|.  hinge_weighted: the signs of b as labels, the same row weights.  logistic_factors: the recipe's penalty factors
    with its two unpenalised coordinates at factor 1 (an unpenalised coordinate with a gradient makes every scale 0)."""
    loss = PATH_LOSS[name]
    cs = wk.case("logistic" if loss == LOGISTIC else "squared", name.endswith("weighted"), name.endswith("factors"), kind, seed=seed, corr=corr,
                 fractions=fractions)
    A, b, w, p, c = cs["A"], cs["b"], cs["w"], cs["p"], None
    if loss == HUBER:
        rng = np.random.default_rng(4300 + seed)
        b = b.copy()
        b[rng.choice(len(b), size=len(b) // 10, replace=False)] += 1.0
        b = b.astype(np.float32).astype(np.float64)
        c = float(np.float32(np.median(np.abs(b))))
    elif loss == HINGE:
        b = np.where(b >= 0.0, 1.0, -1.0)
    if p is not None:
        p = np.where(p == 0.0, 1.0, p)
    g0 = np.abs(gradient(loss, A, np.zeros((A.shape[1], 1)), b, c, w)[:, 0])
    amax = float((g0 / (1.0 if p is None else p)).max())
    a1 = amax * np.geomspace(fractions[0], fractions[1], wk.WEIGHTS)
    alphas = tuple((float(a), float(a) / 10.0 if i % 2 else 0.0) for i, a in enumerate(a1))
    out = dict(loss=loss, A=A, b=b, c=c, w=w, p=p, alphas=alphas, L=lipschitz(loss, A, w))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def certified_case(cs, gap_tol, iters=PATH_ITERS, alphas=None, **loop):
    """tests/_duality.certified on a path_case with the case's own L."""
    return certified(cs["loss"], cs["A"], cs["b"], list(cs["alphas"] if alphas is None else alphas), gap_tol, iters, c=cs["c"], w=cs["w"], p=cs["p"],
                     L=cs["L"], **loop)


# The cases of certified_path that tests/test_gpu_duality.py compares with `certified`: name -> (path_case arguments, gap_tol,
# iterations per round, max_fraction, the number of weights).  Seed, weights and gap_tol were chosen on the reference alone, by the
# rule tests/test_duality_reference.py asserts: every test of the stop rule lies further than STOP_MARGIN of the magnitude of the
# gap's terms from its bound, every scan and growth decision further than SCAN_MARGIN / GROWTH_GAP from its threshold.
#
# A column that has converged has a gap of 0, so its last test has gap_tol P(0) / mag_gap to spare, and mag_gap is about twice P*
# there.  With the recipe's weights (0.9 .. 0.35 of alpha_max) P* is nearly P(0): 5e-5 to spare at GAP_TOL and 5e-4 at 1e-3, for
# every seed - under STOP_MARGIN both.  GAP_TOL was tried first, with the weights 0.9 .. 0.35, 0.3 .. 0.05, 0.1 .. 0.02 and
# 0.03 .. 0.005 of alpha_max and the seeds 11, 12 and 13: no case has a combination that meets the margins (it takes weights below a
# hundredth of alpha_max, where every column is in the first set).  At 1e-3 the strongest of these ladders that does is 0.1 .. 0.02
# (0.03 .. 0.005 for the logistic loss, whose P* falls more slowly), with the first seed of 11, 12, 13 that meets every margin.
# At such weights most of the 256 columns are in the set: 232 to 246 in the first round.
STOP_MARGIN, SCAN_MARGIN, GROWTH_GAP = 100.0 * TOL, 1e-3, 1e-4           # (the last two: the WorkingSet cell's of tests/_handle_pairs.py)
CERTIFIED_TOL = 1e-3
CERTIFIED_ITERS = 100                    # a round: a fifth of PATH_ITERS, which is enough for these cases and keeps their tests quick
CERTIFIED_CASES = {
    "squared_weighted": (("squared_weighted", "f32", 11, 0.0, (0.1, 0.02)), CERTIFIED_TOL, CERTIFIED_ITERS, 1.0, 16),
    "huber": (("huber", "f32", 11, 0.0, (0.1, 0.02)), CERTIFIED_TOL, CERTIFIED_ITERS, 1.0, 16),
    "hinge_weighted": (("hinge_weighted", "f32", 13, 0.0, (0.1, 0.02)), CERTIFIED_TOL, CERTIFIED_ITERS, 1.0, 16),
    # 200 iterations a round and seed 12: at 100 the gap is met in a third round whose test has 2.2e-4 to spare, at 200 seed 11 has 3.0e-5
    "logistic_factors": (("logistic_factors", "f32", 12, 0.0, (0.03, 0.005)), CERTIFIED_TOL, 2 * CERTIFIED_ITERS, 1.0, 16),
    "huber_bf16": (("huber", "bf16", 11, 0.0, (0.1, 0.02)), CERTIFIED_TOL, CERTIFIED_ITERS, 1.0, 16),
    # the first set (237 columns) is within max_fraction * 256 = 243.2 and the grown one (all 256) is not: one round, then the
    # full lockstep - three certificates
    "beyond_max_fraction": (("huber", "f32", 11, 0.0, (0.1, 0.02)), CERTIFIED_TOL, CERTIFIED_ITERS, 0.95, 16),
    # 20 iterations a round: the first round ends with no violator and the gap not met, and the same 249 columns run again
    "same_set_again": (("squared_weighted", "f32", 11, 0.0, (0.03, 0.005)), CERTIFIED_TOL, 20, 1.0, 16),
    # 20 weights - the 16 of the case and its weights 4 .. 7 again - go as a group of 16 and a group of 4 (on their own the first
    # four put an excess value 3.8e-4 from the threshold of the first scan: under SCAN_MARGIN)
    "twenty_weights": (("squared_weighted", "f32", 11, 0.0, (0.1, 0.02)), CERTIFIED_TOL, CERTIFIED_ITERS, 1.0, 20),
}


def certified_weights(name):
    cs = path_case(*CERTIFIED_CASES[name][0])
    count = CERTIFIED_CASES[name][4]
    return (list(cs["alphas"]) + list(cs["alphas"][4:]))[:count]


@functools.lru_cache(maxsize=None)
def certified_reference(name):
    """[(X, info) per group of up to 16 weights] of a case of CERTIFIED_CASES, computed once."""
    args, gap_tol, iters, max_fraction, count = CERTIFIED_CASES[name]
    cs, weights = path_case(*args), certified_weights(name)
    return [certified_case(cs, gap_tol, iters, weights[first:first + 16], max_rounds=PATH_ROUNDS, max_fraction=max_fraction)
            for first in range(0, count, 16)]
