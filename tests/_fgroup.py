"""The fp64 reference of the lockstep with feature groups (group lasso / sparse-group lasso over groups of coordinates of one
fit) and the seeded group layouts and cases its tests share (a helper: no tests in here).

    data term + alpha1 [ (1 - mu) sum_g w_g ||x_g||_2 + mu ||x||_1 ] + 0.5 alpha2 ||x||_2^2

The reference is the oracle's FistaProblem, tests/_logit.LogisticProblem or tests/_weighted's problems with ONE method replaced:
prox (soft threshold at step a1 mu, then the block soft threshold of every group at step a1 (1 - mu) w_g).  gradient and
init_state stay the base class's own, and momentum, restarts and stops the oracle's step / step_delta.  enet=True is the PROX_ENET
form of the update kernels - no ridge term in the gradient, the prox divides by 1 + step a2, tau = t / L - which is the base class
built with a2 = 0 and the prox's own a2 kept aside, so that gradient and init_state are still untouched.
The oracle has no group penalty: tests/test_fgroup_reference.py checks this restatement against the KKT conditions."""
import functools
import math

import numpy as np

from oracle import fos_oracle as orc
from tests import _coord as cd, _data, _forms, _logit as lg, _weighted as wt

ITERS, TOL = lg.ITERS, lg.TOL
MUS = (0.0, 0.5, 1.0)
CLOSE = 1e-4                     # a group whose ||u_g|| / thr lies this close to 1 may fall on either side on the device


# ---- layouts ---------------------------------------------------------------------------------------------------------------
def _small(total, rng):
    """Seeded sizes 1..7 summing to `total`."""
    sizes = []
    while total > 0:
        s = int(min(total, rng.integers(1, 8)))
        sizes.append(s)
        total -= s
    return sizes


def layout(name, n, seed=0):
    """(start, weight or None) of a named layout on n coordinates.
    ones: all groups of size 1.  small: seeded sizes 1..7 (boundaries inside quads).  cross64: one group covering columns 60..69,
    across the first 64-column block boundary, between groups of 4 and 8.  span150 (n >= 200): one group of 150 columns,
    44..193 - it starts inside the first update workgroup, covers the next two and ends in the partial last one of n = 200 -
    beside small groups.  single: one group of n.  weights: seeded sizes 1..7 with weights 0.5..2 times sqrt(size), every
    sixth group and the first with weight 0 (outside the group term)."""
    rng = np.random.default_rng(4000 + seed)
    w = None
    if name == "ones":
        sizes = [1] * n
    elif name == "small":
        sizes = _small(n, rng)
    elif name == "cross64":
        assert n >= 72
        sizes = [4] * 15 + [10] + [8] * ((n - 70) // 8) + ([(n - 70) % 8] if (n - 70) % 8 else [])
    elif name == "span150":
        assert n >= 200
        sizes = _small(44, rng) + [150] + _small(n - 194, rng)
    elif name == "single":
        sizes = [n]
    elif name == "weights":
        sizes = _small(n, rng)
        w = rng.uniform(0.5, 2.0, size=len(sizes)) * np.sqrt(sizes)
        w[::6] = 0.0
        w = np.asarray(w, dtype=np.float32).astype(np.float64)           # as the device stores them
    else:
        raise KeyError(name)
    start = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    assert start[-1] == n and (np.diff(start) > 0).all()
    return start, w


def weights_of(start, w):
    """The group weights in fp64 as the device holds them: the given ones, or sqrt(size) computed in fp32."""
    if w is not None:
        return np.asarray(w, dtype=np.float64)
    return np.sqrt(np.diff(start).astype(np.float32)).astype(np.float64)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def group_prox(v, step, a1, mu, start, w, enet_a2=None):
    """The exact prox of step * (a1 [(1 - mu) sum_g w_g ||x_g|| + mu ||x||_1] (+ 0.5 enet_a2 ||x||^2)) at v; also returns the
    norms ||u_g|| and the thresholds (for the structure checks)."""
    u = orc.prox_l1(v, step * a1 * mu) if a1 > 0 else v
    sizes = np.diff(start)
    nrm = np.sqrt(np.add.reduceat(u * u, start[:-1]))
    thr = step * a1 * (1.0 - mu) * w
    if a1 * (1.0 - mu) != 0.0:                       # mu = 1 (and a1 = 0): no group step - the oracle's own lasso prox
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.where(nrm <= thr, 0.0, 1.0 - thr / nrm)
        s = np.repeat(scale, sizes)
        u = np.where(s == 0.0, 0.0, s * u)
    if enet_a2 is not None:
        u = u / (1.0 + step * enet_a2)
    return u, nrm, thr


def _fgroup_class(base):
    class FGroup(base):
        start = gw = None
        mu = 0.0
        enet_a2 = None
        closest = math.inf           # min over iterations and groups with thr > 0 of | ||u_g|| / thr - 1 |

        def bind(self, start, w, mu, enet_a2=None):
            self.start, self.gw, self.mu, self.enet_a2 = np.asarray(start), weights_of(start, w), float(mu), enet_a2
            return self

        def prox(self, v, step):
            x, nrm, thr = group_prox(v, step, self.a1, self.mu, self.start, self.gw, self.enet_a2)
            if self.a1 * (1.0 - self.mu) != 0.0 and (thr > 0).any():
                self.closest = min(self.closest, float(np.min(np.abs(nrm[thr > 0] / thr[thr > 0] - 1.0))))
            return x

    return FGroup


FGroupFista = _fgroup_class(orc.FistaProblem)
FGroupLogistic = _fgroup_class(lg.LogisticProblem)
FGroupWeightedLogistic = _fgroup_class(wt.WeightedLogisticProblem)


def problem(A, b, alpha1, alpha2, start, gw=None, mu=0.0, *, loss="squared", w=None, enet=False):
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    a2 = 0.0 if enet else alpha2                     # PROX_ENET: the ridge term lives in the prox alone
    if loss == "squared":
        if w is not None:                            # 0.5 ||sqrt(w) (A x - b)||^2: the unmodified data term on scaled rows
            sw = np.sqrt(np.asarray(w, dtype=np.float64))
            A, b = sw[:, None] * A, sw * b
        prob = FGroupFista(A, b, alpha1, a2)
    elif w is None:
        prob = FGroupLogistic(A, b, alpha1, a2)
    else:
        prob = FGroupWeightedLogistic(A, b, w, alpha1, a2)
    return prob.bind(start, gw, mu, alpha2 if enet else None)


def run(A, b, alpha1, alpha2, L, max_iter=ITERS, *, start, gw=None, mu=0.0, loss="squared", w=None, enet=False, delta=None,
        t_init_factor=1.0, tol_ratio=0.0, adaptive_restart=False, restart_threshold=1.0):
    """dict(x, k, restarts, stopped, ratios, moves, closest, prob) of FISTA (FISTA-delta with `delta`) from x0 = 0, as
    tests/_coord.run reports them; L: the constant of the data term."""
    prob = problem(A, b, alpha1, alpha2, start, gw, mu, loss=loss, w=w, enet=enet)
    st = prob.init_state(L, t_init_factor)
    restarts, ratios, moves = 0, [], []
    for _ in range(max_iter):
        if delta is None:
            info = prob.step(st, tol_ratio=tol_ratio, adaptive_restart=adaptive_restart, restart_threshold=restart_threshold)
            restarts += int(adaptive_restart and info["ratio"] > restart_threshold)
        else:
            info = prob.step_delta(st, delta, tol_ratio=tol_ratio)
        ratios.append(info["ratio"])
        moves.append(info["move"])
        if st.stopped:
            break
    return dict(x=st.x, k=st.k, restarts=restarts, stopped=cd.STOP_RATIO if st.stopped else cd.STOP_NONE, ratios=ratios, moves=moves,
                closest=prob.closest, prob=prob)


def smooth_gradient(prob, x, alpha2):
    """The gradient of data term + 0.5 alpha2 ||x||^2 at x, whichever prox form the problem was built for."""
    g = prob.gradient(x)
    return g + alpha2 * x if prob.enet_a2 is not None else g


def kkt_violation(prob, x, alpha1, alpha2):
    """The largest violation of the group KKT conditions at x, relative to alpha1.  With g the smooth gradient:
      active group:    -g_j = alpha1 (1 - mu) w_g x_j / ||x_g|| + alpha1 mu sign(x_j) where x_j != 0, and where x_j = 0 inside an
                       active group |g_j| <= alpha1 mu (the group term is differentiable there and contributes 0)
      inactive group:  || S(g_g, alpha1 mu) ||_2 <= alpha1 (1 - mu) w_g."""
    g = smooth_gradient(prob, np.asarray(x, dtype=np.float64), alpha2)
    mu, worst = prob.mu, 0.0
    for k in range(len(prob.start) - 1):
        sl = slice(prob.start[k], prob.start[k + 1])
        xg, gg, wg = x[sl], g[sl], prob.gw[k]
        nrm = float(np.linalg.norm(xg))
        if nrm > 0:
            nz = xg != 0
            r = gg[nz] + alpha1 * (1.0 - mu) * wg * xg[nz] / nrm + alpha1 * mu * np.sign(xg[nz])
            worst = max(worst, float(np.max(np.abs(r))))
            if (~nz).any():
                worst = max(worst, float(np.max(np.maximum(np.abs(gg[~nz]) - alpha1 * mu, 0.0))))
        else:
            worst = max(worst, max(float(np.linalg.norm(orc.prox_l1(gg, alpha1 * mu))) - alpha1 * (1.0 - mu) * wg, 0.0))
    return worst / alpha1


def alpha_max(g0, start, w, mu):
    """The smallest alpha1 at which x = 0 solves the problem whose smooth gradient at 0 is -g0: every group with a threshold
    has ||S(g0_g, alpha1 mu)||_2 <= alpha1 (1 - mu) w_g (mu = 0: max_g ||g0_g|| / w_g; mu = 1: max |g0|).  Groups with w_g = 0
    are unpenalised at mu = 0 and never leave the model: they are left out.  Bisection on the monotone condition."""
    held = [(slice(start[k], start[k + 1]), w[k]) for k in range(len(start) - 1) if mu > 0 or w[k] > 0]

    def zero(a):
        return all(np.linalg.norm(orc.prox_l1(g0[sl], a * mu)) <= a * (1.0 - mu) * wg for sl, wg in held)
    hi = float(np.max(np.abs(g0))) / mu if mu > 0 else max(float(np.linalg.norm(g0[sl])) / wg for sl, wg in held)
    lo = 0.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if zero(mid) else (mid, hi)
    return hi


def zero_groups(x, start):
    """(entirely zero, entirely non-zero) per group."""
    nz = np.add.reduceat((np.asarray(x) != 0).astype(np.int64), start[:-1])
    return nz == 0, nz == np.diff(start)


# ---- cases -----------------------------------------------------------------------------------------------------------------
FRACTIONS = ((0.5, 0.0), (0.2, 0.5), (0.08, 0.0), (0.3, 0.1))     # of the group alpha_max: without and with the ridge term


def _build(kind, loss, m, n, seed, weighted, lay, mu):
    A, b_sq, xt = _data.synth(m, n, seed)
    A32 = A.astype(np.float32)
    A64 = _forms.bf16_round_np(A32).astype(np.float64) if kind == "bf16" else A32.astype(np.float64)
    b = lg.labels(A, xt, seed) if loss == "logistic" else b_sq.astype(np.float32).astype(np.float64)
    w = wt.as_stored(wt.weights("spread" if seed % 2 else "counts", m, seed)) if weighted else None
    ones = np.ones(m) if w is None else w
    L = wt.lipschitz(A64, ones, seed, loss)
    start, gw = layout(lay, n, seed)
    g0 = A64.T @ (ones * ((b - 0.5) if loss == "logistic" else b))
    amax = alpha_max(g0, start, weights_of(start, gw), mu)
    alphas = tuple((f * amax, a2) for f, a2 in FRACTIONS)
    return dict(A=A64, b=b, w=w, L=L, start=start, gw=gw, mu=mu, amax=amax, alphas=alphas, seed=seed)


def _refs(c, loss, **kw):
    return [run(c["A"], c["b"], a1, a2, c["L"], start=c["start"], gw=c["gw"], mu=c["mu"], loss=loss, w=c["w"], **kw)
            for a1, a2 in c["alphas"]]


def meaningful(c, loss, lay):
    """What a case must show on the reference alone: at every weight the solution has zero groups and non-zero groups (a single
    group: it is non-zero), no group of any iteration lies within CLOSE of its threshold, and under an entry of
    tests/_coord.CONTROL_MENU the controlled FISTA run of one weight at least takes fp32-proof decisions."""
    if not any(cd.fp32_proof(r, ctl["restart_threshold"], ctl["tol_ratio"]) for ctl in cd.CONTROL_MENU for r in _refs(c, loss, **ctl)):
        return False
    for enet in (False, True):
        for r in _refs(c, loss, enet=enet):
            zero, full = zero_groups(r["x"], c["start"])
            held = weights_of(c["start"], c["gw"]) > 0 if c["mu"] == 0 else np.ones(len(zero), bool)
            if lay == "single":
                if zero.all():
                    return False
            elif c["mu"] < 1 and not ((zero & held).any() and (~zero).any()):
                return False
            elif c["mu"] == 1 and not ((r["x"] == 0).any() and (r["x"] != 0).any()):
                return False
            if r["closest"] < CLOSE:
                return False
    return True


@functools.lru_cache(maxsize=None)
def case(kind, loss, m, n, base_seed, weighted, lay, mu):
    """The data of one case, computed once and never modified: the first of the seeds base_seed, base_seed + 1, ... (eight
    tried) whose reference is `meaningful` - decided on the reference alone."""
    for seed in range(base_seed, base_seed + 8):
        c = _build(kind, loss, m, n, seed, weighted, lay, mu)
        if meaningful(c, loss, lay):
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            return c
    raise AssertionError(f"no seed from {base_seed} gives {kind} {loss} {m} x {n} {lay} mu={mu} a meaningful reference")


@functools.lru_cache(maxsize=None)
def reference(kind, loss, m, n, base_seed, weighted, lay, mu, a1, a2, iters=ITERS, enet=False, delta=None, control=False, rows=None):
    """run() on a case; control: False or an index into tests/_coord.CONTROL_MENU as a string; rows: a boolean mask as bytes (the
    training rows of a fold) or None."""
    c = case(kind, loss, m, n, base_seed, weighted, lay, mu)
    A, b, w = c["A"], c["b"], c["w"]
    if rows is not None:
        keep = np.frombuffer(rows, dtype=bool)
        A, b, w = A[keep], b[keep], (None if w is None else w[keep])
    kw = {} if control is False else cd.CONTROL_MENU[int(control)]
    if delta is not None:
        kw = {k: v for k, v in kw.items() if k == "tol_ratio"}       # FISTA-delta has no momentum restart
    ref = run(A, b, a1, a2, c["L"], iters, start=c["start"], gw=c["gw"], mu=mu, loss=loss, w=w, enet=enet, delta=delta, **kw)
    ref["x"].setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def controlled(kind, loss, m, n, base_seed, weighted, lay, mu, enet=False, delta=None):
    """(index into CONTROL_MENU as a string, penalty pairs) of a controlled cell: the first menu entry under which the
    reference's restart and stop decisions are fp32-proof (tests/_coord.fp32_proof) at one pair at least, and those pairs.
    (None, ()) where no entry gives one: the cell has no controlled case, which tests/test_fgroup_reference.py bounds."""
    c = case(kind, loss, m, n, base_seed, weighted, lay, mu)
    for i, ctl in enumerate(cd.CONTROL_MENU):
        keep = []
        for a1, a2 in c["alphas"]:
            r = reference(kind, loss, m, n, base_seed, weighted, lay, mu, a1, a2, enet=enet, delta=delta, control=str(i))
            if cd.fp32_proof(r, None if delta is not None else ctl["restart_threshold"], ctl["tol_ratio"]):
                keep.append((a1, a2))
        if keep:
            return str(i), tuple(keep)
    return None, ()


# ---- what the GPU tests run: (shape name, layout) where the layout bites -----------------------------------------------------
BITES = (("one_tile", "ones"), ("one_tile", "small"), ("one_tile", "single"),
         ("edges", "small"), ("edges", "cross64"), ("edges", "span150"), ("edges", "single"), ("edges", "weights"),
         ("whole_wgs", "ones"), ("whole_wgs", "cross64"), ("whole_wgs", "weights"),
         ("panels", "small"), ("panels", "weights"))
KINDS = ("f32", "bf16")
CPU_CUS = 256                    # the CU count the CPU checks assume for the shapes that depend on it (the MI355X's)


def key(kind, cus, name, lay, mu, loss="squared", weighted=False):
    from tests import _menu_coord as mc
    s = mc.shapes(kind, cus)[name]
    return (kind, loss, s["m"], s["n"], 3 * s["m"] + s["n"], weighted, lay, mu)
