"""The fp64 reference of the lockstep with per-coordinate penalty factors and box bounds, and the seeded recipes its tests share
(a helper: no tests in here).

    data term + alpha1 sum_j p_j |x_j| + 0.5 alpha2 sum_j p_j x_j^2   subject to   lo_j <= x_j <= hi_j

The reference is the oracle's FistaProblem, tests/_logit.LogisticProblem or tests/_weighted's problems with THREE methods replaced:
gradient (ridge term a2 p * y), prox (per-coordinate threshold tau a1 p_j, then the clip to the box: the exact 1-D prox of penalty
plus box, the penalty being convex with its minimum at 0 inside the box) and init_state (tau = t / (L + a2 max p)).  Momentum,
restarts and stops stay the oracle's own step / step_delta.  enet=True is the PROX_ENET form of the update kernel: no ridge
term in the gradient, the prox divides by 1 + tau a2 p_j, tau = t / L.

The bounds' scale comes from the unbounded fit of the same case, so that they bind at every shape: coefficient magnitudes differ by
orders between the shapes the tests use."""
import functools
import math

import numpy as np

from oracle import fos_oracle as orc
from tests import _data, _forms, _logit as lg, _weighted as wt

STOP_NONE, STOP_RATIO = 0, 2
CONTROL = dict(adaptive_restart=True, restart_threshold=0.9, tol_ratio=0.2)


def as_stored(v):
    """A vector as the device keeps it (fp32), in fp64; infinities stay infinite."""
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def _coord_class(base):
    class Coord(base):
        p = lo = hi = None
        enet = False

        def bind(self, p, lo, hi, enet=False):
            n = self.A.shape[1]
            self.p = np.ones(n) if p is None else np.asarray(p, dtype=np.float64)
            self.lo = np.full(n, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
            self.hi = np.full(n, np.inf) if hi is None else np.asarray(hi, dtype=np.float64)
            self.enet = enet
            return self

        def gradient(self, y):
            a2, self.a2 = self.a2, 0.0
            try:
                g = super().gradient(y)                  # the data term of the base class, untouched
            finally:
                self.a2 = a2
            return g + (a2 * self.p) * y if (a2 > 0 and not self.enet) else g

        def prox(self, v, step):
            x = orc.prox_l1(v, step * self.a1 * self.p) if self.a1 > 0 else v
            if self.enet:
                x = x / (1.0 + step * self.a2 * self.p)
            return np.clip(x, self.lo, self.hi)

        def init_state(self, L, t_init_factor=1.0):
            n = self.A.shape[1]
            if self.a2 > 0 and not self.enet:
                L = L + self.a2 * float(self.p.max())
            z = np.zeros(n)
            return orc.FistaState(x=z.copy(), x_old=z.copy(), y=z.copy(), t=1.0, tau=t_init_factor / L)

    return Coord


CoordFista = _coord_class(orc.FistaProblem)
CoordLogistic = _coord_class(lg.LogisticProblem)
CoordWeightedLogistic = _coord_class(wt.WeightedLogisticProblem)


def problem(A, b, alpha1, alpha2, p=None, lo=None, hi=None, *, loss="squared", w=None, enet=False):
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if loss == "squared":
        if w is not None:                                # 0.5 ||sqrt(w) (A x - b)||^2: the unmodified data term on scaled rows
            sw = np.sqrt(np.asarray(w, dtype=np.float64))
            A, b = sw[:, None] * A, sw * b
        prob = CoordFista(A, b, alpha1, alpha2)
    elif w is None:
        prob = CoordLogistic(A, b, alpha1, alpha2)
    else:
        prob = CoordWeightedLogistic(A, b, w, alpha1, alpha2)
    return prob.bind(p, lo, hi, enet)


def run(A, b, alpha1, alpha2, L, max_iter=lg.ITERS, *, p=None, lo=None, hi=None, loss="squared", w=None, enet=False, delta=None,
        t_init_factor=1.0, tol_ratio=0.0, adaptive_restart=False, restart_threshold=1.0):
    """dict(x, k, restarts, stopped, ratios, moves) of FISTA (FISTA-delta with `delta`) from x0 = 0; L: the constant of the data term.
    restarts counts as the device does (the first iteration's infinite ratio included); ratios: this / prev of every iteration."""
    prob = problem(A, b, alpha1, alpha2, p, lo, hi, loss=loss, w=w, enet=enet)
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
    return dict(x=st.x, k=st.k, restarts=restarts, stopped=STOP_RATIO if st.stopped else STOP_NONE, ratios=ratios, moves=moves, prob=prob)


def factors(n, seed):
    """Penalty factors as the device stores them: log-uniform over two decades, about 10 % exact zeros, coordinate 0 among
    them."""
    rng = np.random.default_rng(9000 + seed)
    p = 10.0 ** rng.uniform(-1.0, 1.0, size=n)
    p[rng.random(n) < 0.1] = 0.0
    p[0] = 0.0
    return as_stored(p)


SCALES = (0.25, 0.1, 0.04, 0.016, 0.0064)       # the two-sided bound as a fraction of the unbounded fit's scale (see case)


def bounds(x_unc, seed, frac=SCALES[0]):
    """(lo, hi) as the device stores them, from the fit `x_unc` of the same case with the same factors and without bounds: a
    block with lo = 0, a block with hi = 0, a block of two-sided bounds -s / +s, the rest free.  The coordinates x_unc has
    largest on either side are dealt to the blocks they violate - the most negative to lo = 0, the most positive to hi = 0, the
    next two of either sign to the two-sided block - and s is `frac` of the smallest of their magnitudes and the median nonzero
    magnitude of x_unc, so that the bounds bind at every shape."""
    x_unc = np.asarray(x_unc, dtype=np.float64)
    n = x_unc.shape[0]
    rng = np.random.default_rng(9500 + seed)
    block = rng.integers(0, 5, size=n)                   # 0: lo = 0, 1: hi = 0, 2: two-sided, 3 and 4: free
    order = np.argsort(x_unc)
    neg, pos = order[x_unc[order] < 0.0], order[::-1][x_unc[order[::-1]] > 0.0]
    assert len(neg) >= 2 and len(pos) >= 2, "the unbounded fit needs two coordinates on either side"
    block[neg[0]], block[pos[0]] = 0, 1                  # on the wrong side of a sign constraint
    block[neg[1:3]], block[pos[1:3]] = 2, 2              # beyond the two-sided bounds on either side (two each where there are)
    nz = np.abs(x_unc[x_unc != 0.0])
    s = frac * min(float(np.median(nz)), float(np.abs(x_unc[neg[1:3]]).min()), float(x_unc[pos[1:3]].min()))
    lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
    lo[block == 0] = 0.0
    hi[block == 1] = 0.0
    lo[block == 2], hi[block == 2] = -s, s
    return as_stored(lo), as_stored(hi)


def kkt_violation(prob, x):
    """The largest violation of the optimality conditions of the stated objective at x, over the coordinates: with g the gradient
    of the smooth part (data term + 0.5 a2 sum p_j x_j^2) and s = a1 p_j,
      interior, nonzero:   g_j + s sign(x_j) = 0
      interior, zero:      |g_j| <= s
      at a bound:          the sign condition (at lo_j the subgradient may only push down, at hi_j only up; a bound at 0 keeps
                           the subdifferential [-s, s] of the penalty)."""
    x = np.asarray(x, dtype=np.float64)
    assert (x >= prob.lo).all() and (x <= prob.hi).all()
    enet, prob.enet = prob.enet, False
    try:
        g = prob.gradient(x)
    finally:
        prob.enet = enet
    s = prob.a1 * prob.p
    at_lo, at_hi = x == prob.lo, x == prob.hi
    lo_sub = np.where(x != 0.0, g + s * np.sign(x), g - s)          # the smallest element of g + s d|x|
    hi_sub = np.where(x != 0.0, g + s * np.sign(x), g + s)          # the largest
    # 0 must lie in [lo_sub, hi_sub] + normal cone: (-inf, 0] at a lower bound, [0, inf) at an upper bound
    viol_low = np.where(at_lo, 0.0, np.maximum(lo_sub, 0.0))        # lo_sub > 0 is curable only by the cone of a lower bound
    viol_high = np.where(at_hi, 0.0, np.maximum(-hi_sub, 0.0))
    return float(np.max(np.maximum(viol_low, viol_high)))


def preconditions(ref, x_unc, p, lo, hi):
    """What a case must show on the reference alone for its GPU test to mean something: counts of coordinates exactly at a
    nonzero lower / upper bound, of sign-constrained coordinates the unconstrained fit has on the wrong side, and of nonzero
    unpenalised coordinates."""
    x = ref["x"]
    return dict(at_lower=int(np.sum((x == lo) & (lo < 0))), at_upper=int(np.sum((x == hi) & (hi > 0))),
                wrong_side=int(np.sum(((lo == 0) & (x_unc < 0)) | ((hi == 0) & (x_unc > 0)))),
                unpenalised=int(np.sum((p == 0) & (x != 0))))


def decision_margin(ref, restart_threshold=None, tol_ratio=0.0):
    """The smallest distance of a finite step ratio from a threshold it is compared with (fp32-proof decisions)."""
    r = [v for v in ref["ratios"] if math.isfinite(v)]
    d = [abs(v - restart_threshold) for v in r] if restart_threshold is not None else []
    d += [abs(v - tol_ratio) for v in r] if tol_ratio > 0 else []
    return min(d) if d else math.inf


@functools.lru_cache(maxsize=None)
def case(kind, loss, m, n, seed, weighted=False):
    """The data of one case, computed once and never modified: dict(A (fp64, as the device stores it), b (target or labels),
    w (stored weights or None), L (of the data term), alphas (three penalty pairs), p, x_unc (the oracle's fit at the first
    pair with the factors and without bounds), lo, hi, frac).  The two-sided bound is the first entry of SCALES at which the
    reference, at EVERY one of the three pairs, ends with a coordinate exactly at a nonzero lower bound and one exactly at a
    nonzero upper bound: decided on the reference alone, so that the at-bound checks of the GPU tests are never vacuous."""
    A, b_sq, xt = _data.synth(m, n, seed)
    A32 = A.astype(np.float32)
    A64 = _forms.bf16_round_np(A32).astype(np.float64) if kind == "bf16" else A32.astype(np.float64)
    b = lg.labels(A, xt, seed) if loss == "logistic" else b_sq.astype(np.float32).astype(np.float64)
    w = wt.as_stored(wt.weights("spread" if seed % 2 else "counts", m, seed)) if weighted else None
    ones = np.ones(m) if w is None else w
    L = wt.lipschitz(A64, ones, seed, loss)
    alphas = tuple(wt.alphas(A64, b, ones, loss))
    a1, a2 = alphas[0]                               # the strongest penalty: weaker ones push further past the bounds
    p = factors(n, seed)
    x_unc = run(A64, b, a1, a2, L, p=p, loss=loss, w=w)["x"]
    for frac in SCALES:
        lo, hi = bounds(x_unc, seed, frac)
        fits = [run(A64, b, q1, q2, L, p=p, lo=lo, hi=hi, loss=loss, w=w)["x"] for q1, q2 in alphas]
        if all(((x == lo) & (lo < 0)).any() and ((x == hi) & (hi > 0)).any() for x in fits):
            break
    else:
        raise AssertionError("no entry of SCALES makes both sides of the two-sided bounds bind at every penalty pair")
    out = dict(A=A64, b=b, w=w, L=L, alphas=alphas, x_unc=x_unc, p=p, lo=lo, hi=hi, frac=frac)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(kind, loss, m, n, seed, weighted, a1, a2, iters=lg.ITERS, enet=False, delta=None, control=False, rows=None):
    """run() on a case with its recipe; control: False, True (CONTROL) or an index into CONTROL_MENU as a string (the
    cache must not take 0 for False); rows: a boolean mask as
    bytes (the training rows of a fold) or None."""
    c = case(kind, loss, m, n, seed, weighted)
    A, b, w = c["A"], c["b"], c["w"]
    if rows is not None:
        keep = np.frombuffer(rows, dtype=bool)
        A, b, w = A[keep], b[keep], (None if w is None else w[keep])
    ref = run(A, b, a1, a2, c["L"], iters, p=c["p"], lo=c["lo"], hi=c["hi"], loss=loss, w=w, enet=enet, delta=delta,
              **({} if control is False else CONTROL if control is True else CONTROL_MENU[int(control)]))
    ref["x"].setflags(write=False)
    return ref


MARGIN = 1e-3                            # the "fp32-proof decisions" rule of tests/test_fista_forms.py
EPS32 = float(np.finfo(np.float32).eps)


def fp32_proof(ref, restart_threshold=None, tol_ratio=0.0):
    """Whether the device must take every restart and stop decision of a controlled run as the reference does.  The device's
    iterate carries fp32 rounding (y is handed to product 1 in fp32, the gradient is an fp32 sum): a step is known to about
    eps32 times the iterate's norm, so the ratio of two steps, the smaller of which is `move`, to about 2 eps32 ||x|| / move.
    Every ratio must be further than that, and further than MARGIN, from each threshold it is compared with.  A run that has
    converged to the rounding level decides on noise, on the device and nowhere else: it is no case of a controlled check."""
    scale = float(np.linalg.norm(ref["x"]))
    prev = math.inf
    for ratio, move in zip(ref["ratios"], ref["moves"]):
        if math.isfinite(ratio):
            need = max(MARGIN, 2.0 * EPS32 * scale / max(min(move, prev), 1e-300))
            if restart_threshold is not None and abs(ratio - restart_threshold) < need:
                return False
            if tol_ratio > 0 and abs(ratio - tol_ratio) < need:
                return False
        prev = move
    return scale > 0


def genuine_restarts(ref, restart_threshold):
    """Restarts a controlled run decided on a finite ratio (the first iteration's ratio is infinite and always restarts)."""
    return sum(1 for r in ref["ratios"] if math.isfinite(r) and r > restart_threshold)


CONTROL_MENU = (CONTROL, dict(CONTROL, tol_ratio=0.5))      # the second stops early, while the steps are still large


def controlled(kind, loss, m, n, seed, weighted=False):
    """(control parameters, penalty pairs) of the controlled cells of a case: the first entry of CONTROL_MENU under which the
    controlled runs (both prox kinds) of at least two pairs are fp32_proof on the reference, and those pairs."""
    c = case(kind, loss, m, n, seed, weighted)
    for ctl in CONTROL_MENU:
        keep = []
        for a1, a2 in c["alphas"]:
            refs = [run(c["A"], c["b"], a1, a2, c["L"], p=c["p"], lo=c["lo"], hi=c["hi"], loss=loss, w=c["w"], enet=e, **ctl)
                    for e in (False, True)]
            if all(fp32_proof(r, ctl["restart_threshold"], ctl["tol_ratio"]) for r in refs):
                keep.append((a1, a2))
        if len(keep) >= 2:
            return ctl, keep
    raise AssertionError("no entry of CONTROL_MENU gives the case two controlled runs with fp32-proof decisions")
