"""Reference, error bounds, decision and case table of the Armijo trial layer (a helper: no tests in here), beside
tests/_power.py and tests/_coord.py.

fista(backtracking=True) accepts a step from seven numbers per candidate t_j = t eta^j:
    gd = grad.dlt, dd = ||dlt||^2, nnz = #(dlt != 0), gnorm2 = ||grad||^2, y2 = ||y||^2, q = ||A dlt||^2, rr_y = ||A y - b||^2.
fista_trial_kernel (csrc/reduce_update.hpp) and fista_trial_batch_kernel / fista_trial_batch_bf16_kernel (csrc/batch_trial.hpp)
form the first five, fold_partials_kernel folds their partials, one pass over A adds q, rr_y is what the gradient pass left.
tests/test_armijo_reference.py checks this file on the CPU, tests/test_gpu_armijo.py compares the kernels with it.

Reference.  `reference` restates the arithmetic the kernels document in np.longdouble, every sum rounded once (`fsum`):
    y = x_cur + beta (x_cur - x_prev);  gf = g + alpha2 y (PROX_L1 with alpha2 > 0 only);  v = y - t_j gf;
    xt = soft_threshold(v, t_j alpha1) when alpha1 > 0;  xt /= 1 + t_j alpha2 for PROX_ENET;  d = xt - y.
t_j is formed by repeated t *= eta in fp64, as the kernels and the host form it.  q_j = ||A f32(d_j)||^2 on the stored A: the
device rounds dlt to fp32 before the pass.

Bounds.  `bounds` is derived, not tuned.  With eps = eps64:
  |err d_i|  <= 8 eps (|y_i| + t |gf_i| + t alpha1) =: ed_i   the chain y, gf, t gf, v, t alpha1, |v| - thr, the shrink, xt - y
                                                              has at most eight roundings, with or without fma contraction
  |err y_i|  <= 3 eps (|x_cur_i| + |beta (x_cur_i - x_prev_i)|) =: ey_i             (difference, product, sum)
  |err gf_i| <= 2 eps |gf_i| + alpha2 ey_i =: eg_i                                  (product and sum; the fp32 g is exact in fp64)
  term of gd      gf_i d_i :  |gf_i| ed_i + |d_i| eg_i + eg_i ed_i + eps |gf_i d_i|
  term of dd      d_i^2    :  2 |d_i| ed_i + ed_i^2 + eps d_i^2
  term of gnorm2  gf_i^2   :  2 |gf_i| eg_i + eg_i^2 + eps gf_i^2
  term of y2      y_i^2    :  2 |y_i| ey_i + ey_i^2 + eps y_i^2
plus (n + 16) eps sum |term| for a summation of n terms in any order (partials per thread, wave, workgroup, fold).  The
reference's own error is the same expressions with the longdouble eps and half an ulp for the final sum: it has to stay below
1/16 of the bound (checked on the CPU against exact rational arithmetic).  q takes _data.fp32_pass_tolerances_cols, as
tests/test_gpu_kernel_menu_multi.py takes it for trial_batch.

Decision.  `decide` restates the three clauses of iterative_solvers._armijo_accepts / armijo_decide_kernel over the rows of one
batch and names the first true clause of the accepted candidate - nnz, excess, ball, in that order - or "stall".

Exact inputs.  `exact_inputs`: x (= y: a fresh handle has beta = 0), g, t, eta, alpha1, alpha2 are small dyadic rationals, so
every y, gf, v, threshold comparison and (without the elastic-net shrink) d is exact in fp64 and nnz is an integer known in
advance for every candidate.  Planted classes, EXACT_K coordinates each (h = EXACT_H is the grid step):
  tie        y = 0, |gf| = alpha1                 |v| == thr for every candidate: d = 0, not counted
  above      y = 0, |gf| = alpha1 + h             one step above: d = -+ t_j h, counted; 2^-20 of the largest entries of d
  below      y = 0, |gf| = alpha1 - h             one step below: d = 0, not counted
  zero_in    y = 0, |gf| <= alpha1 / 2            d = 0, not counted
  live_in    y = t_7 u (0 < |u| < alpha1), gf = u |v| <= thr up to candidate 7 at least: d = -y there, counted at every candidate
  tie_at     y = t_J (gf -+ alpha1), J = 3        |v| == thr at candidate J alone, y != 0: counted
  g_zero     g = 0, y != 0                        counted when alpha1 > 0 (d = -t_j alpha1 sign y or -y) or gf != 0
  back       y != 0, gf = -sign(y) alpha1         the step lands back on y: d = 0 while |v| > thr, not counted (alpha1 > 0, L1)
The rest is generic: y and gf on coarse grids, |gf| at least a quarter away from alpha1."""
import fractions
import functools
import math

import numpy as np

from tests import _data, _power

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
EPSLD = float(np.finfo(LD).eps)
NV = 16
ARMIJO_C = 1e-2                                      # iterative_solvers.C
GRAD_EPS = {"f32": 8.0 * EPS32, "f64": 64.0 * EPS64}   # gradient source -> grad_eps (iterative_solvers._armijo_accepts)
SUMS = ("gd", "dd", "gnorm2", "y2")
FIELDS = ("gd", "dd", "nnz", "gnorm2", "y2", "q", "rr_y")


def seed(*key):
    return _power.seed("armijo", *key)


# ---- the arithmetic ------------------------------------------------------------------------------------------------------
def fsum(terms):
    """The sum of longdouble terms to longdouble rounding, whatever cancels: every term splits into two doubles without error,
    math.fsum gives the correctly rounded double s of their exact sum, and a second one the remainder (exact sum - s)."""
    terms = np.asarray(terms, dtype=LD).ravel()
    hi = terms.astype(np.float64)
    parts = np.concatenate([hi, (terms - hi.astype(LD)).astype(np.float64)])
    s = math.fsum(parts)
    return LD(s) + LD(math.fsum(np.append(parts, -s)))


def soft_threshold(v, thr):
    """sign(v) max(|v| - thr, 0) in the type of its arguments (prox_operators.py:3-8)."""
    mag = np.abs(v) - thr
    return np.sign(v) * np.where(mag > 0, mag, 0)


def prox(v, t, prm):
    """The prox of one candidate in the type of v: soft threshold when alpha1 > 0, the elastic-net shrink behind it."""
    one = v.dtype.type(1)
    t, a1, a2 = v.dtype.type(t), v.dtype.type(prm["alpha1"]), v.dtype.type(prm["alpha2"])
    xt = soft_threshold(v, t * a1) if prm["alpha1"] > 0 else v
    return xt / (one + t * a2) if prm["prox"] == "enet" else xt


def smooth_a2(prm):
    """alpha2 where it belongs to the smooth part (PROX_L1): the a2s of the decision."""
    return float(prm["alpha2"]) if (prm["prox"] == "l1" and prm["alpha2"] > 0) else 0.0


def steps(t, eta, nv):
    out, t = [], float(t)
    for _ in range(nv):
        out.append(t)
        t *= float(eta)
    return out


def point(x_cur, x_prev, beta, g, prm):
    """(y, gf) in longdouble."""
    xc, xp, g = (np.asarray(a, dtype=np.float64).astype(LD) for a in (x_cur, x_prev, g))
    y = xc + LD(beta) * (xc - xp)
    gf = g + LD(prm["alpha2"]) * y if smooth_a2(prm) > 0 else g
    return y, gf


def reference(A64, x_cur, x_prev, beta, g, prm, t, eta, nv):
    """The seven quantities for t_j, j < nv: dict(rows = [dict(gd, dd, nnz, gnorm2, y2, q)], t = [t_j], y, gf, d = [d_j] in
    longdouble, D32 = the candidates as the pass sees them (n x nv, fp64 values of the fp32 roundings)).  A64 None: no q."""
    y, gf = point(x_cur, x_prev, beta, g, prm)
    gnorm2, y2 = fsum(gf * gf), fsum(y * y)
    ts = steps(t, eta, nv)
    ds = [prox(y - LD(tj) * gf, tj, prm) - y for tj in ts]
    D32 = np.stack([d.astype(np.float64).astype(np.float32) for d in ds], axis=1).astype(np.float64)
    q = ((np.asarray(A64, dtype=np.float64) @ D32) ** 2).sum(axis=0) if A64 is not None else np.full(nv, np.nan)
    rows = [dict(gd=fsum(gf * d), dd=fsum(d * d), nnz=int(np.count_nonzero(d)), gnorm2=gnorm2, y2=y2, q=float(q[j]))
            for j, d in enumerate(ds)]
    return dict(rows=rows, t=ts, y=y, gf=gf, d=ds, D32=D32)


def _term_bounds(ref, j, x_cur, x_prev, beta, prm, eps):
    """(per-term error, |term|) of the four sums of candidate j for a chain carried at `eps`, as the module docstring derives."""
    y, gf, d = np.abs(ref["y"]), np.abs(ref["gf"]), np.abs(ref["d"][j])
    xc, xp = (np.asarray(a, dtype=np.float64).astype(LD) for a in (x_cur, x_prev))
    t, a1, a2, e = LD(ref["t"][j]), LD(prm["alpha1"]), LD(prm["alpha2"]), LD(eps)
    ed = 8 * e * (y + t * gf + t * a1)
    ey = 3 * e * (np.abs(xc) + np.abs(LD(beta) * (xc - xp)))
    eg = 2 * e * gf + (a2 * ey if smooth_a2(prm) > 0 else 0)
    return dict(gd=(gf * ed + d * eg + eg * ed + e * gf * d, gf * d), dd=(2 * d * ed + ed * ed + e * d * d, d * d),
                gnorm2=(2 * gf * eg + eg * eg + e * gf * gf, gf * gf), y2=(2 * y * ey + ey * ey + e * y * y, y * y))


def bounds(ref, x_cur, x_prev, beta, prm):
    """[dict(gd, dd, gnorm2, y2)]: the error bound of every sum of every candidate of `ref` for a kernel that carries the
    chain in fp64 and sums in any order."""
    n = len(ref["y"])
    out = []
    for j in range(len(ref["t"])):
        tb = _term_bounds(ref, j, x_cur, x_prev, beta, prm, EPS64)
        out.append({k: float(np.sum(err) + (n + 16) * EPS64 * np.sum(mag)) for k, (err, mag) in tb.items()})
    return out


def reference_error(ref, x_cur, x_prev, beta, prm):
    """The same bound for the reference itself: the chain in longdouble, the sum exactly rounded."""
    out = []
    for j in range(len(ref["t"])):
        tb = _term_bounds(ref, j, x_cur, x_prev, beta, prm, EPSLD)
        out.append({k: float(np.sum(err) + EPSLD * np.sum(mag)) for k, (err, mag) in tb.items()})
    return out


def q_bounds(A64, ref):
    """The bound of q_j = ||A dlt_j||^2 of one fp32 pass, per candidate."""
    nv = ref["D32"].shape[1]
    q_ref = np.array([r["q"] for r in ref["rows"]])
    return _data.fp32_pass_tolerances_cols(A64, ref["D32"], None, np.zeros((ref["D32"].shape[0], nv)), q_ref)[1]


def exact_sums(x_cur, x_prev, beta, g, prm, t, eta, nv):
    """gd, dd, gnorm2, y2 and nnz of every candidate in rational arithmetic (small n only): what `reference` is checked against."""
    F = fractions.Fraction
    xc, xp, g = ([F(float(v)) for v in a] for a in (x_cur, x_prev, g))
    a1, a2, b = F(float(prm["alpha1"])), F(float(prm["alpha2"])), F(float(beta))
    y = [c + b * (c - p) for c, p in zip(xc, xp)]
    gf = [gi + a2 * yi for gi, yi in zip(g, y)] if smooth_a2(prm) > 0 else g
    out = []
    for tj in steps(t, eta, nv):
        tj = F(tj)
        d = []
        for yi, gi in zip(y, gf):
            v = yi - tj * gi
            xt = v
            if a1 > 0:
                mag = max(abs(v) - tj * a1, F(0))
                xt = mag if v > 0 else -mag
            if prm["prox"] == "enet":
                xt = xt / (1 + tj * a2)
            d.append(xt - yi)
        out.append(dict(gd=sum(gi * di for gi, di in zip(gf, d)), dd=sum(di * di for di in d), nnz=sum(di != 0 for di in d),
                        gnorm2=sum(gi * gi for gi in gf), y2=sum(yi * yi for yi in y)))
    return out


# ---- the decision --------------------------------------------------------------------------------------------------------
def clauses(tr, t, a2s, C, grad_eps):
    """dict(nnz, excess, ball): the three clauses of one candidate."""
    excess = (1.0 - C) * tr["gd"] + 0.5 * tr["q"] + 0.5 * a2s * tr["dd"]
    g_y = 0.5 * tr["rr_y"] + 0.5 * a2s * tr["y2"]
    noise = max(EPS64 * g_y, grad_eps * math.sqrt(tr["gnorm2"] * tr["dd"]))
    return dict(nnz=tr["nnz"] == 0, excess=excess <= noise, ball=tr["dd"] <= (grad_eps * t) ** 2 * tr["gnorm2"])


def clause_of(tr, t, a2s, C, grad_eps):
    """The first true clause of one candidate (nnz, excess, ball), or None."""
    return next((k for k, v in clauses(tr, t, a2s, C, grad_eps).items() if v), None)


def decide(rows, t, eta, a2s, C, grad_eps):
    """(j, t_j, clause) of the first accepted row, or (None, t eta^len(rows), "stall")."""
    t = float(t)
    for j, tr in enumerate(rows):
        clause = clause_of(tr, t, a2s, C, grad_eps)
        if clause is not None:
            return j, t, clause
        t *= float(eta)
    return None, t, "stall"


# The noise-ball case of the device decision, from x = 0 (y = 0, d_i = -t sign(g_i) max(|g_i| - alpha1, 0)): alpha1 a few ulps of
# the gradient's type below max |g|, so that one coordinate i moves, by t delta with delta <= 8 ulp <= grad_eps ||g||: inside the
# ball at every t.  excess = 0.5 ||a_i||^2 t^2 delta^2 - (1 - C) t |g_i| delta exceeds the noise grad_eps ||g|| t delta once
# t >> 2 |g_i| / (||a_i||^2 delta), about 3e5 (fp32 ulps) or 3e13 (fp64 ulps) for ||a_i||^2 of a few tens: tau = 2^34 / L, 2^64 / L.
BALL_ULPS = {"f32": 3, "f64": 8}


def ball_alpha1(g, source):
    top = np.max(np.abs(np.asarray(g, dtype=np.float64)))
    top = np.float32(top) if source == "f32" else np.float64(top)
    for _ in range(BALL_ULPS[source]):
        top = np.nextafter(top, top.dtype.type(0))
    return float(top)


def ball_tau(L, source):
    return (2.0 ** 34 if source == "f32" else 2.0 ** 64) / L


# ---- the cases -----------------------------------------------------------------------------------------------------------
# route: what plan() has to say.  batch: trial_batch / run_backtracking are served (path 0 and not the row-per-thread plan).
def _c(name, dtype, m, n, layout, route, batch, **kw):
    c = dict(name=name, dtype=dtype, m=m, n=n, layout=layout, route=route, batch=batch)
    c.update(kw)
    return c


_STREAM = dict(path=0, tall=0, colblock=0, resident=0)
SHAPES = {c["name"]: c for c in [
    _c("pad", "f32", 37, 68, "strided", dict(path=0, tall=1, colblock=0, resident=0), True, n_pad=128),  # 60 zero-filled columns
    _c("one_wg", "f32", 130, 256, "strided", _STREAM, True, n_pad=256),                  # no padding, one workgroup
    _c("two_wg", "f32", 37, 260, "strided", _STREAM, True, n_pad=320),                   # second workgroup: 4 live columns
    _c("bf_pad", "bf16", 37, 72, "strided", dict(path=0, tall=1, colblock=0, resident=0), True, n_pad=128),
    _c("bf_two", "bf16", 130, 264, "strided", _STREAM, True, n_pad=384),
    # y-in-LDS plan; trial: 66 partial rows (the fold's second lane trip); trial_batch: n_pad > 64 x 256 (second column trip)
    _c("wide", "f32", 8, 16644, "strided", dict(_STREAM, threads=512, chunks=16, rows=1), True, n_pad=16704),
    # column-block plan; trial: 257 > 256 workgroups (the stride loop's second trip)
    _c("blocks", "f32", 3, 65540, "strided", dict(path=0, colblock=1, resident=0), True, n_pad=65600),
    _c("tall", "f32", 3000, 7, "compact", dict(path=0, tall=1, colblock=0, resident=0), False),
    _c("resident", "f32", 20, 5, "compact", dict(path=0, resident=1), False),
    _c("two_pass", "f32", 513, 1023, "ragged", dict(path=1, resident=0), False),
]}
CELL_SHAPES = ("pad", "two_wg", "bf_pad", "wide")              # the full parameter grid
DECISION_SHAPES = ("pad", "two_wg", "bf_pad")
EIGHT_SHAPES = ("two_wg", "bf_two")
PROX = {                                                        # name -> (prox kind, alpha1 on, alpha2)
    "l1": ("l1", True, 0.0), "l1_ridge": ("l1", True, 0.25), "enet": ("enet", True, 0.25), "no_l1": ("l1", False, 0.25)}
STATES = ("fresh", "three")
SOURCES = ("f32", "f64")
NVS = (1, 5, 16)
ETAS = (0.5, 0.7)
NEAR = 1e-6                                                     # no coordinate this close (relative) to the threshold
# ... and this many times as far in the fp64 rehearsal of `params` (the fp32 pass moves |gf| / alpha1 by a few 1e-7)
REHEARSED = 8.0


def cells():
    """[(shape, prox, state, source)]: the grid on CELL_SHAPES, one representative cell on every other shape.  (`blocks` from
    the fresh state: three iterations leave 50000 live coordinates, and a million (coordinate, candidate) pairs do not all stay
    8e-6 away from their thresholds whatever alpha1 is.)"""
    out = [(s, p, st, src) for s in CELL_SHAPES for p in PROX for st in STATES for src in SOURCES]
    rep = {"one_wg": ("enet", "three", "f32"), "bf_two": ("l1_ridge", "three", "f64"), "blocks": ("l1_ridge", "fresh", "f32"),
           "tall": ("l1_ridge", "three", "f32"), "resident": ("enet", "three", "f32"), "two_pass": ("l1_ridge", "three", "f32")}
    return out + [(s,) + rep[s] for s in SHAPES if s not in CELL_SHAPES]


def trial_grid(n):
    """Workgroups of fista_trial_kernel = partial rows of its fold (grid_1d(n, 256, 256))."""
    return max(1, min(256, (n + 255) // 256))


def batch_grid(n_pad):
    """Workgroups of the candidate kernels (grid_1d(n_pad, 256, 64))."""
    return max(1, min(64, (n_pad + 255) // 256))


@functools.lru_cache(maxsize=None)
def problem(shape):
    """(stored A in fp64, b in fp32, x0 in fp64, L = ||A||_2^2) of a shape, seeded; computed once and shared (read-only).
    x0 is sparse - min(n / 2, 64) entries of magnitude 1..2 - so that with t = ||y|| / ||g|| the live coordinates have
    |v| >> thr and the others, y = 0, have |v| / thr = |gf| / alpha1 at every candidate: `params` keeps those away from 1."""
    c = SHAPES[shape]
    rng = np.random.default_rng(seed(shape))
    A64 = _power.round_to(rng.standard_normal((c["m"], c["n"])), c["dtype"])
    b = rng.standard_normal(c["m"]).astype(np.float32)
    x0 = np.zeros(c["n"])
    live = rng.choice(c["n"], size=max(1, min(c["n"] // 2, 64)), replace=False)
    x0[live] = rng.choice([-1.0, 1.0], len(live)) * (1.0 + rng.random(len(live)))
    L = float(np.linalg.norm(A64, 2)) ** 2
    for a in (A64, b, x0):
        a.setflags(write=False)
    return A64, b, x0, L


def fista_states(A64, b, x0, prm, tau, iters):
    """[(x_k, x_{k-1}, beta_k)] for k = 0..iters of plain FISTA at the fixed step tau, in fp64 (the oracle's loop: t_{k+1} =
    (1 + sqrt(1 + 4 t_k^2)) / 2, beta = (t_k - 1) / t_{k+1}): what `params` rehearses the three-iteration state of the GPU
    cells on.  The GPU tests track the device's own iterates instead."""
    b = np.asarray(b, dtype=np.float64)
    x_cur, x_prev, t_k, beta = np.array(x0, dtype=np.float64), np.array(x0, dtype=np.float64), 1.0, 0.0
    out = [(x_cur, x_prev, beta)]
    for _ in range(iters):
        y = x_cur + beta * (x_cur - x_prev)
        gf = A64.T @ (A64 @ y - b) + smooth_a2(prm) * y
        x_prev, x_cur = x_cur, prox(y - tau * gf, tau, prm)
        t_next = 0.5 * (1.0 + math.sqrt(1.0 + 4.0 * t_k * t_k))
        beta, t_k = (t_k - 1.0) / t_next, t_next
        out.append((x_cur, x_prev, beta))
    return out


def step_for(shape, prm):
    """The fixed step of the three iterations: 1 / (||A||_2^2 + alpha2)."""
    return 1.0 / (problem(shape)[3] + prm["alpha2"])


def states_of(shape, prox):
    """The states a (shape, prox) pair runs in."""
    return sorted({st for s, p, st, _ in cells() if (s, p) == (shape, prox)})


def _rehearsed_gap(shape, prox, prm):
    """The smallest | |v| - thr | / thr over the states of the pair, both eta and all 16 candidates, on the fp64 gradient."""
    A64, b, x0, _ = problem(shape)
    b64, gap = b.astype(np.float64), np.inf
    states = fista_states(A64, b, x0, prm, step_for(shape, prm), 3)
    for x_cur, x_prev, beta in [states[0 if st == "fresh" else 3] for st in states_of(shape, prox)]:
        y = x_cur + beta * (x_cur - x_prev)
        g = A64.T @ (A64 @ y - b64)
        gf = g + smooth_a2(prm) * y
        t = float(np.linalg.norm(y) / np.linalg.norm(g))
        for eta in ETAS:
            for tj in steps(t, eta, NV):
                thr = tj * prm["alpha1"]
                gap = min(gap, float(np.min(np.abs(np.abs(y - tj * gf) - thr)) / thr))
    return gap


@functools.lru_cache(maxsize=None)
def _alpha1(shape, prox):
    A64, b, x0, _ = problem(shape)
    kind, _, a2 = PROX[prox]
    prm = dict(prox=kind, alpha1=0.0, alpha2=a2)
    gf = A64.T @ (A64 @ x0 - b.astype(np.float64)) + smooth_a2(prm) * x0
    s = np.sort(np.abs(gf))
    lo = max(1, len(s) // 10)
    hi = max(lo + 1, len(s) // 4)
    widest = lo + np.argsort(-np.diff(s[lo - 1: hi]))[:32]              # gap k lies between s[k - 1] and s[k]
    best = (-1.0, 0.0)
    for k in widest:
        a1 = float(0.5 * (s[k - 1] + s[k]))
        gap = _rehearsed_gap(shape, prox, dict(prm, alpha1=a1))
        if gap > REHEARSED * NEAR:
            return a1
        best = max(best, (gap, a1))
    return best[1]


def params(shape, prox):
    """dict(prox, alpha1, alpha2) of a cell.  alpha1 sits in the middle of one of the widest gaps between neighbours of the sorted
    |gf| at x0 between their first decile and quartile (small enough that three iterations leave coordinates on both sides): the first of them for which a rehearsal of
    the pair's states in fp64 keeps every coordinate of every candidate REHEARSED * NEAR away from its threshold."""
    kind, l1_on, a2 = PROX[prox]
    return dict(prox=kind, alpha1=_alpha1(shape, prox) if l1_on else 0.0, alpha2=a2)


def near_threshold(ref, prm):
    """Per candidate: (coordinates with |v| <= thr, with |v| > thr, the smallest | |v| - thr | / thr)."""
    out = []
    for tj in ref["t"]:
        v = np.abs(ref["y"] - LD(tj) * ref["gf"])
        thr = LD(tj) * LD(prm["alpha1"])
        out.append((int((v <= thr).sum()), int((v > thr).sum()), float(np.min(np.abs(v - thr)) / thr)))
    return out


# ---- exact inputs --------------------------------------------------------------------------------------------------------
EXACT_K = 3
EXACT_H = 2.0 ** -20
EXACT_T, EXACT_ETA, EXACT_A1, EXACT_A2 = 0.25, 0.5, 0.5, 0.125
EXACT_PROX = {"l1": dict(prox="l1", alpha1=EXACT_A1, alpha2=0.0), "l1_ridge": dict(prox="l1", alpha1=EXACT_A1, alpha2=EXACT_A2),
              "enet": dict(prox="enet", alpha1=EXACT_A1, alpha2=EXACT_A2)}
EXACT_CLASSES = ("tie", "above", "below", "zero_in", "live_in", "tie_at", "g_zero", "back")
EXACT_TIE_AT = 3


def exact_inputs(n, prox):
    """(x, g, prm, classes): x = x_cur = x_prev (so y = x), the gradient to inject (representable in fp32), the parameters, and
    {class: coordinates}.  Needs n >= 2 * len(EXACT_CLASSES) * EXACT_K."""
    prm = EXACT_PROX[prox]
    a1, a2s = prm["alpha1"], smooth_a2(prm)
    rng = np.random.default_rng(seed("exact", n, prox))
    # generic coordinates: y on a grid of 2^-6 in [-2, 2] (a third of them zero), |gf| in [0, 4] on a grid of 2^-6, at least a
    # quarter away from alpha1
    y = rng.integers(-128, 129, n) / 64.0 * (rng.random(n) < 2.0 / 3.0)
    mag = rng.integers(0, 257, n) / 64.0
    mag = np.where(np.abs(mag - a1) < 0.25, mag + 0.5, mag)
    gf = mag * rng.choice([-1.0, 1.0], n)
    slots = rng.permutation(n)[: len(EXACT_CLASSES) * EXACT_K].reshape(len(EXACT_CLASSES), EXACT_K)
    classes = {name: np.sort(slots[i]) for i, name in enumerate(EXACT_CLASSES)}
    sgn = np.array([1.0, -1.0, 1.0])[:EXACT_K]
    tJ, t7 = EXACT_T * EXACT_ETA ** EXACT_TIE_AT, EXACT_T * EXACT_ETA ** 7
    u = np.array([0.25, -0.125, 0.375])[:EXACT_K]
    for name, idx in classes.items():
        if name in ("tie", "above", "below"):
            y[idx] = 0.0
            gf[idx] = sgn * (a1 + {"tie": 0.0, "above": EXACT_H, "below": -EXACT_H}[name])
        elif name == "zero_in":
            y[idx] = 0.0
            gf[idx] = sgn * np.array([0.0, a1 / 2, a1 / 4])[:EXACT_K]
        elif name == "live_in":
            y[idx], gf[idx] = t7 * u, u
        elif name == "tie_at":
            gf[idx] = sgn * 2.0
            y[idx] = tJ * (gf[idx] - sgn * a1)               # v = y - t_J gf = -+ t_J alpha1
        elif name == "g_zero":
            y[idx] = sgn * np.array([1.0, 0.5, 2.0 ** -12])[:EXACT_K]
            gf[idx] = a2s * y[idx]                            # g = gf - a2s y = 0
        elif name == "back":
            y[idx] = sgn * np.array([1.5, 0.75, 0.25])[:EXACT_K]
            gf[idx] = -np.sign(y[idx]) * a1
    g = gf - a2s * y
    assert np.array_equal(g.astype(np.float32).astype(np.float64), g), "the injected gradient has to be representable in fp32"
    return y, g, prm, classes


def exact_counts(y, g, prm, nv=NV):
    """nnz of every candidate in fp64: exact on the exact inputs, where every quantity that decides d != 0 is."""
    gf = g + smooth_a2(prm) * y
    out = []
    for tj in steps(EXACT_T, EXACT_ETA, nv):
        v = y - tj * gf
        xt = soft_threshold(v, tj * prm["alpha1"])
        # the elastic-net shrink is not dyadic, but xt / (1 + t a2) == y holds for xt = y = 0 alone on these inputs
        # (tests/test_armijo_reference.py checks it in rational arithmetic)
        out.append(int(np.count_nonzero((xt != 0) | (y != 0)) if prm["prox"] == "enet" else np.count_nonzero(xt - y)))
    return out
