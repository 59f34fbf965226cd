"""Working-set solve of a sparse regularisation path (extension): the lockstep on the active columns of A.

A lasso, elastic-net or sparse logistic path at useful weights keeps a few percent of the coordinates non-zero, yet every lockstep
iteration of ``fista_path`` / ``logistic_path`` streams all n columns of A twice for all 16 weights.  ``working_set_path`` does
what glmnet, celer and skglm do: per group of up to 16 weights it

  1. solves on the columns that can be non-zero - an ordinary lockstep on a gathered matrix A_ws (fos_gather_columns),
  2. checks the optimality conditions of the FULL problem with one gradient over all columns (fos_gradient_batch, fos_kkt_scan),
  3. adds the violators and repeats.

The result is the minimiser of the full problem, certified by its KKT conditions: a coordinate outside the set is zero and stays
optimal there as long as |g_i| <= alpha1 p_i for every weight of the group.  Almost every iteration reads m x n_ws elements
instead of m x n.  When the set would grow beyond ``max_fraction`` of the columns, or ``max_rounds`` rounds leave violators, the
group is solved by the full lockstep, warm-started, and reported as fallen back: an uncertified answer is never returned silently.

Served: squared and logistic loss, sample weights, penalty factors (p_i = 0 keeps a coordinate in every set).  Not served
(ValueError before any device work): box bounds, feature groups, the group penalty, the multinomial loss, sharded problems.
The multinomial loss and the group penalty over the classes have names of their own: ``multinomial_ws.multinomial_working_set_path``.
"""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import _core
from . import iterative_solvers as _its
from . import multinomial as _mn

WorkingSetInfo = collections.namedtuple("WorkingSetInfo", "rounds sizes full_gradients worst_excess fell_back")
WorkingSetInfo.__doc__ = """What one group of up to 16 weights did: the rounds solved on a working set, the set's size in each, the
number of gradient passes over the full A (each reads A twice), the largest ``excess`` of the final check over the coordinates
outside the set (<= 1 + kkt_tol when certified) and whether the group fell back to the full lockstep."""

PAD_COLUMNS, MIN_COLUMNS = 64, 128      # the gathered matrix: columns rounded up to 64, at least 128


def _handle(A, b, dtype, who):
    """The handle of a call: a prepared one as it is (refused, before any device work, where the working set does not serve it),
    anything else bound here with the squared loss."""
    if not isinstance(A, _core.Problem):
        if b is None:
            raise ValueError(f"{who}: b is needed")
        return _core.Problem(A, b, dtype)
    if A.loss == "multinomial" or getattr(A, "grouped", False):
        raise ValueError(f"{who}: the multinomial loss and the group penalty are not served (squared and logistic loss)")
    if A.lower is not None or A.upper is not None:
        raise ValueError(f"{who}: box bounds are not served: a coordinate at a bound has another optimality condition")
    if A.has_feature_groups:
        raise ValueError(f"{who}: feature groups are not served: the group norm has another optimality condition")
    if getattr(A, "comm", None) is not None or getattr(A, "col_sharded", False):
        raise ValueError(f"{who}: sharded problems are not served")
    if A.b is None:
        raise ValueError(f"{who}: the handle was prepared without b")
    return A


def _family(prob, max_iter):
    """The lockstep family `fista_path` / `logistic_path` / `multinomial_path` give this kind of handle."""
    if prob.loss == "multinomial":
        return _mn._family(prob, max_iter)
    if prob.loss == "logistic":
        return _its._columns(max_iter, True, 4.0)
    if prob.loss in _core.LINK_LOSSES:           # `huber_path` / `hinge_path`: the squared loss's L, the lockstep alone
        return _its._columns(max_iter, True, 1.0)
    return _its._columns(max_iter, _its._weighted(prob) or _its._has_coord(prob))


def _sub_problem(prob, A_ws, p_ws):
    """The problem on the gathered columns: the handle's b (or labels and class count), loss (with the Huber threshold), row
    weights and kind of penalty, and the factors p_ws."""
    if prob.loss == "multinomial":
        sub = _core.Problem.multinomial(A_ws, prob.b, prob.classes, None, prob.sample_weight, p_ws)
        sub.set_grouped(prob.grouped)
        return sub
    if prob.loss in _core.LINK_LOSSES:
        sub = _core.Problem.link(A_ws, prob.b, prob.loss, prob.threshold, sample_weight=prob.sample_weight)
        if p_ws is not None:
            sub.set_penalty(p_ws)
        return sub
    return _core.Problem.penalized(A_ws, prob.b, p_ws, loss=prob.loss, sample_weight=prob.sample_weight)


def _factors(prob):
    """The penalty factors over the device columns (fp32, 1 on the padding), or None."""
    return None if prob._coord[0] is None else prob._coord[0][: prob.n_dev]


def _free(prob):
    """The mask of the unpenalised coordinates (factor 0): they are in every set."""
    pf = _factors(prob)
    return _mask(prob) if pf is None else (pf == 0).to(torch.uint8)


def _check_weights(prob, alphas):
    pf = _factors(prob)
    if any(a1 == 0.0 for a1, _ in alphas) and (pf is None or bool((pf > 0).any())):
        raise ValueError("alpha1 = 0 on a penalised coordinate: the working set would be every column - use fista_path / logistic_path")
    if any(not (np.isfinite(a1) and a1 >= 0.0) for a1, _ in alphas):
        raise ValueError("alpha1 must be finite and >= 0")


def _mask(prob, idx=None):
    mask = torch.zeros(prob.n_dev, dtype=torch.uint8, device=prob.device)
    if idx is not None:
        mask[idx] = 1
    return mask


def _block(prob, xs):
    """Solutions (a list of n-vectors or an n x k array / tensor) as an n_dev x k float64 device block."""
    if isinstance(xs, (list, tuple)):
        xs = torch.stack([torch.as_tensor(np.asarray(x) if not _core.is_tensor(x) else x).to(torch.float64).reshape(-1).cpu() for x in xs], dim=1)
    t = (xs.detach() if _core.is_tensor(xs) else torch.from_numpy(np.asarray(xs, dtype=np.float64))).to(torch.float64)
    if t.dim() == 1:
        t = t.reshape(-1, 1)
    if t.dim() != 2 or t.shape[0] != prob.n:
        raise ValueError(f"X: a vector of length {prob.n}, an {prob.n} x k block or a list of such vectors expected")
    out = torch.zeros(prob.n_dev, t.shape[1], dtype=torch.float64, device=prob.device)
    out[: prob.n] = t.to(prob.device)
    return out


def kkt_excess(prob, X, alphas):
    """The optimality certificate of any X for the weights ``alphas`` (``(alpha1, alpha2)`` pairs, one per column of X; X a list
    of solutions as ``fista_path`` returns it, or an n x k block): ``excess[i] = max_j |g_ij| / (alpha1_j p_i)`` with g_j the
    gradient of the data term at X_j and p the handle's penalty factors (or 1), from one fos_gradient_batch and one fos_kkt_scan
    with an empty set per 16 columns.  Where every X_ij is zero, X is optimal in coordinate i exactly when ``excess[i] <= 1``;
    on the support of a solution the value is 1 for the lasso and carries the ridge pull alpha2 |x| / alpha1 on top for the
    elastic net.  +inf marks a non-zero gradient on an unpenalised coordinate.  Returns n values, of the kind the handle was
    prepared from.  Synchronises."""
    prob = _handle(prob, None, None, "kkt_excess")
    alphas = _its._check_path_args(alphas, None)
    Xd = _block(prob, X)
    if Xd.shape[1] != len(alphas):
        raise ValueError(f"X has {Xd.shape[1]} columns for {len(alphas)} weights")
    return _worst_excess(prob, _steps(prob), Xd, alphas)


def alpha_max(prob):
    """The smallest alpha1 at which X = 0 is optimal: max_i |g_i(0)| / p_i over the penalised coordinates, g(0) the gradient of
    the data term at 0 (one fos_gradient_batch).  Every path starts from it.  With unpenalised coordinates (p_i = 0) X = 0 is
    not a solution at any weight; the value is then the gradient's at 0 all the same, the customary top of a path.
    Synchronises."""
    prob = _handle(prob, None, None, "alpha_max")
    return _top_excess(prob, _steps(prob))


def _lockstep(prob, fam, prms, X0, max_iter):
    """The lockstep of one group on `prob`, warm-started from the columns of X0 (None: from zero, the handles `fista_path`
    makes): the n_dev x nv float64 device block of the iterates after max_iter iterations.  A family of fam.width columns per
    fit has that many handles per parameter set, fit-major (`_run_path`)."""
    handles = []
    for v, prm in enumerate(p for p in prms for _ in range(fam.width)):
        st = _core.Fista(prob)
        st.reset(**prm, x0=None if X0 is None else X0[:, v].contiguous())
        handles.append(st)
    if (fam.refusal is None and len(handles) == 1) or not fam.launch(handles, 0, len(prms)):
        if fam.refusal is not None:
            raise _its._refused(prob, fam.refusal)
        for st in handles:
            st.run(max_iter)
    out = torch.zeros(prob.n_dev, len(handles), dtype=torch.float64, device=prob.device)
    for v, st in enumerate(handles):
        out[: prob.n, v] = st.x_tensor()
    return out


# What the outer loops (`_solve_group`, `duality._certified_group`) and their driver take from a loss family, so that a family
# whose fit spans several columns runs the same loops.  width: columns per fit.  gradient(prob, X) -> the gradient block.
# scan(prob, G, a1s, slack, in_ws) -> (excess, violators), one weight per fit.  certificate(prob, X, a1s, a2s) -> (out64, G), the
# values of a fit at its first column (`duality._certificate` reads them).  groups(count) -> the (first, number) runs of weights
# that share the 16 lockstep columns.  fits(prob, X, number) -> the solutions in the columns of X, of the kind that went in.
_Steps = collections.namedtuple("_Steps", "width gradient scan certificate groups fits")


def _steps(prob):
    P = _core.Problem
    if prob.loss == "multinomial":
        C = prob.classes
        return _Steps(C, P.multinomial_gradient_block, P.multinomial_kkt_scan, P.multinomial_duality_gap_block,
                      lambda count: _its.pack_groups(count, C),
                      lambda prob, X, number: [_core.from_device_vec(X[: prob.n, v * C:(v + 1) * C].contiguous(), prob.like) for v in range(number)])
    return _Steps(1, P.gradient_block, P.kkt_scan, P.duality_gap_block, lambda count: _its._groups(count, _its.LOCKSTEP_COLUMNS),
                  lambda prob, X, number: [_core.from_device_vec(prob.vec_out(X[:, v]), prob.like) for v in range(number)])


def _worst_excess(prob, steps, Xd, alphas):
    """`kkt_excess` on the device block Xd (one fit per weight): the largest excess over the groups, with an empty set."""
    empty, worst, W = _mask(prob), None, steps.width
    for first, number in steps.groups(len(alphas)):
        G = steps.gradient(prob, Xd[:, first * W:(first + number) * W])
        excess, _ = steps.scan(prob, G, [a1 for a1, _ in alphas[first:first + number]], 0.0, empty)
        worst = excess if worst is None else torch.maximum(worst, excess)
    return _core.from_device_vec(prob.vec_out(worst), prob.like)


def _top_excess(prob, steps):
    """`alpha_max`: the largest excess of one fit at X = 0 under weight 1 over the penalised coordinates."""
    G = steps.gradient(prob, torch.zeros(prob.n_dev, steps.width, dtype=torch.float32, device=prob.device))
    excess, _ = steps.scan(prob, G, [1.0], 0.0, _free(prob))
    return float(excess.max())


# ---- the pieces the two outer loops share ---------------------------------------------------------------------------------------
def _initial(prob, initial, what):
    """`initial=` of a path as sorted, distinct device numbers (None stays None); what: "column" or "coordinate"."""
    if initial is None:
        return None
    initial = torch.unique(torch.as_tensor(np.asarray(initial.cpu() if _core.is_tensor(initial) else initial)).to(torch.int64).reshape(-1))
    if initial.numel() == 0 or int(initial[0]) < 0 or int(initial[-1]) >= prob.n:
        raise ValueError(f"initial: {what} numbers in 0 .. {prob.n - 1} expected")
    return initial.to(prob.device)


def _gather(prob, fam, alphas, idx, L, t_init_factor):
    """The set idx as a sub-problem with its lockstep parameters: A_ws with the columns rounded up to 64, at least 128, zero beyond
    the set; the gathered factors (1 on the padding: its columns are zero)."""
    n_ws = int(idx.numel())
    n_ws_pad = max(MIN_COLUMNS, (n_ws + PAD_COLUMNS - 1) // PAD_COLUMNS * PAD_COLUMNS)
    A_ws = prob.gather_columns(idx, n_ws_pad)
    pf, p_ws = _factors(prob), None
    if pf is not None:
        p_ws = torch.ones(n_ws_pad, dtype=torch.float64)
        p_ws[:n_ws] = pf[idx].to("cpu", torch.float64)
        p_ws = p_ws.numpy()
    sub = _sub_problem(prob, A_ws, p_ws)
    return sub, _its._path_params(sub, alphas, L, fam, t_init_factor, None)


def _round(sub, fam, prms, X, idx, first, max_iter):
    """One round on the gathered set: the lockstep from X restricted to the set (from zero in a first round at X = 0), scattered
    back into X."""
    n_ws, X0 = int(idx.numel()), None
    if not first or bool((X != 0).any()):
        X0 = torch.zeros(sub.n, X.shape[1], dtype=torch.float64, device=X.device)
        X0[:n_ws] = X[idx]
    X[idx] = _lockstep(sub, fam, prms, X0, max_iter)[:n_ws]


def _grow(mask, excess, viol, n_ws, grow):
    """The violators join the set; when they are fewer than (grow - 1) |set|, so do the next largest excess values up to that
    number (violators come first)."""
    mask[viol.long()] = 1
    want = int((grow - 1.0) * n_ws)
    if int(viol.numel()) < want:
        vals, cand = torch.topk(excess, min(want, int(excess.numel())))
        mask[cand[vals > 0]] = 1


def _fall_back(prob, fam, alphas, X, L, t_init_factor, max_iter):
    """The full lockstep of the group, warm-started from X."""
    prms = _its._path_params(prob, alphas, L, fam, t_init_factor, None)
    return _lockstep(prob, fam, prms, X if bool((X != 0).any()) else None, max_iter)


def _drive(prob, alphas, steps, group, return_info):
    """A path front end after its checks: group(weights of one run) -> (X, info) over the runs of `steps.groups`."""
    xs, infos = [], []
    for first, number in steps.groups(len(alphas)):
        X, info = group(alphas[first:first + number])
        xs += steps.fits(prob, X, number)
        infos.append(info)
    return (xs, infos) if return_info else xs


def _solve_group(prob, fam, steps, alphas, max_iter, kkt_tol, max_rounds, grow, max_fraction, L, t_init_factor, initial):
    """One group of weights (up to 16 columns): (X as an n_dev x (fits * width) float64 device block, WorkingSetInfo)."""
    nv, a1s = len(alphas) * steps.width, [a1 for a1, _ in alphas]
    X = torch.zeros(prob.n_dev, nv, dtype=torch.float64, device=prob.device)
    full_gradients, sizes = 0, []
    if initial is not None:
        mask = _mask(prob, initial)
        worst = float("nan")
    else:
        free = _free(prob)
        excess, viol = steps.scan(prob, steps.gradient(prob, X), a1s, 0.0, free)
        full_gradients += 1
        mask = free.clone()
        mask[viol.long()] = 1
        worst = float(excess.max())
    limit = max_fraction * prob.n
    fell_back = False
    while True:
        idx = torch.nonzero(mask).reshape(-1)
        n_ws = int(idx.numel())
        if n_ws == 0:                                    # X = 0 passed the check for every weight: it is the solution
            break
        if n_ws > limit or len(sizes) == max_rounds:
            fell_back = True
            break
        sizes.append(n_ws)
        sub, prms = _gather(prob, fam, alphas, idx, L, t_init_factor)
        _round(sub, fam, prms, X, idx, len(sizes) == 1, max_iter)
        del sub                                          # one gathered matrix at a time
        excess, viol = steps.scan(prob, steps.gradient(prob, X), a1s, kkt_tol, mask)
        full_gradients += 1
        worst = float(excess.max())
        if int(viol.numel()) == 0:
            break
        _grow(mask, excess, viol, n_ws, grow)
    if fell_back:
        X = _fall_back(prob, fam, alphas, X, L, t_init_factor, max_iter)
        excess, _ = steps.scan(prob, steps.gradient(prob, X), a1s, kkt_tol, (X != 0).any(dim=1).to(torch.uint8))
        full_gradients += 1
        worst = float(excess.max())
    return X, WorkingSetInfo(len(sizes), sizes, full_gradients, worst, fell_back)


def working_set_path(A, b, alphas, max_iter: int = 500, *, kkt_tol: float = 1e-4, max_rounds: int = 20, grow: float = 2.0,
                     max_fraction: float = 0.5, L=None, t_init_factor: float = 1.0, dtype=None, initial=None,
                     return_info: bool = False):
    """Solve the same problem for several regularisation weights on a working set of columns (see the module).

    ``A``: an array or tensor with ``b`` (squared loss), or a handle from ``prepare`` / ``prepare_weighted`` /
    ``prepare_penalized``, squared or logistic: loss, sample weights and penalty factors belong to the handle.  ``alphas``: a
    sequence of ``(alpha1, alpha2)`` pairs as in ``fista_path``; alpha1 = 0 on a penalised coordinate is a ValueError.  The result
    is the list of solutions, of the kind that went in; with ``return_info=True`` also one ``WorkingSetInfo`` per group of up to
    16 weights.

    Per group: X = 0; the set starts as ``initial`` (column numbers) or as the unpenalised coordinates plus those that leave
    zero for some weight of the group (the KKT scan at X = 0).  Each round gathers A_ws (columns rounded up to 64, at least 128,
    zero beyond the set), runs ``max_iter`` lockstep iterations on it from X restricted to the set - the step comes from the
    sub-problem's own ``estimate_lipschitz`` unless ``L`` is given (lambda_max(A_ws^T W A_ws) <= lambda_max(A^T W A): a
    full-problem L is valid too; for a logistic handle L is the constant of the logistic data term, as in ``logistic_path``) -
    scatters the result back and scans the gradient of the FULL problem with the slack ``kkt_tol``: coordinate i outside the
    set violates when |g_ij| > alpha1_j p_i (1 + kkt_tol) for some weight j.  No violator: done.  Otherwise the violators join
    the set, and when they are fewer than ``(grow - 1) |set|`` so do the next largest ``excess`` values up to that number.  A
    set beyond ``max_fraction * n`` columns, or ``max_rounds`` rounds with violators left, hands the group to the full lockstep,
    warm-started (``fell_back``).  One gathered matrix lives at a time.

    ValueError before any device work: a handle with box bounds, feature groups, the multinomial loss or the group penalty, a
    sharded handle."""
    _its.reset_metrics()
    alphas = _its._check_path_args(alphas, None)
    if not (grow > 1.0 and 0.0 < max_fraction <= 1.0 and max_rounds >= 1 and kkt_tol >= 0.0):
        raise ValueError("working_set_path: grow > 1, 0 < max_fraction <= 1, max_rounds >= 1 and kkt_tol >= 0 expected")
    prob = _handle(A, b, dtype, "working_set_path")
    _check_weights(prob, alphas)
    initial = _initial(prob, initial, "column")
    fam, steps = _family(prob, max_iter), _steps(prob)
    return _drive(prob, alphas, steps, lambda part: _solve_group(prob, fam, steps, part, max_iter, kkt_tol, max_rounds, grow, max_fraction,
                                                                  L, t_init_factor, initial), return_info)
