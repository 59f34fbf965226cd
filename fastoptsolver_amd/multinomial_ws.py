"""Working set and duality gap for the multinomial lockstep (extension): ``working_set_path``, ``certified_path``, ``duality_gap``,
``kkt_excess`` and ``alpha_max`` under names of their own, for the family those refuse.

A multinomial fit occupies C of the 16 lockstep columns, so only floor(16 / C) weights advance per pass over A; the multinomial
lockstep has no stopping rule (``multinomial_path``: exactly ``max_iter`` iterations); and a grouped fit is sparse in whole rows
of X.  The names here are to ``multinomial_path`` what ``working_set_path`` and ``certified_path`` are to ``fista_path``: the
same outer loops (``working_set._solve_group``, ``duality._certified_group``) and driver, given the device steps that see the C
columns of a fit together (``working_set._steps``; include/fos_multinomial_ws.h).

For one fit X (n x C) with the weights (alpha1, alpha2): Z = A X, sigma_i = softmax(z_i), row weights w (or 1), penalty factors p
(or 1), tau = alpha1 p, rho = alpha2 p and G = A^T (w (sigma - onehot(y))) (n x C):

    P = sum_i w_i [logsumexp(z_i) - z_{i,y_i}] + Omega(X)
    s = min(1, min over {rho = 0, v != 0} of tau / v)
    D = sum_i w_i d_i - sum over {rho > 0} of max(s v - tau, 0)^2 / (2 rho),     d_i = -sum_c q_ic log q_ic,
                                                                                 q_i = onehot(y_i) + s (sigma_i - onehot(y_i))

On a plain handle Omega is the l1 penalty and v runs over the entries, v = |G_kc|; on a grouped handle (``prepare_multinomial(...,
grouped=True)``) Omega is the group penalty over the classes and v runs over the rows, v = ||G_k:||_2.  The conjugate of the softmax
cross-entropy is the negative entropy on the simplex, and q_i is a convex combination of two of its points for s in [0, 1]: the
dual value is finite, gap = P - D >= P - P*.  A zero row k of X is optimal when max_c |G_kc| <= alpha1 p_k (l1) or ||G_k:||_2 <=
alpha1 p_k (grouped).  An unpenalised coordinate (p_k = 0) with a non-zero gradient gives s = 0: the bound stays valid and is loose.

The working set is a set of coordinates - rows of X - shared by the classes and the weights of a group of floor(16 / C) weights
(``pack_groups``); the sub-problem is a multinomial ``Problem`` on the gathered matrix with the handle's labels, class count, row
weights, gathered factors and kind of penalty, run by the family of ``multinomial_path`` and warm-started per class column.

Served: the multinomial loss, l1 or grouped, sample weights, penalty factors.  Not served (ValueError before any device work): a
handle of another loss (``working_set_path`` / ``certified_path`` / ``duality_gap`` serve those), box bounds, sharded problems,
alpha1 = 0 on a penalised coordinate.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _core
from . import duality as _du
from . import iterative_solvers as _its
from . import multinomial as _mn
from . import working_set as _ws
from .duality import DualityGap, GapInfo
from .working_set import WorkingSetInfo


def _handle(A, y, classes, dtype, who):
    """The multinomial handle of a call: a prepared one as it is (refused, before any device work, where these names do not serve
    it), anything else bound here."""
    if not isinstance(A, _core.Problem):
        return _core.Problem.multinomial(A, y, classes, dtype)
    if A.loss != "multinomial":
        raise ValueError(f"{who}: a handle of the {A.loss} loss is not served (the multinomial loss): use working_set_path / "
                         "certified_path / duality_gap / kkt_excess / alpha_max")
    if A.lower is not None or A.upper is not None:
        raise ValueError(f"{who}: box bounds are not served: a coordinate at a bound has another optimality condition")
    if getattr(A, "comm", None) is not None or getattr(A, "col_sharded", False):
        raise ValueError(f"{who}: sharded problems are not served")
    if A.b is None:
        raise ValueError(f"{who}: the handle was prepared without labels")
    if classes is not None and int(classes) != A.classes:
        raise ValueError(f"{who}: classes = {classes}, but the handle was prepared with {A.classes} classes")
    return A


def _block(prob, X):
    """Fits (an n x C matrix, an n x C x k block or a list of n x C matrices) as an n_dev x (k * C) float64 device block,
    fit-major: column s * C + c is class c of fit s."""
    if isinstance(X, (list, tuple)):
        X = torch.stack([torch.as_tensor(np.asarray(x) if not _core.is_tensor(x) else x).detach().to(torch.float64).cpu() for x in X], dim=-1)
    Xd, _ = _its._objective_block(prob, X, prob.classes)
    out = torch.zeros(prob.n_dev, Xd.shape[1] * Xd.shape[2], dtype=torch.float64, device=prob.device)
    out[: prob.n] = Xd.permute(0, 2, 1).reshape(prob.n, -1)
    return out


def multinomial_alpha_max(prob):
    """The smallest alpha1 at which X = 0 is optimal on a multinomial handle: max_k v_k(0) / p_k over the penalised coordinates,
    v_k = max_c |G_kc| on a plain handle and ||G_k:||_2 on a grouped one, G the gradient of the data term at 0 (one
    fos_multinomial_gradient_batch).  With unpenalised coordinates the value is the gradient's at 0 all the same, as
    ``alpha_max`` has it.  Synchronises."""
    prob = _handle(prob, None, None, None, "multinomial_alpha_max")
    _mn._grouped(prob)
    return _ws._top_excess(prob, _ws._steps(prob))


def multinomial_kkt_excess(prob, X, alphas):
    """The optimality certificate of the fits X (an n x C x k block, or a list of n x C solutions as ``multinomial_path`` returns
    them) for the weights ``alphas`` (``(alpha1, alpha2)`` pairs, one per fit): ``excess[k] = max over the fits of v_k / (alpha1
    p_k)`` with v_k = max_c |G_kc| (``.grouped``: ||G_k:||_2), from one fos_multinomial_gradient_batch and one
    fos_multinomial_kkt_scan with an empty set per floor(16 / C) fits.  Where row k of every fit is zero, X is optimal in
    coordinate k exactly when ``excess[k] <= 1``; +inf marks a non-zero gradient on an unpenalised coordinate.  Returns n values,
    of the kind the handle was prepared from.  Synchronises."""
    prob = _handle(prob, None, None, None, "multinomial_kkt_excess")
    _mn._grouped(prob)
    alphas = _its._check_path_args(alphas, None)
    Xd, C = _block(prob, X), prob.classes
    if Xd.shape[1] != len(alphas) * C:
        raise ValueError(f"X has {Xd.shape[1] // C} fits for {len(alphas)} weights")
    return _ws._worst_excess(prob, _ws._steps(prob), Xd, alphas)


def multinomial_duality_gap(prob, X, alphas):
    """The duality-gap certificate of the fits X (an n x C x k block, or a list of n x C solutions as ``multinomial_path`` returns
    them; rounded to fp32 for the passes over A) for the weights ``alphas`` (``(alpha1, alpha2)`` pairs, one per fit): a
    ``DualityGap`` of float64 ndarrays with one entry per fit - P, D, P - D >= P - P* and the scale s (module docstring).  On a
    grouped handle the penalty and the dual norm are the group ones.  One fos_multinomial_duality_gap call (three reads of A) per
    floor(16 / C) fits.  Synchronises."""
    prob = _handle(prob, None, None, None, "multinomial_duality_gap")
    _mn._grouped(prob)
    alphas = _its._check_path_args(alphas, None)
    Xd, C = _block(prob, X), prob.classes
    if Xd.shape[1] != len(alphas) * C:
        raise ValueError(f"X has {Xd.shape[1] // C} fits for {len(alphas)} weights")
    return _du._gaps(prob, _ws._steps(prob), Xd, alphas)


def _begin(A, y, alphas, classes, dtype, who, ok, expected):
    _its.reset_metrics()
    alphas = _its._check_path_args(alphas, None)
    if not ok:
        raise ValueError(f"{who}: {expected} expected")
    prob = _handle(A, y, classes, dtype, who)
    _mn._grouped(prob)
    _ws._check_weights(prob, alphas)
    return prob, alphas


def multinomial_working_set_path(A, y, alphas, classes=None, max_iter: int = 500, *, kkt_tol: float = 1e-4, max_rounds: int = 20,
                                 grow: float = 2.0, max_fraction: float = 0.5, L=None, t_init_factor: float = 1.0, dtype=None,
                                 initial=None, return_info: bool = False):
    """``multinomial_path`` on a working set of coordinates: ``working_set_path``'s outer loop for the multinomial loss.

    ``A``, ``y``, ``alphas``, ``classes``, ``L``, ``t_init_factor`` and ``dtype`` are ``multinomial_path``'s (a
    ``prepare_multinomial`` handle carries its weights, factors and ``grouped``); ``max_iter``, ``kkt_tol``, ``max_rounds``,
    ``grow``, ``max_fraction`` and ``initial`` are ``working_set_path``'s.  The result is the list of n x C solutions; with
    ``return_info=True`` also one ``WorkingSetInfo`` per group of floor(16 / C) weights.

    Per group the set holds coordinates - rows of X, all C classes of all weights of the group: it starts as ``initial`` or as
    the unpenalised coordinates plus those that leave zero for some weight (the scan at X = 0); a round gathers A_ws, runs
    ``max_iter`` multinomial lockstep iterations on it, warm-started per class column, and scans the gradient of the FULL problem
    (fos_multinomial_gradient_batch, fos_multinomial_kkt_scan): coordinate k outside the set violates when max_c |G_kc| (grouped:
    ||G_k:||_2) > alpha1 p_k (1 + kkt_tol) for some weight.  Growth, the ways to fall back and their report are
    ``working_set_path``'s.

    ValueError before any device work: a handle of another loss, box bounds, a sharded handle, alpha1 = 0 on a penalised
    coordinate."""
    prob, alphas = _begin(A, y, alphas, classes, dtype, "multinomial_working_set_path",
                          grow > 1.0 and 0.0 < max_fraction <= 1.0 and max_rounds >= 1 and kkt_tol >= 0.0,
                          "grow > 1, 0 < max_fraction <= 1, max_rounds >= 1 and kkt_tol >= 0")
    initial = _ws._initial(prob, initial, "coordinate")
    fam, steps = _ws._family(prob, max_iter), _ws._steps(prob)
    return _ws._drive(prob, alphas, steps, lambda part: _ws._solve_group(prob, fam, steps, part, max_iter, kkt_tol, max_rounds, grow,
                                                                          max_fraction, L, t_init_factor, initial), return_info)


def multinomial_certified_path(A, y, alphas, classes=None, gap_tol: float = 1e-4, max_iter: int = 500, *, max_rounds: int = 20,
                               grow: float = 2.0, max_fraction: float = 0.5, L=None, t_init_factor: float = 1.0, dtype=None,
                               return_info: bool = False):
    """``multinomial_path`` on a working set of coordinates until the duality gap certifies every fit: ``certified_path``'s outer
    loop for the multinomial loss, with ``gap_j <= gap_tol * P_j(0)`` as the stop rule - the stopping rule the multinomial
    lockstep itself does not have.

    Arguments as in ``multinomial_working_set_path`` and ``certified_path``.  The result is the list of n x C solutions; with
    ``return_info=True`` also one ``GapInfo`` per group of floor(16 / C) weights, its arrays with one entry per fit.  Each round
    ends with one fos_multinomial_duality_gap (three reads of A) whose gradient block the scan reads.  ``certified[j]`` is False
    where the bound was not met: an uncertified answer is never returned silently.

    ValueError before any device work: a handle of another loss, box bounds, a sharded handle, alpha1 = 0 on a penalised
    coordinate."""
    prob, alphas = _begin(A, y, alphas, classes, dtype, "multinomial_certified_path",
                          gap_tol >= 0.0 and np.isfinite(gap_tol) and grow > 1.0 and 0.0 < max_fraction <= 1.0 and max_rounds >= 1,
                          "gap_tol >= 0, grow > 1, 0 < max_fraction <= 1 and max_rounds >= 1")
    fam, steps = _ws._family(prob, max_iter), _ws._steps(prob)
    return _ws._drive(prob, alphas, steps, lambda part: _du._certified_group(prob, fam, steps, part, gap_tol, max_iter, max_rounds, grow,
                                                                              max_fraction, L, t_init_factor), return_info)
