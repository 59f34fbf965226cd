"""Duality-gap certificate of lockstep solutions and a path that stops on it (extension).

The lockstep stops on an iteration budget or on the reference's step and ratio rules; ``working_set_path`` certifies which
coordinates are zero (the KKT check), not that the solve on the working set has converged.  The duality gap bounds the
suboptimality itself, ``P(x) - P* <= gap``, for every loss the lockstep serves; it is what ``tol`` means in scikit-learn, glmnet,
celer and skglm.

For a point x with the weights (alpha1, alpha2), z = A x, row weights w (or 1), penalty factors p (or 1), tau = alpha1 p,
rho = alpha2 p, psi = df/dz and G = A^T (w psi):

    P = sum_i w_i f(z_i, b_i) + sum_k (tau_k |x_k| + rho_k x_k^2 / 2)
    s = min(1, min over {k : rho_k = 0, G_k != 0} of tau_k / |G_k|)
    D = sum_i w_i d(z_i, b_i; s) - sum over {k : rho_k > 0} of max(s |G_k| - tau_k, 0)^2 / (2 rho_k)

with d minus the conjugate of the loss at the scaled derivative (include/fos_duality.h lists it per loss).  ``duality_gap`` returns
P, D, P - D and s per column from the device (fos_duality_gap: three reads of A per 16 columns); ``certified_path`` is the outer
loop of ``working_set_path`` with ``gap_j <= gap_tol * P_j(0)`` as the stop rule.

An unpenalised coordinate (p_k = 0) with a non-zero gradient gives s = 0: the bound D = -F*(0) stays valid and is loose - the
dual point is not projected off the free columns - so a handle with unpenalised coordinates seldom certifies at a small gap_tol;
such a column is returned with ``certified`` False, never silently.

Served: squared, logistic, Huber and squared-hinge loss, sample weights, penalty factors.  Not served (ValueError before any device
work): box bounds, feature groups, the group penalty, the multinomial loss, sharded problems.
The multinomial loss and the group penalty over the classes have names of their own: ``multinomial_ws.multinomial_duality_gap`` and
``multinomial_ws.multinomial_certified_path``.
"""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import iterative_solvers as _its
from . import working_set as _ws

DualityGap = collections.namedtuple("DualityGap", "primal dual gap scale")
DualityGap.__doc__ = """float64 ndarrays, one entry per (alpha1, alpha2) pair: the primal value P, the dual value D at the scaled
dual point, gap = P - D >= P - P*, and the scale s in [0, 1] that made the dual point feasible (0: an unpenalised coordinate with a
non-zero gradient - the bound is loose)."""

GapInfo = collections.namedtuple("GapInfo", "rounds sizes certificates primal dual gap scale certified fell_back")
GapInfo.__doc__ = """What one group of up to 16 weights did: the rounds solved on a working set, the set's size in each, the number
of certificates taken (each reads A three times), the last certificate per column (primal, dual, gap, scale: float64 ndarrays),
``certified[j]`` - whether gap_j <= gap_tol * P_j(0) - and whether the group fell back to the full lockstep."""


def _certificate(prob, steps, X, alphas):
    """(primal, dual, gap, scale as float64 ndarrays, one entry per fit in the columns of X - at most 16 columns -, the gradient
    block G).  Synchronises."""
    out64, G = steps.certificate(prob, X, [a1 for a1, _ in alphas], [a2 for _, a2 in alphas])
    out = out64.cpu().numpy().reshape(4, 16)[:, :len(alphas) * steps.width:steps.width].copy()
    return out[0], out[1], out[2], out[3], G


def _gaps(prob, steps, Xd, alphas):
    """`duality_gap` on the device block Xd (one fit per weight): the certificates of the groups, joined."""
    W = steps.width
    parts = [_certificate(prob, steps, Xd[:, first * W:(first + number) * W], alphas[first:first + number])[:4]
             for first, number in steps.groups(len(alphas))]
    return DualityGap(*(np.concatenate([part[i] for part in parts]) for i in range(4)))


def duality_gap(prob, X, alphas):
    """The duality-gap certificate of any X for the weights ``alphas`` (``(alpha1, alpha2)`` pairs, one per column of X; X a list
    of solutions as ``fista_path`` returns it, or an n x k block; it is rounded to fp32 for the passes over A): a ``DualityGap``
    of float64 ndarrays with one entry per pair.  ``prob``: a handle ``kkt_excess`` accepts - squared, logistic, Huber or squared
    hinge, with sample weights and penalty factors; the same ValueErrors, before any device work.  One fos_duality_gap call per
    16 columns.  Synchronises."""
    prob = _ws._handle(prob, None, None, "duality_gap")
    alphas = _its._check_path_args(alphas, None)
    Xd = _ws._block(prob, X)
    if Xd.shape[1] != len(alphas):
        raise ValueError(f"X has {Xd.shape[1]} columns for {len(alphas)} weights")
    return _gaps(prob, _ws._steps(prob), Xd, alphas)


def _certified_group(prob, fam, steps, alphas, gap_tol, max_iter, max_rounds, grow, max_fraction, L, t_init_factor):
    """One group of weights (up to 16 columns; `working_set._Steps`): (X as an n_dev x (fits * width) float64 device block,
    GapInfo)."""
    nv, a1s = len(alphas) * steps.width, [a1 for a1, _ in alphas]
    X = torch.zeros(prob.n_dev, nv, dtype=torch.float64, device=prob.device)
    free = _ws._free(prob)
    primal, dual, gap, scale, G = _certificate(prob, steps, X, alphas)   # at X = 0: P_j(0) and the first violators
    certificates = 1
    bound = gap_tol * primal
    _, viol = steps.scan(prob, G, a1s, 0.0, free)
    mask = free.clone()
    mask[viol.long()] = 1
    limit = max_fraction * prob.n
    sizes, fell_back, sub = [], False, None
    while not bool((gap <= bound).all()):
        if sub is None:                                  # the set changed: gather it (one gathered matrix at a time)
            idx = torch.nonzero(mask).reshape(-1)
            n_ws = int(idx.numel())
        if n_ws == 0 or n_ws > limit or len(sizes) == max_rounds:
            fell_back = True
            break
        sizes.append(n_ws)
        if sub is None:
            sub, prms = _ws._gather(prob, fam, alphas, idx, L, t_init_factor)
        _ws._round(sub, fam, prms, X, idx, len(sizes) == 1, max_iter)
        primal, dual, gap, scale, G = _certificate(prob, steps, X, alphas)
        certificates += 1
        excess, viol = steps.scan(prob, G, a1s, 0.0, mask)   # the certificate's own gradient: no second one is taken
        if int(viol.numel()) == 0:                       # the zeros are right and the gap is not there yet: the same set again
            continue
        _ws._grow(mask, excess, viol, n_ws, grow)        # working_set_path's growth rule
        sub = prms = None
    if fell_back:
        sub = None
        X = _ws._fall_back(prob, fam, alphas, X, L, t_init_factor, max_iter)
        primal, dual, gap, scale, G = _certificate(prob, steps, X, alphas)
        certificates += 1
    return X, GapInfo(len(sizes), sizes, certificates, primal, dual, gap, scale, gap <= bound, fell_back)


def certified_path(A, b, alphas, gap_tol: float = 1e-4, max_iter: int = 500, *, max_rounds: int = 20, grow: float = 2.0,
                   max_fraction: float = 0.5, L=None, t_init_factor: float = 1.0, dtype=None, return_info: bool = False):
    """Solve the same problem for several regularisation weights on a working set of columns until the duality gap certifies
    every solution: ``working_set_path``'s outer loop with ``gap_j <= gap_tol * P_j(0)`` as the stop rule (P_j(0): the primal value
    of weight j at X = 0).

    ``A``, ``b``, ``alphas``, ``max_iter``, ``max_rounds``, ``grow``, ``max_fraction``, ``L``, ``t_init_factor`` and ``dtype`` are
    ``working_set_path``'s; a Huber or squared-hinge handle is served too.  The result is the list of solutions, of the kind that
    went in; with ``return_info=True`` also one ``GapInfo`` per group of up to 16 weights.

    Per group: one certificate at X = 0 gives P_j(0) and the first violators, which with the unpenalised coordinates make the
    first set.  Each round runs ``max_iter`` lockstep iterations on the gathered set, warm-started, then takes one certificate
    (fos_duality_gap) and scans its gradient block with slack 0 (fos_kkt_scan) - no second gradient.  The group is done when every
    column's gap is within its bound.  Otherwise violators join the set (with ``working_set_path``'s growth rule); with no violator
    the next round runs on the same set without gathering again.  A set beyond ``max_fraction * n`` columns, an empty set, or
    ``max_rounds`` rounds hand the group to the full lockstep, warm-started for ``max_iter`` iterations (``fell_back``), and a last
    certificate follows.  ``certified[j]`` is False where the bound was not met: an uncertified answer is never returned
    silently.  With unpenalised coordinates (p_k = 0) the bound is loose (see the module) and a small ``gap_tol`` is seldom met.

    ValueError before any device work: a handle with box bounds, feature groups, the multinomial loss or the group penalty, a
    sharded handle."""
    _its.reset_metrics()
    alphas = _its._check_path_args(alphas, None)
    if not (gap_tol >= 0.0 and np.isfinite(gap_tol) and grow > 1.0 and 0.0 < max_fraction <= 1.0 and max_rounds >= 1):
        raise ValueError("certified_path: gap_tol >= 0, grow > 1, 0 < max_fraction <= 1 and max_rounds >= 1 expected")
    prob = _ws._handle(A, b, dtype, "certified_path")
    _ws._check_weights(prob, alphas)
    fam, steps = _ws._family(prob, max_iter), _ws._steps(prob)
    return _ws._drive(prob, alphas, steps, lambda part: _certified_group(prob, fam, steps, part, gap_tol, max_iter, max_rounds, grow,
                                                                          max_fraction, L, t_init_factor), return_info)
