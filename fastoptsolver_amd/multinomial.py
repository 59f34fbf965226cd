"""Sparse multinomial (softmax) regression on the matrix-core lockstep (extension; the reference has squared loss only).

    minimise over X (n x C)   sum_i logsumexp_c(a_i.x_c) - a_i.x_{y_i}  +  alpha1 sum_c ||x_c||_1  +  0.5 alpha2 sum_c ||x_c||^2

with labels y_i in {0, ..., C-1}, 2 <= C <= 16.  The gradient of class c is A^T (softmax(A X)_c - [y = c]).  The 16 candidate
columns of the lockstep of ``fista_path`` hold the C class vectors of floor(16 / C) fits at once: product 1 computes all class
logits in one read of A, a link kernel couples the C columns of every fit (csrc/softmax_link.hpp: softmax, one-hot, loss),
product 2 computes all class gradients in the other read, and the updates, fold masks, row weights, penalty factors and bounds
are the launches of every other lockstep.  The loss belongs to the problem handle (``prepare(A, y, loss="multinomial")``,
``prepare_multinomial(A, y, classes=C)``; fos_problem_set_multinomial); every other solver refuses such a handle.

This is the symmetric (over-parametrised) softmax model glmnet and scikit-learn fit: with alpha1 > 0 or alpha2 > 0 the penalty
picks the solution.  A per-class intercept is a constant column with penalty factor 0 (``prepare_penalized``); rows weights
(``prepare_weighted``) multiply the data term per row.

A grouped handle (``prepare_multinomial(..., grouped=True)`` or ``Problem.set_grouped``; glmnet's ``type.multinomial =
"grouped"``) replaces the l1 penalty by the group penalty over the classes,

    alpha1 sum_j p_j ||X[j, :]||_2  +  0.5 alpha2 sum_j p_j ||X[j, :]||_2^2 ,

so that a feature is in the model for all C classes or for none: every class handle carries ``group = C``
(fos_fista_params.group) and the update kernel of the lockstep thresholds row j of X across the C columns of a fit together
(csrc/reduce_update.hpp, fista_update_group_kernel).  Like the penalty factors and bounds, the choice belongs to the handle:
``multinomial_path`` / ``multinomial_cv`` / ``multinomial_objective`` keep their signatures and answer with the grouped
quantities on a grouped handle.  Penalty factors compose with it; box bounds do not (ValueError).  Not served: sparse-group mixtures, groups of coefficients within one column, sharded problems.

The fits of a class group are one joint problem, so only plain runs exist: there is no ``tol_ratio``, ``adaptive_restart`` or
``restart_threshold`` here - a stop or restart decided per column would break the fit.  What says how far a result is from the
optimum, and a solve on the active rows of X alone, live in ``multinomial_ws`` (``multinomial_duality_gap``,
``multinomial_certified_path``, ``multinomial_working_set_path``).
"""
from __future__ import annotations

import collections

from . import _core
from . import iterative_solvers as _its
from .iterative_solvers import LOCKSTEP_COLUMNS, pack_groups        # (public here: the packing of the class groups)

MultinomialCVResult = collections.namedtuple("MultinomialCVResult", "alphas logloss mean_logloss best x coefs info")


def prepare_multinomial(A, y, classes=None, dtype=None, *, sample_weight=None, penalty_factor=None, lower=None, upper=None,
                        grouped=False):
    """``prepare(A, y, loss="multinomial")`` with the number of classes given: ``y`` holds one integral class index 0 .. C-1 per
    row (``classes=None``: C = max(y) + 1), 2 <= C <= 16, checked on the host before any device work (ValueError).  With
    ``sample_weight`` the handle is a weighted one (``prepare_weighted``), with ``penalty_factor`` / ``lower`` / ``upper`` one
    with per-coefficient penalty factors and box bounds (``prepare_penalized``; they belong to the coefficient's row of X and
    hold for every class).  Pass the handle as ``A`` (``y`` None) to ``multinomial_path`` / ``multinomial_cv`` /
    ``multinomial_objective``; ``.classes`` is C.  ``grouped=True``: the penalty of the handle is the group penalty over the
    classes (module docstring; ``.grouped``, ``Problem.set_grouped``) - with ``lower`` / ``upper`` a ValueError, before any
    device work."""
    if isinstance(A, _core.Problem):
        raise ValueError("prepare_multinomial binds an array or tensor; this is already a Problem")
    if grouped and (lower is not None or upper is not None):
        raise ValueError(_core.GROUPED_BOUNDS)
    prob = _core.Problem.multinomial(A, y, classes, dtype, sample_weight, penalty_factor, lower, upper)
    prob.set_grouped(grouped)
    return prob


def _problem(A, y, classes, dtype):
    """The multinomial handle on (A, y): a prepared one as it is, anything else bound (and padded) here."""
    if isinstance(A, _core.Problem):
        _core.refuse_link(A, "multinomial_path / multinomial_cv / multinomial_objective")
        if A.loss != "multinomial":
            raise ValueError(f'A was prepared for the {A.loss} loss: use prepare(A, y, loss="multinomial")')
        if classes is not None and int(classes) != A.classes:
            raise ValueError(f"classes = {classes}, but the handle was prepared with {A.classes} classes")
        return A
    return _core.Problem.multinomial(A, y, classes, dtype)


def _grouped(prob):
    """Whether the handle carries the group penalty.  The group penalty and box bounds have no composed closed-form prox: a
    grouped handle that has been given bounds since is refused on the host, before any device work."""
    grouped = bool(getattr(prob, "grouped", False))
    if grouped and (prob.lower is not None or prob.upper is not None):
        raise ValueError(_core.GROUPED_BOUNDS)
    return grouped


def _family(prob, max_iter):
    """C columns per fit, group = C on a grouped handle.  Boehning's bound: the softmax Hessian is <= 1/2 I (x) A^T A (A^T W A on
    a weighted handle), so L = lambda_max / 2 unless given.  A refusal raises."""
    return _its._Family(prob.classes, prob.classes if _grouped(prob) else 0, 2.0,
                        lambda handles, first, number: _core.run_multi(handles, max_iter),
                        "fos_fista_run_multi refused the multinomial lockstep: ")


def multinomial_path(A, y, alphas, classes=None, t_init_factor: float = 1.0, max_iter: int = 500, *, delta=None, L=None,
                     dtype=None, return_info: bool = False):
    """Sparse multinomial regression of the class labels ``y`` (integers 0 .. C-1) on A for several weights at once.

    ``alphas`` is a sequence of ``(alpha1, alpha2)`` pairs; the result is the list of n x C solutions, one per pair (column c
    the coefficients of class c), and with ``return_info=True`` also ``[(iterations, stop_code), ...]``.  ``classes``: C, or
    None for max(y) + 1 (a handle knows its own).  floor(16 / C) pairs advance per lockstep call (``pack_groups``); a call
    reads A twice per iteration whatever the number of pairs and classes in it.

    ``L``, when not given, is ``estimate_lipschitz(A) / 2`` (one power iteration, one draw from the global NumPy stream):
    Boehning's bound, the Hessian of the softmax data term is <= 1/2 I (x) A^T A; on a weighted handle lambda_max(A^T W A) / 2.
    The step is ``t_init_factor / (L + alpha2 max_j p_j)`` (p: the penalty factors of a ``prepare_penalized`` handle, else 1).

    Contract: each result is FISTA (FISTA-Δ with ``delta`` > 2) on the multinomial objective over the stacked unknown from
    X0 = 0 with that step for exactly ``max_iter`` iterations.  No stopping rule and no momentum restart: the columns of a fit
    are one joint problem.  A: an array / tensor (padded on the device as a logistic problem is; at most 16384 device columns)
    or a ``prepare(A, y, loss="multinomial")`` / ``prepare_multinomial`` handle (``y`` may then be None), weighted or penalised
    handles included.

    A grouped handle (``prepare_multinomial(..., grouped=True)``): the group penalty over the classes (module docstring)
    instead of the l1 penalty - row j of every result is zero in all C classes or in none.  Same step, same contract; a grouped
    handle with box bounds raises ValueError."""
    _its.reset_metrics()
    alphas = _its._check_path_args(alphas, delta)
    prob = _problem(A, y, classes, dtype)
    fam = _family(prob, max_iter)
    prms = _its._path_params(prob, alphas, L, fam, t_init_factor, delta)
    return _its._path_result(_its._run_path(prob, prms, fam, max_iter), fam, prob.like, return_info)


def multinomial_cv(A, y, alphas, folds=5, classes=None, t_init_factor: float = 1.0, max_iter: int = 500, *, delta=None, L=None,
                   dtype=None, refit: bool = True, return_coefs: bool = False):
    """K-fold cross-validation of a multinomial regularisation path: ``fista_cv`` with the softmax cross-entropy.

    ``folds`` as in ``fista_cv`` (an int K >= 2 or one fold id per row), validated before any device work.  Every (fold,
    weight) pair is a class group of the masked lockstep on the one device copy of A (fos_fista_run_multi_folds on a
    multinomial problem), floor(16 / C) pairs per call; the held-out losses of a call come from one further pass with the
    complementary mask (fos_residual_batch_folds).  ``L`` comes from the whole A (``estimate_lipschitz(A) / 2`` unless given)
    and is valid for every training set.  Contract: ``coefs[:, :, f, a]`` is what ``multinomial_path(A[train_f], y[train_f],
    [alphas[a]], classes=C, ..., L=L)`` returns.

    Returns ``MultinomialCVResult(alphas, logloss, mean_logloss, best, x, coefs, info)``: ``logloss[f, a]`` the held-out MEAN
    cross-entropy (K x L float64 ndarray; on a weighted handle the weighted sum over the held-out weight sum), ``mean_logloss``
    its mean over the folds, ``best`` the argmin (first on ties), ``x`` the n x C fit on all rows at ``alphas[best]``
    (``refit=True``; else None), ``coefs`` the n x C x K x L fits (``return_coefs=True``; else None), ``info[f][a] =
    (iterations, stop_code)``.

    A grouped handle: every fit (the refit included) carries the group penalty over the classes, as in ``multinomial_path``;
    the held-out score is the same cross-entropy."""
    _its.reset_metrics()
    alphas = _its._check_path_args(alphas, delta)
    ids, sizes = _its._cv_folds(folds, _its._rows(A))
    prob = _problem(A, y, classes, dtype)
    fam = _family(prob, max_iter)
    sizes = _its._cv_sizes(prob, ids, sizes)             # a weighted handle: the weight sums; a zero-weight fold raises here
    prms = _its._path_params(prob, alphas, L, fam, t_init_factor, delta)
    X, total, info = _its._run_cv(prob, ids, len(sizes), prms, fam, max_iter,
                                  "fos_fista_run_multi_folds refused the multinomial lockstep: ")
    return _its._cv_result(MultinomialCVResult, prob.like, alphas, total, sizes,
                           (lambda best: _its._refit(prob, prms[best], fam, max_iter)) if refit else None,
                           X if return_coefs else None, info)


def multinomial_objective(X, A, y, alpha1, alpha2):
    """sum_i logsumexp_c(a_i.x_c) - a_i.x_{y_i} + alpha1 sum |X| + 0.5 alpha2 sum X^2 with the data term from the device
    (fos_residual_batch on a multinomial problem; X is rounded to fp32 for the pass over A; weighted per row on a weighted
    handle).  ``X``: n x C (returns a float) or an n x C x k block (returns k float64 values), floor(16 / C) members per pass.
    Synchronises.  On a handle with penalty factors the penalties are the factored ones, alpha1 sum_j p_j sum_c |x_jc| + 0.5
    alpha2 sum_j p_j sum_c x_jc^2 (the fp32 factors as bound); the box is not checked.  On a grouped handle the l1 term is the
    group penalty alpha1 sum_j p_j ||X[j, :]||_2 (the row norms over the classes, with the factors)."""
    prob = _problem(A, y, None, None)
    grouped = _grouped(prob)
    C = prob.classes
    Xd, single = _its._objective_block(prob, X, C)
    return _its._objective_value(prob, Xd, single, lambda block, number: prob.residual_batch(block, use_b=True)[::C],
                                 alpha1, alpha2, grouped)
