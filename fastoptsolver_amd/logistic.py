"""Sparse logistic regression on the matrix-core lockstep (extension; the reference has squared loss only).

    minimise   sum_i log(1 + exp(a_i.x)) - y_i a_i.x  +  alpha1 ||x||_1  +  0.5 alpha2 ||x||^2 ,   labels y in [0, 1]

The gradient of the data term is A^T (sigma(Ax) - y): the lockstep of ``fista_path`` / ``fista_cv`` with ONE line of product
1's epilogue changed (csrc/batch_trial.hpp, LOSS_LOGISTIC) - product 2, the updates, the per-column restarts and stops on
the device and the fold masks are the launches of the squared loss.  The loss belongs to the problem handle
(``prepare(A, y, loss="logistic")``, fos_problem_set_loss); every entry point that would answer with a squared-loss quantity
refuses such a handle.  An intercept is a constant column appended by the caller AND given the penalty factor 0
(``prepare_penalized``): without the factor the column is shrunk like any other, which fits the wrong model whenever the classes
are unbalanced.

Per-coordinate penalty factors and box bounds (``prepare_penalized(A, y, penalty_factor, lower, upper, loss="logistic")``,
``Problem.set_penalty``, fos_coord_bind): the penalties become alpha1 sum_j p_j |x_j| + 0.5 alpha2 sum_j p_j x_j^2 subject to lower_j <= x_j <= upper_j;
the update kernel of the lockstep applies them per coordinate, the products over A are unchanged.

Per-row sample weights (``prepare_weighted(A, y, w, loss="logistic")``, fos_row_weights_bind): the data term becomes
sum_i w_i (log(1 + exp(a_i.x)) - y_i a_i.x); ``logistic_path`` / ``logistic_cv`` / ``logistic_objective`` take the handle as
``A`` and answer with the weighted quantities, the held-out scores as weighted means.
"""
from __future__ import annotations

import collections

from . import _core
from . import iterative_solvers as _its

LogisticCVResult = collections.namedtuple("LogisticCVResult", "alphas logloss mean_logloss best x coefs info")


def _problem(A, y, dtype):
    """The logistic handle on (A, y): a prepared one as it is, anything else bound (and padded) here."""
    if isinstance(A, _core.Problem):
        _core.refuse_link(A, "logistic_path / logistic_cv / logistic_objective")
        if A.loss != "logistic":
            raise ValueError(f'A was prepared for the {A.loss} loss: use prepare(A, y, loss="logistic")')
        return A
    if y is None:
        raise ValueError("the labels y are needed")
    return _core.Problem(A, y, dtype, None, "logistic")


def _family(max_iter):
    """One column per fit; sigma' <= 1/4 bounds the Hessian A^T diag(sigma') A by A^T A / 4 (A^T W A / 4 on a weighted handle)."""
    return _its._columns(max_iter, True, 4.0)


def logistic_path(A, y, alphas, t_init_factor: float = 1.0, max_iter: int = 500, *, delta=None, L=None, dtype=None,
                  tol_ratio: float = 0.0, adaptive_restart: bool = False, restart_threshold: float = 1.0,
                  return_info: bool = False):
    """Sparse logistic regression of the labels ``y`` (in [0, 1]) on A for several weights at once.

    ``alphas`` is a sequence of ``(alpha1, alpha2)`` pairs; the result is the list of solutions, one per pair, and with
    ``return_info=True`` also ``[(iterations, stop_code), ...]``.  The pairs advance in lockstep groups of up to 16 columns
    on the matrix cores (fos_fista_run_multi on a logistic problem): two GEMM-shaped products per iteration for the whole
    group.  A single pair is a one-column lockstep - there is no one-read single-target logistic pass, so a single fit
    reads A twice per iteration; that is accepted here.

    ``L``, when not given, is ``estimate_lipschitz(A) / 4`` (one power iteration, one draw from the global NumPy stream, like
    ``fista_path``): sigma' <= 1/4 bounds the Hessian A^T diag(sigma') A by A^T A / 4.  When given it is the constant of the
    logistic data term and used as it is.  The step is ``t_init_factor / (L + alpha2)``.

    Contract: each result is FISTA (FISTA-Δ with ``delta`` > 2) on the logistic objective from x0 = 0 with that step, under
    the momentum, restart (``adaptive_restart`` / ``restart_threshold``) and ratio-stop (``tol_ratio``) rules of the
    reference's loop, decided per column on the device.  There is no ``tol`` (the gradient-norm rule), no backtracking and
    no sharding.  A: an array / tensor (zero-padded on the device so that every shape up to 16384 columns is served: see
    ``prepare``) or a ``prepare(A, y, loss="logistic")`` handle (``y`` may then be None).

    A handle with penalty factors or bounds (``prepare_penalized(A, y, ..., loss="logistic")`` / ``Problem.set_penalty``):
    per-coordinate factors p_j >= 0 of both penalties and box bounds lower_j <= 0 <= upper_j.  An intercept is a constant
    column with factor 0.  The step is then ``t_init_factor / (L + alpha2 max_j
    p_j)``; L does not depend on the constraints."""
    _its.reset_metrics()
    alphas = _its._check_path_args(alphas, delta)
    prob, fam = _problem(A, y, dtype), _family(max_iter)
    prms = _its._path_params(prob, alphas, L, fam, t_init_factor, delta, tol_ratio=tol_ratio, adaptive_restart=adaptive_restart,
                             restart_threshold=restart_threshold)
    return _its._path_result(_its._run_path(prob, prms, fam, max_iter), fam, prob.like, return_info)


def logistic_cv(A, y, alphas, folds=5, t_init_factor: float = 1.0, max_iter: int = 500, *, delta=None, L=None, dtype=None,
                tol_ratio: float = 0.0, adaptive_restart: bool = False, restart_threshold: float = 1.0, refit: bool = True,
                return_coefs: bool = False):
    """K-fold cross-validation of a logistic regularisation path: ``fista_cv`` with the log-loss.

    ``folds`` as in ``fista_cv`` (an int K >= 2 or one fold id per row), validated before any device work.  All K x L fits
    are masked columns of the lockstep on the one device copy of A (fos_fista_run_multi_folds on a logistic problem); the
    held-out log-losses of a group come from one further pass with the complementary mask.  ``L`` comes from the whole A
    (``estimate_lipschitz(A) / 4`` unless given) and is valid for every training set: lambda_max(A_train^T A_train) <=
    lambda_max(A^T A).  Contract: ``coefs[:, f, a]`` is what ``logistic_path(A[train_f], y[train_f], [alphas[a]], ..., L=L)``
    returns.  No fold-by-fold slow path exists: padding makes every shape up to 16384 columns served, the rest raises.

    Returns ``LogisticCVResult(alphas, logloss, mean_logloss, best, x, coefs, info)``: ``logloss[f, a]`` the held-out MEAN
    log-loss (K x L float64 ndarray), ``mean_logloss`` its mean over the folds, ``best`` the argmin (first on ties), ``x``
    the fit on all rows at ``alphas[best]`` (``refit=True``; else None), ``coefs`` the n x K x L fits
    (``return_coefs=True``; else None), ``info[f][a] = (iterations, stop_code)``.

    A handle with penalty factors or bounds, as in ``logistic_path``: every fold's fit carries them (they belong to the
    coordinates, not the rows), with the step ``t_init_factor / (L + alpha2 max_j p_j)``."""
    _its.reset_metrics()
    alphas = _its._check_path_args(alphas, delta)
    ids, sizes = _its._cv_folds(folds, _its._rows(A))
    prob, fam = _problem(A, y, dtype), _family(max_iter)
    sizes = _its._cv_sizes(prob, ids, sizes)             # a weighted handle: the weight sums; a zero-weight fold raises here
    prms = _its._path_params(prob, alphas, L, fam, t_init_factor, delta, tol_ratio=tol_ratio, adaptive_restart=adaptive_restart,
                             restart_threshold=restart_threshold)
    out = _its._run_cv(prob, ids, len(sizes), prms, fam, max_iter)
    if out is None:
        raise _its._refused(prob, "fos_fista_run_multi_folds refused the lockstep: ")
    X, total, info = out
    return _its._cv_result(LogisticCVResult, prob.like, alphas, total, sizes,
                           (lambda best: _its._refit(prob, prms[best], fam, max_iter)) if refit else None,
                           X if return_coefs else None, info)


def logistic_objective(x, A, y, alpha1, alpha2):
    """sum_i log(1 + exp(a_i.x)) - y_i a_i.x + alpha1 ||x||_1 + 0.5 alpha2 ||x||^2 with the data term from the device
    (fos_residual_batch on a logistic problem; x is rounded to fp32 for the pass over A).  ``x``: a vector (returns a float) or
    an n x k block (returns k float64 values), 16 columns per pass.  Synchronises.
    On a handle with penalty factors (``Problem.set_penalty``) the penalties are the factored ones, alpha1 sum_j p_j |x_j| +
    0.5 alpha2 sum_j p_j x_j^2 (the fp32 factors as bound); the box is not checked - solver outputs lie inside it by
    construction."""
    prob = _problem(A, y, None)
    if prob.has_feature_groups:      # the separable penalty would answer for another objective
        raise ValueError("logistic_objective: the handle has feature groups (Problem.set_feature_groups): use "
                         'group_lasso_objective(x, handle, None, alpha1, alpha2, groups, ..., loss="logistic")')
    X, single = _its._objective_block(prob, x, 1)
    return _its._objective_value(prob, X, single, lambda block, number: prob.residual_batch(block, use_b=True), alpha1, alpha2)
