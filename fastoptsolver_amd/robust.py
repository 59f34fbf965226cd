"""Huber regression and the squared-hinge classifier on the matrix-core lockstep (extension; the reference has squared loss only).

    Huber          minimise   sum_i w_i rho_c(a_i.x - b_i)          +  alpha1 ||x||_1  +  0.5 alpha2 ||x||^2
                   rho_c(r) = r^2 / 2  (|r| <= c),  c |r| - c^2 / 2  (otherwise);   c = ``threshold`` > 0
    squared hinge  minimise   sum_i w_i max(0, 1 - y_i a_i.x)^2 / 2  +  alpha1 ||x||_1  +  0.5 alpha2 ||x||^2 ,   y in {-1, +1}

Huber is the robust regression for a ``b`` with gross outliers, the squared hinge the sparse linear SVM (L1 / elastic-net
regularised L2-loss SVC).  Both are pointwise in z = a_i.x, so the gradient of the data term is A^T (w * psi(z, b)) with psi =
clip(z - b, -c, c) or -y max(0, 1 - y z): the lockstep of ``fista_path`` / ``fista_cv`` with product 1 in its plain storing form
and ONE kernel between the two products that rewrites the panel in place (csrc/pointwise_link.hpp) - product 2, the updates, the
per-column restarts and stops on the device and the fold masks are the launches of the squared loss.  |psi'| <= 1 (the 1/2 of the
hinge is there for that), so L is the squared loss's lambda_max(A^T W A) and the step is fixed.

The loss belongs to the problem handle (``prepare_huber(A, b, threshold)`` / ``prepare_hinge(A, y)``,
fos_problem_set_link_loss); every entry point that would answer with another loss's quantity refuses such a handle.  Row weights
(``sample_weight=``), penalty factors and box bounds (``Problem.set_penalty``) and feature groups (``Problem.set_feature_groups``)
compose as on a logistic handle; an intercept is a constant column with the penalty factor 0.  ``delta`` is FISTA-Δ's, as
everywhere in this package - hence the name ``threshold`` for Huber's c.
"""
from __future__ import annotations

import collections

from . import _core
from . import iterative_solvers as _its

HuberCVResult = collections.namedtuple("HuberCVResult", "alphas loss mean_loss best x coefs info")
HingeCVResult = collections.namedtuple("HingeCVResult", "alphas loss mean_loss best x coefs info")


def _huber_problem(A, b, threshold, dtype):
    """The Huber handle on (A, b): a prepared one as it is (a threshold that is given must be the handle's), anything else bound
    (and padded) here."""
    if isinstance(A, _core.Problem):
        if A.loss != "huber":
            raise ValueError(f"A was prepared for the {A.loss} loss: use prepare_huber(A, b, threshold)")
        if threshold is not None and float(threshold) != A.threshold:
            raise ValueError(f"threshold = {threshold}, but the handle was prepared with {A.threshold}")
        return A
    if b is None:
        raise ValueError("the targets b are needed")
    if threshold is None:
        raise ValueError("threshold is needed unless A is a prepare_huber handle")
    return _core.Problem.link(A, b, "huber", threshold, dtype)


def _hinge_problem(A, y, dtype):
    """The squared-hinge handle on (A, y): a prepared one as it is, anything else bound (and padded) here."""
    if isinstance(A, _core.Problem):
        if A.loss != "squared_hinge":
            raise ValueError(f"A was prepared for the {A.loss} loss: use prepare_hinge(A, y)")
        return A
    if y is None:
        raise ValueError("the labels y are needed")
    return _core.Problem.link(A, y, "squared_hinge", None, dtype)


def _family(max_iter):
    """One column per fit; |psi'| <= 1 bounds the Hessian by A^T A (A^T W A on a weighted handle): the squared loss's L."""
    return _its._columns(max_iter, True, 1.0)


def _path(prob, alphas, t_init_factor, max_iter, delta, L, tol_ratio, adaptive_restart, restart_threshold, return_info):
    fam = _family(max_iter)
    prms = _its._path_params(prob, alphas, L, fam, t_init_factor, delta, tol_ratio=tol_ratio, adaptive_restart=adaptive_restart,
                             restart_threshold=restart_threshold)
    return _its._path_result(_its._run_path(prob, prms, fam, max_iter), fam, prob.like, return_info)


def _cv(result, prob, alphas, ids, sizes, t_init_factor, max_iter, delta, L, tol_ratio, adaptive_restart, restart_threshold, refit,
        return_coefs):
    fam = _family(max_iter)
    sizes = _its._cv_sizes(prob, ids, sizes)             # a weighted handle: the weight sums; a zero-weight fold raises here
    prms = _its._path_params(prob, alphas, L, fam, t_init_factor, delta, tol_ratio=tol_ratio, adaptive_restart=adaptive_restart,
                             restart_threshold=restart_threshold)
    out = _its._run_cv(prob, ids, len(sizes), prms, fam, max_iter)
    if out is None:
        raise _its._refused(prob, "fos_fista_run_multi_folds refused the lockstep: ")
    X, total, info = out
    return _its._cv_result(result, prob.like, alphas, total, sizes,
                           (lambda best: _its._refit(prob, prms[best], fam, max_iter)) if refit else None,
                           X if return_coefs else None, info)


def _objective(prob, x, alpha1, alpha2, who, own):
    if prob.has_feature_groups:      # the separable penalty would answer for another objective
        raise ValueError(f"{who}: the handle has feature groups (Problem.set_feature_groups); the data term alone is "
                         f"Problem.residual_batch, the group penalty the caller's ({own})")
    X, single = _its._objective_block(prob, x, 1)
    return _its._objective_value(prob, X, single, lambda block, number: prob.residual_batch(block, use_b=True), alpha1, alpha2)


def huber_path(A, b, alphas, threshold=None, t_init_factor: float = 1.0, max_iter: int = 500, *, delta=None, L=None, dtype=None,
               tol_ratio: float = 0.0, adaptive_restart: bool = False, restart_threshold: float = 1.0,
               return_info: bool = False):
    """Sparse Huber regression of ``b`` on A for several weights at once.

    ``alphas`` is a sequence of ``(alpha1, alpha2)`` pairs; the result is the list of solutions, one per pair, and with
    ``return_info=True`` also ``[(iterations, stop_code), ...]``.  The pairs advance in lockstep groups of up to 16 columns on
    the matrix cores (fos_fista_run_multi on a Huber problem): two GEMM-shaped products and the pointwise link per iteration
    for the whole group; a single pair is a one-column lockstep.

    ``threshold`` is Huber's c > 0: required unless ``A`` is a ``prepare_huber`` handle (``b`` may then be None), and a
    ValueError if given and different from the handle's.  ``L``, when not given, is ``estimate_lipschitz(A)`` (one power
    iteration, one draw from the global NumPy stream, like ``fista_path``): |psi'| <= 1.  The step is ``t_init_factor / (L +
    alpha2 max_j p_j)``.

    Contract: each result is FISTA (FISTA-Δ with ``delta`` > 2) on the Huber objective from x0 = 0 with that step, under the
    momentum, restart (``adaptive_restart`` / ``restart_threshold``) and ratio-stop (``tol_ratio``) rules of the reference's
    loop, decided per column on the device.  There is no ``tol`` (the gradient-norm rule), no backtracking and no sharding.
    With ``threshold`` above every |residual| the iterates are those of the squared loss."""
    _its.reset_metrics()
    alphas = _its._check_path_args(alphas, delta)
    return _path(_huber_problem(A, b, threshold, dtype), alphas, t_init_factor, max_iter, delta, L, tol_ratio, adaptive_restart,
                 restart_threshold, return_info)


def huber_cv(A, b, alphas, folds=5, threshold=None, t_init_factor: float = 1.0, max_iter: int = 500, *, delta=None, L=None,
             dtype=None, tol_ratio: float = 0.0, adaptive_restart: bool = False, restart_threshold: float = 1.0,
             refit: bool = True, return_coefs: bool = False):
    """K-fold cross-validation of a Huber regularisation path: ``fista_cv`` with the Huber loss.

    ``folds`` as in ``fista_cv``, validated before any device work.  All K x L fits are masked columns of the lockstep on the
    one device copy of A (fos_fista_run_multi_folds on a Huber problem); the held-out losses of a group come from one further
    pass with the complementary mask.  ``L`` comes from the whole A and is valid for every training set.  Contract:
    ``coefs[:, f, a]`` is what ``huber_path(A[train_f], b[train_f], [alphas[a]], threshold, ..., L=L)`` returns.

    Returns ``HuberCVResult(alphas, loss, mean_loss, best, x, coefs, info)``: ``loss[f, a]`` the held-out MEAN Huber loss (the
    weighted mean on a weighted handle; K x L float64 ndarray), ``mean_loss`` its mean over the folds, ``best`` the argmin
    (first on ties), ``x`` the fit on all rows at ``alphas[best]`` (``refit=True``; else None), ``coefs`` the n x K x L fits
    (``return_coefs=True``; else None), ``info[f][a] = (iterations, stop_code)``."""
    _its.reset_metrics()
    alphas = _its._check_path_args(alphas, delta)
    ids, sizes = _its._cv_folds(folds, _its._rows(A))
    return _cv(HuberCVResult, _huber_problem(A, b, threshold, dtype), alphas, ids, sizes, t_init_factor, max_iter, delta, L,
               tol_ratio, adaptive_restart, restart_threshold, refit, return_coefs)


def huber_objective(x, A, b, alpha1, alpha2, threshold=None):
    """sum_i w_i rho_c(a_i.x - b_i) + alpha1 ||x||_1 + 0.5 alpha2 ||x||^2 with the data term from the device (fos_residual_batch
    on a Huber problem; x is rounded to fp32 for the pass over A).  ``x``: a vector (returns a float) or an n x k block (returns
    k float64 values), 16 columns per pass.  ``threshold`` as in ``huber_path``.  On a handle with penalty factors the
    penalties are the factored ones.  Synchronises."""
    return _objective(_huber_problem(A, b, threshold, None), x, alpha1, alpha2, "huber_objective", "huber")


def hinge_path(A, y, alphas, t_init_factor: float = 1.0, max_iter: int = 500, *, delta=None, L=None, dtype=None,
               tol_ratio: float = 0.0, adaptive_restart: bool = False, restart_threshold: float = 1.0,
               return_info: bool = False):
    """The sparse squared-hinge classifier of the labels ``y`` (exactly -1 or +1; checked on the host) on A for several weights
    at once: ``huber_path`` with the squared hinge, sum_i w_i max(0, 1 - y_i a_i.x)^2 / 2, in place of the Huber loss and no
    threshold.  A: an array / tensor or a ``prepare_hinge(A, y)`` handle (``y`` may then be None)."""
    _its.reset_metrics()
    alphas = _its._check_path_args(alphas, delta)
    return _path(_hinge_problem(A, y, dtype), alphas, t_init_factor, max_iter, delta, L, tol_ratio, adaptive_restart,
                 restart_threshold, return_info)


def hinge_cv(A, y, alphas, folds=5, t_init_factor: float = 1.0, max_iter: int = 500, *, delta=None, L=None, dtype=None,
             tol_ratio: float = 0.0, adaptive_restart: bool = False, restart_threshold: float = 1.0, refit: bool = True,
             return_coefs: bool = False):
    """K-fold cross-validation of a squared-hinge regularisation path: ``huber_cv`` with the squared hinge.  Returns
    ``HingeCVResult(alphas, loss, mean_loss, best, x, coefs, info)`` with ``loss[f, a]`` the held-out MEAN squared-hinge loss
    (its 1/2 included; the weighted mean on a weighted handle)."""
    _its.reset_metrics()
    alphas = _its._check_path_args(alphas, delta)
    ids, sizes = _its._cv_folds(folds, _its._rows(A))
    return _cv(HingeCVResult, _hinge_problem(A, y, dtype), alphas, ids, sizes, t_init_factor, max_iter, delta, L, tol_ratio,
               adaptive_restart, restart_threshold, refit, return_coefs)


def hinge_objective(x, A, y, alpha1, alpha2):
    """sum_i w_i max(0, 1 - y_i a_i.x)^2 / 2 + alpha1 ||x||_1 + 0.5 alpha2 ||x||^2 with the data term from the device
    (fos_residual_batch on a squared-hinge problem), as ``huber_objective``."""
    return _objective(_hinge_problem(A, y, None), x, alpha1, alpha2, "hinge_objective", "squared hinge")
