"""Multi-task lasso / elastic net on the matrix-core lockstep (extension; scikit-learn's MultiTaskLasso / MultiTaskElasticNet,
glmnet's mgaussian): T targets share one support.

    minimise over X (n x T)   0.5 ||A X - B||_F^2  +  alpha1 sum_j p_j ||X[j, :]||_2  +  0.5 alpha2 sum_j p_j ||X[j, :]||_2^2

``fista(A, B)`` with a 2-D B runs T independent lassos in one pass over A; here the T columns of a fit are coupled by the group
penalty: every handle carries ``group = T`` (fos_fista_params.group), the T targets are T adjacent columns of the 16-column
lockstep with their own right-hand sides (fos_fista_run_multi_rhs), and the update kernel thresholds row j of X across the T
columns together (csrc/reduce_update.hpp, fista_update_group_kernel).  floor(16 / T) weight pairs advance per call, each reading
A twice per iteration whatever T is.  p: the penalty factors of a ``prepare_penalized`` handle (else 1).

Not served, by design: cross-validation of the multi-task model (the fold-masked product 1 has no right-hand-side-block form),
sparse-group mixtures (an additional l1 term), groups of coefficients within one column, sharded problems, row weights and box
bounds (group norm plus box has no composed closed-form prox).
"""
from __future__ import annotations

import numpy as np

from . import _core
from . import iterative_solvers as _its
from .iterative_solvers import pack_groups        # (public here: the packing of the target groups)

__all__ = ["multitask_path", "multitask_objective", "pack_groups", "tile_targets"]


def tile_targets(B, number):
    """The right-hand-side block of one lockstep call: B (m x T) once per weight pair, m x (number * T), so that column
    i * T + t is target t of pair i.  Pure (an ndarray gives an ndarray, a tensor a tensor on its device)."""
    if number < 1:
        raise ValueError("number must be >= 1")
    if _core.is_tensor(B):
        return B.repeat(1, number).contiguous()
    return np.tile(np.asarray(B), (1, number))


def _check_targets(B, m=None):
    """B is m x T with 2 <= T <= 16: T (checked on the host, before any device work)."""
    shape = tuple(B.shape) if hasattr(B, "shape") else np.shape(B)
    if len(shape) != 2:
        raise ValueError(f"B: an m x T matrix of targets expected, got shape {shape}")
    T = int(shape[1])
    if not 2 <= T <= _core.MAX_CLASSES:
        raise ValueError(f"B: 2 <= T <= {_core.MAX_CLASSES} targets expected, got {T} (one target is fista / fista_path)")
    if m is not None and int(shape[0]) != m:
        raise ValueError(f"B must have m = {m} rows, got {shape[0]}")
    return T


def _problem(A, dtype):
    """The squared-loss handle on A: a prepared one as it is (penalty factors allowed; row weights and box bounds refused),
    anything else bound here with rows padded to the matrix-core pair's granularity."""
    if isinstance(A, _core.Problem):
        _core.refuse_link(A, "multitask_path / multitask_objective")
        if A.loss != "squared":
            raise ValueError(f"A was prepared for the {A.loss} loss: the multi-task model has the squared loss")
        if A.sample_weight is not None:
            raise ValueError("the multi-task lockstep does not serve row weights")
        if A.lower is not None or A.upper is not None:
            raise ValueError("the group penalty does not compose with box bounds (lower / upper); penalty factors do")
        if getattr(A, "comm", None) is not None:
            raise ValueError("the multi-task lockstep does not serve sharded problems")
        if A.has_feature_groups:
            raise ValueError("the multi-task lockstep does not serve feature groups (Problem.set_feature_groups): the two group "
                             "norms do not compose")
        return A
    return _core.Problem(A, None, dtype, True)


def _data_handle(prob):
    """The handle whose fos_residual_batch_rhs answers for the data term: the problem itself, or - penalty factors bound, which
    that entry point refuses although the data term does not depend on them - a bare handle borrowing the same device A."""
    return _core.Problem(prob.A, None) if prob.has_coord else prob


def multitask_path(A, B, alphas, t_init_factor: float = 1.0, max_iter: int = 500, *, delta=None, L=None, dtype=None,
                   return_info: bool = False):
    """Multi-task lasso / elastic net of the T targets ``B`` (m x T, 2 <= T <= 16) on A for several weights at once.

    ``alphas`` is a sequence of ``(alpha1, alpha2)`` pairs; the result is the list of n x T solutions, one per pair (column t
    the coefficients of target t; row j is zero for all targets or for none), and with ``return_info=True`` also
    ``[(iterations, stop_code), ...]``.  floor(16 / T) pairs advance per lockstep call (``pack_groups(count, T)``); the
    right-hand-side block of a call is B tiled once per pair (``tile_targets``).

    ``L``, when not given, is ``estimate_lipschitz(A)`` (one power iteration, one draw from the global NumPy stream).  The step
    is ``t_init_factor / (L + alpha2 max_j p_j)``.

    Contract: each result is FISTA (FISTA-Δ with ``delta`` > 2) on 0.5 ||A X - B||_F^2 + the group penalty of the module
    docstring from X0 = 0 with that step for exactly ``max_iter`` iterations.  No stopping rule and no momentum restart: the
    columns of a fit are one joint problem.  A: an array / tensor, or a prepared squared-loss handle (``prepare``, or
    ``prepare_penalized`` with factors only; its own b is not used).  The shape needs the matrix-core pair (more than 64 and at
    most 16384 device columns); anything else raises FosError.  Out of scope: cross-validation, sparse-group mixtures, groups
    within one column, sharded problems (module docstring)."""
    _its.reset_metrics()
    alphas = _its._check_path_args(alphas, delta)
    T = _check_targets(B, _its._rows(A))
    prob = _problem(A, dtype)
    L_val = _its._lipschitz(prob, L)                     # (estimated before B goes to the device)
    Bfull = tile_targets(_core.to_device(B, prob.device), pack_groups(len(alphas), T)[0][1])
    fam = _its._Family(T, T, 1.0, lambda handles, first, number: _core.run_multi_rhs(handles, Bfull[:, :number * T], max_iter),
                       "fos_fista_run_multi_rhs refused the multi-task lockstep: ")
    prms = _its._path_params(prob, alphas, L_val, fam, t_init_factor, delta)
    return _its._path_result(_its._run_path(prob, prms, fam, max_iter), fam, prob.like, return_info)


def multitask_objective(X, A, B, alpha1, alpha2):
    """0.5 ||A X - B||_F^2 + alpha1 sum_j p_j ||X[j, :]||_2 + 0.5 alpha2 sum_j p_j ||X[j, :]||_2^2 with the data term from the
    device (fos_residual_batch_rhs; X is rounded to fp32 for the pass over A).  ``X``: n x T (returns a float) or an n x T x k
    block (returns k float64 values), floor(16 / T) members per pass.  p: the fp32 penalty factors of the handle as bound
    (else 1).  Synchronises."""
    T = _check_targets(B, _its._rows(A))
    prob = _problem(A, None)
    Xd, single = _its._objective_block(prob, X, T)
    data = _data_handle(prob)
    Bfull = tile_targets(_core.to_device(B, prob.device), pack_groups(Xd.shape[2], T)[0][1])

    def half_squares(block, number):
        q = data.residual_batch_rhs(block, Bfull[:, :number * T])
        if q is None:
            raise _its._refused(prob, "fos_residual_batch_rhs does not serve this shape: ")
        return (0.5 * np.asarray(q, dtype=np.float64).reshape(number, T).sum(axis=1)).tolist()
    return _its._objective_value(prob, Xd, single, half_squares, alpha1, alpha2, row_groups=True)
