"""MI355X drop-in for the reference's ``objective_functions.py`` (one residual pass over A, kernel K5)."""
import numpy as np
import torch

from . import _core


def compute_objective(x, A, b, reg_type, alpha1, alpha2):
    """f(x) = ½‖Ax−b‖² (+ ½α₂‖x‖² for ridge/elasticnet) (+ α₁‖x‖₁ for lasso/elasticnet).
    objective_functions.py:3-30; ValueError for any other reg_type (:28).
    Several targets: with x of shape (n, k) and b of shape (m, k), k >= 2, the sum over the columns (½‖AX−B‖²_F plus the
    regulariser of X): 16 residual norms per pass over A on the matrix cores where the shape has that pass."""
    if reg_type not in ("lasso", "ridge", "elasticnet"):
        raise ValueError(f"Unsupported reg_type='{reg_type}'")
    from .iterative_solvers import _targets
    if _targets(A, b) is not None:
        return _objective_targets(x, A, b, reg_type, alpha1, alpha2)
    prob = _core.as_problem(A, b)
    xt = _core.to_device_vec(x, prob.device)
    rr, x2, x1 = prob.residual_objective(xt)
    return _value(reg_type, alpha1, alpha2, rr, x2, x1)


def _value(reg_type, alpha1, alpha2, rr, x2, x1):
    g = 0.5 * rr
    if reg_type in ("ridge", "elasticnet"):
        g += 0.5 * alpha2 * x2
    h = alpha1 * x1 if reg_type in ("lasso", "elasticnet") else 0.0
    return g + h


def _as_device_block(M, device):
    t = M.detach() if _core.is_tensor(M) else torch.from_numpy(np.ascontiguousarray(np.asarray(M)))
    return t.to(device=device, dtype=torch.float32).contiguous()


def _objective_targets(X, A, B, reg_type, alpha1, alpha2):
    from .operators import vec_stats
    prob = _core.prepare(A)
    Bt, Xt = _as_device_block(B, prob.device), _as_device_block(X, prob.device)
    k = int(Bt.shape[1])
    if Bt.shape[0] != prob.m:
        raise ValueError("b must have m rows")
    if Xt.dim() != 2 or tuple(Xt.shape) != (prob.n, k):
        raise ValueError(f"x must have shape ({prob.n}, {k}) for a b with {k} columns")
    total = 0.0
    for g0 in range(0, k, 16):
        g1 = min(k, g0 + 16)
        rrs = prob.residual_batch_rhs(Xt[:, g0:g1], Bt[:, g0:g1]) if g1 - g0 >= 2 else None
        for i, j in enumerate(range(g0, g1)):
            xj = Xt[:, j].contiguous()
            if rrs is None:                      # no matrix-core pass for this shape: one residual pass per column
                rr, x2, x1 = prob.sibling(Bt[:, j].contiguous()).residual_objective(xj)
            else:
                st = vec_stats(xj, None, None)
                rr, x2, x1 = rrs[i], st[0], st[4]
            total += _value(reg_type, alpha1, alpha2, rr, x2, x1)
    return total
