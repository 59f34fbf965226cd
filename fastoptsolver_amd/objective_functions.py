"""MI355X drop-in for the reference's ``objective_functions.py`` (one residual pass over A, kernel K5)."""
from . import _core
from .iterative_solvers import _objective_by_reg, _targets
from .operators import vec_stats


def compute_objective(x, A, b, reg_type, alpha1, alpha2):
    """f(x) = ½‖Ax−b‖² (+ ½α₂‖x‖² for ridge/elasticnet) (+ α₁‖x‖₁ for lasso/elasticnet).
    objective_functions.py:3-30; ValueError for any other reg_type (:28).
    Several targets: with x of shape (n, k) and b of shape (m, k), k >= 2, the sum over the columns (½‖AX−B‖²_F plus the
    regulariser of X): 16 residual norms per pass over A on the matrix cores where the shape has that pass."""
    value = _objective_by_reg(reg_type, alpha1, alpha2)
    if _targets(A, b) is not None:
        return _objective_targets(x, A, b, value)
    prob = _core.as_problem(A, b)
    xt = _core.to_device_vec(x, prob.device)
    return value(*prob.residual_objective(xt))


def _objective_targets(X, A, B, value):
    prob = _core.prepare(A)
    Bt, Xt = _core.to_device(B, prob.device), _core.to_device(X, prob.device)
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
            total += value(rr, x2, x1)
    return total
