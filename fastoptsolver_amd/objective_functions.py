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


def group_lasso_objective(x, A, b, alpha1, alpha2, groups, group_weight=None, l1_ratio=0.0, *, loss="squared", sample_weight=None):
    """data term + alpha1 [(1 - l1_ratio) sum_g w_g ||x_g||_2 + l1_ratio ||x||_1] + 0.5 alpha2 ||x||_2^2 in fp64 on the host:
    the objective of a handle with feature groups (``prepare_grouped``).  The data term is sum_i w_i 0.5 (a_i.x - b_i)^2 or
    (``loss="logistic"``) sum_i w_i (log(1 + e^{a_i.x}) - b_i a_i.x), w = ``sample_weight`` (None: 1).  ``groups`` /
    ``group_weight`` / ``l1_ratio`` as ``prepare_grouped`` takes them.  A: an array / tensor, or a handle - its stored A (bf16
    storage: the rounded values), its b, loss and weights are then used where the arguments are None / default.  ``x``: a vector
    (returns a float) or an n x k block (returns k float64 values).  No device work on arrays."""
    import numpy as np
    import torch

    def host(v):
        if v is None:
            return None
        return (v.detach().to("cpu", torch.float64).numpy() if _core.is_tensor(v) else np.asarray(v, dtype=np.float64))
    if isinstance(A, _core.Problem):
        prob = A
        A = prob.A[:, : prob.n]
        b = prob.b if b is None else b
        loss = prob.loss if loss == "squared" else loss
        sample_weight = prob.sample_weight if sample_weight is None else sample_weight
    if loss not in ("squared", "logistic"):
        raise ValueError(f'loss: "squared" or "logistic" expected, got {loss!r}')
    Ah, bh, wh, xh = host(A), host(b), host(sample_weight), host(x)
    if Ah.ndim != 2 or bh is None or bh.shape != (Ah.shape[0],):
        raise ValueError("A must be 2-D and b must have m entries")
    n = Ah.shape[1]
    vector = xh.ndim == 1
    X = xh.reshape(n, 1) if vector else xh
    if X.ndim != 2 or X.shape[0] != n:
        raise ValueError(f"x: a vector of length {n} or an {n} x k block expected")
    start, w, mix = _core.checked_feature_groups(groups, group_weight, l1_ratio, n)
    rw = np.ones(Ah.shape[0]) if wh is None else wh
    Z = Ah @ X
    if loss == "squared":
        data = 0.5 * (rw[:, None] * (Z - bh[:, None]) ** 2).sum(axis=0)
    else:
        data = (rw[:, None] * (np.logaddexp(0.0, Z) - bh[:, None] * Z)).sum(axis=0)
    norms = np.sqrt(np.add.reduceat(X * X, start[:-1], axis=0))          # ngroups x k
    val = (data + float(alpha1) * ((1.0 - mix) * (w[:, None] * norms).sum(axis=0) + mix * np.abs(X).sum(axis=0)) +
           0.5 * float(alpha2) * (X * X).sum(axis=0))
    return float(val[0]) if vector else val
