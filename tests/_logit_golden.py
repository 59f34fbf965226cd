"""The squared-loss calls whose results tests/golden/logit_parent.npz records from the commit before the logistic loss (a
helper: no tests in here).  tests/test_gpu_logit_guard.py repeats them and compares bitwise: adding the loss to the problem
handle and the LOSS flag to product 1 changed no squared-loss result."""
import numpy as np

from tests import _data

M, N, SEED, ITERS, K = 1001, 200, 4242, 30, 5


def inputs():
    A, b, _ = _data.synth(M, N, SEED)
    A32 = A.astype(np.float32)
    b = b.astype(np.float32).astype(np.float64)
    amax = float(np.max(np.abs(A32.astype(np.float64).T @ b)))
    alphas = [(0.3 * amax, 0.0), (0.1 * amax, 0.5), (0.03 * amax, 0.0), (0.2 * amax, 0.0), (0.05 * amax, 1.0)]
    L = 1.05 * float(np.linalg.norm(A32.astype(np.float64), 2) ** 2)      # a fixed, valid constant: no power iteration involved
    return A32, b, alphas, L


def compute(fos, torch):
    """{name: float64 ndarray} of one fp32 and one bf16 fista_path and fista_cv call."""
    A32, b, alphas, L = inputs()
    out = {}
    for kind, tdtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        At = torch.as_tensor(A32).to(tdtype).cuda()
        xs = fos.fista_path(At, b, alphas, max_iter=ITERS, L=L)                       # five weights: the matrix-core lockstep
        out[f"path_{kind}"] = np.stack([x.detach().cpu().numpy().astype(np.float64) for x in xs], axis=1)
        xs = fos.fista_path(At, b, alphas[:3], max_iter=ITERS, L=L, adaptive_restart=True, tol_ratio=1e-3)
        out[f"path_ctrl_{kind}"] = np.stack([x.detach().cpu().numpy().astype(np.float64) for x in xs], axis=1)
        res = fos.fista_cv(At, b, alphas[:3], K, max_iter=ITERS, L=L, return_coefs=True)
        out[f"cv_coefs_{kind}"] = res.coefs.detach().cpu().numpy().astype(np.float64)
        out[f"cv_mse_{kind}"] = np.asarray(res.mse, dtype=np.float64)
        out[f"cv_x_{kind}"] = res.x.detach().cpu().numpy().astype(np.float64)
    return out
