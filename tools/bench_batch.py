"""Batches of small problems: one batched fista call (one workgroup per problem, fos_fista_run_batch) against the loop of
single calls on the same inputs, and fista(A, B) on a 1000 x 5 A with 16 targets as one batch against the column-by-column
fallback it replaced.

    python tools/bench_batch.py [--out FILE] [--sizes 1,16,80,256,1024] [--reps 3]

P standardised Boston-like problems (generate_correlated_boston_like_data, 1000 x 5, distinct seeds); fista lasso and
elasticnet, 500 iterations, tol = 1e-6, fixed step and Armijo with t_init 2.0.  Times are synchronised wall times of the
whole call (power iteration included), the best of --reps.  One JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastoptsolver_amd as fos                                          # noqa: E402
from fastoptsolver_amd.easy_boston_data import generate_correlated_boston_like_data   # noqa: E402


def problems(P):
    A, b = [], []
    for s in range(P):
        a, y, _ = generate_correlated_boston_like_data(m=1000, seed=1000 + s)
        a = (a - a.mean(0)) / a.std(0)
        A.append(a.astype(np.float32))
        b.append((y - y.mean()).astype(np.float32))
    return np.stack(A), np.stack(b)


def timed(fn, reps):
    best, out = float("inf"), None
    for _ in range(reps):
        torch.cuda.synchronize()
        np.random.seed(0)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,80,256,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    A, b = problems(max(int(v) for v in a.sizes.split(",")))
    fos.fista(A[:2], b[:2], "lasso", 0.1, 0.0, max_iter=5)                     # warm-up (library, allocator)
    for P in (int(v) for v in a.sizes.split(",")):
        for reg, a2 in (("lasso", 0.0), ("elasticnet", 0.1)):
            for bt in (False, True):
                kw = dict(max_iter=500, tol=1e-6, backtracking=bt, t_init_factor=2.0 if bt else 1.0)
                t_b, X = timed(lambda: fos.fista(A[:P], b[:P], reg, 0.1, a2, **kw), a.reps)
                loop_reps = a.reps if P <= 80 else 1
                t_l, Xs = timed(lambda: [fos.fista(A[i], b[i], reg, 0.1, a2, **kw) for i in range(P)], loop_reps)
                diff = max(float(np.max(np.abs(X[i] - Xs[i]))) for i in range(P))
                emit(dict(case="batch", P=P, reg=reg, backtracking=bt, batch_s=t_b, loop_s=t_l, speedup=t_l / t_b,
                          max_abs_diff=diff))
    # several targets on a resident A: one batch (now) against the column-by-column fallback (before)
    A1, B = A[0], b[:16].T.copy()
    for bt in (False, True):
        kw = dict(max_iter=500, tol=1e-6, backtracking=bt, t_init_factor=2.0 if bt else 1.0)
        t_new, X = timed(lambda: fos.fista(A1, B, "lasso", 0.1, 0.0, **kw), a.reps)

        def columns():                           # what the fallback ran: L once, then one single-target solve per column
            prob = fos.prepare(A1)
            L = fos.estimate_lipschitz(prob)
            return np.stack([fos.fista(A1, B[:, j], "lasso", 0.1, 0.0, L=L, **kw) for j in range(B.shape[1])], axis=1)
        t_old, Xo = timed(columns, a.reps)
        emit(dict(case="targets_1000x5_k16", backtracking=bt, batch_s=t_new, column_by_column_s=t_old,
                  speedup=t_old / t_new, max_abs_diff=float(np.max(np.abs(X - Xo)))))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
