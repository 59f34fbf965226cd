"""The public path / CV calls whose results tests/golden/front_end_parent.npz records from the commit before the four model
families got one host driver (a helper: no tests in here).  tests/test_gpu_front_end_guard.py repeats them and compares bitwise.

compute(): each of fista_path / fista_cv, logistic_path / logistic_cv, multinomial_path / multinomial_cv and multitask_path
once per handle kind it accepts, on the 1001 x 200 recipe of tests/_logit_golden.py (rows padded, the last 64-column update
workgroup partial) with the derived inputs of tests/_lockstep_golden.inputs(), fp32 and bf16 storage, 30 iterations, L given:
5 weights per path, 3 folds x 3 weights per CV.  A goes in as an ndarray, so every result comes back as float64."""
import numpy as np

from tests import _lockstep_golden as base

M, N, ITERS, FOLDS = base.M, base.N, base.ITERS, 3
SCALES = ((0.3, 0.0), (0.1, 0.5), (0.03, 0.0), (0.2, 0.0), (0.05, 1.0))     # (alpha1 / max |gradient at 0|, alpha2)


def _alphas(amax):
    return [(s * amax, a2) for s, a2 in SCALES]


def _path(out, name, xs, info):
    out[name + "/x"] = np.stack([np.asarray(x) for x in xs], axis=-1)
    out[name + "/info"] = np.asarray(info, dtype=np.int64)


def _cv(out, name, res):
    out[name + "/score"] = np.asarray(res[1])
    out[name + "/best"] = np.asarray(res.best, dtype=np.int64)
    out[name + "/x"] = np.asarray(res.x)
    out[name + "/info"] = np.asarray(res.info, dtype=np.int64)


def compute(fos):
    """{name: ndarray}: x and info of every path call; the held-out scores, best, x and info of every CV call."""
    d = base.inputs()
    A, L, folds = d["A"], d["L"], np.arange(M) % FOLDS
    groups = list(base.FGROUP_SIZES)
    Bt = d["B"][:, :3]
    amax_task = float(np.max(np.linalg.norm(A.astype(np.float64).T @ Bt.astype(np.float64), axis=1)))
    out = {}
    for kind in ("f32", "bf16"):
        dt = None if kind == "f32" else "bf16"
        for fam, t, amax, path, cv in (("squared", d["b"], d["amax"], fos.fista_path, fos.fista_cv),
                                       ("logistic", d["y"], d["amax_logit"], fos.logistic_path, fos.logistic_cv)):
            handles = {"plain": fos.prepare(A, t, dt, loss=fam),
                       "weighted": fos.prepare_weighted(A, t, d["w"], dt, loss=fam),
                       "penalised": fos.prepare_penalized(A, t, d["p"], d["lo"], d["hi"], dt, loss=fam),
                       "fgroups": fos.prepare_grouped(A, t, groups, None, 0.5, dt, loss=fam)}
            for tag, P in handles.items():
                _path(out, f"{kind}/{fam}_path_{tag}", *path(P, None, _alphas(amax), max_iter=ITERS, L=L, return_info=True))
                _cv(out, f"{kind}/{fam}_cv_{tag}", cv(P, None, _alphas(amax)[:3], folds, max_iter=ITERS, L=L))
        for tag, grouped in (("plain", False), ("grouped", True)):
            P = fos.prepare_multinomial(A, d["cls"], 3, dt, grouped=grouped)
            _path(out, f"{kind}/multinomial_path_{tag}",
                  *fos.multinomial_path(P, None, _alphas(d["amax_soft"]), max_iter=ITERS, L=L, return_info=True))
            _cv(out, f"{kind}/multinomial_cv_{tag}", fos.multinomial_cv(P, None, _alphas(d["amax_soft"])[:3], folds, max_iter=ITERS, L=L))
        for tag, P in (("plain", A), ("factors", fos.prepare_penalized(A, d["b"], d["p"], dtype=dt))):
            _path(out, f"{kind}/multitask_path_{tag}",
                  *fos.multitask_path(P, Bt, _alphas(amax_task), max_iter=ITERS, L=L, dtype=dt, return_info=True))
    return out
