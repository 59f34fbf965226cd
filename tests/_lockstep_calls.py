"""The calls the seven path / CV front ends make into the lockstep, recorded without a GPU (a helper: no tests in here).
tests/golden/lockstep_calls.json holds run() from the commit before the four model families got one host driver;
tests/test_lockstep_calls.py repeats it and compares for equality: no launch, launch order, parameter, result, message or metric
count changed.

install() puts stand-ins in place of what the front ends reach at call time - _core.Fista, the three _core.run_multi*
launches, _core.fold_ids_tensor, iterative_solvers._EventTimer and _cv_fold_by_fold - and problem() is a _core.Problem that
touches no device.  Handle i (in creation order) answers x = i everywhere and the status (k = 7, stopped = 0), so the results
show which handle became which output; every launch is logged with the full parameter set of each handle."""
import types

import numpy as np
import torch

import fastoptsolver_amd as fos
from fastoptsolver_amd import _core, iterative_solvers as its

M, N, ITERS, K_DONE, L = 37, 9, 11, 7, 4.0
REFUSAL = b"scripted refusal"


def alphas(count):
    return [(2.0 ** -i, 0.5 * (i % 2)) for i in range(count)]


class _Problem(_core.Problem):
    def __init__(self, log, loss, classes, weighted, grouped, factors, scores):
        self.m, self.n, self.n_dev, self.loss, self.classes, self.grouped = M, N, N + 3, loss, classes, grouped
        self.device, self.dtype, self.like = torch.device("cpu"), "f32", _core.Like(np.zeros(1))
        self.penalty_max = 2.0 if factors else 1.0
        self._coord = (torch.full((N + 3,), 2.0) if factors else None, None, None)
        self.sample_weight = torch.full((M,), 0.5) if weighted else None
        self.b = torch.zeros(M)
        self.lib = types.SimpleNamespace(fos_last_error=lambda: REFUSAL)
        self._log, self._scores = log, scores

    def residual_batch_folds(self, X, fold_ids, held):
        self._log.append(["residual_batch_folds", list(X.shape), X[0].tolist(), list(fold_ids.shape), list(held)])
        return [float(j + 1) for j in range(X.shape[1])] if self._scores else None


def install(monkeypatch, served=()):
    """The stand-ins; `served`: the answers of the launches in order (True once they run out).  (log, problem factory)."""
    log, answers, created = [], list(served), []

    class Fista:
        def __init__(self, prob):
            self.prob, self.lib, self.index, self.prm = prob, prob.lib, len(created), None
            created.append(self)

        def reset(self, tau, alpha1, alpha2, mode=0, prox_kind=0, delta=0.0, adaptive_restart=False, restart_threshold=1.0,
                  tol_step=0.0, tol_ratio=0.0, tol_grad=0.0, x0=None, group=0):
            self.prm = dict(tau=tau, alpha1=alpha1, alpha2=alpha2, mode=mode, prox_kind=prox_kind, delta=delta,
                            adaptive_restart=adaptive_restart, restart_threshold=restart_threshold, tol_step=tol_step,
                            tol_ratio=tol_ratio, tol_grad=tol_grad, x0=x0, group=group)

        def run(self, iters):
            log.append(["run", iters, [self.index, self.prm]])

        def status(self):
            return types.SimpleNamespace(k=K_DONE, restarts=0, stopped=0)

        def x_tensor(self):
            return torch.full((self.prob.n,), float(self.index), dtype=torch.float64)

    def launch(entry, handles, iters, *more):
        log.append([entry, iters, [[st.index, st.prm] for st in handles], *more])
        return answers.pop(0) if answers else True

    class Timer:
        def __init__(self, sink):
            assert sink is its.grad_call_times
            self.sink, self.counts = sink, []

        def start(self):
            return None

        def stop(self, ev0, count=1):
            self.counts.append(count)

        def recount(self, count):
            self.counts[-1] = count

        def flush(self):
            log.append(["flush", list(self.counts)])
            self.sink.extend([0.0] * sum(self.counts))
            self.counts = []

    def fold_ids_tensor(ids, device):
        log.append(["fold_ids_tensor", np.asarray(ids).tolist(), str(device)])
        return torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint8))

    def fold_by_fold(prob, ids, K, prms, max_iter):
        log.append(["cv_fold_by_fold", K, prms, max_iter])
        X = torch.zeros(prob.n, K, len(prms), dtype=torch.float64)
        return X, np.ones((K, len(prms))), [[(max_iter, 0)] * len(prms) for _ in range(K)]

    monkeypatch.setattr(_core, "Fista", Fista)
    monkeypatch.setattr(_core, "run_multi", lambda hs, iters: launch("run_multi", hs, iters))
    monkeypatch.setattr(_core, "run_multi_rhs", lambda hs, B, iters: launch("run_multi_rhs", hs, iters, list(B.shape), B[0].tolist()))
    monkeypatch.setattr(_core, "run_multi_folds",
                        lambda hs, ids, held, iters: launch("run_multi_folds", hs, iters, list(ids.shape), list(held)))
    monkeypatch.setattr(_core, "fold_ids_tensor", fold_ids_tensor)
    monkeypatch.setattr(its, "_EventTimer", Timer)
    monkeypatch.setattr(its, "_cv_fold_by_fold", fold_by_fold)

    def problem(loss="squared", classes=None, weighted=False, grouped=False, factors=False, scores=True):
        return _Problem(log, loss, classes, weighted, grouped, factors, scores)
    return log, problem


def _plain(v):
    """v as JSON holds it: ndarrays and tuples as lists, a CV result as a dict."""
    if hasattr(v, "_asdict"):
        return {k: _plain(x) for k, x in v._asdict().items()}
    if isinstance(v, (np.ndarray, torch.Tensor)):
        return v.tolist()
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v.item() if isinstance(v, np.generic) else v


def _squared(P):
    return P()


def _weighted(P):
    return P(weighted=True)


def _logit(P):
    return P("logistic")


def _wlogit(P):
    return P("logistic", weighted=True)


def _soft(classes, **kw):
    return lambda P: P("multinomial", classes, **kw)


B3 = np.arange(M * 3, dtype=np.float32).reshape(M, 3)
KW = dict(max_iter=ITERS, L=L)

# name: (handle, call(fos, handle), the launches' answers)
SCENARIOS = {
    "fista_path/plain_3": (_squared, lambda P: fos.fista_path(P, None, alphas(3), return_info=True, **KW), ()),
    "fista_path/plain_7": (_squared, lambda P: fos.fista_path(P, None, alphas(7), return_info=True, **KW), ()),
    "fista_path/plain_7_refused": (_squared, lambda P: fos.fista_path(P, None, alphas(7), return_info=True, **KW), (False,)),
    "fista_path/plain_1": (_squared, lambda P: fos.fista_path(P, None, alphas(1), **KW), ()),
    "fista_path/plain_20_tol": (_squared, lambda P: fos.fista_path(P, None, alphas(20), tol=0.25, tol_ratio=0.5,
                                                                     adaptive_restart=True, restart_threshold=0.75, **KW), ()),
    "fista_path/weighted_1": (_weighted, lambda P: fos.fista_path(P, None, alphas(1), return_info=True, **KW), ()),
    "fista_path/weighted_7": (_weighted, lambda P: fos.fista_path(P, None, alphas(7), return_info=True, **KW), ()),
    "fista_path/weighted_20": (_weighted, lambda P: fos.fista_path(P, None, alphas(20), **KW), ()),
    "fista_path/factors_3": (lambda P: P(factors=True), lambda P: fos.fista_path(P, None, alphas(3), **KW), ()),
    "fista_path/weighted_refused": (_weighted, lambda P: fos.fista_path(P, None, alphas(7), **KW), (False,)),
    "fista_path/weighted_tol": (_weighted, lambda P: fos.fista_path(P, None, alphas(2), tol=0.5, **KW), ()),
    "fista_path/delta_3": (_squared, lambda P: fos.fista_path(P, None, alphas(5), delta=3.0, **KW), ()),
    "fista_path/delta_2": (_squared, lambda P: fos.fista_path(P, None, alphas(5), delta=2.0, **KW), ()),
    "fista_cv/plain_4x2": (_squared, lambda P: fos.fista_cv(P, None, alphas(2), 4, return_coefs=True, **KW), ()),
    "fista_cv/weighted_4x2": (_weighted, lambda P: fos.fista_cv(P, None, alphas(2), 4, return_coefs=True, **KW), ()),
    "fista_cv/plain_3x7_second_refused": (_squared, lambda P: fos.fista_cv(P, None, alphas(7), 3, **KW), (True, False)),
    "fista_cv/plain_first_refused": (_squared, lambda P: fos.fista_cv(P, None, alphas(2), 4, **KW), (False,)),
    "fista_cv/weighted_first_refused": (_weighted, lambda P: fos.fista_cv(P, None, alphas(2), 4, **KW), (False,)),
    "fista_cv/plain_no_refit": (_squared, lambda P: fos.fista_cv(P, None, alphas(2), 4, refit=False, tol_ratio=0.5,
                                                                  adaptive_restart=True, restart_threshold=0.75, **KW), ()),
    "fista_cv/bad_folds": (_squared, lambda P: fos.fista_cv(P, None, alphas(2), 1, **KW), ()),
    "fista_cv/zero_weight_fold": (lambda P: _zero_fold(P(weighted=True)), lambda P: fos.fista_cv(P, None, alphas(2), 4, **KW), ()),
    "fista_cv/delta_3": (_squared, lambda P: fos.fista_cv(P, None, alphas(2), 2, delta=3.0, **KW), ()),
    "fista_cv/delta_2": (_squared, lambda P: fos.fista_cv(P, None, [], 2, delta=2.0, **KW), ()),
    "fista_cv/no_alphas": (_squared, lambda P: fos.fista_cv(P, None, [], 2, **KW), ()),
    "logistic_path/7": (_logit, lambda P: fos.logistic_path(P, None, alphas(7), return_info=True, **KW), ()),
    "logistic_path/20": (_logit, lambda P: fos.logistic_path(P, None, alphas(20), tol_ratio=0.5, adaptive_restart=True,
                                                               restart_threshold=0.75, **KW), ()),
    "logistic_path/weighted_1": (_wlogit, lambda P: fos.logistic_path(P, None, alphas(1), return_info=True, **KW), ()),
    "logistic_path/refused": (_logit, lambda P: fos.logistic_path(P, None, alphas(7), **KW), (False,)),
    "logistic_path/delta_3": (_logit, lambda P: fos.logistic_path(P, None, alphas(2), delta=3.0, **KW), ()),
    "logistic_path/delta_2": (_logit, lambda P: fos.logistic_path(P, None, [], delta=2.0, **KW), ()),
    "logistic_cv/3x7": (_logit, lambda P: fos.logistic_cv(P, None, alphas(7), 3, return_coefs=True, **KW), ()),
    "logistic_cv/weighted_3x7": (_wlogit, lambda P: fos.logistic_cv(P, None, alphas(7), 3, return_coefs=True, **KW), ()),
    "logistic_cv/refused": (_logit, lambda P: fos.logistic_cv(P, None, alphas(7), 3, **KW), (False,)),
    "logistic_cv/second_refused": (_logit, lambda P: fos.logistic_cv(P, None, alphas(7), 3, **KW), (True, False)),
    "logistic_cv/refit_refused": (_logit, lambda P: fos.logistic_cv(P, None, alphas(7), 3, **KW), (True, True, False)),
    "logistic_cv/no_refit": (_logit, lambda P: fos.logistic_cv(P, None, alphas(2), 3, refit=False, **KW), ()),
    "logistic_cv/delta_3": (_logit, lambda P: fos.logistic_cv(P, None, alphas(2), 3, delta=3.0, **KW), ()),
    "logistic_cv/delta_2": (_logit, lambda P: fos.logistic_cv(P, None, alphas(2), 1, delta=2.0, **KW), ()),
    "logistic_cv/bad_folds": (_logit, lambda P: fos.logistic_cv(P, None, alphas(2), 1, **KW), ()),
    "multitask_path/T3_7": (_squared, lambda P: fos.multitask_path(P, B3, alphas(7), return_info=True, **KW), ()),
    "multitask_path/T3_factors": (lambda P: P(factors=True), lambda P: fos.multitask_path(P, B3, alphas(2), **KW), ()),
    "multitask_path/refused": (_squared, lambda P: fos.multitask_path(P, B3, alphas(7), **KW), (True, False)),
    "multitask_path/delta_3": (_squared, lambda P: fos.multitask_path(P, B3, alphas(2), delta=3.0, **KW), ()),
    "multitask_path/delta_2": (_squared, lambda P: fos.multitask_path(P, B3, alphas(2), delta=2.0, **KW), ()),
}
for _C in (3, 5):
    for _tag, _kw in (("plain", {}), ("grouped", dict(grouped=True))):
        SCENARIOS[f"multinomial_path/C{_C}_{_tag}"] = (
            _soft(_C, **_kw), lambda P: fos.multinomial_path(P, None, alphas(7), return_info=True, **KW), ())
        SCENARIOS[f"multinomial_cv/C{_C}_{_tag}_3x3"] = (
            _soft(_C, **_kw), lambda P: fos.multinomial_cv(P, None, alphas(3), 3, return_coefs=True, **KW), ())
SCENARIOS.update({
    "multinomial_path/refused": (_soft(3), lambda P: fos.multinomial_path(P, None, alphas(7), **KW), (True, False)),
    "multinomial_path/weighted_factors": (_soft(3, weighted=True, factors=True),
                                          lambda P: fos.multinomial_path(P, None, alphas(2), **KW), ()),
    "multinomial_path/delta_3": (_soft(3), lambda P: fos.multinomial_path(P, None, alphas(2), delta=3.0, **KW), ()),
    "multinomial_path/delta_2": (_soft(3), lambda P: fos.multinomial_path(P, None, [], delta=2.0, **KW), ()),
    "multinomial_cv/refused": (_soft(3), lambda P: fos.multinomial_cv(P, None, alphas(3), 3, **KW), (False,)),
    "multinomial_cv/scores_refused": (_soft(3, scores=False), lambda P: fos.multinomial_cv(P, None, alphas(3), 3, **KW), ()),
    "multinomial_cv/weighted_no_refit": (_soft(3, weighted=True), lambda P: fos.multinomial_cv(P, None, alphas(3), 3, refit=False, **KW), ()),
    "multinomial_cv/refit_refused": (_soft(3), lambda P: fos.multinomial_cv(P, None, alphas(3), 3, **KW), (True, True, False)),
    "multinomial_cv/delta_3": (_soft(3, grouped=True), lambda P: fos.multinomial_cv(P, None, alphas(2), 3, delta=3.0, **KW), ()),
    "multinomial_cv/delta_2": (_soft(3), lambda P: fos.multinomial_cv(P, None, alphas(2), 1, delta=2.0, **KW), ()),
    "multinomial_cv/bad_folds": (_soft(3), lambda P: fos.multinomial_cv(P, None, alphas(2), 1, **KW), ()),
})


def _zero_fold(prob):
    prob.sample_weight[: (M + 3) // 4] = 0.0          # the rows of the first of four contiguous folds
    return prob


def run_one(monkeypatch, name):
    """{log, result or raises / text, grad_num_calls} of one scenario."""
    handle, call, served = SCENARIOS[name]
    with monkeypatch.context() as mp:
        log, problem = install(mp, served)
        rec = {}
        try:
            rec["result"] = _plain(call(handle(problem)))
        except Exception as e:                         # what a front end raises is part of the record
            rec["raises"], rec["text"] = type(e).__name__, str(e)
        rec["log"] = _plain(log)
        rec["grad_num_calls"] = fos.get_metrics()["grad_num_calls"]
    return rec


def run(monkeypatch):
    return {name: run_one(monkeypatch, name) for name in SCENARIOS}
