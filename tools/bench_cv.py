#!/usr/bin/env python3
"""K-fold cross-validation in lockstep: 5 folds x 3 weights = 15 columns of the masked two-product pass
(fos_fista_run_multi_folds) against the unmasked two-product pass at 15 columns (fos_fista_run_multi_rhs, every column the
problem's own b) in the same process, the two interleaved repeat by repeat - cfg2 (65536 x 8192 fp32) and the bf16 shard of
config 5 (131072 x 16384).  Then the whole fista_cv call against the same folds run one by one on gathered copies of the
training rows.  HIP-event time of whole iterations; A-pass kernel time from fos_problem_profile.

    python tools/bench_cv.py [OUT.json]
        FOS_BENCH_ITERS   timed iterations per repeat (default 30)
        FOS_BENCH_REPEATS interleaved repeats (default 7)
        FOS_BENCH_TREE    import the package from this checkout instead (one without the fold entry point times the unmasked
                          pass alone: the baseline of an earlier commit, measured by the same script)"""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ.get("FOS_BENCH_TREE", ROOT))
import fastoptsolver_amd as fos
from fastoptsolver_amd import _core, _lib, iterative_solvers as its
from bench import make_shard, WORKLOADS
torch.cuda.set_device(0)
ITERS = int(os.environ.get("FOS_BENCH_ITERS", "30"))
REPEATS = int(os.environ.get("FOS_BENCH_REPEATS", "7"))
CV_ITERS = 50
K, WEIGHTS = 5, 3
HAVE_FOLDS = hasattr(_core, "run_multi_folds")


def interleaved(runs):
    """{name: [us per iteration, one entry per repeat]}: every repeat times each form once, in turn."""
    for run in runs.values():
        run(3)
    torch.cuda.synchronize()
    out = {name: [] for name in runs}
    for _ in range(REPEATS):
        for name, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(ITERS); e1.record(); e1.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / ITERS)
    return out


def a_pass_us(run, prob):
    prob.profile(1); prob.profile_read(); run(5); ms, cnt = prob.profile_read(); prob.profile(0)
    return ms * 1e3 / max(cnt, 1)


def spread(v):
    return dict(min=min(v), median=float(np.median(v)), max=max(v), runs=v)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


out = {"tree": os.environ.get("FOS_BENCH_TREE", ROOT) != ROOT and "other" or "this", "have_folds": HAVE_FOLDS,
       "iters": ITERS, "repeats": REPEATS, "columns": K * WEIGHTS}
for name, cfg in (("cfg2", WORKLOADS["cfg2"]), ("cfg5_shard", dict(WORKLOADS["cfg5"], m=131072))):
    dev = torch.device("cuda", 0)
    A, b = make_shard(cfg, 0, cfg["m"], dev)
    m = cfg["m"]
    P = fos.prepare(A, b)
    L = 4.0 * m
    lam = 1e3 if name == "cfg2" else 1e5
    alphas = [(lam * 0.9 ** a, cfg["a2"]) for a in range(WEIGHTS)]
    nv = K * WEIGHTS
    B = b[:, None].expand(m, nv).contiguous()       # the unmasked pass: every column against the problem's own b

    def handles():
        hs = [_core.Fista(P) for _ in range(nv)]
        for j, st in enumerate(hs):
            st.reset(1.0 / L, alphas[j % WEIGHTS][0], cfg["a2"])
        return hs

    runs, res = {}, {}
    hr = handles()
    assert _core.run_multi_rhs(hr, B, 2)
    runs["unmasked_rhs"] = lambda it: _core.run_multi_rhs(hr, B, it)
    if HAVE_FOLDS:
        ids = np.repeat(np.arange(K), m // K + 1)[:m]
        ids_dev = _core.fold_ids_tensor(ids, dev)
        held = [f for f in range(K) for _ in range(WEIGHTS)]
        hf = handles()
        assert _core.run_multi_folds(hf, ids_dev, held, 2)
        runs["folds"] = lambda it: _core.run_multi_folds(hf, ids_dev, held, it)
    t = interleaved(runs)
    res["unmasked_rhs_us_per_iteration"] = spread(t["unmasked_rhs"])
    res["unmasked_rhs_a_pass_us"] = a_pass_us(runs["unmasked_rhs"], P)
    if HAVE_FOLDS:
        res["folds_us_per_iteration"] = spread(t["folds"])
        res["folds_a_pass_us"] = a_pass_us(runs["folds"], P)
        res["folds_over_unmasked_median"] = res["folds_us_per_iteration"]["median"] / res["unmasked_rhs_us_per_iteration"]["median"]
        lo, hi = res["unmasked_rhs_us_per_iteration"]["min"], res["unmasked_rhs_us_per_iteration"]["max"]
        res["folds_median_within_unmasked_spread"] = bool(lo <= res["folds_us_per_iteration"]["median"] <= hi)
        del hf
    del hr, runs
    print(name, json.dumps(res), flush=True)
    if HAVE_FOLDS:
        # the whole call: lockstep on the one bound A against fold by fold on gathered copies (what a user could do before)
        kw = dict(max_iter=CV_ITERS, L=L, refit=False)
        fos.fista_cv(P, None, alphas, K, **dict(kw, max_iter=3))
        cv_s = min(wall(lambda: fos.fista_cv(P, None, alphas, K, **kw)) for _ in range(3))
        prms = [its._params(its._tau(L, a2, 1.0), a1, a2, mode=_lib.MODE_FISTA) for a1, a2 in alphas]
        its._cv_fold_by_fold(P, ids.astype(np.uint8), K, prms, 3)
        torch.cuda.empty_cache()
        gathered_s = min(wall(lambda: its._cv_fold_by_fold(P, ids.astype(np.uint8), K, prms, CV_ITERS)) for _ in range(3))
        res.update(fista_cv_s=cv_s, fold_by_fold_gathered_s=gathered_s, fista_cv_speedup=gathered_s / cv_s, cv_iters=CV_ITERS)
        print(name, "whole call", json.dumps({k: res[k] for k in ("fista_cv_s", "fold_by_fold_gathered_s", "fista_cv_speedup")}),
              flush=True)
    out[name] = res
    del P, A, b, B
    torch.cuda.empty_cache()
print(json.dumps(out))
if len(sys.argv) > 1:                           # optional: also write the results to the given JSON file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
