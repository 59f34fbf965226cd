#!/usr/bin/env python3
"""Several targets for L-BFGS: LBFGSSolver.fit(A, B) with k columns in lockstep (fos_lbfgs_minimize_multi, one fp64
multi-point pass per round on the matrix cores) against the same k columns fitted one by one - cfg3
(LBFGSSolver("ridge", 0, 1.0) on 65536 x 8192 fp32, column 0 = the cfg2 b, the others seeded random targets) and the bf16
shard of config 5 (131072 x 16384), k = 3, 4, 8, 16.  Reports us per round (HIP events around the fit / rounds), us per
product kernel (fos_problem_profile brackets each product launch), whole-fit ms and whole-fit ms one by one.

    python tools/bench_lbfgs_multi.py [OUT.json]"""
import json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fastoptsolver_amd as fos
from fastoptsolver_amd.iterative_solvers import get_metrics
from fastoptsolver_amd.lbfgs import LBFGSSolver
from bench import make_shard, WORKLOADS
torch.cuda.set_device(0)


def fit_ms(fn):
    """(best ms over 2 repeats after one warm-up, result of the last call)"""
    r = fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); r = fn(); e1.record(); e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best, r


out = {}
for name, cfg in (("cfg3", WORKLOADS["cfg2"]), ("cfg5_shard", dict(WORKLOADS["cfg5"], m=131072))):
    dev = torch.device("cuda", 0)
    A, b = make_shard(cfg, 0, cfg["m"], dev)
    m = cfg["m"]
    g = torch.Generator(device=dev); g.manual_seed(11)
    B = torch.randn(m, 16, dtype=torch.float32, device=dev, generator=g) * b.std()
    B[:, 0] = b
    P = fos.prepare(A)
    sibs = [P.sibling(B[:, j].contiguous()) for j in range(16)]
    solver = lambda: LBFGSSolver("ridge", 0, 1.0)
    res = {}
    for k in (3, 4, 8, 16):
        row = {}
        ms_one, _ = fit_ms(lambda: [solver().fit(s, None) for s in sibs[:k]])
        ms, s = fit_ms(lambda: solver().fit(P, B[:, :k]))
        rounds = get_metrics()["grad_num_calls"]
        P.profile(1); P.profile_read()
        solver().fit(P, B[:, :k])
        p_ms, launches = P.profile_read(); P.profile(0)
        row.update(fit_ms=ms, one_by_one_fit_ms=ms_one, speedup=ms_one / ms, rounds=rounds,
                   sum_nfev=int(s.nfev_.sum()), max_nfev=int(s.nfev_.max()), us_per_round=ms * 1e3 / max(rounds, 1),
                   us_per_product=p_ms * 1e3 / max(launches, 1), product_launches=int(launches))
        res[k] = row
        print(name, k, json.dumps(row), flush=True)
    out[name] = res
    del P, sibs, A, b, B
    torch.cuda.empty_cache()
print(json.dumps(out))
if len(sys.argv) > 1:                           # optional: also write the results to the given JSON file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
