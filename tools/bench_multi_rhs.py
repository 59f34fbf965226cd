#!/usr/bin/env python3
"""Several targets: k right-hand sides in lockstep (fos_fista_run_multi_rhs: multi-vector VALU pass up to 4 columns where the
shape has one, two matrix-core products with the B-block epilogue otherwise) against the same k solved one by one and against
fista_path with k weights on one shared b (the pass without the B block) - cfg2 (65536 x 8192 fp32) and the bf16 shard of
config 5 (131072 x 16384).  HIP-event time of whole iterations; A-pass kernel time from fos_problem_profile.

    python tools/bench_multi_rhs.py [OUT.json]      (FOS_BENCH_ITERS: timed iterations per repeat, default 30)"""
import json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fastoptsolver_amd as fos
from fastoptsolver_amd import _core
from bench import make_shard, WORKLOADS
torch.cuda.set_device(0)
ITERS = int(os.environ.get("FOS_BENCH_ITERS", "30"))


def timed(run, prob):
    """(best us per iteration over 3 repeats, A-pass kernel us per launch)"""
    run(3)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(ITERS); e1.record(); e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / ITERS)
    prob.profile(1); prob.profile_read(); run(5); ms, cnt = prob.profile_read(); prob.profile(0)
    return best, ms * 1e3 / max(cnt, 1)


out = {}
for name, cfg in (("cfg2", WORKLOADS["cfg2"]), ("cfg5_shard", dict(WORKLOADS["cfg5"], m=131072))):
    dev = torch.device("cuda", 0)
    A, b = make_shard(cfg, 0, cfg["m"], dev)
    m = cfg["m"]
    g = torch.Generator(device=dev); g.manual_seed(7)
    B = torch.randn(m, 16, dtype=torch.float32, device=dev, generator=g) * 30.0
    B[:, 0] = b
    P = fos.prepare(A)                         # A bound once, no b: the multi-target problem
    shared = P.sibling(b)                      # same device A, one b: fista_path's lockstep and the one-by-one baseline
    sibs = [P.sibling(B[:, j].contiguous()) for j in range(16)]
    L = 4.0 * m
    lam = 1e3 if name == "cfg2" else 1e5
    res = {}
    for k in (1, 2, 4, 8, 16):
        row = {}
        # one by one: each column on its own problem (borrowing the same A)
        one = [_core.Fista(s) for s in sibs[:k]]
        for st in one:
            st.reset(1.0 / L, lam, cfg["a2"])
        us, _ = timed(lambda it: [st.run(it) for st in one], shared)
        row["one_by_one_us_per_iteration"] = us
        if k > 1:
            hs = [_core.Fista(P) for _ in range(k)]
            for st in hs:
                st.reset(1.0 / L, lam, cfg["a2"])
            if _core.run_multi_rhs(hs, B[:, :k], 2):
                us, a_us = timed(lambda it: _core.run_multi_rhs(hs, B[:, :k], it), P)
                row.update(multi_rhs_us_per_iteration=us, multi_rhs_us_per_column_iteration=us / k, multi_rhs_a_pass_us=a_us,
                           speedup_vs_one_by_one=row["one_by_one_us_per_iteration"] / us)
            else:
                row["multi_rhs"] = "not served"
            hp = [_core.Fista(shared) for _ in range(k)]
            for i, st in enumerate(hp):
                st.reset(1.0 / L, lam * 0.9 ** i, cfg["a2"])
            if _core.run_multi(hp, 2):
                us, a_us = timed(lambda it: _core.run_multi(hp, it), shared)
                row.update(path_us_per_iteration=us, path_a_pass_us=a_us)
                if "multi_rhs_us_per_iteration" in row:
                    row["multi_rhs_over_path"] = row["multi_rhs_us_per_iteration"] / us
            del hs, hp
        del one
        res[k] = row
        print(name, k, json.dumps(row), flush=True)
    out[name] = res
    del P, shared, sibs, A, b, B
    torch.cuda.empty_cache()
print(json.dumps(out))
if len(sys.argv) > 1:                           # optional: also write the results to the given JSON file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
