#!/usr/bin/env python3
"""Sparse logistic regression in the lockstep: 16 weights of the logistic two-product pass (fos_fista_run_multi on a logistic
problem, what logistic_path runs) against 16 weights of the squared-loss two-product pass (what fista_path runs with the
cluster form switched off: like is compared with like) on the SAME bound A in the same process, the two interleaved region
by region - cfg2 (65536 x 8192 fp32), the bf16 shard of config 5 (131072 x 16384) and 262144 x 256 fp32, where the epilogue's
share of the pass is largest.  HIP-event time of whole lockstep iterations, microseconds per iteration.

    python tools/bench_logistic.py [OUT.json]
        FOS_BENCH_ITERS   timed iterations per region (default 30)
        FOS_BENCH_REPEATS interleaved regions per form (default 5)
        FOS_BENCH_SHAPES  comma-separated subset of cfg2,cfg5_shard,narrow"""
import json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fastoptsolver_amd as fos
from fastoptsolver_amd import _core
from bench import make_shard, WORKLOADS
torch.cuda.set_device(0)
ITERS = int(os.environ.get("FOS_BENCH_ITERS", "30"))
REPEATS = int(os.environ.get("FOS_BENCH_REPEATS", "5"))
NV = 16
SHAPES = {"cfg2": WORKLOADS["cfg2"], "cfg5_shard": dict(WORKLOADS["cfg5"], m=131072),
          "narrow": dict(WORKLOADS["cfg2"], m=262144, n=256)}


def interleaved(runs):
    """{name: [us per iteration, one entry per region]}: every repeat times each form once, in turn."""
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


def spread(v):
    return dict(min=min(v), median=float(np.median(v)), max=max(v), runs=v)


out = {"iters": ITERS, "repeats": REPEATS, "columns": NV}
for name in os.environ.get("FOS_BENCH_SHAPES", "cfg2,cfg5_shard,narrow").split(","):
    cfg = SHAPES[name]
    dev = torch.device("cuda", 0)
    A, b = make_shard(cfg, 0, cfg["m"], dev)
    m = cfg["m"]
    y = (b > b.median()).to(torch.float32)
    P = fos.prepare(A, b)
    P.replan(cluster=False)                         # the squared loss in the two-product form as well
    PL = fos.prepare(A, y, loss="logistic")         # borrows the same device A
    assert PL.A.data_ptr() == P.A.data_ptr()
    L = 4.0 * m
    lam = 1e3 if cfg["dtype"] == "f32" else 1e5

    def handles(prob, L_data, scale):
        hs = [_core.Fista(prob) for _ in range(NV)]
        for j, st in enumerate(hs):
            st.reset(1.0 / L_data, scale * lam * 0.9 ** j, cfg["a2"])
        return hs

    hs, hl = handles(P, L, 1.0), handles(PL, L / 4.0, 1e-3)
    runs = {"squared": lambda it: _core.run_multi(hs, it), "logistic": lambda it: _core.run_multi(hl, it)}
    assert runs["squared"](2) and runs["logistic"](2)
    t = interleaved(runs)
    res = {"shape": [m, cfg["n"], cfg["dtype"]], "squared_us_per_iteration": spread(t["squared"]),
           "logistic_us_per_iteration": spread(t["logistic"])}
    res["logistic_over_squared_median"] = res["logistic_us_per_iteration"]["median"] / res["squared_us_per_iteration"]["median"]
    lo, hi = res["squared_us_per_iteration"]["min"], res["squared_us_per_iteration"]["max"]
    res["squared_spread_max_over_min"] = hi / lo
    res["logistic_median_within_squared_spread"] = bool(lo <= res["logistic_us_per_iteration"]["median"] <= hi)
    res["plan_cluster"] = int(P.plan()["cluster"])
    print(name, json.dumps(res), flush=True)
    out[name] = res
    del hs, hl, runs, P, PL, A, b, y
    torch.cuda.empty_cache()
print(json.dumps(out))
if len(sys.argv) > 1:                           # optional: also write the results to the given JSON file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
