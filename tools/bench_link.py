#!/usr/bin/env python3
"""The Huber and squared-hinge losses in the lockstep: 16 weights of the Huber and of the squared-hinge pass (fos_fista_run_multi
on a fos_problem_set_link_loss problem, what huber_path / hinge_path run: plain product 1, the link kernel of
csrc/pointwise_link.hpp, product 2) against two passes on the SAME bound A in the same process - the squared two-product pass (a
prepare_weighted handle with unit weights) and the logistic pass - the four interleaved region by region: cfg2 (65536 x 8192
fp32), the bf16 shard of config 5 (131072 x 16384) and 262144 x 256 fp32, where the link kernel's share of the pass is largest.
HIP-event time of whole lockstep iterations, microseconds per iteration.  Each ratio is reported beside the baseline's own
region-to-region spread and beside the traffic bound: the link reads 64 B and writes 64 B of the panel and reads 4-9 B of row
data (b, a weight, a fold id) per row, next to 2 * esz * n B of A per row, if the panel came from HBM.

    python tools/bench_link.py [OUT.json]
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
    """{name: [us per iteration, one entry per region]}: every repeat times each form once, in turn.  One untimed pass through
    all forms at full region length comes first: a cold first region would otherwise set the spread the ratio is held against."""
    for run in runs.values():
        run(ITERS)
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
    m, n = cfg["m"], cfg["n"]
    y01 = (b > b.median()).to(torch.float32)
    probs = {"squared": fos.prepare_weighted(A, b, torch.ones(m, device=dev)), "logistic": fos.prepare(A, y01, loss="logistic"),
             "huber": fos.prepare_huber(A, b, float(b.abs().median())), "hinge": fos.prepare_hinge(A, 2.0 * y01 - 1.0)}
    assert all(P.A.data_ptr() == probs["squared"].A.data_ptr() for P in probs.values())        # all borrow the same device A
    L = 4.0 * m
    lam = 1e3 if cfg["dtype"] == "f32" else 1e5

    def handles(prob, L_data):
        hs = [_core.Fista(prob) for _ in range(NV)]
        for j, st in enumerate(hs):
            st.reset(1.0 / L_data, 1e-3 * lam * 0.9 ** j, cfg["a2"])
        return hs

    hs = {k: handles(P, L / 4.0 if k == "logistic" else L) for k, P in probs.items()}
    runs = {k: (lambda it, h=h: _core.run_multi(h, it)) for k, h in hs.items()}
    assert all(run(2) for run in runs.values())
    t = interleaved(runs)
    esz = 4 if cfg["dtype"] == "f32" else 2
    res = {"shape": [m, n, cfg["dtype"]], "traffic_bound_ratio": 1.0 + (128.0 + 4.0) / (2.0 * esz * n)}
    for k in runs:
        res[k + "_us_per_iteration"] = spread(t[k])
    for base in ("squared", "logistic"):
        lo, hi = res[base + "_us_per_iteration"]["min"], res[base + "_us_per_iteration"]["max"]
        res[base + "_spread_max_over_min"] = hi / lo
        for k in ("huber", "hinge"):
            res[f"{k}_over_{base}_median"] = res[k + "_us_per_iteration"]["median"] / res[base + "_us_per_iteration"]["median"]
    print(name, json.dumps(res), flush=True)
    out[name] = res
    del hs, runs, probs, A, b, y01
    torch.cuda.empty_cache()
print(json.dumps(out))
if len(sys.argv) > 1:                           # optional: also write the results to the given JSON file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
