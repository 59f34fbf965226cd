#!/usr/bin/env python3
"""Multinomial regression in the lockstep: 16 columns (four fits of C = 4 classes) of the multinomial two-product pass
(fos_fista_run_multi on a multinomial problem, what multinomial_path runs: plain product 1, the link kernel of
csrc/softmax_link.hpp, product 2) against 16 weights of the logistic two-product pass (what logistic_path runs) on the SAME bound
A in the same process, the two interleaved region by region - cfg2 (65536 x 8192 fp32), the bf16 shard of config 5
(131072 x 16384) and 262144 x 256 fp32, where the link kernel's share of the pass is largest.  HIP-event time of whole lockstep
iterations, microseconds per iteration.  The derived bound of the link kernel's cost: at most 128 B of R plus 4 B of label per
row next to 2 * esz * n B of A per row, if R came from HBM.

    python tools/bench_multinomial.py [OUT.json]
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
NV, CLASSES = 16, 4
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


out = {"iters": ITERS, "repeats": REPEATS, "columns": NV, "classes": CLASSES}
for name in os.environ.get("FOS_BENCH_SHAPES", "cfg2,cfg5_shard,narrow").split(","):
    cfg = SHAPES[name]
    dev = torch.device("cuda", 0)
    A, b = make_shard(cfg, 0, cfg["m"], dev)
    m, n = cfg["m"], cfg["n"]
    y = (b > b.median()).to(torch.float32)
    q = torch.quantile(b[:: max(1, m // 65536)].float(), torch.tensor([0.25, 0.5, 0.75], device=dev))
    cls = torch.bucketize(b.float(), q).to(torch.float32)          # four classes of about equal size
    PL = fos.prepare(A, y, loss="logistic")
    PM = fos.prepare_multinomial(A, cls, classes=CLASSES)           # borrows the same device A
    assert PM.A.data_ptr() == PL.A.data_ptr()
    L = 4.0 * m
    lam = 1e3 if cfg["dtype"] == "f32" else 1e5

    def handles(prob, L_data, group):
        hs = [_core.Fista(prob) for _ in range(NV)]
        for j, st in enumerate(hs):
            st.reset(1.0 / L_data, 1e-3 * lam * 0.9 ** (j // group), cfg["a2"])      # a class group shares its parameters
        return hs

    hl, hm = handles(PL, L / 4.0, 1), handles(PM, L / 2.0, CLASSES)
    runs = {"logistic": lambda it: _core.run_multi(hl, it), "multinomial": lambda it: _core.run_multi(hm, it)}
    assert runs["logistic"](2) and runs["multinomial"](2)
    t = interleaved(runs)
    esz = 4 if cfg["dtype"] == "f32" else 2
    res = {"shape": [m, n, cfg["dtype"]], "logistic_us_per_iteration": spread(t["logistic"]),
           "multinomial_us_per_iteration": spread(t["multinomial"])}
    res["multinomial_over_logistic_median"] = res["multinomial_us_per_iteration"]["median"] / res["logistic_us_per_iteration"]["median"]
    lo, hi = res["logistic_us_per_iteration"]["min"], res["logistic_us_per_iteration"]["max"]
    res["logistic_spread_max_over_min"] = hi / lo
    res["derived_bound_ratio"] = 1.0 + 132.0 / (2.0 * esz * n)
    res["multinomial_median_within_logistic_spread"] = bool(lo <= res["multinomial_us_per_iteration"]["median"] <= hi)
    res["ratio_within_spread_or_bound"] = bool(res["multinomial_median_within_logistic_spread"] or
                                               res["multinomial_over_logistic_median"] <= max(hi / lo, res["derived_bound_ratio"]))
    print(name, json.dumps(res), flush=True)
    out[name] = res
    del hl, hm, runs, PL, PM, A, b, y, cls
    torch.cuda.empty_cache()
print(json.dumps(out))
if len(sys.argv) > 1:                           # optional: also write the results to the given JSON file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
