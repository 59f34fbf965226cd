#!/usr/bin/env python3
"""The group penalty in the lockstep: 16 columns (four fits of C = 4 classes) of the multinomial two-product pass with the
grouped update (fos_fista_params.group = 4: one launch of fista_update_group_kernel, grid (nupd, 4), which walks the four columns
of a fit in turn) against the same 16 columns with the separable update (group = 0: fista_update_multi_kernel, grid (nupd, 16))
on the SAME bound A and labels in the same process, the two interleaved region by region - cfg2 (65536 x 8192 fp32), the bf16
shard of config 5 (131072 x 16384) and 262144 x 256 fp32, where the update's share of the iteration is largest.  The products
and the link kernel are the same launches in both forms; only the update differs.  HIP-event time of whole lockstep iterations,
microseconds per iteration; the grouped median is held against the ungrouped form's own run-to-run spread.

    python tools/bench_group.py [OUT.json]
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
    q = torch.quantile(b[:: max(1, m // 65536)].float(), torch.tensor([0.25, 0.5, 0.75], device=dev))
    cls = torch.bucketize(b.float(), q).to(torch.float32)          # four classes of about equal size
    PM = fos.prepare_multinomial(A, cls, classes=CLASSES)
    L = 4.0 * m
    lam = 1e3 if cfg["dtype"] == "f32" else 1e5

    def handles(group):
        hs = [_core.Fista(PM) for _ in range(NV)]
        for j, st in enumerate(hs):
            st.reset(2.0 / L, 1e-3 * lam * 0.9 ** (j // CLASSES), cfg["a2"], group=group)      # a class group shares its parameters
        return hs

    hu, hg = handles(0), handles(CLASSES)
    runs = {"ungrouped": lambda it: _core.run_multi(hu, it), "grouped": lambda it: _core.run_multi(hg, it)}
    assert runs["ungrouped"](2) and runs["grouped"](2)
    t = interleaved(runs)
    res = {"shape": [m, n, cfg["dtype"]], "ungrouped_us_per_iteration": spread(t["ungrouped"]),
           "grouped_us_per_iteration": spread(t["grouped"])}
    res["grouped_over_ungrouped_median"] = res["grouped_us_per_iteration"]["median"] / res["ungrouped_us_per_iteration"]["median"]
    lo, hi = res["ungrouped_us_per_iteration"]["min"], res["ungrouped_us_per_iteration"]["max"]
    res["ungrouped_spread_max_over_min"] = hi / lo
    res["grouped_median_within_ungrouped_spread"] = bool(lo <= res["grouped_us_per_iteration"]["median"] <= hi)
    print(name, json.dumps(res), flush=True)
    out[name] = res
    del hu, hg, runs, PM, A, b, cls
    torch.cuda.empty_cache()
print(json.dumps(out))
if len(sys.argv) > 1:                           # optional: also write the results to the given JSON file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
