#!/usr/bin/env python3
"""Plain lockstep of mixed families: 16 state machines of two families (8 FISTA, 8 FISTA-delta) in one fos_fista_run_multi
call against 16 of one family on the SAME bound A in the same process, the two forms interleaved region by region - cfg2
(65536 x 8192), fp32 and bf16 storage.  Both forms are the two products plus ONE separable update launch per iteration
(launch_separable_update: the prox kind travels per column); before that launch existed the mixed form took 16 update launches
per iteration.  HIP-event time of whole lockstep iterations, microseconds per iteration.

    python tools/bench_mixed_family.py [OUT.json]
        FOS_BENCH_ITERS   timed iterations per region (default 30)
        FOS_BENCH_REPEATS interleaved regions per form (default 5)"""
import json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fastoptsolver_amd as fos
from fastoptsolver_amd import _core, _lib
from bench import make_shard, WORKLOADS
torch.cuda.set_device(0)
ITERS = int(os.environ.get("FOS_BENCH_ITERS", "30"))
REPEATS = int(os.environ.get("FOS_BENCH_REPEATS", "5"))
NV = 16

cfg = WORKLOADS["cfg2"]
m, n = cfg["m"], cfg["n"]
A32, b = make_shard(cfg, 0, m, torch.device("cuda", 0))
lam, L = float((A32.T @ b).abs().max()), 4.0 * m
out = {"iters": ITERS, "repeats": REPEATS, "columns": NV, "shape": [m, n]}
for kind in ("f32", "bf16"):
    P = fos.prepare(A32 if kind == "f32" else A32.to(torch.bfloat16), b)
    P.replan(cluster=False)                         # the two-product form for both: like is compared with like
    hs = {"one_family": [], "mixed_families": []}
    for form, handles in hs.items():
        for j in range(NV):
            st = _core.Fista(P)
            delta = form == "mixed_families" and j >= NV // 2
            st.reset(1.0 / L, 0.2 * lam * 0.8 ** j, 0.0, mode=_lib.MODE_DELTA if delta else _lib.MODE_FISTA, delta=3.0 if delta else 0.0)
            handles.append(st)
    runs = {form: (lambda it, h=h: _core.run_multi(h, it)) for form, h in hs.items()}
    assert all(run(3) for run in runs.values())
    torch.cuda.synchronize()
    t = {form: [] for form in runs}
    for _ in range(REPEATS):
        for form, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(ITERS); e1.record(); e1.synchronize()
            t[form].append(e0.elapsed_time(e1) * 1e3 / ITERS)
    res = {form + "_us_per_iteration": dict(min=min(v), median=float(np.median(v)), max=max(v), runs=v) for form, v in t.items()}
    res["mixed_over_one_family_median"] = res["mixed_families_us_per_iteration"]["median"] / res["one_family_us_per_iteration"]["median"]
    print(kind, json.dumps(res), flush=True)
    out[kind] = res
    del hs, runs, P
print(json.dumps(out))
if len(sys.argv) > 1:                           # optional: also write the results to the given JSON file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
