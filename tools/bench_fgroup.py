#!/usr/bin/env python3
"""Group lasso over feature groups in the lockstep: 16 penalty weights of the two-product pass with feature groups bound
(fos_fista_run_multi on a handle after fos_feature_groups_bind, what fista_path / logistic_path run on a prepare_grouped handle)
against 16 of the two-product pass without them on the SAME bound A in the same process (squared loss with the cluster form
switched off: like is compared with like), for the squared and for the logistic loss, the forms interleaved region by region -
cfg2 (65536 x 8192 fp32), the bf16 shard of config 5 (131072 x 16384) and 262144 x 256 fp32, where the update's share of the
pass is largest.  The two products are the same launches in all forms; the update is one launch without groups and three with
them (u, the group norms, the scaling: 16 x n more doubles written and read twice per iteration).  Two layouts: groups of 8, and
a few groups of 1024 among groups of 8 (two groups of 64 at n = 256).  l1_ratio = 0.5, so both thresholds are live.  HIP-event
time of whole lockstep iterations, microseconds per iteration.

    python tools/bench_fgroup.py [OUT.json]
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
LAYOUTS = ("g8", "big")


def layout(name, n):
    """Group sizes: all of 8, or three large groups (1024 columns; 64 at n = 256) spread among groups of 8."""
    if name == "g8":
        return [8] * (n // 8)
    big = 1024 if n >= 4096 else 64
    rest = (n - 3 * big) // 8
    q = rest // 4
    return [8] * q + [big] + [8] * q + [big] + [8] * q + [big] + [8] * (rest - 3 * q)


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


out = {"iters": ITERS, "repeats": REPEATS, "columns": NV, "l1_ratio": 0.5}
for name in os.environ.get("FOS_BENCH_SHAPES", "cfg2,cfg5_shard,narrow").split(","):
    cfg = SHAPES[name]
    dev = torch.device("cuda", 0)
    A, b = make_shard(cfg, 0, cfg["m"], dev)
    m, n = cfg["m"], cfg["n"]
    y = (b > b.median()).to(torch.float32)
    P = fos.prepare(A, b)
    P.replan(cluster=False)                         # the squared loss without groups in the two-product form as well
    probs = {"squared": P, "logistic": fos.prepare(A, y, loss="logistic")}
    for lay in LAYOUTS:
        sizes = layout(lay, n)
        assert sum(sizes) == n
        probs["squared_" + lay] = fos.prepare(A, b)
        probs["logistic_" + lay] = fos.prepare(A, y, loss="logistic")
        probs["squared_" + lay].set_feature_groups(sizes, None, 0.5)
        probs["logistic_" + lay].set_feature_groups(sizes, None, 0.5)
    assert all(q.A.data_ptr() == P.A.data_ptr() for q in probs.values())          # one device copy of A
    L = 4.0 * m
    lam = 1e3 if cfg["dtype"] == "f32" else 1e5
    hs = {}
    for form, prob in probs.items():
        logit = form.startswith("logistic")
        hs[form] = [_core.Fista(prob) for _ in range(NV)]
        for j, st in enumerate(hs[form]):
            st.reset(1.0 / ((L / 4.0 if logit else L) + cfg["a2"]), (1e-3 if logit else 1.0) * lam * 0.9 ** j, cfg["a2"])
    runs = {form: (lambda it, h=h: _core.run_multi(h, it)) for form, h in hs.items()}
    assert all(run(2) for run in runs.values())
    t = interleaved(runs)
    res = {"shape": [m, n, cfg["dtype"]], "plan_cluster": int(P.plan()["cluster"]), "groups": {lay: len(layout(lay, n)) for lay in LAYOUTS}}
    for form in runs:
        res[form + "_us_per_iteration"] = spread(t[form])
    for base in ("squared", "logistic"):
        u = res[base + "_us_per_iteration"]
        res[base + "_spread_max_over_min"] = u["max"] / u["min"]
        for lay in LAYOUTS:
            v = res[f"{base}_{lay}_us_per_iteration"]
            res[f"{base}_{lay}_over_plain_median"] = v["median"] / u["median"]
            res[f"{base}_{lay}_median_within_plain_spread"] = bool(u["min"] <= v["median"] <= u["max"])
    x = hs["squared_g8"][0].x_tensor()[:n].cpu().numpy().reshape(-1, 8)
    res["squared_g8_fraction_of_zero_groups"] = float((~x.any(axis=1)).mean())
    print(name, json.dumps(res), flush=True)
    out[name] = res
    del hs, runs, probs, P, A, b, y
    torch.cuda.empty_cache()
print(json.dumps(out))
if len(sys.argv) > 1:                           # optional: also write the results to the given JSON file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
