#!/usr/bin/env python3
"""Resampled fits in the lockstep: 16 resampled columns (fos_fista_run_multi_resampled with bootstrap counts: plain product 1, the
link kernel of csrc/resample_link.hpp, product 2) against the two-product pass of a prepare_weighted handle with unit weights on
the SAME bound A in the same process, for the squared and the logistic loss, the forms interleaved region by region: cfg2 (65536
x 8192 fp32), the bf16 shard of config 5 (131072 x 16384) and 262144 x 256 fp32, where the link kernel's share of the pass is
largest.  HIP-event time of whole lockstep iterations, microseconds per iteration, each ratio beside the baseline's own
region-to-region spread and the traffic bound: the link reads 64 B and writes 64 B of the panel and reads 4 B of b and 8 B of
counts per row, next to 2 * esz * n B of A per row, if the panel came from HBM.

Then one stability_selection of 16 subsamples x 4 weights (four lockstep groups on one handle) against the only way there was:
16 prepare_weighted handles, one per subsample, each solving its 4 weights (fista_path) - wall time, at cfg2.

    python tools/bench_resample.py [OUT.json]
        FOS_BENCH_ITERS   timed iterations per region (default 30)
        FOS_BENCH_REPEATS interleaved regions per form (default 5)
        FOS_BENCH_SHAPES  comma-separated subset of cfg2,cfg5_shard,narrow
        FOS_BENCH_STABILITY  0 skips the stability comparison"""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fastoptsolver_amd as fos
from fastoptsolver_amd import _core, resample
from bench import make_shard, WORKLOADS
torch.cuda.set_device(0)
ITERS = int(os.environ.get("FOS_BENCH_ITERS", "30"))
REPEATS = int(os.environ.get("FOS_BENCH_REPEATS", "5"))
NV = 16
SHAPES = {"cfg2": WORKLOADS["cfg2"], "cfg5_shard": dict(WORKLOADS["cfg5"], m=131072),
          "narrow": dict(WORKLOADS["cfg2"], m=262144, n=256)}


def interleaved(runs):
    """{name: [us per iteration, one entry per region]}: every repeat times each form once, in turn, after one untimed pass
    through all forms at full region length."""
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
dev = torch.device("cuda", 0)
for name in os.environ.get("FOS_BENCH_SHAPES", "cfg2,cfg5_shard,narrow").split(","):
    cfg = SHAPES[name]
    A, b = make_shard(cfg, 0, cfg["m"], dev)
    m, n = cfg["m"], cfg["n"]
    y01 = (b > b.median()).to(torch.float32)
    ones = torch.ones(m, device=dev)
    base = {"squared": fos.prepare_weighted(A, b, ones), "logistic": fos.prepare_weighted(A, y01, ones, loss="logistic")}
    plain = {"squared": fos.prepare(A, b, pad=True), "logistic": fos.prepare(A, y01, loss="logistic")}
    words = resample.pack_counts(torch.from_numpy(resample.bootstrap_counts(m, NV, 0)).to(dev))
    L = 16.0 * m                                   # room for a bootstrap column: the iterates stay bounded, the timing does not depend on it
    lam = 1e3 if cfg["dtype"] == "f32" else 1e5

    def handles(prob, L_data):
        hs = [_core.Fista(prob) for _ in range(NV)]
        for j, st in enumerate(hs):
            st.reset(1.0 / L_data, 1e-3 * lam * 0.9 ** j, cfg["a2"])
        return hs

    runs = {}
    for k in ("squared", "logistic"):
        hb, hr = handles(base[k], L / 4.0 if k == "logistic" else L), handles(plain[k], L / 4.0 if k == "logistic" else L)
        runs[k] = lambda it, h=hb: _core.run_multi(h, it)
        runs[k + "_resampled"] = lambda it, h=hr: resample._run(h, words, it) or True
    assert all(run(2) for run in runs.values())
    t = interleaved(runs)
    esz = 4 if cfg["dtype"] == "f32" else 2
    res = {"shape": [m, n, cfg["dtype"]], "traffic_bound_ratio": 1.0 + (128.0 + 4.0 + 8.0) / (2.0 * esz * n)}
    for k in runs:
        res[k + "_us_per_iteration"] = spread(t[k])
    for k in ("squared", "logistic"):
        lo, hi = res[k + "_us_per_iteration"]["min"], res[k + "_us_per_iteration"]["max"]
        res[k + "_spread_max_over_min"] = hi / lo
        res[f"{k}_resampled_over_{k}_median"] = res[k + "_resampled_us_per_iteration"]["median"] / res[k + "_us_per_iteration"]["median"]
    print(name, json.dumps(res), flush=True)
    out[name] = res
    if name == "cfg2" and os.environ.get("FOS_BENCH_STABILITY", "1") != "0":
        # 16 subsamples x 4 weights, 30 iterations each: one handle and four lockstep groups against 16 weighted handles
        alphas = [(1e-3 * lam * f, 0.0) for f in (1.0, 0.5, 0.25, 0.125)]
        counts = resample.subsample_counts(m, 16, 0.5, seed=0)
        P = plain["squared"]
        for rep in range(2):                       # the second pass is the warm one
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fos.stability_selection(P, alphas, n_pairs=8, seed=0, max_iter=ITERS, L=float(m))
            torch.cuda.synchronize(); t_lock = time.perf_counter() - t0
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for r in range(16):
                Pw = fos.prepare_weighted(A, b, counts[:, r].astype(np.float64))
                fos.fista_path(Pw, None, alphas, max_iter=ITERS, L=float(m))
            torch.cuda.synchronize(); t_one = time.perf_counter() - t0
        out["stability_cfg2"] = {"subsamples": 16, "weights": 4, "iterations": ITERS, "lockstep_seconds": t_lock,
                                 "one_by_one_seconds": t_one, "one_by_one_over_lockstep": t_one / t_lock}
        print("stability_cfg2", json.dumps(out["stability_cfg2"]), flush=True)
    del runs, base, plain, A, b, y01, words
    torch.cuda.empty_cache()
print(json.dumps(out))
if len(sys.argv) > 1:                           # optional: also write the results to the given JSON file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
