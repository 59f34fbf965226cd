#!/usr/bin/env python3
"""The duality-gap certificate against the gradient it contains, and the gap-stopped path against the KKT-stopped one.

1. One fos_duality_gap call against one fos_gradient_batch call on the SAME handle, 16 columns, HIP events around each, the two
   interleaved: cfg2 (65536 x 8192 fp32), the bf16 shard of config 5 (131072 x 16384) and 262144 x 256 fp32.  The certificate is
   the gradient's launches, a column pass, product 1 once more with the fp64 row pass behind it and a finish: three reads of A
   against two, so about 1.5 x is expected from the traffic.
2. certified_path against working_set_path on the planted-support problem of tools/bench_working_set.py (64 non-zeros, noise
   0.1, 16 weights from 0.5 to 0.05 of alpha_max), same handle, same max_iter and L: wall time with the device idle before and
   after, rounds, set sizes, certificates, and the device's gap of both answers.
Nothing is gated on a time.

    python tools/bench_duality.py [OUT.json]
        FOS_BENCH_ITERS   lockstep iterations per round (default 500)
        FOS_BENCH_REPEATS timed calls per form, interleaved (default 5)
        FOS_BENCH_SHAPES  comma-separated subset of cfg2,cfg5_shard,narrow"""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fastoptsolver_amd as fos
from bench import make_shard, WORKLOADS
torch.cuda.set_device(0)
ITERS = int(os.environ.get("FOS_BENCH_ITERS", "500"))
REPEATS = int(os.environ.get("FOS_BENCH_REPEATS", "5"))
NV, SUPPORT = 16, 64
SHAPES = {"cfg2": WORKLOADS["cfg2"], "cfg5_shard": dict(WORKLOADS["cfg5"], m=131072),
          "narrow": dict(WORKLOADS["cfg2"], m=262144, n=256)}


def planted(A, seed=1):
    """tools/bench_working_set.py's right-hand side: b = A x + 0.1 noise for an x with SUPPORT non-zeros of magnitude 1..2."""
    m, n = A.shape
    rng = np.random.default_rng(seed)
    x = np.zeros(n, dtype=np.float32)
    x[rng.choice(n, size=SUPPORT, replace=False)] = (rng.choice([-1.0, 1.0], SUPPORT) * rng.uniform(1.0, 2.0, SUPPORT)).astype(np.float32)
    xd = torch.from_numpy(x).to(A.device)
    b = torch.empty(m, dtype=torch.float32, device=A.device)
    g = torch.Generator(device=A.device).manual_seed(seed)
    for r0 in range(0, m, 8192):
        b[r0:r0 + 8192] = A[r0:r0 + 8192].float() @ xd
    return b + 0.1 * torch.randn(m, generator=g, device=A.device)


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(v):
    return dict(min=min(v), median=float(np.median(v)), max=max(v), runs=v)


out = {"iters": ITERS, "repeats": REPEATS, "weights": NV, "support": SUPPORT}
for name in os.environ.get("FOS_BENCH_SHAPES", "cfg2,cfg5_shard,narrow").split(","):
    cfg = SHAPES[name]
    A, _ = make_shard(cfg, 0, cfg["m"], torch.device("cuda", 0))
    m, n = cfg["m"], cfg["n"]
    P = fos.prepare(A, planted(A))
    np.random.seed(0)
    L = fos.estimate_lipschitz(P)
    amax = fos.alpha_max(P)
    alphas = [(float(a), 0.0) for a in amax * np.geomspace(0.5, 0.05, NV)]
    a1s, a2s = [a for a, _ in alphas], [a for _, a in alphas]
    # 1. one certificate against one gradient, at a sparse point (the columns of a short path)
    X = torch.stack(fos.fista_path(P, None, alphas, max_iter=20, L=L), dim=1).float()
    forms = {"gradient_us": lambda: P.gradient_block(X), "certificate_us": lambda: P.duality_gap_block(X, a1s, a2s)}
    for fn in forms.values():                      # warm-up: plans, workspaces, the first touch of every kernel
        fn()
    t = {k: [] for k in forms}
    for _ in range(REPEATS):
        for k, fn in forms.items():
            t[k].append(events(fn))
    res = {"shape": [m, n, cfg["dtype"]], "L": L, "alpha_max": amax, **{k: spread(v) for k, v in t.items()}}
    res["certificate_over_gradient_median"] = res["certificate_us"]["median"] / res["gradient_us"]["median"]
    # 2. the gap-stopped path against the KKT-stopped one
    paths = {"certified": lambda: fos.certified_path(P, None, alphas, 1e-4, ITERS, L=L, return_info=True),
             "working_set": lambda: fos.working_set_path(P, None, alphas, ITERS, L=L, return_info=True)}
    for fn in paths.values():
        fn()
    w = {k: [] for k in paths}
    got = {}
    for _ in range(REPEATS):
        for k, fn in paths.items():
            dt, got[k] = wall(fn)
            w[k].append(dt * 1e3)
    ci, wi = got["certified"][1][0], got["working_set"][1][0]
    gap_ws = fos.duality_gap(P, got["working_set"][0], alphas)
    res.update({"certified_path_ms": spread(w["certified"]), "working_set_path_ms": spread(w["working_set"]),
                "certified": dict(rounds=ci.rounds, sizes=ci.sizes, certificates=ci.certificates, fell_back=ci.fell_back,
                                  all_certified=bool(ci.certified.all()), gap_over_primal_max=float((ci.gap / ci.primal).max())),
                "working_set": dict(rounds=wi.rounds, sizes=wi.sizes, full_gradients=wi.full_gradients, fell_back=wi.fell_back,
                                    gap_over_primal_max=float((gap_ws.gap / gap_ws.primal).max()))})
    res["certified_over_working_set_median"] = res["certified_path_ms"]["median"] / res["working_set_path_ms"]["median"]
    print(name, json.dumps(res), flush=True)
    out[name] = res
    del P, A, X, got
    torch.cuda.empty_cache()
print(json.dumps(out))
if len(sys.argv) > 1:                           # optional: also write the results to the given JSON file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
