#!/usr/bin/env python3
"""Working-set solve against the full lockstep: working_set_path and fista_path on the SAME handle in the same process, same
max_iter and L, 16 weights from 0.5 to 0.05 of alpha_max on a planted-support problem (64 non-zeros, noise 0.1) - cfg2
(65536 x 8192 fp32), the bf16 shard of config 5 (131072 x 16384) and 262144 x 256 fp32, where a working set has little to
save.  fista_path is the full lockstep as it stands, so its time is the baseline.  Wall time around each call with the device
idle before and after (the outer loop's host work - index bookkeeping, the sub-handle, the power iteration of no sub-problem: L
is given - is part of what a caller pays).  Rounds, set sizes and gradient passes are recorded, and the distance between the two
answers.  Then the gather kernel alone on the final set's size (HIP events) against fos_stream_read_probe over the same A.
Nothing is gated on a time.

    python tools/bench_working_set.py [OUT.json]
        FOS_BENCH_ITERS   lockstep iterations per solve / per round (default 500)
        FOS_BENCH_REPEATS timed calls per form, interleaved (default 3)
        FOS_BENCH_SHAPES  comma-separated subset of cfg2,cfg5_shard,narrow"""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fastoptsolver_amd as fos
from fastoptsolver_amd import _core
from bench import make_shard, WORKLOADS
torch.cuda.set_device(0)
ITERS = int(os.environ.get("FOS_BENCH_ITERS", "500"))
REPEATS = int(os.environ.get("FOS_BENCH_REPEATS", "3"))
NV, SUPPORT = 16, 64
SHAPES = {"cfg2": WORKLOADS["cfg2"], "cfg5_shard": dict(WORKLOADS["cfg5"], m=131072),
          "narrow": dict(WORKLOADS["cfg2"], m=262144, n=256)}


def planted(A, seed=1):
    """b = A x + 0.1 noise for an x with SUPPORT non-zeros of magnitude 1..2 (row blocks: no fp32 copy of a bf16 A)."""
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
    forms = {"working_set": lambda: fos.working_set_path(P, None, alphas, ITERS, L=L, return_info=True),
             "fista_path": lambda: fos.fista_path(P, None, alphas, max_iter=ITERS, L=L)}
    for fn in forms.values():                      # warm-up: plans, workspaces, the first-touch of every kernel
        fn()
    t = {k: [] for k in forms}
    for _ in range(REPEATS):
        for k, fn in forms.items():
            dt, res = wall(fn)
            t[k].append(dt * 1e3)
            if k == "working_set":
                xs, infos = res
            else:
                ys = res
    info = infos[0]
    X, Y = torch.stack(xs, dim=1).double(), torch.stack(ys, dim=1).double()
    res = {"shape": [m, n, cfg["dtype"]], "L": L, "alpha_max": amax, "rounds": info.rounds, "sizes": info.sizes,
           "full_gradients": info.full_gradients, "worst_excess": info.worst_excess, "fell_back": info.fell_back,
           "working_set_ms": spread(t["working_set"]), "fista_path_ms": spread(t["fista_path"]),
           "nonzeros_per_weight": [int(v) for v in (X != 0).sum(dim=0).tolist()],
           "relative_distance_to_fista_path": [float(v) for v in ((X - Y).norm(dim=0) / Y.norm(dim=0).clamp_min(1e-300)).tolist()]}
    res["fista_path_over_working_set_median"] = res["fista_path_ms"]["median"] / res["working_set_ms"]["median"]
    # the gather kernel alone, on a set of the final size spread over all columns, against a read-only pass over the same A
    n_ws = max(info.sizes) if info.sizes else max(1, n // 16)
    idx = torch.from_numpy(np.sort(np.random.default_rng(2).choice(n, size=n_ws, replace=False))).cuda()
    n_pad = max(128, (n_ws + 63) // 64 * 64)
    buf = torch.empty(m, n_pad, dtype=A.dtype, device="cuda")
    P.gather_columns(idx, n_pad, out=buf)
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); P.gather_columns(idx, n_pad, out=buf); e1.record(); e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    probe_gbps, probe_us = _core.stream_read_probe(A)
    esz = A.element_size()
    lines = len(np.unique(idx.cpu().numpy() * esz // 128))
    res["gather"] = {"n_ws": n_ws, "n_ws_pad": n_pad, "us": spread(us), "read_probe_us": probe_us, "read_probe_gbps": probe_gbps,
                     "lines_touched_fraction_of_row": lines * 128 / (n * esz),
                     "gbps_of_full_A_plus_write": (m * n * esz + m * n_pad * esz) / (float(np.median(us)) * 1e-6) / 1e9,
                     "gather_over_read_probe": float(np.median(us)) / probe_us}
    print(name, json.dumps(res), flush=True)
    out[name] = res
    del P, A, buf, xs, ys, X, Y
    torch.cuda.empty_cache()
print(json.dumps(out))
if len(sys.argv) > 1:                           # optional: also write the results to the given JSON file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
