#!/usr/bin/env python3
"""The working set and the duality gap of the multinomial lockstep against what they stand beside.

1. One fos_multinomial_duality_gap call against one fos_multinomial_gradient_batch call on the SAME handle, 16 columns (four fits
   of C = 4) and 14 (two of C = 7), HIP events around each, the two interleaved: cfg2 (65536 x 8192 fp32), the bf16 shard of config
   5 (131072 x 16384) and 262144 x 256 fp32.  The certificate is the gradient's launches, a column pass, product 1 once more with
   the fp64 row pass behind it and a finish: three reads of A against two, so about 1.5 x is expected from the traffic.
2. multinomial_working_set_path and multinomial_certified_path against multinomial_path on the same handle with the same L and
   max_iter, on a planted-support problem (64 rows of X non-zero, labels drawn from the softmax of the planted logits scaled to a
   standard deviation of 2, 8 weights from 0.5 to 0.05 of multinomial_alpha_max; l1 and grouped): wall time with the device idle
   before and after, rounds, set sizes, certificates, the device's gap of every answer and the distance between the answers.
Nothing is gated on a time.

    python tools/bench_multinomial_ws.py [OUT.json]
        FOS_BENCH_ITERS   lockstep iterations per round and of multinomial_path (default 500)
        FOS_BENCH_REPEATS timed calls per form, interleaved (default 5)
        FOS_BENCH_SHAPES  comma-separated subset of cfg2,cfg5_shard,narrow
        FOS_BENCH_CLASSES comma-separated class counts (default 4,7)"""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fastoptsolver_amd as fos
from fastoptsolver_amd import iterative_solvers as its
from bench import make_shard, WORKLOADS
torch.cuda.set_device(0)
ITERS = int(os.environ.get("FOS_BENCH_ITERS", "500"))
REPEATS = int(os.environ.get("FOS_BENCH_REPEATS", "5"))
CLASSES = [int(c) for c in os.environ.get("FOS_BENCH_CLASSES", "4,7").split(",")]
WEIGHTS, SUPPORT = 8, 64
SHAPES = {"cfg2": WORKLOADS["cfg2"], "cfg5_shard": dict(WORKLOADS["cfg5"], m=131072),
          "narrow": dict(WORKLOADS["cfg2"], m=262144, n=256)}


def planted_labels(A, C, seed=1):
    """Labels drawn from the softmax of A X for an X with SUPPORT non-zero rows (the Gumbel trick), the logits scaled to a
    standard deviation of 2."""
    m, n = A.shape
    rng = np.random.default_rng(seed)
    X = np.zeros((n, C), dtype=np.float32)
    X[rng.choice(n, size=SUPPORT, replace=False)] = rng.standard_normal((SUPPORT, C)).astype(np.float32)
    Xd = torch.from_numpy(X).to(A.device)
    Z = torch.empty(m, C, dtype=torch.float32, device=A.device)
    for r0 in range(0, m, 8192):
        Z[r0:r0 + 8192] = A[r0:r0 + 8192].float() @ Xd
    Z *= 2.0 / float(Z.std())
    g = torch.Generator(device=A.device).manual_seed(seed)
    u = torch.rand(m, C, generator=g, device=A.device).clamp_(1e-12, 1.0 - 1e-7)
    return torch.argmax(Z - torch.log(-torch.log(u)), dim=1).cpu().numpy()


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


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


out = {"iters": ITERS, "repeats": REPEATS, "weights": WEIGHTS, "support": SUPPORT}
for name in os.environ.get("FOS_BENCH_SHAPES", "cfg2,cfg5_shard,narrow").split(","):
    cfg = SHAPES[name]
    A, _ = make_shard(cfg, 0, cfg["m"], torch.device("cuda", 0))
    m, n = cfg["m"], cfg["n"]
    for C in CLASSES:
        y = planted_labels(A, C)
        res = {"shape": [m, n, cfg["dtype"]], "classes": C}
        for grouped in (False, True):
            P = fos.prepare_multinomial(A, y, C, grouped=grouped)
            np.random.seed(0)
            L = its._lipschitz(P, None, divisor=2.0)          # what multinomial_path takes when no L is given
            amax = fos.multinomial_alpha_max(P)
            alphas = [(float(a), 0.0) for a in amax * np.geomspace(0.5, 0.05, WEIGHTS)]
            per = 16 // C
            r = {"L": L, "alpha_max": amax}
            # 1. one certificate against one gradient, at a sparse point (the fits of a short path)
            fits = fos.multinomial_path(P, None, alphas[:per], max_iter=20, L=L)
            X = torch.cat([torch.as_tensor(f).float().cuda() for f in fits], dim=1)
            a1s, a2s = [a for a, _ in alphas[:per]], [a for _, a in alphas[:per]]
            forms = {"gradient_us": lambda: P.multinomial_gradient_block(X), "certificate_us": lambda: P.multinomial_duality_gap_block(X, a1s, a2s)}
            for fn in forms.values():              # warm-up: plans, workspaces, the first touch of every kernel
                fn()
            t = {k: [] for k in forms}
            for _ in range(REPEATS):
                for k, fn in forms.items():
                    t[k].append(events(fn))
            r.update({k: spread(v) for k, v in t.items()})
            r["certificate_over_gradient_median"] = r["certificate_us"]["median"] / r["gradient_us"]["median"]
            # 2. the two paths against multinomial_path
            paths = {"full": lambda: (fos.multinomial_path(P, None, alphas, max_iter=ITERS, L=L), None),
                     "working_set": lambda: fos.multinomial_working_set_path(P, None, alphas, max_iter=ITERS, L=L, return_info=True),
                     "certified": lambda: fos.multinomial_certified_path(P, None, alphas, None, 1e-4, ITERS, L=L, return_info=True)}
            for fn in paths.values():
                fn()
            w, got = {k: [] for k in paths}, {}
            for _ in range(REPEATS):
                for k, fn in paths.items():
                    dt, got[k] = wall(fn)
                    w[k].append(dt * 1e3)
            r.update({k + "_path_ms": spread(v) for k, v in w.items()})
            for k in ("working_set", "certified"):
                xs, infos = got[k]
                gap = fos.multinomial_duality_gap(P, xs, alphas)
                r[k] = dict(rounds=[i.rounds for i in infos], sizes=[list(i.sizes) for i in infos], fell_back=[bool(i.fell_back) for i in infos],
                            gap_over_primal_max=float((gap.gap / gap.primal).max()),
                            distance_from_full_max=max(rel(a, b) for a, b in zip(xs, got["full"][0])))
                r[k + "_speedup_median"] = r["full_path_ms"]["median"] / r[k + "_path_ms"]["median"]
            r["certified"]["certificates"] = [i.certificates for i in got["certified"][1]]
            r["certified"]["all_certified"] = all(bool(i.certified.all()) for i in got["certified"][1])
            gap = fos.multinomial_duality_gap(P, got["full"][0], alphas)
            r["full"] = dict(gap_over_primal_max=float((gap.gap / gap.primal).max()))
            res["grouped" if grouped else "l1"] = r
            del P, X, got
        print(name, json.dumps(res), flush=True)
        out[f"{name}_c{C}"] = res
    del A
    torch.cuda.empty_cache()
print(json.dumps(out))
if len(sys.argv) > 1:                           # optional: also write the results to the given JSON file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
