#!/usr/bin/env python3
"""One fos_kkt_scan, one fos_duality_gap and one fos_gradient_batch call on the SAME handle, HIP events around each, the three
interleaved: the scan alone, which tools/bench_working_set.py and tools/bench_duality.py only time inside whole paths.

Shapes of those tools: cfg2 (65536 x 8192 fp32) and the bf16 shard of config 5 (131072 x 16384).  16 columns at a sparse X (1 % of
the entries non-zero), weights from 0.3 to 0.9 of the largest gradient entry, alpha2 = 0 on the even columns and 0.5 on the odd
ones, every seventh coordinate in the set, slack 1e-4.  The scan runs on a resident G and is enqueued through the C ABI (the
`Problem` method waits for the violator count).  Two warm-up calls per form.  Nothing is gated on a time.

    python tools/bench_ws_calls.py [OUT.json]
        FOS_BENCH_REPEATS timed calls per form, interleaved (default 9)
        FOS_BENCH_SHAPES  comma-separated subset of cfg2,cfg5_shard
        FOS_BENCH_LIB     another build of libfos_hip.so to load instead of the tree's (a build of another commit, for an A/B in
                          one visit: run the two alternately, each in a process of its own)"""
import ctypes as C
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastoptsolver_amd import _lib
if os.environ.get("FOS_BENCH_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["FOS_BENCH_LIB"])
import numpy as np
import torch
import fastoptsolver_amd as fos
from bench import make_shard, WORKLOADS
torch.cuda.set_device(0)
REPEATS = int(os.environ.get("FOS_BENCH_REPEATS", "9"))
NV = 16
SHAPES = {"cfg2": WORKLOADS["cfg2"], "cfg5_shard": dict(WORKLOADS["cfg5"], m=131072)}


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def spread(v):
    return dict(min=min(v), median=float(np.median(v)), max=max(v), runs=v)


ptr = lambda t: C.c_void_p(t.data_ptr())
out = {"lib": _lib.LIB_PATH, "repeats": REPEATS, "columns": NV}
for name in os.environ.get("FOS_BENCH_SHAPES", "cfg2,cfg5_shard").split(","):
    cfg = SHAPES[name]
    A, b = make_shard(cfg, 0, cfg["m"], torch.device("cuda", 0))
    P = fos.prepare(A, b)
    n = P.n_dev
    g = torch.Generator(device="cuda").manual_seed(1)
    X = (0.05 * torch.randn(n, NV, generator=g, device="cuda") * (torch.rand(n, NV, generator=g, device="cuda") < 0.01)).float()
    G = P.gradient_block(X)
    top = float(G.abs().max())
    a1s = [top * (0.3 + 0.04 * j) for j in range(NV)]
    a2s = [0.0 if j % 2 == 0 else 0.5 for j in range(NV)]
    a1 = (C.c_double * NV)(*a1s)
    in_ws = (torch.arange(n, device="cuda") % 7 == 0).to(torch.uint8)
    excess = torch.empty(n, dtype=torch.float32, device="cuda")
    viol = torch.empty(n, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")

    def scan():
        with P.ctx():
            _lib.check(P.lib.fos_kkt_scan(ptr(G), NV, a1, 1e-4, ptr(in_ws), P.h, ptr(excess), ptr(viol), ptr(count)), "fos_kkt_scan")

    forms = {"scan_us": scan, "certificate_us": lambda: P.duality_gap_block(X, a1s, a2s), "gradient_us": lambda: P.gradient_block(X)}
    for fn in forms.values():                      # warm-up: plans, workspaces, the first touch of every kernel
        fn(); fn()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(REPEATS):
        for k, fn in forms.items():
            t[k].append(events(fn))
    res = {"shape": [cfg["m"], cfg["n"], cfg["dtype"]], "violators": int(count.item()), **{k: spread(v) for k, v in t.items()}}
    print(name, json.dumps(res), flush=True)
    out[name] = res
    del P, A, X, G
    torch.cuda.empty_cache()
print(json.dumps(out))
if len(sys.argv) > 1:                           # optional: also write the results to the given JSON file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(out, open(sys.argv[1], "w"), indent=1)
