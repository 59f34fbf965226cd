#!/usr/bin/env python3
"""Rows per burst of the packed gradient pass, in one process on one handle: replan(pack_rows=R) for R = 1, 2, 3 in
interleaved rounds, both row orders, on an m x 16384 fp32 matrix (default 131072 rows, 8 GiB).  A second view beside the
parent / branch runs of bench.py (profiles/packed/README.md); each replan packs again, which is not timed.

    python tools/bench_pack_rows.py [m]
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastoptsolver_amd as fos      # noqa: E402

torch.cuda.set_device(0)
m, n = (int(sys.argv[1]) if len(sys.argv) > 1 else 131072), 16384
gen = torch.Generator(device="cuda")
gen.manual_seed(0)
A = torch.randn(m, n, device="cuda", generator=gen)
b = torch.randn(m, device="cuda", generator=gen)
y = torch.randn(n, device="cuda", generator=gen)
prob = fos.prepare(A, b)
for il in (False, True):
    res = {}
    for rnd in range(3):
        for R in (1, 2, 3):
            prob.replan(interleave=il, pack=True, pack_rows=R)
            for _ in range(3):
                prob.gemv_pair(y)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(40):
                prob.gemv_pair(y)
            torch.cuda.synchronize()
            res.setdefault(R, []).append((time.perf_counter() - t0) / 40 * 1e6)
            assert prob.plan()["packed"] == 1 and prob.plan()["pack_rows"] == R
    for R in (1, 2, 3):
        print(f"interleave={il} pack_rows={R} us per gemv_pair call (3 rounds of 40): " + " ".join(f"{t:.1f}" for t in res[R]), flush=True)
