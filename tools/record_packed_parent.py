"""Record tests/golden/packed_parent.npz: the packed gradient pass of the build in THIS tree on the cases of
tests/test_packed_rows_gpu.py (rr of every case, the whole fp32 gradient of FIXTURE_GRADIENTS).  Run it from a checkout of
the commit whose bits are to be kept (the one before rows per burst: it takes no pack_rows argument) with this file and that
test module copied in, on the part the tests run on (256 CUs: the rows a workgroup sums depend on the grid):

    python tools/record_packed_parent.py OUT.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import fastoptsolver_amd as fos                                    # noqa: E402
from tests.test_packed_gpu import _case                            # noqa: E402
from tests.test_packed_rows_gpu import CASES, FIXTURE_GRADIENTS, gradient, key   # noqa: E402


def main(out):
    torch.cuda.set_device(0)
    rec = {}
    for (m, n, il, wb) in CASES:
        A, b, y, _, _ = _case(m, n)
        prob = fos.prepare(A, b if wb else None)
        prob.replan(no_resident=True, interleave=il, pack=True)
        g, rr = gradient(prob, y)
        plan = prob.plan()
        assert plan["packed"] == 1 and plan["cus"] == 256, plan
        rec["rr_" + key(m, n, il, wb)] = np.float64(rr)
        if (m, n, il, wb) in FIXTURE_GRADIENTS:
            rec["g_" + key(m, n, il, wb)] = g.view(np.float32)
    np.savez(out, **rec)
    print(f"{out}: {len(rec)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
