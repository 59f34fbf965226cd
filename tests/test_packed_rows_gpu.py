"""Rows per burst of the packed gradient pass (csrc/gemv_packed.hpp): the pass drains its loads every R rows, R picked per
plan with replan(pack_rows=).  Every row sees the same operations in the same order for every R, so the gradient, rr and
whole FISTA runs must agree BIT FOR BIT between the R of one handle, and R = 1 with the build before bursts
(tests/golden/packed_parent.npz, recorded with tools/record_packed_parent.py on an MI355X with 256 CUs); the fp64 oracle keeps
those identities from passing on garbage."""
import os

import numpy as np
import pytest
import torch

from tests import _data
from tests.test_packed_gpu import TOL, _case          # the matrices with planted out-of-window elements, built once per shape

pytestmark = pytest.mark.gpu

# On 256 CUs: 257 rows: one workgroup has 2 rows, the rest 1 (a burst that is all tail); 515: 3 and 2 rows per workgroup (exact and
# tail bursts for R = 2, 3); 1283: 6 and 5 rows (several full bursts, then a tail of 1 or 2); 3: workgroups with no rows at all;
# 16368 columns: dead threads; 8192 and 4112 columns: the 512-thread geometry, the latter with a partly filled last plane.
SHAPES = [(257, 16384), (515, 16384), (1283, 16384), (3, 16384), (37, 16368), (515, 8192), (260, 4112)]
CASES = [(m, n, il, wb) for (m, n) in SHAPES for il in (False, True) for wb in (True, False)]
# cases whose whole gradient is in the fixture (every case has its rr there): 400 KB of fp32
FIXTURE_GRADIENTS = [(515, 16384, False, True), (515, 16384, True, True), (1283, 16384, True, True), (257, 16384, False, True),
                     (37, 16368, False, True), (515, 8192, False, True), (515, 8192, True, True), (260, 4112, True, True)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_parent.npz")


def key(m, n, il, wb):
    return f"{m}x{n}_{'il' if il else 'blocks'}_{'b' if wb else 'nob'}"


def rows_of(n):
    """Rows per burst instantiated for the geometry of n columns (512 threads up to 8192 columns, 1024 above)."""
    return (1, 2, 3, 4) if n <= 8192 else (1, 2, 3)


def planner_rows(n, il):
    return 4 if n <= 8192 else (3 if il else 2)         # fos_plan.hip pack_rows


def gradient(prob, y):
    """(g as fp32 bits, rr as a float) of one packed gradient at alpha2 = 0.3."""
    rr = torch.zeros(1, dtype=torch.float64, device="cuda")
    g = prob.gemv_pair(torch.as_tensor(y, device="cuda"), alpha2=0.3, rr_out=rr).cpu().numpy()
    return g.view(np.uint32).copy(), float(rr.cpu())


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("m,n,il,wb", CASES, ids=[key(*c) for c in CASES])
def test_gradient_same_bits_for_every_rows_per_burst(fos, golden, m, n, il, wb):
    A, b, y, ref_b, ref_0 = _case(m, n)
    g_ref, rr_ref = ref_b if wb else ref_0
    prob = fos.prepare(A, b if wb else None)
    got = {}
    for R in rows_of(n):
        prob.replan(no_resident=True, interleave=il, pack=True, pack_rows=R)
        assert prob.plan()["pack_rows"] == R and prob.plan()["packed"] == 0
        got[R] = gradient(prob, y)
        plan = prob.plan()
        assert plan["packed"] == 1 and plan["pack_rows"] == R and plan["interleave"] == int(il), plan
    g1, rr1 = got[1]
    # (c) the oracle: the bitwise checks below cannot all pass on garbage
    assert _data.rel(g1.view(np.float32).astype(np.float64), g_ref) < TOL
    assert rr1 == pytest.approx(rr_ref, rel=TOL)
    # (a) R > 1 against R = 1 on the same handle
    for R in rows_of(n)[1:]:
        assert (got[R][0] == g1).all() and got[R][1] == rr1, f"R = {R} differs from R = 1"
    # (b) R = 1 against the build before bursts
    k = key(m, n, il, wb)
    assert rr1 == float(golden["rr_" + k]), (rr1, float(golden["rr_" + k]))
    if (m, n, il, wb) in FIXTURE_GRADIENTS:
        assert (g1 == golden["g_" + k].view(np.uint32)).all()


@pytest.mark.parametrize("m,n", SHAPES)
@pytest.mark.parametrize("il", [False, True])
def test_fista_same_bits_for_every_rows_per_burst(fos, m, n, il):
    A, b, y, ref_b, ref_0 = _case(m, n)
    A64 = A.astype(np.float64)
    L = float((A64 * A64).sum())                            # ||A||_F^2 >= ||A||_2^2: a valid step without a power iteration
    lam = 0.1 * float(np.abs(A64.T @ b.astype(np.float64)).max())
    prob = fos.prepare(A, b)
    xs = {}
    for R in rows_of(n):
        prob.replan(no_resident=True, interleave=il, pack=True, pack_rows=R)
        x = fos.fista(prob, None, "elasticnet", lam, 0.5, max_iter=8, L=L)
        xs[R] = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).copy()
        plan = prob.plan()
        assert plan["packed"] == 1 and plan["pack_rows"] == R, plan
    assert np.isfinite(xs[1]).all() and np.abs(xs[1]).max() > 0
    for R in rows_of(n)[1:]:
        assert xs[R].tobytes() == xs[1].tobytes(), f"R = {R} differs from R = 1"


def test_pack_rows_is_reported_and_dropped_with_the_copy(fos):
    A, b, y, _, _ = _case(515, 16384)
    prob = fos.prepare(A, b)
    for il in (False, True):
        prob.replan(no_resident=True, interleave=il, pack=True)
        assert prob.plan()["pack_rows"] == planner_rows(16384, il)          # the planner's, before and after packing
        g_plan = gradient(prob, y)
        assert prob.plan()["packed"] == 1 and prob.plan()["pack_rows"] == planner_rows(16384, il)
        prob.replan(no_resident=True, interleave=il, pack=True, pack_rows=1)
        g1 = gradient(prob, y)
        assert prob.plan()["packed"] == 1 and prob.plan()["pack_rows"] == 1
        assert (g1[0] == g_plan[0]).all() and g1[1] == g_plan[1]
        prob.tune(1024, 4, 1)                               # an invalidating call drops the copy and the override with it
        assert prob.plan()["packed"] == 0 and prob.plan()["pack_rows"] == planner_rows(16384, il)
        g2 = gradient(prob, y)
        assert prob.plan()["packed"] == 1 and (g2[0] == g1[0]).all()
        prob.replan(no_resident=True, interleave=il, pack=True, pack_rows=1)
        prob.replan(no_resident=True, interleave=il, pack=True)             # so does a replan without the argument
        assert prob.plan()["pack_rows"] == planner_rows(16384, il)
    from fastoptsolver_amd._lib import FosError
    with pytest.raises(FosError):
        prob.replan(pack=True, pack_rows=4)                 # 1024 threads: 1 .. 3 were measured and are instantiated
    with pytest.raises(ValueError):
        prob.replan(pack=True, pack_rows=5)
    A8, b8, y8, _, _ = _case(515, 8192)
    p8 = fos.prepare(A8, b8)
    p8.replan(no_resident=True, pack=True)
    assert p8.plan()["pack_rows"] == planner_rows(8192, False) == 4
