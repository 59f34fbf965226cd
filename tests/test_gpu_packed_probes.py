"""GPU: the packed gradient pass per element, per exception and per exception list (tests/_packed_probes.py names the probes,
the matrices and the bounds; tests/test_packed_probes.py proves the bounds on a NumPy model and shows which faults each probe
catches).  Every probe is one Problem.gemv_pair on a plan forced to pack (replan(no_resident=True, pack=True)): a row probe
returns a row of A - in-window elements bit for bit, exceptions through two roundings - a column probe the exact ||s A_j||^2,
the sum probes on `heavy` a gradient and a residual norm that are exact in every summation order, through a column of 130 and
a row of 200 exceptions.  The device packer, the byte permutes of the decode, the host's CSR / CSC sort and the two sparse
kernels have no other way to produce these numbers than to be right."""
import numpy as np
import pytest
import torch

from tests import _packed_probes as PP
from tests.test_packed_rows_gpu import rows_of

pytestmark = pytest.mark.gpu

NARROW = tuple(range(80, 257, 16)) + (512,)     # every multiple of 16 from 80 on, asked in turn for the narrowest served


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


class Device:
    """Two handles on one device matrix, forced to pack: one with a b of its own, which a probe overwrites in place (the
    handle borrows Problem.b: no re-preparation, the packed copy stays), one without b.  run(probe) -> (g, rr)."""

    def __init__(self, fos, case, interleave, At=None, pack_rows=None, packed=1):
        self.case, self.packed = case, packed
        if At is None:
            At = torch.as_tensor(case.A).cuda()
        self.pb, self.p0 = fos.prepare(At, np.zeros(case.m, dtype=np.float32)), fos.prepare(At, None)
        for p in (self.pb, self.p0):
            p.replan(no_resident=True, interleave=interleave, pack=True, **({} if pack_rows is None else dict(pack_rows=pack_rows)))
            assert p.plan()["packed"] == 0 and p.plan()["pack_rows"] == (pack_rows or p.plan()["pack_rows"]) != 0, p.plan()
        self.first = {id(self.pb): True, id(self.p0): True}
        self.rr = torch.zeros(1, dtype=torch.float64, device="cuda")

    def run(self, probe):
        b, y, alpha2 = probe
        p = self.p0 if b is None else self.pb
        if b is not None:
            p.b.copy_(torch.as_tensor(np.asarray(b, dtype=np.float32)))
        g = p.gemv_pair(torch.as_tensor(np.asarray(y, dtype=np.float32), device="cuda"), alpha2=alpha2, rr_out=self.rr).cpu().numpy()
        if self.first.pop(id(p), False):
            assert p.plan()["packed"] == self.packed, (self.case.name, p.plan())      # after each first gradient
        return g.copy(), float(self.rr.cpu())


def _report(case, il, worst):
    print(f"{case.name} {'interleaved' if il else 'blocks'}: window {case.e0}, {int(case.out.sum())} exceptions, "
          f"worst row error / bound {worst[0]:.2f}, worst column rr error / bound {worst[1]:.2f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


@pytest.mark.parametrize("il", [False, True])
@pytest.mark.parametrize("name", ["edges37x16368", "edges260x4112", "edges1x16384", "low", "high", "unsampled"])
def test_row_and_column_probes(fos, name, il):
    """edges: every special value at every position of a thread, at the first and last live thread, in the first, the last and
    a tail row.  low / high: the windows 2 and 238 (E0_MAX: the top byte E0 / 2 + 7 is at its limit of 126).  unsampled: row 1,
    which the window's sample skips, holds 7000 exceptions - packed all the same (0.93e-3), and rows 0, 1, 2 and a column
    through one of row 1's scaled elements come back right."""
    case = PP.case(name)
    dev = Device(fos, case, il)
    _report(case, il, PP.all_checks(case, dev.run))
    assert not dev.first and dev.pb.plan()["packed"] == 1 and dev.p0.plan()["packed"] == 1


@pytest.mark.parametrize("il", [False, True])
@pytest.mark.parametrize("R", rows_of(PP.HEAVY_SHAPE[1]))
def test_heavy_sum_probes_for_every_rows_per_burst(fos, R, il):
    """heavy: 930 exceptions (0.87e-3), a column with 130 (the lane loop of pk_dtr_kernel takes a third trip), a row with 200
    of which 32 fill two threads (the slot hand-out of pack_rows_kernel, the host's re-sort): the sum probes bit for bit, and
    the row and column probes, at every rows-per-burst the geometry instantiates."""
    case = PP.case("heavy")
    dev = Device(fos, case, il, pack_rows=R)
    _report(case, il, PP.all_checks(case, dev.run))
    assert dev.pb.plan()["pack_rows"] == R and dev.pb.plan()["packed"] == 1


@pytest.mark.parametrize("il", [False, True])
def test_over_the_cap_the_raw_pass_holds_the_probes(fos, il):
    """heavy with 360 more exceptions (1.2e-3): refused, and the same probes hold on the raw pass."""
    case = PP.case("heavy_over_cap")
    dev = Device(fos, case, il, packed=0)
    _report(case, il, PP.all_checks(case, dev.run))
    assert dev.pb.plan()["packed"] == 0 and dev.p0.plan()["packed"] == 0


@pytest.mark.parametrize("il", [False, True])
def test_row_strided_matrix(fos, il):
    """edges as the first n columns of a tensor n + 32 wide whose other columns are NaN: packed (a NaN read by the packer or by
    the window's sample would have refused it), and every probe bit for bit what the contiguous copy gives."""
    case = PP.case("edges260x4112")
    wide = torch.full((case.m, case.n + 32), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :case.n] = torch.as_tensor(case.A)
    view = wide[:, :case.n]
    assert view.stride(0) == case.n + 32
    strided, dense = Device(fos, case, il, At=view), Device(fos, case, il)
    assert strided.pb.lda == case.n + 32 and strided.pb.A.data_ptr() == wide.data_ptr()       # borrowed, not copied

    def both(probe):
        g, rr = strided.run(probe)
        g2, rr2 = dense.run(probe)
        assert g.tobytes() == g2.tobytes() and rr == rr2, (case.name, "strided differs from contiguous")
        return g, rr
    _report(case, il, PP.all_checks(case, both))
    assert strided.pb.plan()["packed"] == 1 and strided.p0.plan()["packed"] == 1


def test_narrowest_served_width(fos):
    """The narrowest n the packed pass is served for, found by asking the planner - 144 where the row-per-thread plans end at
    128 columns: 9 live threads of 512 beside 503 dead ones, on the grid of the narrowest streaming geometry."""
    for n in NARROW:
        probe = fos.prepare(torch.zeros(515, n, device="cuda"), None)
        probe.replan(no_resident=True, pack=True)
        if probe.plan()["pack_rows"] != 0:
            break
    else:
        pytest.skip(f"no width of {NARROW} is served by the packed pass")
    print(f"narrowest width served: {n}")
    case = PP.case(f"edges515x{n}")
    for il in (False, True):
        dev = Device(fos, case, il)
        _report(case, il, PP.all_checks(case, dev.run))
        assert dev.pb.plan()["packed"] == 1
