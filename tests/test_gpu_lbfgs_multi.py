"""GPU: several targets for L-BFGS - LBFGSSolver.fit(A, B) with a 2-D B (m x k).  On every dispatch branch (lockstep groups
of 3..16 columns on the fp64 matrix-core pair, groups plus a remainder, column by column for k = 2 and n <= 64) column j
must take the single-target native fit's decisions (nit_, nfev_, task_) and match its x_, final_obj_ and history_ to 1e-9
(same fp64 arithmetic, other summation order), and match the oracle's L-BFGS on the stored A to 1e-5.  The multi-point
pass on its own must match nv separate fos_gemv_pair_dd calls to 1e-12, reading and writing nothing past its operands."""
import numpy as np
import pytest
import torch

from oracle import fos_oracle as orc
from tests import _data

pytestmark = pytest.mark.gpu

TOL = 1e-5
SAME = 1e-9


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def _case(kind, m, n, k, seed, zero_col=1):
    """Device A (fp32 / bf16), its fp64 value as stored, and B (m x k fp32, column `zero_col` all zeros)."""
    rng = np.random.default_rng(seed)
    A, _, _ = _data.synth(m, n, seed)
    At = torch.as_tensor(A.astype(np.float32)).to(torch.bfloat16 if kind == "bf16" else torch.float32).cuda()
    A64 = At.to(torch.float64).cpu().numpy()
    X = np.zeros((n, k))
    for j in range(k):
        idx = rng.choice(n, max(1, n // 20), replace=False)
        X[idx, j] = rng.standard_normal(idx.size) * (1.0 + j % 3)
    B = (A64 @ X + 0.1 * (1.0 + np.arange(k) % 4) * rng.standard_normal((m, k))).astype(np.float32)
    if zero_col is not None and zero_col < k:
        B[:, zero_col] = 0.0
    return At, A64, B


REGS = {"ridge": ("ridge", 0.0, 1.0), "enet": ("elasticnet", 0.05, 0.5), "lasso": ("lasso", 0.05, 0.0)}


def _single(fos, P, B, j, reg, max_iter):
    from fastoptsolver_amd.lbfgs import LBFGSSolver
    sib = P.sibling(torch.as_tensor(B[:, j].copy()).cuda())
    return LBFGSSolver(*REGS[reg], max_iter=max_iter).fit(sib, None)


def _compare(fos, kind, m, n, k, reg, max_iter=40, seed=0, oracle_cols=None):
    from fastoptsolver_amd.lbfgs import LBFGSSolver
    At, A64, B = _case(kind, m, n, k, seed + 7 * n + k)
    P = fos.prepare(At)
    s = LBFGSSolver(*REGS[reg], max_iter=max_iter).fit(P, B)
    X = _np(s.x_)
    assert X.shape == (n, k)
    assert s.nit_.shape == (k,) and s.nfev_.shape == (k,) and len(s.task_) == k and s.final_obj_.shape == (k,)
    assert len(s.history_) == k and s.iterates_ == []
    assert s.nit_[1] == 0 and s.task_[1].startswith("CONVERGENCE: NORM") and np.all(X[:, 1] == 0.0)
    for j in range(k):
        one = _single(fos, P, B, j, reg, max_iter)
        assert (s.nit_[j], s.nfev_[j], s.task_[j]) == (one.nit_, one.nfev_, one.task_), j
        x1 = _np(one.x_)
        assert _data.rel(X[:, j], x1) <= SAME, (j, _data.rel(X[:, j], x1))
        assert abs(s.final_obj_[j] - one.final_obj_) <= SAME * max(abs(one.final_obj_), 1e-300), j
        assert len(s.history_[j]) == len(one.history_) and np.allclose(s.history_[j], one.history_, rtol=SAME, atol=0), j
    for j in (oracle_cols if oracle_cols is not None else range(k)):
        ref = orc.LBFGSSolver(*REGS[reg], max_iter=max_iter).fit(A64, B[:, j].astype(np.float64))
        assert _data.rel(X[:, j], ref.x_) < TOL, (j, _data.rel(X[:, j], ref.x_))
    return s


CASES = [("f32", 4096, 512, 3, "ridge"), ("f32", 4096, 512, 16, "ridge"),
         ("f32", 2000, 256, 17, "enet"),                       # a group plus a lone column
         ("f32", 1500, 384, 40, "ridge"),                      # 16 + 16 + 8
         ("bf16", 2000, 1024, 16, "enet"),
         ("f32", 1200, 1030, 5, "ridge"),                      # ragged n: padded device A
         ("f32", 70000, 128, 9, "ridge"),                      # two row panels
         ("f32", 3000, 512, 2, "ridge"),                       # k = 2: column by column
         ("f32", 500, 16, 3, "ridge"),                         # n <= 64: no multi-point pass, column by column
         ("f32", 3000, 2304, 4, "lasso"),                      # whole-chip direction (n >= 2048), smooth part only
         ("bf16", 4000, 2048, 6, "enet")]


@pytest.mark.parametrize("kind,m,n,k,reg", CASES)
def test_fit_multi_target_per_column(fos, kind, m, n, k, reg):
    oracle_cols = None if k <= 17 else (0, 15, 16, 31, 32, k - 1)
    _compare(fos, kind, m, n, k, reg, oracle_cols=oracle_cols)


def test_one_column_hits_max_iter(fos):
    """Columns stop on their own: with max_iter just below the slowest column's iteration count, that column stops on the
    limit while the others converge - each exactly as its single-target fit does."""
    from fastoptsolver_amd.lbfgs import LBFGSSolver
    At, A64, B = _case("f32", 3000, 512, 6, 41)
    B[:, 3] *= 50.0
    P = fos.prepare(At)
    free = LBFGSSolver("ridge", 0.0, 0.05, max_iter=500).fit(P, B)
    cap = int(np.max(free.nit_)) - 1
    assert cap >= 1 and np.sum(free.nit_ > cap) < 6
    s = LBFGSSolver("ridge", 0.0, 0.05, max_iter=cap).fit(P, B)
    hit = [j for j in range(6) if s.task_[j].startswith("STOP")]
    assert hit and len(hit) < 6, s.task_
    assert all(s.task_[j].startswith("CONVERGENCE") for j in range(6) if j not in hit)
    for j in range(6):
        one = LBFGSSolver("ridge", 0.0, 0.05, max_iter=cap).fit(P.sibling(torch.as_tensor(B[:, j].copy()).cuda()), None)
        assert (s.nit_[j], s.nfev_[j], s.task_[j]) == (one.nit_, one.nfev_, one.task_), j
        assert _data.rel(_np(s.x_)[:, j], _np(one.x_)) <= SAME, j


def test_passes_over_A_are_rounds(fos):
    """Both products of the multi-point pass are bracketed by the launch profiler: a lockstep fit of 16 columns on one row
    panel makes two A-pass launches per round, one gradient call per round, and far fewer passes than sum_j nfev_j."""
    from fastoptsolver_amd.iterative_solvers import get_metrics
    from fastoptsolver_amd.lbfgs import LBFGSSolver
    At, A64, B = _case("f32", 4096, 512, 16, 5)
    P = fos.prepare(At)
    P.profile(1)
    P.profile_read()
    s = LBFGSSolver("ridge", 0.0, 1.0, max_iter=40).fit(P, B)
    _, launches = P.profile_read()
    P.profile(0)
    rounds = get_metrics()["grad_num_calls"]
    assert launches == 2 * rounds, (launches, rounds)
    assert rounds >= int(np.max(s.nfev_)) and rounds < int(np.sum(s.nfev_)), (rounds, s.nfev_)


def test_result_types_follow_the_caller(fos):
    from fastoptsolver_amd.lbfgs import LBFGSSolver
    At, A64, B = _case("f32", 2000, 256, 4, 9)
    s = LBFGSSolver("ridge", 0.0, 1.0, max_iter=10).fit(At, torch.as_tensor(B).cuda())
    assert isinstance(s.x_, torch.Tensor) and tuple(s.x_.shape) == (256, 4) and s.x_.dtype == torch.float32
    s = LBFGSSolver("ridge", 0.0, 1.0, max_iter=10).fit(At.cpu().numpy(), B)
    assert isinstance(s.x_, np.ndarray) and s.x_.shape == (256, 4) and s.x_.dtype == np.float64
    assert s.nit_.dtype.kind == "i" and s.nfev_.dtype.kind == "i" and s.final_obj_.dtype == np.float64


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_pair_dd_multi_matches_single_passes(fos, kind):
    """fos_gemv_pair_dd_multi against nv separate fos_gemv_pair_dd calls (1e-12), nv = 1..16.  X, B, G and rr sit inside
    NaN-filled allocations with gaps between the columns: a read past an operand turns the result into NaN, a write past
    it leaves a non-NaN in the gaps."""
    from fastoptsolver_amd import _core, _lib
    lib = _lib.load()
    m, n, a2 = 3000, 520, 0.7
    At, A64, B = _case(kind, m, n, 16, 77, zero_col=None)
    P = fos.prepare(At)
    rng = np.random.default_rng(3)
    Xh = rng.standard_normal((16, n))
    pad, ldx = 64, n + 3
    for nv in range(1, 17):
        ldb = nv + 2
        xbuf = torch.full((2 * pad + nv * ldx,), float("nan"), dtype=torch.float64, device="cuda")
        gbuf = torch.full_like(xbuf, float("nan"))
        bbuf = torch.full((2 * pad + m * ldb,), float("nan"), dtype=torch.float32, device="cuda")
        rbuf = torch.full((2 * pad + nv,), float("nan"), dtype=torch.float64, device="cuda")
        Xv = xbuf[pad: pad + nv * ldx].view(nv, ldx)
        Xv[:, :n] = torch.as_tensor(Xh[:nv]).cuda()
        bbuf[pad: pad + m * ldb].view(m, ldb)[:, :nv] = torch.as_tensor(B[:, :nv]).cuda()
        with P.ctx():
            _lib.check(lib.fos_gemv_pair_dd_multi(P.h, _core.ptr(Xv), nv, ldx, _core.ptr(bbuf[pad:]), ldb, a2,
                                                  _core.ptr(gbuf[pad:]), _core.ptr(rbuf[pad:])), "fos_gemv_pair_dd_multi")
        torch.cuda.synchronize()
        G = gbuf[pad: pad + nv * ldx].view(nv, ldx)
        assert torch.isnan(gbuf[:pad]).all() and torch.isnan(gbuf[pad + nv * ldx:]).all()
        assert torch.isnan(G[:, n:]).all(), "write into the gap between columns"
        assert torch.isnan(rbuf[:pad]).all() and torch.isnan(rbuf[pad + nv:]).all()
        Gm, rr = G[:, :n].cpu().numpy(), rbuf[pad: pad + nv].cpu().numpy()
        assert np.all(np.isfinite(Gm)) and np.all(np.isfinite(rr))
        for j in range(nv):
            sib = P.sibling(torch.as_tensor(B[:, j].copy()).cuda())
            out = torch.empty(n + 1, dtype=torch.float64, device="cuda")
            xj = torch.as_tensor(Xh[j]).cuda()
            with sib.ctx():
                _lib.check(lib.fos_gemv_pair_dd(sib.h, _core.ptr(xj), a2, _core.ptr(out)), "fos_gemv_pair_dd")
            ref = out.cpu().numpy()
            assert _data.rel(Gm[j], ref[:n]) < 1e-12, (nv, j, _data.rel(Gm[j], ref[:n]))
            assert abs(rr[j] - ref[n]) <= 1e-12 * ref[n], (nv, j)
