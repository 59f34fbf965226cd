"""CPU, world_size 2, gloo: the row-sharded FISTA choreography of fastoptsolver_amd.distributed with a stand-in
engine built on the oracle (the HIP engine needs a GPU).  Checks: every rank ends with bit-identical iterates,
and they equal the unsharded oracle; sharded power iteration equals the unsharded one."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fastoptsolver_amd import distributed as fd   # noqa: E402
from oracle import fos_oracle as orc              # noqa: E402
from tests import _data                           # noqa: E402


class OracleShardEngine:
    """Same interface as HipShardEngine; arithmetic from the oracle (test infrastructure only)."""

    def __init__(self, A, b, tau, a1, a2):
        self.A, self.b = A, b
        self.n = A.shape[1]
        self.tau, self.a1, self.a2 = tau, a1, a2
        self.xk = np.zeros(self.n)
        self.xp = np.zeros(self.n)
        self.t, self.beta = 1.0, 0.0
        self.gbuf = torch.zeros(self.n + 4, dtype=torch.float64)

    def _y(self):
        return self.xk + self.beta * (self.xk - self.xp)

    def grad(self):
        g, rr = orc.gram_gradient(self.A, self._y(), self.b, 0.0)     # WITHOUT alpha2*y, like fos_fista_grad
        self.gbuf[: self.n] = torch.from_numpy(g)
        self.gbuf[self.n] = rr

    def update(self):
        y = self._y()
        g = self.gbuf[: self.n].numpy() + (self.a2 * y if self.a2 > 0 else 0.0)
        v = y - self.tau * g
        xn = orc.prox_l1(v, self.tau * self.a1) if self.a1 > 0 else v
        t_new = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * self.t ** 2))
        self.beta = (self.t - 1.0) / t_new
        self.t = t_new
        self.xp, self.xk = self.xk, xn

    def x(self):
        return self.xk


class NumpyVecOps:
    @staticmethod
    def norm(v):
        return float(torch.linalg.norm(v))

    @staticmethod
    def scale(v, a):
        return v * a


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    A, b, _ = _data.synth(1001, 48, 9)                       # ragged: 1001 rows over 2 ranks
    lam = float(np.max(np.abs(A.T @ b)))
    a1, a2 = 0.05 * lam, 0.5
    lo, hi = fd.shard_rows(A.shape[0], world, rank)
    As = torch.from_numpy(A[lo:hi])
    np.random.seed(0)
    v0 = torch.from_numpy(np.random.randn(48))
    L = fd.sharded_lipschitz(lambda v: As.T @ (As @ v), 48, v0, ops=NumpyVecOps)
    eng = OracleShardEngine(A[lo:hi], b[lo:hi], 1.0 / (L + a2), a1, a2)
    solver = fd.ShardedFista(eng)
    solver.run(40)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), x=solver.x(), L=L, rr=float(eng.gbuf[48]))
    dist.barrier()
    dist.destroy_process_group()


def test_shard_rows_cover_everything():
    for m in (1, 7, 1000, 65536, 2 ** 20):
        for world in (1, 2, 3, 4, 8):
            edges = [fd.shard_rows(m, world, r) for r in range(world)]
            assert edges[0][0] == 0 and edges[-1][1] == m
            assert all(edges[i][1] == edges[i + 1][0] for i in range(world - 1))
            sizes = [hi - lo for lo, hi in edges]
            assert max(sizes) - min(sizes) <= 1


@pytest.mark.timeout(300)
def test_two_rank_gloo_sharded_fista(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0 = np.load(tmp_path / "rank0.npz")
    r1 = np.load(tmp_path / "rank1.npz")
    assert np.array_equal(r0["x"], r1["x"]), "replicated iterates drifted apart"
    assert float(r0["L"]) == float(r1["L"])
    A, b, _ = _data.synth(1001, 48, 9)
    lam = float(np.max(np.abs(A.T @ b)))
    np.random.seed(0)
    v0 = np.random.randn(48)
    L_ref = orc.estimate_lipschitz(A, v0=v0)
    assert float(r0["L"]) == pytest.approx(L_ref, rel=1e-12)
    x_ref = orc.fista(A, b, "elasticnet", 0.05 * lam, 0.5, max_iter=40, L=L_ref)
    assert _data.rel(r0["x"], x_ref) < 1e-10


# --------------------------------------------------------------------------------------------------
# row-sharded L-BFGS: one all-reduce per fg, the real LBFGSSolver.fit with stand-in primitives
# --------------------------------------------------------------------------------------------------
class _NoTimer:
    def start(self):
        return None

    def stop(self, ev, count=1):
        pass

    def flush(self):
        pass


class OracleLbfgsOps:
    """Same interface as fastoptsolver_amd.lbfgs._HipOps; float64 torch CPU tensors, arithmetic from the oracle."""

    def __init__(self, A, b):
        self.A, self.b, self.n = A, b, A.shape[1]
        self.rr = torch.zeros(1, dtype=torch.float64)

    def timer(self, sink):
        return _NoTimer()

    def comm_buffer(self):
        return torch.zeros(self.n + 1, dtype=torch.float64)

    def new_x(self):
        return torch.zeros(self.n, dtype=torch.float64)

    def new_g(self):
        return torch.empty(self.n, dtype=torch.float64)

    def new_history(self, cap):
        return torch.zeros(cap, self.n, dtype=torch.float64), torch.zeros(cap, self.n, dtype=torch.float64)

    def grad(self, x, a2, g):
        gg, rr = orc.gram_gradient(self.A, x.numpy(), self.b, a2)
        g.copy_(torch.from_numpy(gg))
        self.rr[0] = rr

    def stats(self, x, g, d):
        z = torch.zeros(self.n, dtype=torch.float64)
        xx, dd_ = (x if x is not None else z), (d if d is not None else z)
        return [float(xx @ xx), float(g @ dd_), float(dd_ @ dd_), float(g.abs().max()), float(xx.abs().sum()),
                float(self.rr[0])]

    def direction(self, g, S, Y, hist, head):
        cap = S.shape[0]
        idx = [(head + i) % cap for i in range(hist)]
        return torch.from_numpy(orc.two_loop_direction(g.numpy(), [S[i].numpy() for i in idx], [Y[i].numpy() for i in idx]))

    def step_to(self, x_old, stp, d):
        return x_old + stp * d

    def store_pair(self, S, Y, slot, stp, d, g, g_old):
        S[slot] = stp * d
        Y[slot] = g - g_old

    def to_caller(self, x):
        return x.numpy().copy()


def _lbfgs_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from fastoptsolver_amd.lbfgs import LBFGSSolver
    A, b, _ = _data.synth(1001, 48, 9)
    lo, hi = fd.shard_rows(A.shape[0], world, rank)
    s = LBFGSSolver("elasticnet", 3.0, 0.7).fit(None, None, group=dist.group.WORLD, ops=OracleLbfgsOps(A[lo:hi], b[lo:hi]))
    np.savez(os.path.join(out_dir, f"lbfgs{rank}.npz"), x=s.x_, f=s.final_obj_, nit=s.nit_, nfev=s.nfev_,
             hist=np.asarray(s.history_))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_gloo_sharded_lbfgs(tmp_path):
    world = 2
    mp.spawn(_lbfgs_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0, r1 = np.load(tmp_path / "lbfgs0.npz"), np.load(tmp_path / "lbfgs1.npz")
    assert np.array_equal(r0["x"], r1["x"]) and int(r0["nfev"]) == int(r1["nfev"]), "replicas drifted apart"
    A, b, _ = _data.synth(1001, 48, 9)
    ref = orc.LBFGSSolver("elasticnet", 3.0, 0.7).fit(A, b)            # unsharded oracle (alpha2*x counted once)
    assert _data.rel(r0["x"], ref.x_) < 1e-8
    assert float(r0["f"]) == pytest.approx(ref.final_obj_, rel=1e-10)
    assert abs(int(r0["nit"]) - len(ref.history_)) <= 1
    k = min(len(r0["hist"]), len(ref.history_))
    assert np.allclose(r0["hist"][:k], ref.history_[:k], rtol=1e-9)    # callback objective incl. alpha1*||x||_1


# --------------------------------------------------------------------------------------------------
# split-form sharding of the FULL loop (backtracking, history, restart, stops): the product's driver
# (iterative_solvers._drive + _GroupReducer) with a NumPy stand-in for the device state machine
# --------------------------------------------------------------------------------------------------
class _Status:
    pass


class _HostTimer(_NoTimer):
    def __init__(self, sink):
        self.sink, self.pending = sink, []

    def stop(self, ev, count=1):
        self.sink.extend([0.0] * count)


class _FakeProblem:
    """What _drive / _GroupReducer touch on a Problem: gbuf, n, n_dev, device, residual_objective."""

    def __init__(self, A, b):
        self.A, self.b = A, b
        self.n = self.n_dev = A.shape[1]
        self.device = torch.device("cpu")
        self.gbuf = torch.zeros(self.n + 4, dtype=torch.float64)

    def residual_objective(self, x):
        x = x.numpy()
        r = self.A @ x - self.b
        return float(r @ r), float(x @ x), float(np.abs(x).sum())


class OracleFistaState:
    """Interface of fastoptsolver_amd._core.Fista (reset / grad / trial / update / status / x_tensor), arithmetic of
    reduce_update.hpp restated in NumPy float64 on THIS RANK's rows; test infrastructure only."""
    make_timer = _HostTimer

    def __init__(self, prob):
        self.p = prob

    def reset(self, tau, alpha1, alpha2, mode=0, prox_kind=0, delta=0.0, adaptive_restart=False, restart_threshold=1.0,
              tol_step=0.0, tol_ratio=0.0, x0=None):
        n = self.p.n
        self.tau, self.a1, self.a2, self.mode, self.delta = tau, alpha1, alpha2, mode, delta
        self.restart, self.thr, self.tol_step, self.tol_ratio = adaptive_restart, restart_threshold, tol_step, tol_ratio
        self.xc, self.xp = np.zeros(n), np.zeros(n)
        self.t, self.beta, self.k, self.stopped = 1.0, 0.0, 0, 0
        self.this_step, self.rr_x, self.x1, self.x2 = 0.0, 0.0, 0.0, 0.0

    def _y(self):
        return self.xc + self.beta * (self.xc - self.xp)

    def set_tau(self, tau):
        self.tau = tau

    def grad(self, dual=False):
        if self.stopped:
            return
        r = self.p.A @ self._y() - self.p.b
        self.p.gbuf[: self.p.n] = torch.from_numpy(self.p.A.T @ r)
        self.p.gbuf[self.p.n] = float(r @ r)
        if dual:
            rx = self.p.A @ self.xc - self.p.b
            self.rr_x = float(rx @ rx)

    def _trial_point(self, t):
        y = self._y()
        gf = self.p.gbuf[: self.p.n].numpy() + (self.a2 * y if self.a2 > 0 else 0.0)
        v = y - t * gf
        return y, gf, (orc.prox_l1(v, t * self.a1) if self.a1 > 0 else v)

    def trial(self, t, with_residual=True):
        y, gf, xt = self._trial_point(t)
        d = xt - y
        Ad = self.p.A @ d
        return dict(gd=float(gf @ d), dd=float(d @ d), nnz=float(np.count_nonzero(d)), gnorm2=float(gf @ gf),
                    y2=float(y @ y), q=float(Ad @ Ad) if with_residual else 0.0, rr_y=float(self.p.gbuf[self.p.n]))

    def trial_batch(self, t, eta, nv):
        return None

    def run_resident(self, *a, **k):
        return None

    def run_history(self, iters):
        return None

    def update(self):
        if self.stopped:
            return
        _, _, xn = self._trial_point(self.tau)
        step = float(np.linalg.norm(xn - self.xc))
        prev = self.this_step
        ratio = step / prev if prev > 0 else float("inf")
        if self.mode == 0:
            if self.restart and ratio > self.thr:
                t_new, beta = 1.0, 0.0
            else:
                t_new = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * self.t ** 2))
                beta = (self.t - 1.0) / t_new
            self.t = t_new
        elif self.mode == 1:
            kk = float(self.k + 1)
            beta = kk / (kk + 1.0 + self.delta)
        else:
            beta = 0.0
        self.beta, self.this_step = beta, step
        self.xp, self.xc = self.xc, xn
        self.x1, self.x2 = float(np.abs(xn).sum()), float(xn @ xn)
        self.k += 1
        if self.tol_step > 0 and step < self.tol_step:
            self.stopped = 1
        elif self.tol_ratio > 0 and ratio < self.tol_ratio:
            self.stopped = 2

    def status(self):
        s = _Status()
        s.stopped, s.k, s.rr_x, s.xnorm1, s.xnorm2, s.this_step = self.stopped, self.k, self.rr_x, self.x1, self.x2, self.this_step
        return s

    def x_tensor(self):
        return torch.from_numpy(self.xc.copy())


FLAG_CASES = [dict(), dict(backtracking=True, t_init=2.0), dict(adaptive_restart=True), dict(tol=2e-3), dict(tol_ratio=0.9),
              dict(mode=1, delta=3.0, backtracking=True, t_init=1.0)]


def _flags_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from fastoptsolver_amd import iterative_solvers as its
    A, b, _ = _data.synth(1001, 48, 9)
    lam = float(np.max(np.abs(A.T @ b)))
    a1, a2 = 0.05 * lam, 0.5
    L = float(np.linalg.norm(A, 2) ** 2)
    lo, hi = fd.shard_rows(A.shape[0], world, rank)
    out = {}
    for i, c in enumerate(FLAG_CASES):
        prob = _FakeProblem(A[lo:hi], b[lo:hi])
        history = {"x": [], "obj": []}
        mode = c.get("mode", 0)
        st = its._drive(prob, np.zeros(1), mode=mode, prox_kind=0, alpha1=a1, alpha2=a2, tau=c.get("t_init", 1.0) / (L + a2),
                        delta=c.get("delta", 0.0), backtracking=c.get("backtracking", False), max_iter=50,
                        tol=c.get("tol", 0.0), tol_ratio=c.get("tol_ratio", 0.0),
                        adaptive_restart=c.get("adaptive_restart", False), grad_tol_check=(mode == 0),
                        history=history, history_obj=its._objective_by_alpha(a1, a2),
                        reducer=its._GroupReducer(prob, dist.group.WORLD), state=OracleFistaState(prob))
        out[f"x{i}"], out[f"obj{i}"] = st.x_tensor().numpy(), np.asarray(history["obj"])
        out[f"ls{i}"] = np.asarray(its.get_metrics()["ls_iters_total"])
        its.reset_metrics()
    np.savez(os.path.join(out_dir, f"flags{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_gloo_every_flag_of_the_loop(tmp_path):
    """Backtracking (sum of ||A_p dlt||^2), history (sum of ||A_p x - b_p||^2, closing residual pass), adaptive
    restart and the three stopping rules on a row-sharded problem equal the unsharded oracle: same iterates, same
    objective history, same stopping iteration, same number of Armijo shrinks."""
    world = 2
    mp.spawn(_flags_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0, r1 = np.load(tmp_path / "flags0.npz"), np.load(tmp_path / "flags1.npz")
    for k in r0.files:
        assert np.array_equal(r0[k], r1[k]), f"replicas drifted apart: {k}"
    A, b, _ = _data.synth(1001, 48, 9)
    lam = float(np.max(np.abs(A.T @ b)))
    a1, a2 = 0.05 * lam, 0.5
    L = float(np.linalg.norm(A, 2) ** 2)
    for i, c in enumerate(FLAG_CASES):
        kw = dict(backtracking=c.get("backtracking", False), t_init_factor=c.get("t_init", 1.0), max_iter=50,
                  tol=c.get("tol", 0.0), tol_ratio=c.get("tol_ratio", 0.0), return_history=True, L=L)
        if c.get("mode", 0) == 1:
            ref = orc.fista_delta(A, b, "elasticnet", a1, a2, c["delta"], **kw)
        else:
            ref = orc.fista(A, b, "elasticnet", a1, a2, adaptive_restart=c.get("adaptive_restart", False), **kw)
        x_ref, h_ref = ref
        assert len(r0[f"obj{i}"]) == len(h_ref["obj"]), c
        assert _data.rel(r0[f"x{i}"], x_ref) < 1e-9 and np.allclose(r0[f"obj{i}"], h_ref["obj"], rtol=1e-9), c
        if c.get("backtracking"):
            assert int(r0[f"ls{i}"]) == orc_ls_total(A, b, a1, a2, c, L), c


def orc_ls_total(A, b, a1, a2, c, L):
    kw = dict(backtracking=True, t_init_factor=c.get("t_init", 1.0), max_iter=50, L=L, return_metrics=True)
    if c.get("mode", 0) == 1:
        _, met = orc.fista_delta(A, b, "elasticnet", a1, a2, c["delta"], **kw)
    else:
        _, met = orc.fista(A, b, "elasticnet", a1, a2, **kw)
    return met["ls_iters_total"]


# --------------------------------------------------------------------------------------------------
# the record sink of the solver runs (iterative_solvers._Records): it receives tensors and makes no device call, so its
# bookkeeping - rows of the caller's kind, objectives now or one pass late, the log, the metric shares - is checked here
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tensor_caller", [False, True])
def test_record_sink_bookkeeping(tensor_caller):
    from fastoptsolver_amd import _core, iterative_solvers as its
    its.reset_metrics()
    like = _core.Like(torch.zeros(1, dtype=torch.float32) if tensor_caller else np.zeros(1))
    a1, a2 = 0.3, 0.2
    history, log = {"x": ["x0"], "obj": []}, {"x": [], "t": [], "delta": []}
    rec = its._Records(like, history, its._objective_by_alpha(a1, a2), log, timer=_HostTimer)
    assert rec.recording and rec.objectives
    xs = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    hs = np.array([[8.0, 1.0, 2.0, 9.0], [6.0, 1.5, 2.5, 4.0], [4.0, 2.0, 3.0, 1.0]])     # rr, ||x||_1, ||x||_2^2, ||dx||^2
    rec.block(xs, hs, taus=torch.tensor([0.5, 0.25, 0.25], dtype=torch.float64))
    rec.block(xs[:2] + 100.0, hs[:2], taus=[0.125, 0.125], rr_known=False)           # residuals come one pass late
    assert len(history["obj"]) == 3 and len(rec.owed) == 2
    rec.settle([5.0])
    s = _Status()
    s.xnorm1, s.xnorm2, s.this_step = 7.0, 11.0, 0.75
    rec.one(torch.full((4,), -1.0, dtype=torch.float64), s, 0.0625)
    rec.settle([3.0])
    rec.settle([2.0], [(70.0, 110.0)])                     # a closing residual pass brings its own norms
    assert rec.owed == []
    f = lambda rr, x1, x2: 0.5 * rr + 0.5 * a2 * x2 + a1 * x1                        # noqa: E731
    assert history["obj"] == [f(8.0, 1.0, 2.0), f(6.0, 1.5, 2.5), f(4.0, 2.0, 3.0), f(5.0, 1.0, 2.0), f(3.0, 1.5, 2.5),
                              f(2.0, 70.0, 110.0)]
    assert history["x"][0] == "x0" and len(history["x"]) == 7 and len(log["x"]) == 6
    want = [xs[0], xs[1], xs[2], xs[0] + 100.0, xs[1] + 100.0, torch.full((4,), -1.0, dtype=torch.float64)]
    for got, ref, logged in zip(history["x"][1:], want, log["x"]):
        if tensor_caller:
            assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.device.type == "cpu"
            assert torch.equal(got, ref.float())
        else:
            assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, ref.numpy())
        assert logged is got                                # one conversion serves history and log
    assert log["t"] == [0.5, 0.25, 0.25, 0.125, 0.125, 0.0625]
    assert log["delta"] == [3.0, 2.0, 1.0, 3.0, 2.0, 0.75]
    # metrics: the searches' wall time in equal shares, the timer's count trimmed to the gradients that belong to the run
    rec.searches([1, 0, 3], 3.0)
    rec.searches([2], 0.25)
    assert (its.ls_call_times, its.ls_call_iters) == ([1.0, 1.0, 1.0, 0.25], [1, 0, 3, 2])
    rec.timer.stop(None, 5)
    rec.gradients(4)
    assert its.get_metrics()["grad_num_calls"] == 4
    rec.timer.stop(None, 2)
    rec.gradients()
    assert its.get_metrics()["grad_num_calls"] == 6
    assert its._shares(2, 1.0, 4) == [0.25, 0.25] and its._shares(0, 1.0) == []       # members of a batch launch
    # a sink without history or log records metrics only
    plain = its._Records(like)
    assert not plain.recording and not plain.objectives
    plain.searches([4, 4], 2.0)
    assert its.get_metrics()["ls_iters_total"] == 14 and its.get_metrics()["ls_num_calls"] == 6
    its.reset_metrics()
