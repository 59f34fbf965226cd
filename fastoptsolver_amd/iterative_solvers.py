"""MI355X drop-in for the reference's ``iterative_solvers.py``: same names, positional order, defaults,
return shapes, history keys, metric keys, exceptions and RNG consumption — the loop bodies are HIP kernels.

Reference lines cited as ``ref:LINE`` are ``iterative_solvers.py:LINE`` of ElBaldo1/FastOptSolver.

Extensions are keyword-only: ``L=`` (skip the power iteration), ``dtype="bf16"`` (store A in bf16,
accumulate in fp32), ``check_every=`` (how often the host polls the device stop flag).
``A`` may be an ndarray, a tensor or a ``prepare(A, b)`` handle; results come back as the kind that went in
(ndarray float64 / tensor float32).
"""
from __future__ import annotations

import collections
import math
import time

import numpy as np
import torch

from . import _core, _lib
from .operators import ElasticNetProx, L1Prox, LeastSquares

# ref:11 — Armijo sufficient-decrease constant, read at call time (callers may monkey-patch it)
C: float = 1e-2
_EPS64 = float(np.finfo(np.float64).eps)
_EPS32 = float(np.finfo(np.float32).eps)

# ref:16-18 — module-level metric lists (seconds; device time where a kernel is what was timed)
grad_call_times = []
ls_call_times = []
ls_call_iters = []


def reset_metrics() -> None:
    """ref:20-24"""
    grad_call_times.clear()
    ls_call_times.clear()
    ls_call_iters.clear()


def get_metrics():
    """ref:26-40 — the same seven keys.  With the fused step, "gradient time" is the device time of the
    gradient kernels (host-driven mode) or the per-iteration share of the fused run (device-driven mode)."""
    return {
        'grad_num_calls':   len(grad_call_times),
        'grad_time_total':  sum(grad_call_times),
        'grad_time_mean':   np.mean(grad_call_times) if grad_call_times else 0.0,
        'ls_num_calls':     len(ls_call_times),
        'ls_time_total':    sum(ls_call_times),
        'ls_time_mean':     np.mean(ls_call_times) if ls_call_times else 0.0,
        'ls_iters_total':   sum(ls_call_iters),
    }


class _EventTimer:
    """Pairs of device events on the current stream; resolved to seconds at flush()."""

    def __init__(self, sink):
        self.sink = sink
        self.pending = []

    def start(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def stop(self, ev0, count=1):
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record()
        self.pending.append((ev0, ev1, count))

    def recount(self, count):
        """The pair stopped last covered `count` units after all (a device-side stop ended the run early)."""
        ev0, ev1, _ = self.pending[-1]
        self.pending[-1] = (ev0, ev1, count)

    def flush(self):
        if not self.pending:
            return
        self.pending[-1][1].synchronize()
        for ev0, ev1, count in self.pending:
            if count > 0:
                dt = ev0.elapsed_time(ev1) * 1e-3 / count
                self.sink.extend([dt] * count)
        self.pending.clear()


# ---------------------------------------------------------------------
# Estimate Lipschitz constant L = λ_max(AᵀA)                    ref:45-60
# ---------------------------------------------------------------------
def estimate_lipschitz(A, n_iter: int = 100, tol: float = 1e-6, *, group=None) -> float:
    """Power iteration on the device (w = Aᵀ(Av) is the single-pass GEMV-pair kernel with b = 0).
    Draws ``np.random.randn(n)`` from the global legacy stream exactly like ref:50.

    Row-sharded problems: with a ``Comm`` attached to the problem the kernels' all-reduce makes this the power
    iteration of the whole matrix as it stands; ``group=`` (a torch.distributed group, split-form sharding) sums
    w over the ranks here.  Every rank must draw the same v0 (seed the global stream identically).
    A batch (a 3-D A or a sequence of matrices) gives a length-P float64 ndarray: the draws of P single calls, in
    problem order, and one power iteration per problem in one launch.
    A handle with sample weights (``prepare_weighted``): lambda_max(A^T W A), the same power iteration with one
    fos_gram_apply per step and v kept in fp64 on the host."""
    if _weighted(A):
        if group is not None:
            raise ValueError("a weighted handle cannot be combined with group=")
        return _weighted_lipschitz(A, np.random.randn(A.n), n_iter, tol)
    if _is_batch(A):
        if group is not None:
            raise ValueError("a batch (3-D A or a sequence of matrices) cannot be combined with group=")
        mats = list(A) if isinstance(A, (list, tuple)) else [A[i] for i in range(int(A.shape[0]))]
        for i, Ai in enumerate(mats):
            if _ndim(Ai) != 2:
                raise ValueError(f"batch member {i}: A must be 2-D")
        L, _ = _batch_lipschitz(mats, [None] * len(mats), None, n_iter, tol)
        return np.asarray(L, dtype=np.float64)
    prob = _core.prepare(A)
    v0 = np.random.randn(prob.n)
    if group is not None:
        from .distributed import sharded_lipschitz
        bare = prob if prob.b is None else _core.Problem(prob.A, None, prob.dtype, pad=False)   # same A, b = 0 (ref:54)
        return sharded_lipschitz(lambda v: bare.gemv_pair(v, 0.0), prob.n, prob.vec_in(v0)[: prob.n], n_iter, tol,
                                 group=group)
    L, _, _ = prob.power_iter(v0, n_iter=n_iter, tol=tol)
    return L


def _weighted(A):
    """Whether A is a handle with sample weights bound (`prepare_weighted`): it runs on the matrix-core lockstep alone."""
    return isinstance(A, _core.Problem) and A.sample_weight is not None


def _has_coord(A):
    """Whether A is a handle with penalty factors or bounds (`Problem.set_penalty`) or feature groups
    (`Problem.set_feature_groups`) bound: it runs on the matrix-core lockstep alone."""
    return isinstance(A, _core.Problem) and (A.has_coord or A.has_feature_groups)


def _refuse_multinomial(A, who):
    """A multinomial handle (`prepare(..., loss="multinomial")`) belongs to multinomial_path / multinomial_cv /
    multinomial_objective: its lockstep columns are class groups, which no squared-loss or logistic solver forms."""
    if isinstance(A, _core.Problem) and A.loss == "multinomial":
        raise ValueError(f"{who}: A was prepared for the multinomial loss: use multinomial_path / multinomial_cv / "
                         "multinomial_objective")
    _core.refuse_link(A, who)        # a Huber or squared-hinge handle likewise


def _weighted_lipschitz(prob, v0, n_iter=100, tol=1e-6):
    """ref:45-60 on A^T W A: w = A^T (W (A v)) is one fos_gram_apply per step (v rounded to fp32 for the pass), the norms and v
    itself stay in fp64 here.  max(w) lambda_max(A^T A) is not used: with class weights {1, r} it is loose by up to r."""
    v = np.asarray(v0, dtype=np.float64)
    v = v / np.linalg.norm(v)
    prev, L = 0.0, 0.0
    for _ in range(n_iter):
        w = prob.gram_apply(torch.from_numpy(v).reshape(-1, 1))[:, 0].to("cpu", torch.float64).numpy()
        L = float(np.linalg.norm(w))
        v = w / L
        if abs(L - prev) < tol:
            break
        prev = L
    return L


class _GroupReducer:
    """Split-form sharding over a torch.distributed group (any backend): the sums over row blocks that the device
    would do itself with a Comm attached are done here, between the kernels, in the order every rank follows."""

    def __init__(self, prob, group):
        import torch.distributed as dist
        self.dist, self.group, self.prob = dist, group, prob
        self.on_device = dist.get_backend(group) == "nccl"
        self.gbuf64 = None          # precise mode (backtracking): the fp64 [gradient ; ||r||^2] of the state machine

    def grad(self):
        """[partial gradient ; partial ||r||^2] -> global, in gbuf (n + 1 floats: the one exchange per iteration; n + 1
        doubles in precise mode)."""
        buf = self.gbuf64 if self.gbuf64 is not None else self.prob.gbuf
        self.dist.all_reduce(buf[: self.prob.n_dev + 1], op=self.dist.ReduceOp.SUM, group=self.group)

    def rr_global(self):
        buf = self.gbuf64 if self.gbuf64 is not None else self.prob.gbuf
        return float(buf[self.prob.n_dev])

    def sum(self, vals):
        t = torch.tensor(list(vals), dtype=torch.float64, device=self.prob.device if self.on_device else "cpu")
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)
        return t.tolist()


# ---------------------------------------------------------------------
# Armijo acceptance (ref:191, :306, :101) in cancellation-free form
# ---------------------------------------------------------------------
_BATCH = 16      # candidate steps decided per pass over A (MFMA N dimension)
_HISTORY_CHUNK_BYTES = 256 << 20   # device-resident x history is read back in chunks of at most this size


def _armijo_accepts(tr, t_k, smooth_a2, grad_eps=8.0 * _EPS32):
    """g(x_tmp) <= g(y) + C*grad.dlt  <=>  (1-C)*grad.dlt + 0.5||A dlt||^2 + 0.5*a2*||dlt||^2 <= 0  (g quadratic).

    Resolution of the test: (a) the reference compares two float64 evaluations of g, so differences below
    eps64*g(y) read as "equal" there (and x_tmp == y ends its loop); (b) grad.dlt is only known to
    ~grad_eps*||grad||*||dlt||, where grad_eps is the relative resolution of the gradient pass; (c) a trial step
    shorter than t*grad_eps*||grad|| lies inside the noise ball of y_k: its direction is rounding noise, the
    decision meaningless and the step harmless - the counterpart of the reference's exact "x_tmp == y" exit.
    grad_eps: 8*eps32 for the fp32 pass; 64*eps64 in precise mode (fos_fista_set_precise: fp64-accumulating pass at the
    unrounded y_k, what fista(backtracking=True) runs), where (b) and (c) shrink to the reference's own rounding level."""
    excess = (1.0 - C) * tr["gd"] + 0.5 * tr["q"] + 0.5 * smooth_a2 * tr["dd"]
    g_y = 0.5 * tr["rr_y"] + 0.5 * smooth_a2 * tr["y2"]
    noise = max(_EPS64 * g_y, grad_eps * math.sqrt(tr["gnorm2"] * tr["dd"]))
    in_noise_ball = tr["dd"] <= (grad_eps * t_k) ** 2 * tr["gnorm2"]
    return tr["nnz"] == 0 or excess <= noise or in_noise_ball


# ---------------------------------------------------------------------
# shared FISTA / FISTA-Δ / fused-ISTA driver
# ---------------------------------------------------------------------
def _pos(v):
    """A tolerance for which non-positive means "off", as the device takes it."""
    return v if v > 0.0 else 0.0


def _params(tau, alpha1, alpha2, *, mode, prox_kind=_lib.PROX_L1, delta=None, tol=0.0, tol_ratio=0.0, grad_rule=False,
            adaptive_restart=False, restart_threshold=1.0, group=0):
    """The fields of fos_fista_params from the solvers' arguments, under the names `_core.Fista.reset` and
    `_lib.FistaParams` take them.  `tol` is the step stop and, where `grad_rule` says so, the gradient-norm rule (ref:179) as
    well; momentum restarts exist for FISTA only.  Tolerances reach the device as given: a caller for which a non-positive
    one means "off" passes `_pos(tol)`."""
    prm = dict(tau=float(tau), alpha1=float(alpha1), alpha2=float(alpha2), delta=float(delta or 0.0),
               restart_threshold=float(restart_threshold), tol_step=float(tol), tol_ratio=float(tol_ratio), mode=int(mode),
               prox_kind=int(prox_kind), adaptive_restart=int(bool(adaptive_restart) and mode == _lib.MODE_FISTA))
    if grad_rule:                   # absent means 0.0, off: stand-in states without the rule (CPU tests) never meet the field
        prm["tol_grad"] = float(tol)
    if group:                       # likewise absent means 0, the separable penalty (fos_fista_params.group)
        prm["group"] = int(group)
    return prm


def _new_state(prob, prm):
    st = _core.Fista(prob)
    st.reset(**prm)
    return st


def _shares(n, seconds, of=None):
    """n of the `of` (default: n) equal shares of `seconds`: the device does not time the phases of a launch."""
    return [seconds / max(n if of is None else of, 1)] * n


def _ngrad(done, stopped):
    """One gradient per completed iteration, plus the one whose norm ended the run (ref:173-180)."""
    return done + (1 if stopped == _lib.STOP_GRAD else 0)


class _Records:
    """What a run leaves to its caller besides x: the `history` of fista / fista_delta (ref:224-232, :319-322), the `log` of
    ista (ref:117-120) and the entries of the metric lists.  The execution strategies hand over what the device recorded;
    the conversion to the caller's kind, the objective and the shares of the timings are decided here."""

    def __init__(self, like, history=None, obj=None, log=None, timer=_EventTimer):
        self.like, self.history, self.obj, self.log = like, history, obj, log
        self.timer = timer(grad_call_times)
        self.recording = history is not None or log is not None
        self.objectives = history is not None
        self.owed = []          # (||x||_1, ||x||_2^2) of recorded iterates whose ||A x - b||^2 is not known yet

    def _rows(self, xs):
        """[k, n] device block -> k rows of the caller's kind: tensors row by row, ndarrays out of one copy to the host."""
        if self.like.tensor:
            return [_core.from_device_vec(xs[i], self.like) for i in range(xs.shape[0])]
        return list(xs.cpu().numpy())

    def block(self, xs, hs, taus=None, rr_known=True):
        """k iterations recorded on the device: xs [k, n] device rows, hs [k, 4] host rows {||A x - b||^2, ||x||_1, ||x||_2^2,
        ||dx||^2}, taus the steps used (host list or device tensor; the log only).  rr_known=False: hs[:, 0] is not filled,
        the residuals come later through settle()."""
        rows = self._rows(xs)
        if self.history is not None:
            self.history["x"].extend(rows)
            if rr_known:
                self.history["obj"].extend(self.obj(float(r[0]), float(r[2]), float(r[1])) for r in hs)
            else:
                self.owed.extend((float(r[1]), float(r[2])) for r in hs)
        if self.log is not None:                            # ista's log (ref:117-120): x, the step used, ||dx||
            self.log["x"].extend(rows)
            self.log["t"].extend(taus.cpu().tolist() if _core.is_tensor(taus) else taus)
            self.log["delta"].extend(float(math.sqrt(r[3])) for r in hs)

    def one(self, x, s, tau):
        """The iteration the host finished itself: the device iterate, its status (norms, step length), the step used."""
        row = _core.from_device_vec(x, self.like)
        if self.history is not None:
            self.history["x"].append(row)
            self.owed.append((s.xnorm1, s.xnorm2))
        if self.log is not None:
            self.log["x"].append(row)
            self.log["t"].append(tau)
            self.log["delta"].append(s.this_step)

    def settle(self, rrs, norms=None):
        """||A x - b||^2 of the oldest iterates still owed their objective: f(x after iteration t) is seen by iteration
        t + 1's gradient pass, or by a closing residual pass (which brings `norms` of its own)."""
        self.history["obj"].extend(self.obj(rr, x2, x1) for rr, (x1, x2) in zip(rrs, norms or self.owed))
        del self.owed[:len(rrs)]

    def gradients(self, n=None):
        """The run's own timer bracketed its launches: resolve it, and keep the `n` gradient passes that belong to the run
        (None: all that were counted)."""
        self.timer.flush()
        if n is not None:
            del grad_call_times[n:]

    def searches(self, shrinks, seconds):
        """One Armijo search per entry of `shrinks` (ref:183-197) in `seconds` of wall time together."""
        ls_call_iters.extend(int(v) for v in shrinks)
        ls_call_times.extend(_shares(len(shrinks), seconds))


class _Run:
    """One solver run: the state machine, what the caller asked for, and the record sink.  Each execution strategy is a
    method that returns True when it ran the whole job and False when this problem / plan has no such form (the dispatcher
    `_drive` then tries the next one)."""

    def __init__(self, prob, st, rec, *, tau, eta, max_iter, tol, tol_ratio, backtracking, grad_tol_check, check_every,
                 reducer, smooth_a2, grad_eps, batch_trials):
        self.prob, self.st, self.rec = prob, st, rec
        self.tau, self.eta, self.max_iter, self.tol, self.tol_ratio = tau, eta, max_iter, tol, tol_ratio
        self.backtracking, self.grad_tol_check = backtracking, grad_tol_check
        self.check_every, self.reducer = check_every, reducer
        self.smooth_a2, self.grad_eps, self.use_batch = smooth_a2, grad_eps, batch_trials

    # ---- 1. nothing needs the host per iteration: enqueue everything, poll for stops -------------------------------
    def enqueue_only(self):
        st, rec = self.st, self.rec
        stops_possible = self.tol > 0.0 or self.tol_ratio > 0.0
        chunk = self.max_iter if not stops_possible else max(1, int(self.check_every or 8))
        done = 0
        while done < self.max_iter:
            todo = min(chunk, self.max_iter - done)
            ev = rec.timer.start()
            st.run(todo)
            rec.timer.stop(ev, todo)
            done += todo
            if stops_possible and st.status().stopped != _lib.STOP_NONE:
                break
        rec.gradients()
        if stops_possible:
            # only the iterations that really ran count as gradient calls
            s_end = st.status()
            rec.gradients(_ngrad(int(s_end.k), s_end.stopped))
        return True

    # ---- 2. small problems (A fits one CU's LDS): every host-driven feature - backtracking, gradient-norm stop, history,
    #         ISTA log - runs inside ONE launch of the LDS-resident loop; the host only unpacks what the device recorded
    def resident(self):
        st, rec = self.st, self.rec
        ev = rec.timer.start()
        ls_t0 = time.perf_counter()
        res = st.run_resident(self.max_iter, backtracking=self.backtracking, eta=self.eta, armijo_c=C,
                              grad_tol=self.tol if (self.grad_tol_check and self.tol > 0.0) else 0.0,
                              record=rec.recording)
        if res is None:
            rec.timer.pending.clear()
            return False
        ngrad = _ngrad(res["done"], st.status().stopped)
        rec.timer.stop(ev, max(ngrad, 1))
        rec.gradients(ngrad)
        if self.backtracking:                                    # ref:183-197: one search per completed iteration
            rec.searches(res["ls"], time.perf_counter() - ls_t0)
        if rec.recording:
            rec.block(res["x"], res["hist"].cpu().numpy(), res["taus"])
        return True

    # ---- 3. history of a PLAIN run without any per-iteration host round trip: x and the objective ingredients are
    #         recorded on the device by the same two kernels of the plain run and read back once (ref:224-232, :319-322)
    def history_plain(self):
        st, rec = self.st, self.rec
        chunk = max(1, min(self.max_iter, _HISTORY_CHUNK_BYTES // (8 * self.prob.n_dev)))   # bound the device-side x history
        done = 0
        while done < self.max_iter:
            todo = min(chunk, self.max_iter - done)
            ev = rec.timer.start()
            out = st.run_history(todo)
            if out is None:
                rec.timer.pending.clear()
                return False
            rec.timer.stop(ev, todo)
            xh, hs = out
            rec.block(xh, hs.cpu().numpy())
            done += todo
        rec.gradients()
        return True

    # ---- the Armijo search on the host (ref:183-197 / :298-312 / :92-108): used by the host-driven loop and to finish a
    #      search the device parked (all 16 candidates of a batch rejected: the reference's step-underflow regime)
    def search_on_host(self, t_k, bt_steps):
        st, reducer = self.st, self.reducer
        while True:
            # candidates t_k, t_k*eta, ... decided by ONE pass over A on the matrix cores (fos.h); ragged
            # problems (two-pass fallback) evaluate one candidate per pass.
            rows = st.trial_batch(t_k, self.eta, _BATCH) if self.use_batch else None
            if rows is None:
                self.use_batch = False
                rows = [st.trial(t_k, with_residual=True)]
            if reducer is not None:                        # ||A dlt||^2 = sum over the row blocks; ||r||^2 likewise
                for tr, q in zip(rows, reducer.sum([tr["q"] for tr in rows])):
                    tr["q"] = q
                    tr["rr_y"] = reducer.rr_global()
            for tr in rows:
                if _armijo_accepts(tr, t_k, self.smooth_a2, self.grad_eps):
                    return t_k, bt_steps
                t_k *= self.eta                            # ref:195
                bt_steps += 1

    # ---- 4. data-dependent control on the device - no host round trip per iteration:
    #   backtracking (fos_fista_run_backtracking): gradient, one matrix-core batch of 16 candidates, a decision kernel,
    #     the update with the accepted step, the bookkeeping - all enqueued;
    #   with history / ista's log (fos_fista_run_recorded; also adaptive restart and the stopping rules without
    #     backtracking): iterates and their norms recorded per iteration, ||A x - b||^2 of every iterate out of the NEXT
    #     iteration's gradient pass, the last objective closed by one residual pass.
    # The host polls every `check_every` iterations for stops and for a parked search, which it finishes itself before
    # handing the loop back to the device.
    def device_driven(self):
        st, rec, prob, backtracking, recording = self.st, self.rec, self.prob, self.backtracking, self.rec.recording
        cap = _HISTORY_CHUNK_BYTES // (8 * prob.n_dev) if recording else self.max_iter
        chunk = max(1, min(int(self.check_every or (16 if recording else 8)), cap))
        done, started_total, ls_t0 = 0, 0, time.perf_counter()
        rr_seen, shrinks = [], []              # rr_seen[t]: residual of the iterate iteration t started from
        while done < self.max_iter:
            todo = min(chunk, self.max_iter - done)
            ev = rec.timer.start()
            if recording:
                out = st.run_recorded(todo, backtracking, self.eta, C, self.grad_eps, want_rr=rec.objectives)
            else:
                pair = st.run_backtracking(todo, self.eta, C, self.grad_eps)
                out = None if pair is None else dict(ls=pair[0], taus=pair[1])
            if out is None:                                   # this plan has no candidate pass: the host drives
                rec.timer.pending.clear()
                return False
            s = st.status()                                   # synchronises: k, stop / stall flag
            ran = int(s.k) - done
            stalled = s.stopped == _lib.STOP_LS_STALL
            started = ran + (1 if (stalled or s.stopped == _lib.STOP_GRAD) else 0)
            rec.timer.stop(ev, max(started, 1))
            started_total += started
            if backtracking:
                shrinks.extend(out["ls"][:ran].cpu().tolist())
            if recording:
                if rec.objectives:
                    rr_seen.extend(out["rr_seen"][:started].cpu().tolist())
                rec.block(prob.vec_out(out["x"][:ran]), out["hist"][:ran].cpu().numpy(),
                          out["taus"][:ran] if backtracking else [self.tau] * ran, rr_known=False)
            done += ran
            if stalled:                                       # finish this iteration's search on the host
                tau = st.resume_after_stall()
                tau, steps = self.search_on_host(tau, _BATCH)
                self.tau = tau
                shrinks.append(steps)
                st.set_tau(tau)
                st.update()
                s = st.status()
                if recording:
                    rec.one(st.x_tensor(), s, tau)
                done += 1
            if s.stopped != _lib.STOP_NONE:
                break
        rec.gradients(started_total)
        if backtracking:
            rec.searches(shrinks, time.perf_counter() - ls_t0)
        # f(x after iteration t) needs ||A x - b||^2 of that iterate: seen by iteration t + 1, or by a closing pass
        if rec.objectives:
            rr_of = rr_seen[1:done + 1]
            if len(rr_of) < done:
                rr_of.append(prob.residual_objective(st.x_tensor())[0])
            rec.settle(rr_of)
        return True

    # ---- 5. the host drives every iteration: split-form sharding over torch.distributed (the all-reduce sits between
    #         the gradient and the update), generic callables, plans without the candidate pass.
    # History objective f(x_k) without the reference's extra pass per iteration (ref:225-230, :321): the DUAL gradient
    # pass of iteration k also returns ||A x_k - b||^2, so f(x_k) is appended one iteration late and only the very last
    # iterate needs a residual pass of its own.
    def host_driven(self):
        st, rec, prob, reducer, tol, tol_ratio = self.st, self.rec, self.prob, self.reducer, self.tol, self.tol_ratio

        def rr_x_of(status):         # ||A x_k - b||^2 over ALL rows (split-form sharding: summed here)
            return reducer.sum([status.rr_x])[0] if reducer is not None else status.rr_x

        for _ in range(self.max_iter):
            ev = rec.timer.start()
            st.grad(dual=bool(rec.owed))                          # ref:173-175 (alpha2*y is added by the consumers)
            if reducer is not None:
                reducer.grad()
            rec.timer.stop(ev)
            if self.grad_tol_check and tol > 0.0:                 # ref:179
                if math.sqrt(st.trial(self.tau, with_residual=False)["gnorm2"]) < tol:
                    if rec.owed:
                        rec.settle([rr_x_of(st.status())])
                    break
            if self.backtracking:                                 # ref:183-197 / ref:298-312 / ref:92-108
                ls_t0 = time.perf_counter()
                self.tau, bt_steps = self.search_on_host(self.tau, 0)
                rec.searches([bt_steps], time.perf_counter() - ls_t0)
                st.set_tau(self.tau)
            st.update()                                           # ref:200-221
            if rec.recording:
                xk = st.x_tensor()
                s = st.status()
                if rec.owed:
                    rec.settle([rr_x_of(s)])
                rec.one(xk, s, self.tau)
            else:
                s = st.status() if (tol > 0.0 or tol_ratio > 0.0) else None
            if s is not None and s.stopped != _lib.STOP_NONE:     # ref:238, :242
                break
        if rec.owed:
            rr, x2, x1 = prob.residual_objective(st.x_tensor())
            if reducer is not None:
                rr = reducer.sum([rr])[0]
            rec.settle([rr], [(x1, x2)])
        rec.gradients()
        return True


def _drive(prob, like, *, mode, prox_kind, alpha1, alpha2, tau, delta=0.0, backtracking=False, eta=0.5,
           max_iter=500, tol=0.0, tol_ratio=0.0, adaptive_restart=False, restart_threshold=1.0,
           grad_tol_check=False, history=None, history_obj=None, x0=None, check_every=None, log=None,
           batch_trials=True, reducer=None, state=None):
    """Run the state machine with the first execution strategy of `_Run` that serves this configuration: device-driven
    wherever nothing needs a per-iteration host decision, host-driven otherwise (split-form sharding, ref:179 / :183-197 /
    :224-232 on plans without the device forms).  `like`: a `_core.Like` or the caller's own array.
    batch_trials=False: the searches of a streaming problem run in the host-driven loop with one candidate per pass over A
    (fos_fista_trial) - the sequential search that tests and tools hold the 16-candidate one against."""
    like = like if isinstance(like, _core.Like) else _core.Like(like)
    st = state if state is not None else _core.Fista(prob)      # `state`: a stand-in with the same interface (CPU tests)
    x0_dev = None if x0 is None else _core.to_device_vec(x0, prob.device).double()   # padded by Fista.reset
    # reducer: split-form sharding - the all-reduce sits between the gradient and the update, so the host drives
    host_needed = backtracking or history is not None or log is not None or reducer is not None
    # gradient-norm stop (ref:179): on the device (fos_fista_params.tol_grad) when the run is enqueue-only, by the host
    # between grad() and update() when the host drives anyway
    device_loop = reducer is None                               # every such configuration has an enqueue-only form
    dev_grad_stop = grad_tol_check and tol > 0.0 and (not host_needed or device_loop)
    prm = _params(tau, alpha1, alpha2, mode=mode, prox_kind=prox_kind, delta=delta, tol=_pos(tol), tol_ratio=_pos(tol_ratio),
                  grad_rule=dev_grad_stop, adaptive_restart=adaptive_restart, restart_threshold=restart_threshold)
    st.reset(x0=x0_dev, **prm)
    # Backtracking decides on a cancelling sum (grad.dlt): take the gradient from the fp64-accumulating pass then; in
    # split-form sharding the state machine keeps it in a tensor of ours and the reducer sums the n + 1 doubles
    grad_eps = 8.0 * _EPS32
    if backtracking and hasattr(st, "set_precise"):
        if reducer is None:
            st.set_precise(True)
            grad_eps = 64.0 * _EPS64
        elif not prob.plan()["resident"]:       # (LDS-resident plans have no split-form fp64 pass: they keep the fp32 gbuf)
            st.set_precise(True, own_buffer=True)
            reducer.gbuf64 = st.gbuf64
            grad_eps = 64.0 * _EPS64
    rec = _Records(like, history, history_obj, log, timer=getattr(st, "make_timer", _EventTimer))   # stand-in states bring a host timer
    run = _Run(prob, st, rec, tau=tau, eta=eta, max_iter=max_iter, tol=tol, tol_ratio=tol_ratio, backtracking=backtracking,
               grad_tol_check=grad_tol_check, check_every=check_every, reducer=reducer,
               smooth_a2=alpha2 if (prox_kind == _lib.PROX_L1 and alpha2 > 0) else 0.0, grad_eps=grad_eps,
               batch_trials=batch_trials)
    if not host_needed:
        run.enqueue_only()
        return st
    on_device = reducer is None and max_iter > 0
    if on_device and run.resident():
        return st
    plain = not prm["adaptive_restart"] and tol == 0.0 and tol_ratio == 0.0
    if on_device and history is not None and log is None and not backtracking and plain and run.history_plain():
        return st
    if on_device and batch_trials and hasattr(st, "run_recorded") and (rec.recording or backtracking) and run.device_driven():
        return st
    run.host_driven()
    return st


def _tau(L, alpha2, t_init_factor, penalty_max=1.0):
    """First step: t_init_factor / L, the ridge term being part of the smooth function (ref:156-158).  penalty_max: max_j p_j of
    a handle with penalty factors - its ridge term 0.5 alpha2 sum_j p_j x_j^2 has the Lipschitz constant alpha2 max_j p_j."""
    return t_init_factor / (L + (alpha2 * penalty_max if alpha2 > 0 else 0.0))


class _Loop(collections.namedtuple("_Loop", "delta alpha1 alpha2 backtracking eta t_init_factor max_iter tol tol_ratio "
                                            "adaptive_restart restart_threshold")):
    """The arguments of the reference's loop as fista (delta None) and fista_delta take them, and what follows from them
    alone: every form of a call - single, several targets, batch - hands them on as they are."""
    __slots__ = ()

    @property
    def mode(self):
        return _lib.MODE_FISTA if self.delta is None else _lib.MODE_DELTA

    def tau(self, L):
        return _tau(L, self.alpha2, self.t_init_factor)

    def params(self, tau):
        """`_params` of a run that starts from x = 0 and carries all its stopping rules on the device (lockstep and batch
        launches): fista's tol is also the gradient-norm rule, fista_delta's a step stop only."""
        return _params(tau, self.alpha1, self.alpha2, mode=self.mode, delta=self.delta, tol=_pos(self.tol),
                       tol_ratio=_pos(self.tol_ratio), grad_rule=self.delta is None, adaptive_restart=self.adaptive_restart,
                       restart_threshold=self.restart_threshold)

    def drive(self, prob, like, tau, **kw):
        return _drive(prob, like, mode=self.mode, prox_kind=_lib.PROX_L1, alpha1=self.alpha1, alpha2=self.alpha2, tau=tau,
                      delta=self.delta, backtracking=self.backtracking, eta=self.eta, max_iter=self.max_iter, tol=self.tol,
                      tol_ratio=self.tol_ratio, adaptive_restart=self.adaptive_restart,
                      restart_threshold=self.restart_threshold, grad_tol_check=self.delta is None, **kw)


def _objective_by_alpha(alpha1, alpha2):
    """History objective of fista(): driven by alpha>0, not by reg_type.  ref:225-230"""
    def obj(rr, x2, x1):
        val = 0.5 * rr
        if alpha2 > 0:
            val += 0.5 * alpha2 * x2
        if alpha1 > 0:
            val += alpha1 * x1
        return val
    return obj


def _objective_by_reg(reg_type, alpha1, alpha2):
    """compute_objective semantics (objective_functions.py:3-30), used by fista_delta ref:321."""
    if reg_type not in ("lasso", "ridge", "elasticnet"):
        raise ValueError(f"Unsupported reg_type='{reg_type}'")

    def obj(rr, x2, x1):
        val = 0.5 * rr
        if reg_type in ("ridge", "elasticnet"):
            val += 0.5 * alpha2 * x2
        if reg_type in ("lasso", "elasticnet"):
            val += alpha1 * x1
        return val
    return obj


# ---------------------------------------------------------------------
# ISTA                                                          ref:65-125
# ---------------------------------------------------------------------
def ista(x0, g, grad_g, prox_h, L, backtracking: bool = False, eta: float = 0.5, t_init_factor: float = 1.0,
         max_iter: int = 500, tol: float = 0.0, return_history: bool = False):
    """Proximal gradient over callables.  When ``g``/``grad_g`` come from one ``LeastSquares`` object and
    ``prox_h`` is an ``L1Prox``/``ElasticNetProx`` the fused device state machine runs (single pass over A per
    gradient); any other callables are invoked as given on float32 device tensors, with the loop's own vector
    arithmetic still on the device."""
    reset_metrics()
    ls = getattr(g, "__self__", g)
    fused = (isinstance(ls, LeastSquares) and getattr(grad_g, "__self__", None) is ls
             and isinstance(prox_h, (L1Prox, ElasticNetProx)))
    t = t_init_factor / L                                                     # ref:81
    if fused:
        prob = ls.prob
        if isinstance(prox_h, ElasticNetProx):
            if ls.alpha2 != 0.0:
                fused = False          # l2 both in g and in the prox: not a state-machine configuration
            else:
                kind, a1, a2 = _lib.PROX_ENET, prox_h.alpha1, prox_h.alpha2
        else:
            kind, a1, a2 = _lib.PROX_L1, prox_h.alpha1, ls.alpha2
    if fused:
        x0_dev = _core.to_device_vec(x0, prob.device).double()
        log = {"x": [_core.from_device_vec(x0_dev, x0)], "t": [t], "delta": []} if return_history else None
        st = _drive(prob, x0, mode=_lib.MODE_ISTA, prox_kind=kind, alpha1=a1, alpha2=a2, tau=t,
                    backtracking=backtracking, eta=eta, max_iter=max_iter, tol=tol, x0=x0_dev, log=log)
        x = _core.from_device_vec(st.x_tensor(), x0)
        return (x, log) if return_history else x

    # ---- generic callables ----
    # The loop's own vector arithmetic runs on the device.  The callables are the caller's code: they get float32
    # device tensors; a callable written for ndarrays (what a user of the reference has: closures over a NumPy A)
    # is detected on its first call and from then on fed float64 ndarrays, its result moved back to the device.
    from .operators import vec_axpby, vec_stats
    x = _core.to_device_vec(x0).clone()                                        # ref:79
    wants_numpy = {}

    def call(fn, *args):
        key = id(fn)
        if not wants_numpy.get(key, False):
            try:
                return fn(*args)
            except (TypeError, RuntimeError, ValueError, AttributeError):
                if _core.is_tensor(x0):
                    raise
                wants_numpy[key] = True
        host = [a.detach().to("cpu", torch.float64).numpy() if _core.is_tensor(a) else a for a in args]
        out = fn(*host)
        return _core.to_device_vec(out) if isinstance(out, np.ndarray) and out.ndim == 1 else out

    log = {"x": [_core.from_device_vec(x, x0)], "t": [t], "delta": []} if return_history else None
    gtimer = _EventTimer(grad_call_times)
    for _ in range(max_iter):
        ev = gtimer.start()
        grad = _core.to_device_vec(call(grad_g, x))                             # ref:87-89
        gtimer.stop(ev)
        if backtracking:                                                        # ref:92-108
            bt_steps = 0
            ls_t0 = time.perf_counter()
            t_k = t
            gx = float(call(g, x))
            while True:
                x_new = _core.to_device_vec(call(prox_h, vec_axpby(1.0, x, -t_k, grad), t_k))
                diff = vec_axpby(1.0, x_new, -1.0, x)
                gd = vec_stats(None, grad, diff)[1]
                if float(call(g, x_new)) <= gx + C * gd:
                    break
                t_k *= eta
                bt_steps += 1
            ls_call_times.append(time.perf_counter() - ls_t0)
            ls_call_iters.append(bt_steps)
            t = t_k
        else:
            x_new = _core.to_device_vec(call(prox_h, vec_axpby(1.0, x, -t, grad), t))   # ref:110-111
            diff = vec_axpby(1.0, x_new, -1.0, x)
        delta = math.sqrt(vec_stats(None, None, diff)[2])                        # ref:114
        x = x_new
        if return_history:
            log["x"].append(_core.from_device_vec(x, x0))
            log["t"].append(t)
            log["delta"].append(delta)
        if tol > 0.0 and delta < tol:                                           # ref:122
            break
    gtimer.flush()
    out = _core.from_device_vec(x, x0)
    return (out, log) if return_history else out


def _lipschitz_cols(prob, comm, cols, n_iter=100, tol=1e-6):
    """estimate_lipschitz (ref:45-60) for a column-sharded matrix: v is partitioned like x; w_p = A_p^T (sum_q A_q v_q) is
    the two-phase pass with its one m-vector exchange, ||w|| sums the blocks' squares over the ranks.  Draws the n_total
    normals of ref:50 from the global stream on every rank (same seed everywhere) and keeps this rank's slice."""
    lo, hi, n_total = cols
    v = torch.from_numpy(np.random.randn(n_total)[lo:hi].copy()).to(prob.device, torch.float32)
    bare = prob if prob.b is None else None
    if bare is None:
        bare = _core.Problem(prob.A, None, prob.dtype, pad=False)               # same A, b = 0 (ref:54)
        bare.set_comm_cols(comm)
    nrm = lambda t: math.sqrt(float(comm.allreduce((t.double() @ t.double()).reshape(1))[0]))   # noqa: E731
    v = v / nrm(v)
    prev, L = 0.0, None
    for _ in range(n_iter):
        w = bare.gemv_pair(v, 0.0)
        L = nrm(w)
        v = w / L
        if abs(L - prev) < tol:
            break
        prev = L
    return L


def _sharded_problem(A, b, dtype, comm, group, cols=None):
    """(problem, reducer) for the solver front-ends: plain, Comm-attached (reductions under the C ABI, reducer None)
    or split-form over a torch.distributed group (reducer does the sums).  cols = (lo, hi, n_total): COLUMN sharding -
    A holds this rank's columns [lo, hi) of an m x n_total matrix, b is whole, the returned x is this rank's block."""
    if comm is None and group is None:
        return _core.as_problem(A, b, dtype), None
    if cols is not None:
        if comm is None:
            raise ValueError("column sharding needs a distributed.Comm (comm=)")
        prob = A if isinstance(A, _core.Problem) else _core.Problem(A, b, dtype, pad=False)
        if not getattr(prob, "col_sharded", False):
            prob.set_comm_cols(comm)
        return prob, None
    import torch.distributed as dist
    prob = A if isinstance(A, _core.Problem) else _core.Problem(A, b, dtype, pad=True)   # same n_dev on every rank
    if comm is not None:
        if getattr(prob, "comm", None) is not comm:
            prob.set_comm(comm)
        return prob, None
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return prob, None
    return prob, _GroupReducer(prob, group)


# ---------------------------------------------------------------------
# Several targets: fista(A, B) / fista_delta(A, B) with a 2-D B (extension)
# ---------------------------------------------------------------------
def _targets(A, b):
    """The right-hand sides of a multi-target call - a 2-D b with k >= 2 columns against an A without a b of its own - or
    None.  A 1-D b, a b of shape (m, 1) or (1, m) and a Problem prepared with its own b keep the single-target path."""
    if b is None or (isinstance(A, _core.Problem) and A.b is not None):
        return None
    shape = tuple(b.shape) if hasattr(b, "shape") else np.shape(b)
    if len(shape) != 2 or shape[1] < 2:
        return None
    m = A.m if isinstance(A, _core.Problem) else (A.shape[0] if hasattr(A, "shape") else np.shape(A)[0])
    return None if shape[0] * shape[1] == m else b


def _metrics_of(fn):
    """Run `fn` (one sub-solve) against empty metric lists - its own bookkeeping indexes them from their start - and return
    (its result, the three lists it recorded); the earlier entries are back in place afterwards."""
    lists = (grad_call_times, ls_call_times, ls_call_iters)
    saved = [list(v) for v in lists]
    reset_metrics()
    try:
        return fn(), tuple(list(v) for v in lists)
    finally:
        for v, old in zip(lists, saved):
            v[:] = old


def _metrics_add(recorded):
    for v, new in zip((grad_call_times, ls_call_times, ls_call_iters), recorded):
        v.extend(new)


def _solve_targets(A, B, lp, L, dtype, check_every):
    """X[:, j] = fista(A, B[:, j], ...) (fista_delta when `delta` is given) for every column j, with A bound once and L
    estimated once.  Groups of up to 16 columns advance in lockstep on one read of A per iteration
    (fos_fista_run_multi_rhs); what the lockstep does not serve - shapes without a multi-vector kernel, a last group of
    one column, backtracking, fista's gradient-norm rule (tol > 0) - runs column by column on sibling problems that borrow
    the same device A.  A that fits one CU's LDS (the resident plan): every column in one launch, one workgroup each."""
    prob = _core.prepare(A, None, dtype)
    like = prob.like
    Bt = _core.to_device(B, prob.device)
    if Bt.shape[0] != prob.m:
        raise ValueError("b must have m rows")
    k = int(Bt.shape[1])
    tau = lp.tau(_lipschitz(prob, L))                                                  # once for all columns
    prm = lp.params(tau)
    # fista's tol is also the gradient-norm rule, which sits before the update; fista_delta's is a step stop only
    lockstep = not lp.backtracking and (lp.tol == 0.0 or lp.delta is not None)

    if prob.plan()["resident"]:
        # A fits one CU's LDS: all k columns in ONE launch, one workgroup per column on the shared A (fos_fista_run_batch),
        # each computing what the column's own single-target run computes - backtracking and tol > 0 included
        bt = _Batch.targets(prob, Bt)
        xs = []
        for x, _, recorded in _run_batch_group(bt, prob.dtype, range(k), [_lib.FistaParams(**prm)] * k, lp):
            xs.append(x)
            _metrics_add(recorded)
        return _core.from_device_vec(torch.stack(xs, dim=1), like)
    X = torch.zeros(prob.n, k, dtype=torch.float64, device=prob.device)
    width = 4 if k <= 4 else 16            # up to 4: the multi-vector VALU pass where the shape has one; else matrix cores
    for g0 in range(0, k, width):
        g1 = min(k, g0 + width)
        if lockstep and g1 - g0 >= 2:
            handles = [_new_state(prob, prm) for _ in range(g0, g1)]
            gtimer = _EventTimer(grad_call_times)
            ev = gtimer.start()
            if _core.run_multi_rhs(handles, Bt[:, g0:g1], lp.max_iter):
                gtimer.stop(ev, lp.max_iter)                  # one gradient per lockstep iteration, as fista_path counts
                gtimer.flush()
                for j, st in zip(range(g0, g1), handles):
                    X[:, j] = st.x_tensor()
                continue
        for j in range(g0, g1):
            st, recorded = _metrics_of(lambda: lp.drive(prob.sibling(Bt[:, j].contiguous()), like, tau,
                                                        check_every=check_every))
            _metrics_add(recorded)
            X[:, j] = st.x_tensor()
    return _core.from_device_vec(X, like)


# ---------------------------------------------------------------------
# Batches of small independent problems: fista(A, b) / fista_delta(A, b) with a 3-D A or a sequence of matrices (extension)
# ---------------------------------------------------------------------
def _is_batch(A):
    """A batch call: a 3-D A (P, m, n) or a list / tuple of 2-D matrices.  A 2-D A with a 2-D b stays multi-target."""
    if isinstance(A, (list, tuple)):
        return True
    return not isinstance(A, _core.Problem) and len(getattr(A, "shape", ())) == 3


def _ndim(x):
    return len(x.shape) if hasattr(x, "shape") else np.ndim(x)


def _batch_members(A, b):
    """The problems of a batch call as (matrices, vectors) - 2-D / 1-D host or device objects, not yet converted - after
    the checks that refuse a call before any device work."""
    if b is None:
        raise ValueError("a batch needs b: (P, m) for a 3-D A, a sequence of vectors for a sequence of matrices")
    if not isinstance(b, (list, tuple)) and _ndim(b) == 3:
        raise ValueError("b must not be 3-D: a batch takes one right-hand side per problem")
    mats = list(A) if isinstance(A, (list, tuple)) else [A[i] for i in range(int(A.shape[0]))]
    if isinstance(b, (list, tuple)):
        vecs = list(b)
    elif _ndim(b) == 2:
        vecs = [b[i] for i in range(int(b.shape[0]))]
    else:
        raise ValueError("a batch needs one right-hand side per problem: b of shape (P, m) or a sequence of vectors")
    if len(mats) != len(vecs):
        raise ValueError(f"a batch of {len(mats)} matrices needs as many right-hand sides (got {len(vecs)})")
    for i, (Ai, bi) in enumerate(zip(mats, vecs)):
        if _ndim(Ai) != 2:
            raise ValueError(f"batch member {i}: A must be 2-D")
        if _ndim(bi) != 1 or (bi.shape[0] if hasattr(bi, "shape") else len(bi)) != Ai.shape[0]:
            raise ValueError(f"batch member {i}: b must be a vector of m = {Ai.shape[0]} entries")
    return mats, vecs


def _batch_L(L, P):
    if L is None:
        return None
    vals = [float(v) for v in L] if isinstance(L, (list, tuple, np.ndarray)) or _core.is_tensor(L) else [float(L)] * P
    if len(vals) != P:
        raise ValueError(f"L= needs one value per problem ({P}) or a scalar")
    return vals


class _Batch:
    """The members of a batch bound to the device: every problem within the LDS-resident limits (resident.hpp) gets its
    slice of one device buffer of A elements (per storage dtype) and of one of right-hand sides, converted exactly as
    Problem / to_device_vec convert a single call's inputs; the others keep their host / device objects and run one by
    one through the single path."""

    def __init__(self, mats, vecs, dtype):
        self.mats, self.vecs, self.P = mats, vecs, len(mats)
        self.likes = [_core.Like(Ai) for Ai in mats]
        self.shapes = [(int(Ai.shape[0]), int(Ai.shape[1])) for Ai in mats]
        self.kinds = ["bf16" if _core.stores_bf16(Ai, dtype) else "f32" for Ai in mats]
        self.fits = [_core.resident_fits(m, n) for m, n in self.shapes]
        self.groups = {}                         # dtype -> dict(idx, A, B, items)
        if any(self.fits):
            _core.require_gpu()
            self.device = next((Ai.device for Ai in mats if _core.is_tensor(Ai) and Ai.is_cuda),
                               torch.device("cuda", torch.cuda.current_device()))
        for kind in ("f32", "bf16"):
            idx = [i for i in range(self.P) if self.fits[i] and self.kinds[i] == kind]
            if idx:
                self.groups[kind] = self._bind(idx, torch.bfloat16 if kind == "bf16" else torch.float32)
        self.ldx = max([n for (m, n), ok in zip(self.shapes, self.fits) if ok] or [1])

    @classmethod
    def targets(cls, prob, Bt):
        """One bound A within the resident limits with the k columns of Bt (m x k, device) as right-hand sides: k members
        on the same elements, whose results stay on the device (likes None)."""
        bt, k, m = cls.__new__(cls), int(Bt.shape[1]), prob.m
        bt.P, bt.shapes, bt.likes, bt.device, bt.ldx = k, [(m, prob.n)] * k, [None] * k, prob.device, prob.n_dev
        bt.groups = {prob.dtype: dict(idx=list(range(k)), A=prob.A, B=Bt.t().contiguous(),     # (k, m): column j at j*m
                                      items=[(0, prob.lda, j * m, m, prob.n_dev) for j in range(k)])}
        return bt

    def _bind(self, idx, tdtype):
        dev = self.device
        a_off, b_off, items, ao, bo = [], [], [], 0, 0
        for i in idx:
            m, n = self.shapes[i]
            items.append((ao, n, bo, m, n))
            a_off.append(ao)
            b_off.append(bo)
            ao += m * n
            bo += m
        Abuf = torch.empty(max(ao, 1), dtype=tdtype, device=dev)
        Bbuf = torch.empty(max(bo, 1), dtype=torch.float32, device=dev)
        for i, o, q in zip(idx, a_off, b_off):
            m, n = self.shapes[i]
            Ai, dst = self.mats[i], Abuf[o:o + m * n].view(m, n)
            if _core.is_tensor(Ai):
                At = Ai.detach()
                if At.is_cuda:
                    dst.copy_(At.to(device=dev, dtype=tdtype))           # Problem: At.to(device, dtype).contiguous()
                else:
                    _core.upload_matrix(At, dst)
            else:
                _core.upload_matrix(torch.from_numpy(np.asarray(Ai)), dst)
            if self.vecs[i] is not None:
                Bbuf[q:q + m].copy_(_core.to_device_vec(self.vecs[i], dev))
        return dict(idx=idx, A=Abuf, B=Bbuf, items=items)

    def problem(self, i):
        """The single path's Problem of member i (members outside the resident limits)."""
        return _core.Problem(self.mats[i], self.vecs[i], "bf16" if self.kinds[i] == "bf16" else None)


def _batch_lipschitz(mats, vecs, dtype, n_iter=100, tol=1e-6, batch=None):
    """estimate_lipschitz of every member (ref:45-60): np.random.randn(n_i) drawn in problem order, as P single calls
    would draw them; one batched power iteration for the resident members, Problem.power_iter for the others."""
    bt = batch if batch is not None else _Batch(mats, vecs, dtype)
    v0s = [np.random.randn(n) for (m, n) in bt.shapes]
    L = [0.0] * bt.P
    for kind, g in bt.groups.items():
        V = torch.zeros(len(g["idx"]), bt.ldx, dtype=torch.float32, device=bt.device)
        for r, i in enumerate(g["idx"]):
            V[r, : bt.shapes[i][1]] = _core.to_device_vec(v0s[i], bt.device)      # Problem.vec_in's conversion
        Ls, _ = _core.power_iter_batch(g["A"], kind, g["items"], V, n_iter=n_iter, tol=tol)
        for i, Li in zip(g["idx"], Ls):
            L[i] = Li
    probs = {}
    for i in range(bt.P):
        if not bt.fits[i]:
            probs[i] = bt.problem(i)
            L[i] = probs[i].power_iter(v0s[i], n_iter=n_iter, tol=tol)[0]
    return L, probs


def _solve_batch(A, b, reg_type, lp, return_history, L, dtype):
    """X[i] = fista(A[i], b[i], ...) (fista_delta when `delta` is given) for every member, the resident ones in one
    launch (one workgroup per problem, fos_fista_run_batch), the others one by one through the single path."""
    mats, vecs = _batch_members(A, b)
    P = len(mats)
    L_given = _batch_L(L, P)
    bt = _Batch(mats, vecs, dtype)
    if L_given is None:
        L_vals, probs = _batch_lipschitz(mats, vecs, dtype, batch=bt)
    else:
        L_vals, probs = L_given, {}
    obj = (_objective_by_alpha(lp.alpha1, lp.alpha2) if lp.delta is None
           else _objective_by_reg(reg_type, lp.alpha1, lp.alpha2))
    fields = lp.params(1.0)                          # the members' parameters differ in the first step only
    results = [None] * P                             # per problem: (x, history or None, the metric entries it recorded)
    for kind, g in bt.groups.items():
        idx = g["idx"]
        # the device-side x history is bounded like the single path's chunks: split the batch where it would exceed it
        per = max(1, _HISTORY_CHUNK_BYTES // (8 * max(lp.max_iter, 1) * bt.ldx)) if return_history else len(idx)
        for c0 in range(0, len(idx), per):
            sub = range(c0, min(len(idx), c0 + per))
            params = [_lib.FistaParams(**dict(fields, tau=lp.tau(L_vals[idx[r]]))) for r in sub]
            for r, res in zip(sub, _run_batch_group(bt, kind, sub, params, lp, return_history, obj)):
                results[idx[r]] = res
    for i in range(P):
        if not bt.fits[i]:
            res, recorded = _metrics_of(lambda: _solve_one(probs.get(i) or bt.problem(i), None, reg_type, lp, return_history,
                                                           L_vals[i]))
            results[i] = (res if return_history else (res, None)) + (recorded,)
    for _, _, recorded in results:
        _metrics_add(recorded)
    xs, hists = [r[0] for r in results], [r[1] for r in results]
    if isinstance(A, (list, tuple)):
        X = xs
    elif _core.is_tensor(A):                 # each row is the single call's result (a tensor of that kind): stacked
        like = _core.Like(A)
        X = torch.stack(xs) if P else torch.zeros(0, int(A.shape[2]), dtype=like.dtype, device=like.device)
    else:
        X = np.stack(xs) if P else np.zeros((0, int(A.shape[2])))
    return (X, hists) if return_history else X


def _run_batch_group(bt, kind, sub, params, lp, record=False, obj=None):
    """One fos_fista_run_batch launch (two for a ragged batch) over the members r in `sub` of the group bt.groups[kind].
    Per member: (x, its history or None, the three metric lists it recorded)."""
    g, backtracking = bt.groups[kind], lp.backtracking
    idx = [g["idx"][r] for r in sub]
    items = [g["items"][r] for r in sub]
    t0 = time.perf_counter()
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    with torch.cuda.device(bt.device):
        ev0.record()
        out = _core.run_batch(g["A"], kind, g["B"], items, params, lp.max_iter, backtracking=backtracking, eta=lp.eta,
                              armijo_c=C, ldx=bt.ldx, record=record)
        ev1.record()
        ev1.synchronize()
    wall = time.perf_counter() - t0
    done = out["done"].cpu().tolist()
    stopped = out["stopped"].cpu().tolist()
    ls = out["ls"].cpu().tolist() if backtracking else None
    xs_dev = out["x"]
    # the launch's time in equal shares over the gradients of all its members, the searches' wall time over all its searches
    ngrad = [_ngrad(k, s) for k, s in zip(done, stopped)]
    dev_s, ngrad_all, done_all = ev0.elapsed_time(ev1) * 1e-3, sum(ngrad), sum(done)
    hs = out["hist"].cpu().numpy() if record else None
    results = []
    for r, i in enumerate(idx):
        n, like, k = bt.shapes[i][1], bt.likes[i], done[r]
        x = xs_dev[r, :n] if like is None else _core.from_device_vec(xs_dev[r, :n], like)     # None: stays on the device
        h = None
        if record:
            zero = torch.zeros(n, dtype=torch.float64, device=bt.device)
            h = {"x": [_core.from_device_vec(zero, like)] if lp.delta is None else [], "obj": []}   # ref:160 / ref:279
            _Records(like, h, obj).block(out["x_hist"][r, :k, :n], hs[r, :k])
        results.append((x, h, (_shares(ngrad[r], dev_s, ngrad_all), _shares(k, wall, done_all) if backtracking else [],
                               [int(v) for v in ls[r][:k]] if backtracking else [])))
    return results


# ---------------------------------------------------------------------
# FISTA                                                        ref:132-245
# FISTA-Δ                                                      ref:251-344
# ---------------------------------------------------------------------
def _lipschitz(prob, L, *, comm=None, cols=None, group=None, divisor=1.0):
    """L as the caller gave it, or estimated the way the problem is sharded (ref:155 / :273): one power iteration, one draw
    from the global NumPy stream.  divisor: what bounds the Hessian of the data term by lambda_max(A^T A) / divisor."""
    if L is not None:
        return float(L)
    if _weighted(prob):              # lambda_max(A^T W A); sigma' <= 1/4 bounds the weighted logistic Hessian by a quarter of it,
        return estimate_lipschitz(prob) / (4.0 if prob.loss == "logistic" else divisor)     # whichever front end took the handle
    if cols is not None:
        return _lipschitz_cols(prob, comm, cols)
    return estimate_lipschitz(prob, group=group) / divisor


def _solve(A, b, reg_type, lp, return_history, L, dtype, check_every, comm, group, cols):
    """The front end of fista and fista_delta: a batch, several targets or one problem, sharded or not."""
    reset_metrics()
    _refuse_multinomial(A, "fista / fista_delta")
    batch = _is_batch(A)
    B = None if batch else _targets(A, b)
    if batch or B is not None:
        if any(v is not None for v in (comm, group, cols)):
            what = "a batch (3-D A or a sequence of matrices)" if batch else "a 2-D b (several targets)"
            raise ValueError(f"{what} cannot be combined with comm= / group= / cols=")
        if batch:
            return _solve_batch(A, b, reg_type, lp, return_history, L, dtype)
        if return_history:
            raise ValueError("return_history=True is not available with a 2-D b (several targets)")
        return _solve_targets(A, B, lp, L, dtype, check_every)
    prob, reducer = _sharded_problem(A, b, dtype, comm, group, cols)
    return _solve_one(prob, reducer, reg_type, lp, return_history, L, check_every, comm, cols, group)


def _solve_one(prob, reducer, reg_type, lp, return_history, L, check_every=None, comm=None, cols=None, group=None):
    """One problem bound to the device: fista (ref:132-245), or fista_delta (ref:251-344) when `delta` is given.  The two
    differ in the momentum rule, in fista's gradient-norm stop and restarts, and in what the history holds."""
    like = prob.like
    L_val = _lipschitz(prob, L, comm=comm, cols=cols, group=group if reducer is not None else None)
    history = obj = None
    if lp.delta is None:
        obj = _objective_by_alpha(lp.alpha1, lp.alpha2)
        if return_history:
            zero = torch.zeros(prob.n, dtype=torch.float64, device=prob.device)
            history = {"x": [_core.from_device_vec(zero, like)], "obj": []}      # ref:160
    elif return_history:
        history, obj = {"x": [], "obj": []}, _objective_by_reg(reg_type, lp.alpha1, lp.alpha2)   # ref:279 (no x0 entry)
    st = lp.drive(prob, like, lp.tau(L_val), history=history, history_obj=obj, check_every=check_every, reducer=reducer)
    x_k = _core.from_device_vec(st.x_tensor(), like)
    return (x_k, history) if return_history else x_k


def fista(A, b, reg_type: str, alpha1: float, alpha2: float, backtracking: bool = False, eta: float = 0.5,
          t_init_factor: float = 1.0, max_iter: int = 500, tol: float = 0.0, tol_ratio: float = 0.0,
          adaptive_restart: bool = False, restart_threshold: float = 1.0, return_history: bool = False,
          *, L=None, dtype=None, check_every=None, comm=None, group=None, cols=None):
    """``comm=`` / ``group=``: A, b are THIS RANK's rows of a row-sharded problem (one process per GPU); every flag
    of the reference's loop works sharded - backtracking, history, restart, the stopping rules.  ``comm`` (a
    `distributed.Comm`) puts the one all-reduce per iteration on the kernels' stream under the C ABI; ``group`` (a
    torch.distributed group, any backend) does it between the kernels from Python.
    ``cols=(lo, hi, n_total)`` with ``comm=``: COLUMN sharding for very wide A - A is this rank's columns [lo, hi) of
    all rows, b the whole vector; x is partitioned (the result and the history are this rank's block), one all-reduce of
    an m-vector per iteration (backtracking: plus ONE all-reduce of the 16 candidates' m-vectors per search).
    Several targets: a 2-D ``b`` of shape (m, k), k >= 2, returns x of shape (n, k) whose column j is
    ``fista(A, b[:, j], ...)`` with the same L (estimated once); up to 16 columns share each read of A."""
    lp = _Loop(None, alpha1, alpha2, backtracking, eta, t_init_factor, max_iter, tol, tol_ratio, adaptive_restart,
               restart_threshold)
    return _solve(A, b, reg_type, lp, return_history, L, dtype, check_every, comm, group, cols)


def fista_delta(A, b, reg_type: str, alpha1: float, alpha2: float, delta: float, backtracking: bool = False,
                eta: float = 0.5, t_init_factor: float = 1.0, max_iter: int = 500, tol: float = 0.0,
                tol_ratio: float = 0.0, return_history: bool = False, *, L=None, dtype=None, check_every=None,
                comm=None, group=None, cols=None):
    reset_metrics()
    # Course requirement: delta > 2 for convergence guarantee                   ref:268
    assert delta > 2, "In FISTA-Δ, delta must be > 2 for convergence (course requirement)"
    lp = _Loop(delta, alpha1, alpha2, backtracking, eta, t_init_factor, max_iter, tol, tol_ratio, False, 1.0)
    return _solve(A, b, reg_type, lp, return_history, L, dtype, check_every, comm, group, cols)


# ---------------------------------------------------------------------
# Regularisation path (extension)
# ---------------------------------------------------------------------
# The host driver of the lockstep, shared by the four model families (squared and logistic here and in logistic.py, multinomial.py,
# multitask.py).  A family states what differs: how many adjacent columns one fit takes, fos_fista_params.group, the divisor of
# lambda_max(A^T A) in L, the launch of one group of fits, and what a refusal means.
LOCKSTEP_COLUMNS = 16

# width: columns per fit.  group: fos_fista_params.group of every handle.  divisor: L = lambda_max(A^T A) / divisor.
# launch(handles, first, number) -> served: `number` fits from fit `first` on, their width * number handles in one lockstep call.
# refusal: the text of the FosError a refused launch raises (fos_last_error appended), or None for the plain squared-loss path -
# what the lockstep does not serve, and a single fit, runs one by one (Fista.run).
_Family = collections.namedtuple("_Family", "width group divisor launch refusal")


def _columns(max_iter, lockstep_only, divisor=1.0):
    """The family of one column per fit on the problem's own b (fos_fista_run_multi): squared loss, and logistic with divisor 4.
    lockstep_only: a handle with sample weights, penalty factors, bounds, feature groups or the logistic loss."""
    return _Family(1, 0, divisor, lambda handles, first, number: _core.run_multi(handles, max_iter),
                   "fos_fista_run_multi refused the lockstep: " if lockstep_only else None)


def _refused(prob, text):
    return _lib.FosError(text + prob.lib.fos_last_error().decode("utf-8", "replace"))


def _rows(A):
    return A.m if isinstance(A, _core.Problem) else int(A.shape[0] if hasattr(A, "shape") else np.shape(A)[0])


def _check_path_args(alphas, delta):
    alphas = [(float(a1), float(a2)) for a1, a2 in alphas]
    if not alphas:
        raise ValueError("alphas: at least one (alpha1, alpha2) pair is needed")
    if delta is not None and not delta > 2:
        raise ValueError("delta: FISTA-Δ needs delta > 2")
    return alphas


def _groups(count, per):
    return [(first, min(per, count - first)) for first in range(0, count, per)]


def pack_groups(count, classes):
    """How `count` fits of a C-class model share the 16 lockstep columns: ``[(first, number), ...]``, floor(16 / C) fits per
    group, the last group partial.  Fit i of a group owns columns ``i * C .. i * C + C - 1``.  Pure: no device work."""
    classes = int(classes)
    if not 2 <= classes <= _core.MAX_CLASSES:
        raise ValueError(f"classes: 2 <= C <= {_core.MAX_CLASSES} expected, got {classes}")
    if count < 0:
        raise ValueError("count must be >= 0")
    return _groups(count, LOCKSTEP_COLUMNS // classes)


def _path_params(prob, alphas, L, fam, t_init_factor, delta, *, comm=None, cols=None, **control):
    """One parameter set per weight pair: the step from L of the family's data term (estimated unless given: one draw from the
    global NumPy stream) and the handle's largest penalty factor; control: the stopping and restart fields of `_params`."""
    L_val = _lipschitz(prob, L, comm=comm, cols=cols, divisor=fam.divisor)
    mode = _lib.MODE_FISTA if delta is None else _lib.MODE_DELTA
    return [_params(_tau(L_val, a2, t_init_factor, prob.penalty_max), a1, a2, mode=mode, delta=delta, group=fam.group, **control)
            for a1, a2 in alphas]


def _run_path(prob, prms, fam, max_iter, cols=None):
    """fam.width state machines per parameter set on `prob`, fit-major, advanced max_iter iterations in lockstep groups of up
    to 16 columns; one grad_call_times entry per lockstep iteration per group.  The handles.  A family with a refusal text has
    the lockstep as its one form: groups of 16 columns, a group of one included.  The plain squared-loss path (fam.refusal
    None) takes groups of 4 for up to 4 weights - the multi-vector VALU pass where the shape has one."""
    W = fam.width
    handles = [_new_state(prob, prm) for prm in prms for _ in range(W)]
    gtimer = _EventTimer(grad_call_times)
    per = 4 if fam.refusal is None and len(prms) <= 4 and cols is None else LOCKSTEP_COLUMNS // W
    for first, number in _groups(len(prms), per):
        group = handles[first * W:(first + number) * W]
        ev = gtimer.start()
        if (fam.refusal is None and len(group) == 1) or not fam.launch(group, first, number):
            if fam.refusal is not None:
                raise _refused(prob, fam.refusal)
            for st in group:
                st.run(max_iter)
        gtimer.stop(ev, max_iter)
    gtimer.flush()
    return handles


def _path_result(handles, fam, like, return_info):
    """What a path call returns: per fit x (a vector, or n x width with the fit's columns stacked) as the kind that went in, and
    with return_info (iterations, stop_code) read from the first handle of every fit."""
    W = fam.width
    xs = [_core.from_device_vec(handles[i].x_tensor() if W == 1 else torch.stack([st.x_tensor() for st in handles[i:i + W]], dim=1),
                                like) for i in range(0, len(handles), W)]
    if return_info:
        stats = [st.status() for st in handles[::W]]
        return xs, [(int(s.k), int(s.stopped)) for s in stats]
    return xs


def _objective_block(prob, X, width):
    """The members an objective is asked for as an n x width x k float64 device block, and whether one member came in: a vector
    (width 1) or an n x width matrix, or k of them along a last axis.  ValueError for any other shape."""
    xt = X.detach() if _core.is_tensor(X) else torch.from_numpy(np.asarray(X, dtype=np.float64))
    member = (prob.n,) if width == 1 else (prob.n, width)
    single = xt.dim() == len(member)
    if xt.dim() not in (len(member), len(member) + 1) or tuple(xt.shape[:len(member)]) != member:
        raise ValueError(f"x: a vector of length {prob.n} or an {prob.n} x k block expected" if width == 1 else
                         f"X: an {prob.n} x {width} matrix or an {prob.n} x {width} x k block expected, got shape {tuple(xt.shape)}")
    return xt.reshape(prob.n, width, 1 if single else xt.shape[-1]).to(device=prob.device, dtype=torch.float64), single


def _objective_value(prob, Xd, single, data_term, alpha1, alpha2, row_groups=False):
    """data term + penalties of every member of Xd (`_objective_block`): a float for a single member, else k float64 values.
    data_term(block, number) -> the data terms of `number` members, block their n x (number * width) columns member-major, at
    most 16.  The penalties are alpha1 sum_j p_j |x_j| - with row_groups alpha1 sum_j p_j ||X[j, :]||_2 - plus 0.5 alpha2 sum_j p_j
    x_j^2 over all columns of a member, p the fp32 penalty factors of the handle as bound (else 1)."""
    n, W, k = Xd.shape
    data = []
    for first, number in _groups(k, LOCKSTEP_COLUMNS // W):
        data += data_term(Xd[:, :, first:first + number].permute(0, 2, 1).reshape(n, number * W), number)
    Xh = Xd.cpu().numpy()
    pf = np.ones(n) if prob.penalty_factor is None else prob.penalty_factor.to("cpu", torch.float64).numpy()
    l1 = (pf[:, None] * np.sqrt((Xh * Xh).sum(axis=1))).sum(axis=0) if row_groups else (pf[:, None, None] * np.abs(Xh)).sum(axis=(0, 1))
    val = (np.asarray(data, dtype=np.float64) + float(alpha1) * l1 +
           0.5 * float(alpha2) * (pf[:, None, None] * Xh * Xh).sum(axis=(0, 1)))
    return float(val[0]) if single else val


def fista_path(A, b, alphas, t_init_factor: float = 1.0, max_iter: int = 500, *, delta=None, L=None, dtype=None,
               comm=None, cols=None, tol: float = 0.0, tol_ratio: float = 0.0, adaptive_restart: bool = False,
               restart_threshold: float = 1.0, return_info: bool = False):
    """Solve the same (A, b) for several regularisation weights at once.

    ``alphas`` is a sequence of ``(alpha1, alpha2)`` pairs.  The result is the list of solutions that
    ``fista(A, b, ..., alpha1, alpha2, t_init_factor=t_init_factor, max_iter=max_iter, L=L)`` (or ``fista_delta``
    when ``delta`` is given) would return one by one - same iterates - but the weights advance in lockstep: up to four
    share one read of A per iteration in the multi-vector form of the single-pass kernel (fp32, n <= 8192); five to
    sixteen run on the matrix cores as two GEMM-shaped products per iteration for all of them (fp32 and bf16 storage,
    any streaming shape: csrc/gram_batch.hpp).  Shapes without such a kernel simply run one by one.  L is estimated once (one power iteration, one draw from the global
    NumPy stream) unless given.
    ``adaptive_restart`` / ``restart_threshold`` / ``tol_ratio`` (fista's arguments of the same names) keep the lockstep:
    momentum restarts and the ratio stop are decided per weight on the device every iteration and a stopped weight
    becomes a masked column of the block (three or more weights, matrix-core pass).  ``tol`` adds the reference's
    gradient-norm rule, which sits before the update: those runs go one by one.  ``return_info=True`` also returns
    ``[(iterations, stop_code), ...]`` per weight.
    ``cols=(lo, hi, n_total)`` with ``comm=``: COLUMN sharding (A is this rank's columns, b whole, each returned x this
    rank's block) - the lockstep keeps ONE exchange per row panel, the panel's 16 residual columns between the two
    products, plus 64 doubles of step norms per iteration.
    A handle with penalty factors or bounds (``prepare_penalized`` / ``Problem.set_penalty``): the objective is 0.5 ||Ax - b||^2
    + alpha1 sum_j p_j |x_j| + 0.5 alpha2 sum_j p_j x_j^2 subject to lower_j <= x_j <= upper_j (``lower=0.0``: the non-negative
    lasso; p_j = 0: an unpenalised coordinate).  Such a problem runs on the matrix-core lockstep alone, a single weight as a one-column lockstep, with the step t_init_factor / (L + alpha2 max_j p_j)
    (L is the constant of the data term and does not depend on the constraints); ``tol``, ``comm=`` and ``cols=`` are
    ValueErrors and a refusal raises.
    A handle with feature groups (``prepare_grouped`` / ``Problem.set_feature_groups``): the penalty is alpha1 [(1 - l1_ratio)
    sum_g w_g ||x_g||_2 + l1_ratio ||x||_1] + 0.5 alpha2 ||x||_2^2, the (sparse-)group lasso; the lockstep alone likewise, with
    the step of the separable penalty, t_init_factor / (L + alpha2)."""
    reset_metrics()
    _refuse_multinomial(A, "fista_path")
    if delta is not None:
        assert delta > 2, "In FISTA-Δ, delta must be > 2 for convergence (course requirement)"
    weighted = _weighted(A) or _has_coord(A)
    if weighted and (tol != 0.0 or comm is not None or cols is not None):
        raise ValueError("a handle with sample weights, penalty factors, bounds or feature groups runs on the lockstep alone: no tol (the "
                         "gradient-norm rule), comm= or cols=")
    # comm: A, b are this rank's rows (matrix-core pass, one all-reduce of the 16 gradients per iteration)
    prob, _ = _sharded_problem(A, b, dtype, comm, None, cols)
    fam = _columns(max_iter, weighted)
    # the tolerances go to the device as given: a negative one is refused there (fos_fista_reset), not read as "off"
    prms = _path_params(prob, alphas, L, fam, t_init_factor, delta, comm=comm, cols=cols, tol=tol, tol_ratio=tol_ratio,
                        grad_rule=delta is None, adaptive_restart=adaptive_restart, restart_threshold=restart_threshold)
    return _path_result(_run_path(prob, prms, fam, max_iter, cols), fam, prob.like, return_info)


# ---------------------------------------------------------------------
# K-fold cross-validation of a regularisation path (extension)
# ---------------------------------------------------------------------
CVResult = collections.namedtuple("CVResult", "alphas mse mean_mse best x coefs info")

CV_MAX_FOLDS = 255                       # fold ids are bytes 0..254 on the device; 255 stands for "no fold"


def _cv_folds(folds, m):
    """The fold id of every row (uint8 ndarray of length m) and the fold sizes, from `folds` as fista_cv takes it: an int
    K >= 2 (contiguous blocks, the first m % K folds one row longer) or an integer array of m ids 0..K-1, K <= 255.
    ValueError for anything else and for an empty fold; no device work."""
    if isinstance(folds, (int, np.integer)) and not isinstance(folds, (bool, np.bool_)):
        K = int(folds)
        if K < 2 or K > CV_MAX_FOLDS:
            raise ValueError(f"folds: an int K needs 2 <= K <= {CV_MAX_FOLDS}, got {K}")
        if K > m:
            raise ValueError(f"folds: {K} folds of {m} rows leave a fold empty")
        sizes = np.array([m // K + (1 if f < m % K else 0) for f in range(K)], dtype=np.int64)
        return np.repeat(np.arange(K, dtype=np.uint8), sizes), sizes
    arr = folds.detach().cpu().numpy() if _core.is_tensor(folds) else np.asarray(folds)
    if arr.ndim != 1 or arr.shape[0] != m:
        raise ValueError(f"folds: an int K or one fold id per row ({m}) expected, got shape {arr.shape}")
    if arr.dtype.kind not in "iu":
        raise ValueError("folds: integer fold ids expected")
    if arr.min() < 0 or arr.max() > CV_MAX_FOLDS - 1:
        raise ValueError(f"folds: ids must lie in 0..{CV_MAX_FOLDS - 1}")
    sizes = np.bincount(arr.astype(np.int64), minlength=int(arr.max()) + 1)
    if len(sizes) < 2:
        raise ValueError("folds: at least two folds are needed")
    if (sizes == 0).any():
        raise ValueError(f"folds: fold {int(np.argmin(sizes))} is empty")
    return arr.astype(np.uint8), sizes.astype(np.int64)


def _cv_weight_sums(prob, ids, K):
    """The weight sum of every fold of a weighted handle (float64, length K): the denominators of the held-out scores.
    ValueError for a fold whose weights sum to zero - nothing could be scored on it - before any solver launch."""
    w = prob.sample_weight.to("cpu", torch.float64).numpy()
    sums = np.bincount(np.asarray(ids, dtype=np.int64), weights=w, minlength=K).astype(np.float64)
    if (sums <= 0.0).any():
        raise ValueError(f"folds: the sample weights of fold {int(np.argmin(sums))} sum to zero")
    return sums


def _cv_sizes(prob, ids, sizes):
    """The denominators of the held-out scores: the fold sizes, on a weighted handle the folds' weight sums."""
    return _cv_weight_sums(prob, ids, len(sizes)) if _weighted(prob) else sizes


def _run_cv(prob, ids, K, prms, fam, max_iter, refusal=None):
    """Every (fold, weight) pair as fam.width columns of the masked lockstep on the one bound A: groups of up to 16 columns,
    fold-major, each one fos_fista_run_multi_folds call and one fos_residual_batch_folds pass.  (x n x K x L float64 device - n x
    width x K x L for a family of several columns per fit -, held-out totals K x L, info).  A refused launch raises `refusal`
    (fos_last_error appended); with None the result is None where the entry point does not serve the problem, which the first
    group decides."""
    W, La = fam.width, len(prms)
    pairs = [(f, a) for f in range(K) for a in range(La)]
    ids_dev = _core.fold_ids_tensor(ids, prob.device)
    X = torch.zeros(prob.n, W, K, La, dtype=torch.float64, device=prob.device)
    total = np.zeros((K, La))
    info = [[None] * La for _ in range(K)]
    gtimer = _EventTimer(grad_call_times)
    for first, number in _groups(len(pairs), LOCKSTEP_COLUMNS // W):
        grp = pairs[first:first + number]
        held = [f for f, _ in grp for _ in range(W)]
        handles = [_new_state(prob, prms[a]) for _, a in grp for _ in range(W)]
        ev = gtimer.start()
        if not _core.run_multi_folds(handles, ids_dev, held, max_iter):
            if refusal is not None:
                raise _refused(prob, refusal)
            if first == 0:
                return None
            raise _lib.FosError("fos_fista_run_multi_folds refused a later group of a problem it served")
        gtimer.stop(ev, max_iter)
        xg = torch.stack([st.x_tensor() for st in handles], dim=1)   # enqueued behind the run; the status reads below wait for it
        q = prob.residual_batch_folds(xg, ids_dev, held)
        if q is None:
            raise _refused(prob, f"fos_residual_batch_folds refused the {'multinomial ' if prob.classes else ''}problem: ")
        stats = [st.status() for st in handles[::W]]             # a fit's status is that of its first handle
        if W == 1:                                               # (the columns of a joint fit have no stopping rule)
            gtimer.recount(max(int(s.k) for s in stats))         # the lockstep iterations actually run
        for i, (f, a) in enumerate(grp):
            X[:, :, f, a] = xg[:, i * W:(i + 1) * W]
            total[f, a] = q[i * W]
            info[f][a] = (int(stats[i].k), int(stats[i].stopped))
    gtimer.flush()
    return (X[:, 0] if W == 1 else X), total, info


def _refit(prob, prm, fam, max_iter):
    """The fit on all rows at one parameter set, through the path driver."""
    return _path_result(_run_path(prob, [prm], fam, max_iter), fam, prob.like, False)[0]


def _cv_result(kind, like, alphas, total, sizes, refit, X, info):
    """The CV result tuple `kind` from the held-out totals (K x L) and their denominators: the scores, their mean over the folds,
    the argmin, x = refit(best) (refit None: no refit) and the fits X as the kind that went in (None: not asked for)."""
    score = total / sizes[:, None].astype(np.float64)       # weighted: the held-out weighted sum over the held-out weight sum
    mean = score.mean(axis=0)
    best = int(np.argmin(mean))
    x = None if refit is None else refit(best)
    return kind(alphas, score, mean, best, x, None if X is None else _core.from_device_vec(X, like), info)


def _cv_fold_by_fold(prob, ids, K, prms, max_iter):
    """The slow path, for what the masked lockstep refuses: per fold the training rows gathered into a device copy (one
    fold's copy alive at a time), the path run on the copy, the held-out rows gathered and scored with
    fos_residual_objective.  Same results, K copies and K times the reads."""
    La = len(prms)
    idt = torch.from_numpy(ids.astype(np.int64)).to(prob.device)
    X = torch.zeros(prob.n, K, La, dtype=torch.float64, device=prob.device)
    sse = np.zeros((K, La))
    info = [[None] * La for _ in range(K)]
    for f in range(K):
        rows = torch.nonzero(idt != f).squeeze(1)
        sub = _core.Problem(prob.A.index_select(0, rows), prob.b.index_select(0, rows), prob.dtype)
        handles, recorded = _metrics_of(lambda: _run_path(sub, prms, _columns(max_iter, False), max_iter))
        _metrics_add(recorded)
        del sub
        rows = torch.nonzero(idt == f).squeeze(1)
        held = _core.Problem(prob.A.index_select(0, rows), prob.b.index_select(0, rows), prob.dtype)
        for a, st in enumerate(handles):
            x = st.x_tensor()
            s = st.status()
            X[:, f, a] = x[: prob.n]
            sse[f, a] = held.residual_objective(x)[0]
            info[f][a] = (int(s.k), int(s.stopped))
        del handles, held
    return X, sse, info


def fista_cv(A, b, alphas, folds=5, t_init_factor: float = 1.0, max_iter: int = 500, *, delta=None, L=None, dtype=None,
             tol_ratio: float = 0.0, adaptive_restart: bool = False, restart_threshold: float = 1.0, refit: bool = True,
             return_coefs: bool = False):
    """K-fold cross-validation of a regularisation path: which of ``alphas`` (``(alpha1, alpha2)`` pairs, as in
    ``fista_path``) predicts held-out rows best.

    ``folds``: an int K >= 2 - contiguous blocks of rows, the first ``m % K`` folds one row longer - or an integer array
    with one fold id 0..K-1 per row, K <= 255 (shuffled or stratified splits are such arrays).  Every fold must be
    non-empty; anything else raises ValueError before any device work.

    All K x L fits (K folds, L weights) advance in lockstep on the ONE device copy of A: fit (f, a) is column
    ``f * L + a`` of the matrix-core pass of ``fista_path`` whose residual is zero on the rows of fold f, so it solves the
    problem of the other rows; up to 16 columns share each read of A (fos_fista_run_multi_folds) and no row is ever
    gathered.  The held-out squared errors of a group come from one further pass with the complementary mask.

    ``L`` is estimated once, on the whole A, unless given (one power iteration, one draw from the global NumPy stream, like
    ``fista_path``) and used for every fold: lambda_max(A_train^T A_train) <= lambda_max(A^T A), so the step 1 / L is valid
    for every training set.  Contract: ``coefs[:, f, a]`` is what ``fista(A[train_f], b[train_f], ..., alpha1, alpha2, L=L)``
    returns (``fista_delta`` with ``delta``) for that L, with the same ``t_init_factor``, ``max_iter``, ``tol_ratio``,
    ``adaptive_restart`` and ``restart_threshold``; momentum restarts and the ratio stop are decided per column on the device.
    There is no ``tol`` (the gradient-norm rule), no backtracking and no sharding here.

    Returns ``CVResult(alphas, mse, mean_mse, best, x, coefs, info)``: ``mse[f, a]`` the held-out mean squared error
    (K x L float64 ndarray), ``mean_mse`` its mean over the folds, ``best`` the argmin (first on ties), ``x`` the fit on ALL
    rows at ``alphas[best]`` with the same L and parameters (``refit=True``; else None), ``coefs`` the n x K x L fits
    (``return_coefs=True``; else None), ``info[f][a] = (iterations, stop_code)``.  ``grad_call_times`` gets one entry per
    lockstep iteration actually run per group of columns.

    The slow path: problems the lockstep does not serve (A that fits one CU's LDS, n <= 64, ragged or misaligned rows,
    rows wider than 16384 columns) run fold by fold on gathered device copies of the training rows, one copy alive at a
    time - the same results at K copies and K times the reads of A.

    A handle with sample weights (``prepare_weighted``): every fit minimises the weighted objective of its training rows,
    ``mse[f, a]`` is the weighted held-out sum of squares over the held-out weight sum (a fold whose weights sum to zero is a
    ValueError before any solver launch), the refit runs in the lockstep too, and a refusal raises - there is no slow path.

    A handle with penalty factors or bounds (``prepare_penalized``), as in ``fista_path``: the constraints belong to
    the coordinates, so every fold's fit carries them; the step is t_init_factor / (L + alpha2 max_j p_j); the refit runs in
    the lockstep and a refusal raises - there is no slow path.

    A handle with feature groups (``prepare_grouped``) likewise: every fold's fit is the (sparse-)group lasso of its training
    rows."""
    reset_metrics()
    _refuse_multinomial(A, "fista_cv")
    if delta is not None:
        assert delta > 2, "In FISTA-Δ, delta must be > 2 for convergence (course requirement)"
    alphas = [(float(a1), float(a2)) for a1, a2 in alphas]
    if not alphas:
        raise ValueError("alphas: at least one (alpha1, alpha2) pair is needed")
    ids, sizes = _cv_folds(folds, _rows(A))
    K = len(sizes)
    prob = _core.as_problem(A, b, dtype)
    if prob.b is None:
        raise ValueError("fista_cv needs b")
    lockstep_only = _weighted(prob) or _has_coord(prob)
    sizes = _cv_sizes(prob, ids, sizes)
    fam = _columns(max_iter, lockstep_only)
    prms = _path_params(prob, alphas, L, fam, t_init_factor, delta, tol_ratio=tol_ratio, adaptive_restart=adaptive_restart,
                        restart_threshold=restart_threshold)
    out = _run_cv(prob, ids, K, prms, fam, max_iter)
    if out is None:
        if lockstep_only:            # no unweighted or unconstrained slow path may answer for such a handle
            raise _refused(prob, "fos_fista_run_multi_folds refused the lockstep of a handle with sample weights, penalty factors or bounds: ")
        out = _cv_fold_by_fold(prob, ids, K, prms, max_iter)
    X, sse, info = out

    def refit_at(best):
        if lockstep_only:
            return _refit(prob, prms[best], fam, max_iter)
        st = _new_state(prob, prms[best])                        # a plain handle: the single-target run, no metric entries
        st.run(max_iter)
        return _core.from_device_vec(st.x_tensor(), prob.like)
    return _cv_result(CVResult, prob.like, alphas, sse, sizes, refit_at if refit else None, X if return_coefs else None, info)
