"""GPU: every ordered pair of FISTA run forms on ONE handle (tests/_forms.py names the forms, families, classes and which
forms each family serves; tests/test_fista_forms.py guards the table and shows that a wrong transition moves the answer by
100 x the tolerance checked here).

A pair cell takes a fresh handle, runs form X for nx iterations, form Y for ny, a closer (run(2); two grad + update pairs on
the resident families; X again for 2 in the backtracking class, whose step plain run does not search) and status().  A second
handle on the same Problem with other weights runs the same sequence, call by call in turn, so that every workspace shared
through the Problem changes hands between any two calls of a handle.  Both must be the fp64 oracle's run on the stored A -
iterate to 1e-5, k / restarts / stopped exactly, t_prev and beta to 1e-14, step norms to 1e-4, ||x||_1 and ||x||^2 to 1e-5 -
and the uninterrupted run(total) of a third handle to 1e-6; the second handle is checked the same way right after Y as well
(the first one goes on unasked).  The oracle runs once per (family, class, parameters, weights)
and the uninterrupted run once per total; cells only look them up.

A form that waits grid-wide with a time bound (run_fused, run_chip, run routed to either) may answer FOS_ERR_STATE on a
shared machine: the cell then checks that k and the iterate are as before the call, runs grad + update for those iterations
instead and counts the event; the last test fails if that happened in more than one in ten of such cells.  No cell repeats
a call that answered so, and nothing here provokes a time-out.  Two cases the count cannot see: on T, fos_fista_run routed to
the chip loop takes the two launches itself when the chip loop answers so (a run_routed cell there checks the result, not
which loop ran); and fos_fista_run_fused documents its state as INVALID after a wait that ran out, so such an event on
S-f32 fails its cell at "the state is the one before the call" instead of being counted."""
import numpy as np
import pytest
import torch

from tests import _data, _forms as F

pytestmark = pytest.mark.gpu

WAITS = dict(cells=0, events=0, counted=0)          # cells with a grid-wide wait, waits that ran out, cells that reported


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


class Env:
    """One family: the device matrix, its Problems (default plan and routed plan), and the caches of the oracle's runs."""

    def __init__(self, fos, family, cus):
        from fastoptsolver_amd import _core
        self.family, self.cus, self.spec = family, cus, F.families(cus)[family]
        bf16 = self.spec["dtype"] == "bf16"
        rounder = (lambda a: torch.as_tensor(a).to(torch.bfloat16).to(torch.float32).numpy()) if bf16 else None
        self.A, self.b, self.L, self.lam = F.make_data(family, cus, rounder)
        At = torch.as_tensor(self.A.astype(np.float32)).to(torch.bfloat16 if bf16 else torch.float32).cuda()
        assert np.array_equal(At.to(torch.float64).cpu().numpy(), self.A)
        b32 = self.b.astype(np.float32)
        self.prob = {"default": fos.prepare(At, b32)}
        if self.spec["routed"]:
            self.prob["routed"] = fos.prepare(At, b32)
            self.prob["routed"].replan(**self.spec["routed"])
        bt = torch.as_tensor(b32).cuda()
        self.B = bt[:, None].repeat(1, 3).contiguous()                               # run_multi_rhs: B = b repeated
        self.fold_ids = _core.fold_ids_tensor(np.arange(self.spec["m"]) % 3, At.device)
        self.oracle, self.whole = {}, {}

    def states(self, cls, prm, w, tau_switch=None):
        key = (cls, prm["name"], w, tau_switch)
        if key not in self.oracle:
            f1, a2 = F.weights(self.family, cls)[w]
            self.oracle[key] = F.oracle_states(self.A, self.b, self.L, prm, f1 * self.lam, a2, F.WINDOW,
                                               backtracking=cls == "backtracking", tau_switch=tau_switch)
        return self.oracle[key]


_ENVS = {}


@pytest.fixture(scope="module")
def env_of(fos):
    cus = int(fos.prepare(torch.zeros(8, 68, device="cuda")).plan()["cus"])

    def get(family):
        if family not in _ENVS:
            _ENVS[family] = Env(fos, family, cus)
        return _ENVS[family]
    yield get
    _ENVS.clear()


class Handle:
    """A fos_fista handle with what a caller keeps beside it: its parameters, the current step of a search, the log of the
    searches, and the other handles of its lockstep calls."""

    def __init__(self, env, cls, prm, w, plan="default", weights=None):
        from fastoptsolver_amd import _core, _lib
        self.env, self.cls, self.prm, self.w, self.plan = env, cls, prm, w, plan
        f1, self.a2 = weights if weights is not None else F.weights(env.family, cls)[w]
        self.a1 = f1 * env.lam
        self.tau = F.tau_of(prm, env.L, self.a2)
        self.st = _core.Fista(env.prob[plan])
        self.st.reset(self.tau, self.a1, self.a2, mode={"fista": _lib.MODE_FISTA, "delta": _lib.MODE_DELTA, "ista": _lib.MODE_ISTA}[prm["mode"]],
                      prox_kind=_lib.PROX_ENET if prm["prox"] == "enet" else _lib.PROX_L1, delta=prm.get("delta", 0.0),
                      adaptive_restart=prm.get("adaptive_restart", False), restart_threshold=prm.get("restart_threshold", 1.0),
                      tol_ratio=prm.get("tol_ratio", 0.0))
        self.ls, self.taus, self.others = [], [], []
        self.waited, self.done = 0, 0                       # grid-wide waits that ran out; iterations asked for so far

    def siblings(self, count):
        while len(self.others) < count:
            self.others.append(Handle(self.env, self.cls, self.prm, self.w, self.plan, F.SIBLING_WEIGHTS[len(self.others)]))
        return [self.st] + [h.st for h in self.others[:count]]

    def x(self):
        return self.st.x_tensor().cpu().numpy()


def _search_on_host(h):
    """One iteration as iterative_solvers' host-driven loop runs it: grad, candidates, set_tau, update."""
    from fastoptsolver_amd import iterative_solvers as its
    st, eta = h.st, h.prm.get("eta", F.ETA_DEFAULT)
    smooth_a2 = h.a2 if h.prm["prox"] == "l1" and h.a2 > 0 else 0.0
    st.grad()
    t, steps = h.tau, 0
    while True:
        rows = st.trial_batch(t, eta, 16)                   # (served on every family with a backtracking class)
        hit = False
        for tr in rows:
            if its._armijo_accepts(tr, t, smooth_a2, F.GRAD_EPS):
                hit = True
                break
            t *= eta
            steps += 1
        if hit:
            break
    st.set_tau(t)
    st.update()
    h.tau = t
    h.ls.append(steps)
    h.taus.append(t)
    return True


def _device_search(h, iters, recorded):
    eta = h.prm.get("eta", F.ETA_DEFAULT)
    if recorded:
        out = h.st.run_recorded(iters, True, eta, F.ARMIJO_C, F.GRAD_EPS)
        pair = None if out is None else (out["ls"], out["taus"])
    else:
        pair = h.st.run_backtracking(iters, eta, F.ARMIJO_C, F.GRAD_EPS)
    if pair is None:
        return False
    s = h.st.status()                                 # the step lives on the device: a caller reads it there
    h.ls += pair[0][:iters].cpu().tolist()
    h.taus += pair[1][:iters].cpu().tolist()
    h.tau = float(s.tau)
    return True


def _pair(h, dual):
    h.st.grad(dual=dual)
    h.st.update()
    return True


def calls(h, form, iters):
    """The calls of `iters` iterations of a form, as thunks that answer True (ran) or False (refused: not served)."""
    from fastoptsolver_amd import _core
    st = h.st
    if form in ("run", "run_routed"):
        assert form == "run" or h.plan == "routed"
        return [lambda: st.run(iters) is None]
    if form in ("grad_update", "graddual_update"):
        return [lambda: _pair(h, form == "graddual_update")] * iters
    if form == "host_search":
        return [lambda: _search_on_host(h)] * iters
    one = {
        "run_history": lambda: st.run_history(iters) is not None,
        "run_recorded": lambda: st.run_recorded(iters, False, F.ETA_DEFAULT, F.ARMIJO_C, F.GRAD_EPS) is not None,
        "run_fused": lambda: st.run_fused(iters),
        "run_chip": lambda: st.run_chip(iters),
        "run_resident": lambda: st.run_resident(iters) is not None,
        "run_resident_rec": lambda: st.run_resident(iters, record=True) is not None,
        "run_multi4": lambda: _core.run_multi(h.siblings(3), iters),
        "run_multi5": lambda: _core.run_multi(h.siblings(4), iters),
        "run_multi_rhs": lambda: _core.run_multi_rhs(h.siblings(2), h.env.B, iters),
        "run_multi_folds": lambda: _core.run_multi_folds(h.siblings(1), h.env.fold_ids, [-1, -1], iters),
        "run_backtracking": lambda: _device_search(h, iters, False),
        "run_recorded_bt": lambda: _device_search(h, iters, True),
    }
    return [one[form]]


def guarded(h, form, iters, thunk):
    """A call of a form with a bounded grid-wide wait: FOS_ERR_STATE means "the state is the one before the call" - checked -
    and the iterations run as grad + update pairs instead.  The event is counted; the call is not repeated."""
    from fastoptsolver_amd import _lib
    if form not in F.GRID_WAIT_FORMS:
        return thunk()
    before, k = h.x(), h.done                          # (a copy of x: no call that would touch the mirror before the form)
    try:
        return thunk()
    except _lib.FosError as err:
        if "code -3" not in str(err) or "timed out" not in str(err):
            raise
    assert int(h.st.status().k) == k and np.array_equal(h.x(), before), (form, "FOS_ERR_STATE moved the handle")
    h.waited += 1
    for _ in range(iters):
        _pair(h, False)
    return True


def run_in_turn(handles, form, iters):
    """The calls of a form on every handle, call by call in turn.  True when all ran, False when all refused."""
    seqs = [calls(h, form, iters) for h in handles]
    got = set()
    for step in zip(*seqs):
        for h, thunk in zip(handles, step):
            got.add(bool(guarded(h, form, iters, thunk)))
    assert len(got) == 1, (form, got)
    for h in handles:
        h.done += iters if True in got else 0
    return got.pop()


def whole_run(env, cls, prm, w, total):
    """x after an uninterrupted run(total) on a handle of its own, once per (class, parameters, weights, total)."""
    key = (cls, prm["name"], w, total)
    if key not in env.whole:
        h = Handle(env, cls, prm, w)
        h.st.run(total)
        env.whole[key] = h.x()
    return env.whole[key]


def close(a, b, rel):
    return abs(a - b) <= rel * abs(b) if b != 0.0 else abs(a) <= rel


def check(h, total, what, uninterrupted=True):
    """The handle against the oracle's state after `total` iterations (and the uninterrupted run)."""
    env = h.env
    o = env.states(h.cls, h.prm, h.w)[total]
    s, x = h.st.status(), h.x()
    tag = (env.family, h.cls, h.prm["name"], h.w) + tuple(what)
    assert int(s.k) == o["k"], (tag, int(s.k), o["k"])
    assert int(s.restarts) == o["restarts"] and int(s.stopped) == o["stopped"], (tag, int(s.restarts), o["restarts"], int(s.stopped))
    err = _data.rel(x, o["x"])
    assert err < F.TOL, (tag, "iterate vs oracle", err)
    if uninterrupted:
        err = _data.rel(x, whole_run(env, h.cls, h.prm, h.w, total))
        assert err < 1e-6, (tag, "iterate vs uninterrupted run", err)
    assert close(s.t_prev, o["t"], 1e-14) and close(s.beta, o["beta"], 1e-14), (tag, s.t_prev, o["t"], s.beta, o["beta"])
    assert close(s.this_step, o["this"], 1e-4) and close(s.prev_step, o["prev"], 1e-4), (tag, s.this_step, o["this"], s.prev_step, o["prev"])
    assert close(s.xnorm1, o["x1"], 1e-5) and close(s.xnorm2, o["x2"], 1e-5), (tag, s.xnorm1, o["x1"], s.xnorm2, o["x2"])


def plan_of(*forms):
    return "routed" if "run_routed" in forms else "default"


def closer(handles, X):
    env = handles[0].env
    if handles[0].cls == "backtracking":
        return run_in_turn(handles, X, F.CLOSER)
    return run_in_turn(handles, "grad_update" if env.family.startswith("R") else "run", F.CLOSER)


def has_wait(*forms):
    return any(f in F.GRID_WAIT_FORMS for f in forms)


def count_waits(handles, *forms):
    WAITS["counted"] += 1
    if has_wait(*forms):
        WAITS["cells"] += 1
        WAITS["events"] += 1 if any(h.waited for h in handles) else 0


PLAIN_CELLS = [(family, cls, X, Y) for (family, cls) in F.SERVED if cls != "backtracking" for X, Y in F.pair_cells(family, cls)]
BT_CELLS = [(family, X, Y) for (family, cls) in F.SERVED if cls == "backtracking" for X, Y in F.pair_cells(family, cls)]


def test_families_are_planned_as_the_table_says(fos, env_of):
    for family in F.families(256):
        env = env_of(family)
        plan = env.prob["default"].plan()
        m, n = env.spec["m"], env.spec["n"]
        assert plan["resident"] == int(F.resident_fits(m, n)) and plan["tall"] == int(n <= F.TALL_MAX_N) and plan["path"] == 0, (family, plan)
        if env.spec["routed"]:
            routed = env.prob["routed"].plan()
            assert routed["fused_mfma"] == int(family == "S-f32") and routed["chip_resident"] == int(family == "T"), routed


@pytest.mark.parametrize("family,cls", sorted(F.SERVED))
def test_unserved_forms_refuse_and_leave_the_handle_alone(fos, env_of, family, cls):
    env = env_of(family)
    # (the families without a backtracking class have no candidate pass: the two device searches refuse there as well)
    searches = () if "backtracking" in env.spec["classes"] else ("run_backtracking", "run_recorded_bt")
    for form in F.unserved(family, cls) + searches:
        for prm in F.class_params(family, cls)[:1]:
            h = Handle(env, cls, prm, 0, plan_of(form))
            _pair(h, False)
            _pair(h, False)
            k, x = int(h.st.status().k), h.x()
            assert run_in_turn([h], form, 2) is False, (family, cls, form, "listed as not served, but ran")
            assert int(h.st.status().k) == k == 2 and np.array_equal(h.x(), x), (family, cls, form)
            _pair(h, False)                                   # ... and goes on as if the call had not been made
            check(h, 3, (form, "refused"))


@pytest.mark.parametrize("family,cls,X,Y", PLAIN_CELLS, ids=["/".join(c) for c in PLAIN_CELLS])
def test_pair_of_forms(fos, env_of, family, cls, X, Y):
    """Plain and controlled classes: X(nx), Y(ny), closer, for both count patterns and every parameter set of the class."""
    env = env_of(family)
    for nprm in range(len(F.class_params(family, cls))):
        for nx, ny in F.COUNTS:
            handles = [Handle(env, cls, F.class_params(family, cls, w)[nprm], w, plan_of(X, Y)) for w in (0, 1)]
            for form, iters in ((X, nx), (Y, ny)):
                assert run_in_turn(handles, form, iters) is True, (family, cls, form, "listed as served, but refused")
            # the second handle is also asked right after Y: a bookkeeping that closes ONE plain iteration (plain_count < 2,
            # the previous step taken from the device scalars) happens only here - the closer's iterations are otherwise
            # counted with Y's; the first handle goes on unasked, with whatever Y left pending
            check(handles[1], nx + ny, (X, nx, Y, ny, "right after Y"))
            assert closer(handles, X)
            for h in handles:
                check(h, nx + ny + F.CLOSER, (X, nx, Y, ny))
            count_waits(handles, X, Y)


INSPECTOR_CELLS = [(family, cls, X, I) for (family, cls), forms in sorted(F.SERVED.items()) if cls != "backtracking"
                   for X in forms for I in F.INSPECTORS]


def inspect(h, name):
    st = h.st
    if name == "status":
        return int(st.status().k)
    if name == "trial":
        st.trial(h.tau, with_residual=True)
    elif name == "trial_batch":
        st.trial_batch(h.tau, 0.5, 16)                       # (None on plans without the candidate pass: nothing ran)
    elif name == "x_tensor":
        st.x_tensor()
    elif name == "set_precise":
        st.set_precise(True, own_buffer=True)
        st.set_precise(False)
    elif name == "set_tau":
        st.set_tau(h.tau)
    return None


@pytest.mark.parametrize("family,cls,X,I", INSPECTOR_CELLS, ids=["/".join(c) for c in INSPECTOR_CELLS])
def test_inspectors_do_not_move_a_handle(fos, env_of, family, cls, X, I):
    """X(3), inspector, X(2) is the uninterrupted run; right after the inspector the iterate is unchanged bit for bit (first
    handle) and so is k (second handle: asking for k is itself an inspector, so the first handle goes on without)."""
    env = env_of(family)
    prm = [F.class_params(family, cls, w)[0] for w in (0, 1)]
    handles = [Handle(env, cls, prm[w], w, plan_of(X)) for w in (0, 1)]
    assert run_in_turn(handles, X, 3) is True
    before = [h.x() for h in handles]
    for h in handles:
        k = inspect(h, I)
        assert k in (None, 3)
    assert int(handles[1].st.status().k) == 3
    for h, x in zip(handles, before):
        assert np.array_equal(h.x(), x), (family, cls, X, I, "the inspector moved the iterate")
    assert run_in_turn(handles, X, 2) is True
    for h in handles:
        check(h, 5, (X, I))
    count_waits(handles, X)


STICKY_CELLS = [(family, X, Y) for (family, cls) in sorted(F.SERVED) if cls == "controlled" for X, Y in F.pair_cells(family, cls)]


@pytest.mark.parametrize("family,X,Y", STICKY_CELLS, ids=["/".join(c) for c in STICKY_CELLS])
def test_stopped_is_sticky(fos, env_of, family, X, Y):
    """The ratio rule stops the oracle after 2 of the 5 iterations asked of X: every form Y afterwards, and the closer after
    it, leaves k, the stop code and the iterate as they are, bit for bit (include/fos.h: iterations on a stopped handle are
    no-ops)."""
    env = env_of(family)
    prm = F.stop_params(family)
    handles = [Handle(env, "controlled", prm, w, plan_of(X, Y)) for w in (0, 1)]
    assert run_in_turn(handles, X, 5) is True
    snaps = []
    for h in handles:
        o = env.states("controlled", prm, h.w)[5]
        s = h.st.status()
        assert 0 < o["k"] < 5 and int(s.k) == o["k"] and int(s.stopped) == F.STOP_RATIO == o["stopped"], (family, X, int(s.k), o["k"], int(s.stopped))
        assert _data.rel(h.x(), o["x"]) < F.TOL
        snaps.append((int(s.k), h.x()))
    for form in (Y, "closer"):
        assert (closer(handles, X) if form == "closer" else run_in_turn(handles, form, 3)) is True
        for h, (k, x) in zip(handles, snaps):
            s = h.st.status()
            assert int(s.k) == k and int(s.stopped) == F.STOP_RATIO and np.array_equal(h.x(), x), (family, X, form, "a stopped handle moved")
    if "run_resident" in F.SERVED[(family, "controlled")]:
        for h in handles:
            assert h.st.run_resident(3)["done"] == 0          # *iters_done = 0 on a stopped handle
    count_waits(handles, X, Y)


STALL, STALL_WEIGHTS = F.STALL, F.STALL_WEIGHTS
STALL_FORMS = F.SERVED[("S-f32", "plain")] + ("run_backtracking", "run_recorded_bt")     # ... and a second device search
STALL_ERR_STATE = ("run_history", "run_multi4", "run_multi5", "run_multi_rhs", "run_multi_folds")
STALL_CELLS = [(Y, Z) for Y in STALL_FORMS for Z in STALL_FORMS]


@pytest.mark.parametrize("Y,Z", STALL_CELLS, ids=["/".join(c) for c in STALL_CELLS])
def test_a_stalled_search_is_sticky(fos, env_of, Y, Z):
    """A plain-class handle (no restart, no tolerance) whose device search parked itself: on S-f32 with a first step 4 / L and
    eta = 0.7 the oracle's seventh search needs 89 shrinks (the reference's step underflow), more than the 16 candidates of
    a batch, so fos_fista_run_backtracking stops with FOS_STOP_LS_STALL at k = 6.  Two forms in a row afterwards - the first
    may leave the mirror in a state that lets the second one move - leave k, the stop code and the iterate as they are; the
    forms with outputs or other handles to account for (run_history, the plain lockstep) answer FOS_ERR_STATE instead, as
    include/fos.h says."""
    from fastoptsolver_amd import _lib
    env = env_of("S-f32")
    h = Handle(env, "plain", STALL, 0, plan_of(Y, Z), STALL_WEIGHTS)
    assert h.st.run_backtracking(8, STALL["eta"], F.ARMIJO_C, F.GRAD_EPS) is not None
    s = h.st.status()
    assert int(s.stopped) == _lib.STOP_LS_STALL and int(s.k) == F.STALL_K, (int(s.stopped), int(s.k))
    x = h.x()
    for form in (Y, Z):
        if form in STALL_ERR_STATE:
            with pytest.raises(_lib.FosError, match="code -3"):
                run_in_turn([h], form, 2)
        else:
            assert run_in_turn([h], form, 2) is True
        s = h.st.status()
        assert int(s.k) == F.STALL_K and int(s.stopped) == _lib.STOP_LS_STALL and np.array_equal(h.x(), x), (Y, Z, form, "a stalled handle moved")
    count_waits([h], Y, Z)


def _check_searches(h, total, what):
    """Shrink counts as tests/test_gpu_parity.py::_check_linesearch_counts compares them - exactly: the window holds no
    step-underflow search (>= 40 shrinks) and no stagnating iteration, which tests/test_fista_forms.py checks on the oracle -
    and the accepted steps to 1e-12."""
    o = h.env.states(h.cls, h.prm, h.w, what.get("tau_switch"))
    ref_ls, ref_tau = [s["ls"] for s in o[1:total + 1]], [s["tau"] for s in o[1:total + 1]]
    assert max(ref_ls) < 40
    assert h.ls == ref_ls, (what, h.ls, ref_ls)
    assert np.allclose(h.taus, ref_tau, rtol=1e-12, atol=0.0), (what, h.taus, ref_tau)


@pytest.mark.parametrize("family,X,Y", BT_CELLS, ids=["/".join(c) for c in BT_CELLS])
def test_pair_of_backtracking_forms(fos, env_of, family, X, Y):
    """The three forms that search: the shrink count of every iteration and the step - after X, and the one Y's first
    iteration starts from (its accepted step and its count together) - equal the oracle's, so the step carries over the
    switch; then the same with fos_fista_set_tau between the forms: Y searches from the new value, not from the step held
    on the device."""
    env = env_of(family)
    for nprm in range(len(F.class_params(family, "backtracking"))):
        for nx, ny in F.COUNTS:
            for switch in (False, True):
                handles = [Handle(env, "backtracking", F.class_params(family, "backtracking", w)[nprm], w) for w in (0, 1)]
                assert run_in_turn(handles, X, nx) is True
                what = []
                for h in handles:
                    o = env.states("backtracking", h.prm, h.w)
                    assert close(h.tau, o[nx]["tau"], 1e-12), (family, X, nx, h.tau, o[nx]["tau"])
                    sw = (nx, 2.0 * o[nx]["tau"]) if switch else None
                    if switch:
                        h.st.set_tau(sw[1])
                        h.tau = sw[1]
                    what.append(dict(cell=(family, X, nx, Y, ny), tau_switch=sw))
                assert run_in_turn(handles, Y, ny) is True
                assert closer(handles, X)
                total = nx + ny + F.CLOSER
                for h, wh in zip(handles, what):
                    _check_searches(h, total, wh)
                    o = env.states("backtracking", h.prm, h.w, wh["tau_switch"])[total]
                    s = h.st.status()
                    assert int(s.k) == total and int(s.stopped) == 0 and _data.rel(h.x(), o["x"]) < F.TOL, (wh, int(s.k), _data.rel(h.x(), o["x"]))
                    assert close(s.this_step, o["this"], 1e-4) and close(s.t_prev, o["t"], 1e-14) and close(s.beta, o["beta"], 1e-14), wh


BT_INSPECTOR_CELLS = [(family, X, I) for (family, cls), forms in sorted(F.SERVED.items()) if cls == "backtracking"
                      for X in forms for I in F.INSPECTORS]


@pytest.mark.parametrize("family,X,I", BT_INSPECTOR_CELLS, ids=["/".join(c) for c in BT_INSPECTOR_CELLS])
def test_inspectors_do_not_move_a_searching_handle(fos, env_of, family, X, I):
    """X(3), inspector, X(2) for the three forms that search: the shrink counts and steps of all five iterations are the
    oracle's, so neither set_tau(the step the caller holds) - which hands the step back to the host - nor trial / trial_batch
    - which overwrite the partials and the candidate block a device search uses - nor status(), through which the step is
    read, disturbs the search; right after the inspector the iterate (first handle) and k (second handle) are unchanged."""
    env = env_of(family)
    for nprm in range(len(F.class_params(family, "backtracking"))):
        handles = [Handle(env, "backtracking", F.class_params(family, "backtracking", w)[nprm], w) for w in (0, 1)]
        assert run_in_turn(handles, X, 3) is True
        before = [h.x() for h in handles]
        for h in handles:
            assert inspect(h, I) in (None, 3)
        assert int(handles[1].st.status().k) == 3
        for h, x in zip(handles, before):
            assert np.array_equal(h.x(), x), (family, X, I, "the inspector moved the iterate")
        assert run_in_turn(handles, X, 2) is True
        for h in handles:
            _check_searches(h, 5, dict(cell=(family, X, I)))
            o = env.states("backtracking", h.prm, h.w)[5]
            s = h.st.status()
            assert int(s.k) == 5 and int(s.stopped) == 0 and _data.rel(h.x(), o["x"]) < F.TOL, (family, X, I, int(s.k))
            assert close(s.this_step, o["this"], 1e-4) and close(s.t_prev, o["t"], 1e-14) and close(s.beta, o["beta"], 1e-14)
    count_waits(handles, X)


@pytest.mark.parametrize("again", ["run_backtracking", "run_recorded_bt"])
def test_a_parked_search_is_resumed_on_the_host_and_handed_back(fos, env_of, again):
    """The transition iterative_solvers runs when a device search parks itself: device search -> FOS_STOP_LS_STALL ->
    fos_fista_resume_after_stall -> the host finishes that search (trial_batch, set_tau, update) -> device search again,
    against the oracle across its step-underflow iteration.  The step handed over is the one the iteration started from
    times eta^16 (the batch the device rejected); the search ends after about as many shrinks as the oracle's
    (_check_linesearch_counts: a >= r - 10 from 40 shrinks on - decided by float64 rounding on both sides); the step is then
    too short to move y, on both sides, so iterations 7 and 8 are y_6 and y_7 of the oracle."""
    from fastoptsolver_amd import _lib
    env = env_of("S-f32")
    h = Handle(env, "plain", STALL, 0, "default", STALL_WEIGHTS)
    f1, a2 = STALL_WEIGHTS
    key = ("stall",)
    if key not in env.oracle:
        env.oracle[key] = F.oracle_states(env.A, env.b, env.L, STALL, f1 * env.lam, a2, F.WINDOW, backtracking=True)
    o = env.oracle[key]
    assert _device_search(h, F.WINDOW, False) is True
    s = h.st.status()
    assert int(s.stopped) == _lib.STOP_LS_STALL and int(s.k) == F.STALL_K
    assert h.ls[:F.STALL_K] == [st["ls"] for st in o[1:F.STALL_K + 1]]
    del h.ls[F.STALL_K:], h.taus[F.STALL_K:]
    tau = h.st.resume_after_stall()
    assert close(tau, o[F.STALL_K]["tau"] * STALL["eta"] ** F.BATCH, 1e-12), (tau, o[F.STALL_K]["tau"])
    s = h.st.status()
    assert int(s.stopped) == 0 and int(s.k) == F.STALL_K and close(s.tau, tau, 0.0)
    h.tau = tau
    _search_on_host(h)
    shrinks, ref = F.BATCH + h.ls[-1], o[F.STALL_K + 1]["ls"]
    assert ref >= 40 and shrinks >= ref - 10, (shrinks, ref)
    s = h.st.status()
    assert int(s.k) == F.STALL_K + 1 and int(s.stopped) == 0
    assert _data.rel(h.x(), o[F.STALL_K + 1]["x"]) < F.TOL
    assert run_in_turn([h], again, 1) is True                 # the host's step goes back to the device (set_tau)
    s = h.st.status()
    assert int(s.k) == F.STALL_K + 2 and int(s.stopped) == 0 and s.tau <= h.taus[F.STALL_K], (int(s.k), int(s.stopped), s.tau)
    assert _data.rel(h.x(), o[F.STALL_K + 2]["x"]) < F.TOL
    assert close(s.t_prev, o[F.STALL_K + 2]["t"], 1e-14) and close(s.beta, o[F.STALL_K + 2]["beta"], 1e-14)


def expected_reports():
    """(cells that report to count_waits, those among them with a grid-wide wait) when the whole file runs."""
    cells = [(X, Y) for family, cls, X, Y in PLAIN_CELLS for _prm in F.class_params(family, cls) for _counts in F.COUNTS]
    cells += [(X,) for _, _, X, _ in INSPECTOR_CELLS] + [(X, Y) for _, X, Y in STICKY_CELLS] + list(STALL_CELLS)
    cells += [(X,) for _, X, _ in BT_INSPECTOR_CELLS]
    return len(cells), sum(has_wait(*c) for c in cells)


def test_grid_wide_waits_were_rare():
    """Counted by the cells above (this test runs after them): a bounded grid-wide wait ran out in at most one in ten of the
    cells that contain such a form.  Expected: none.  When the whole file ran, the cells counted are the table's."""
    print(f"cells with a grid-wide wait: {WAITS['cells']}, waits that ran out: {WAITS['events']}")
    assert WAITS["events"] * 10 <= WAITS["cells"], WAITS
    reports, waits = expected_reports()
    assert waits > 0
    if WAITS["counted"] == reports:
        assert WAITS["cells"] == waits, (WAITS, waits)
