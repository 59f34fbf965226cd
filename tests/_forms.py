"""Table of the FISTA run forms of one fos_fista handle (a helper: no tests in here), beside the tests/_menu*.py tables.

A handle can be advanced by about a dozen entry points, and between calls it carries a host mirror of the device scalars
(struct fos_fista, csrc/fos_internal.hpp: host_valid, pending, plain_count, y_valid, tau_on_device, h_t, h_beta, h_k).  A
wrong flag does not crash: it yields ONE wrong iteration in the call after.  This table names every FORM (a way to advance
a handle through fastoptsolver_amd._core), every INSPECTOR (must not move the iterate, but touches the mirror), the
FAMILIES (smallest shapes on which the forms run) with their parameter CLASSES, and which forms each (family, class)
serves - stated here, not worked out at run time.  tests/test_fista_forms.py keeps the table in step with include/fos.h and
csrc/fos_fista.hip and checks on the CPU that a wrong transition moves the answer by far more than the tolerance;
tests/test_gpu_fista_forms.py runs every ordered pair of served forms on one handle against the fp64 oracle.

form               entry points (fos_fista_*)                        notes
reset              reset                                             the start of every cell
run                run                                               the family's default plan
run_routed         run                                               on the family's ROUTED problem: replan(fused_mfma=True) on
                                                                     S-f32 (run -> run_fused), replan(chip_resident=True) on T
                                                                     (run -> run_chip); a cell with this form runs all its
                                                                     calls, closer included, on the routed problem
grad_update        grad, update                                      one pair per iteration
graddual_update    grad_dual, update
run_history        run_history
run_recorded       run_recorded(backtracking=False)
run_fused          run_fused
run_chip           run_chip
run_resident       run_resident
run_resident_rec   run_resident(record=True)
run_multi4         run_multi, 4 handles                              fp32 streaming plain: the multi-vector VALU pass
run_multi5         run_multi, 5 handles                              the two matrix-core products
run_multi_rhs      run_multi_rhs, 3 handles, B = b repeated
run_multi_folds    run_multi_folds, 2 handles, held = -1
run_backtracking   run_backtracking                                  backtracking class only
run_recorded_bt    run_recorded(backtracking=True)
host_search        grad, trial_batch, set_tau, update                the search iterative_solvers._Driver.search_on_host runs;
                   resume_after_stall                                the families with a backtracking class all serve
                                                                     trial_batch, so its one-candidate fallback (trial) runs
                                                                     as an inspector only; resume_after_stall: the cell
                                                                     parked search -> resume -> host_search -> device search
"""
import math

import numpy as np

from oracle import fos_oracle as orc

TOL = 1e-5                       # the project's parity tolerance (tests/test_gpu_parity.py)
WINDOW = 8                       # iterations of a pair cell: nx + ny + the closer's 2 at most
COUNTS = ((3, 1), (2, 3))        # (nx, ny): Y starts on both parities of the part2 slot; asked right after Y, it closes with
                                 # plain_count < 2 and >= 2 (finish_part2's two branches)
CLOSER = 2
ETA_DEFAULT, ARMIJO_C = 0.5, orc.ARMIJO_C
GRAD_EPS = 8.0 * float(np.finfo(np.float32).eps)     # resolution of the fp32 gradient pass (iterative_solvers._armijo_accepts)

# form -> exported entry points it goes through
FORMS = {
    "reset": ("fos_fista_reset",),
    "run": ("fos_fista_run",),
    "run_routed": ("fos_fista_run",),
    "grad_update": ("fos_fista_grad", "fos_fista_update"),
    "graddual_update": ("fos_fista_grad_dual", "fos_fista_update"),
    "run_history": ("fos_fista_run_history",),
    "run_recorded": ("fos_fista_run_recorded",),
    "run_fused": ("fos_fista_run_fused",),
    "run_chip": ("fos_fista_run_chip",),
    "run_resident": ("fos_fista_run_resident",),
    "run_resident_rec": ("fos_fista_run_resident",),
    "run_multi4": ("fos_fista_run_multi",),
    "run_multi5": ("fos_fista_run_multi",),
    "run_multi_rhs": ("fos_fista_run_multi_rhs",),
    "run_multi_folds": ("fos_fista_run_multi_folds",),
    "run_backtracking": ("fos_fista_run_backtracking",),
    "run_recorded_bt": ("fos_fista_run_recorded",),
    "host_search": ("fos_fista_grad", "fos_fista_trial_batch", "fos_fista_set_tau", "fos_fista_update", "fos_fista_resume_after_stall"),
}
# inspector -> exported entry points
INSPECTORS = {
    "status": ("fos_fista_status_get",),
    "trial": ("fos_fista_trial",),
    "trial_batch": ("fos_fista_trial_batch",),
    "x_tensor": ("fos_fista_get_x",),
    "set_precise": ("fos_fista_set_precise", "fos_fista_set_gbuf64"),      # on with a buffer of the caller's, then off
    "set_tau": ("fos_fista_set_tau",),                                       # the same tau
}
# cannot change what a handle does between two iterations
PASSIVE = ("fos_fista_create", "fos_fista_destroy", "fos_fista_x", "fos_fista_gbuf", "fos_fista_history_workspace")
# takes no handle (its first parameter is a matrix): not part of the state machine
NOT_A_HANDLE = ("fos_fista_batch_workspace", "fos_fista_run_batch")

# the helpers that may assign the mirror (the comment of struct fos_fista names them as "begin_plain ... hand_to_device")
MIRROR_FIELDS = ("host_valid", "pending", "plain_count", "y_valid", "tau_on_device", "h_t", "h_beta", "h_k")
MIRROR_WRITERS = ("fos_fista_reset", "fos_fista_set_tau", "finish_plain", "begin_plain", "advance_plain", "momentum_sequence",
                  "restore_momentum", "ensure_y", "restart_plain", "hand_to_device", "run_device_driven")

BT_FORMS = ("run_backtracking", "run_recorded_bt", "host_search")
PLAIN_UNIVERSE = tuple(f for f in FORMS if f not in BT_FORMS and f != "reset")
GRID_WAIT_FORMS = ("run_fused", "run_chip", "run_routed")   # forms with a time-bounded grid-wide wait

# ---- parameter classes: reset() fixes them for the life of a handle ---------------------------------------------------
# plain: the momentum sequence does not depend on the data (host mirror valid); controlled: decided on the device
PLAIN = (dict(name="fista", mode="fista", prox="l1"),
         dict(name="delta", mode="delta", prox="l1", delta=3.0),
         dict(name="ista_enet", mode="ista", prox="enet"))
# restart_threshold per (family, weight) / tol_ratio: the oracle restarts inside the window - besides the restart every run
# takes after its first iteration, whose ratio is infinite (reference :205-213) - and never stops in it
# (tests/test_fista_forms.py checks both on the oracle); stop_ratio: a tol_ratio with which the oracle stops inside X's request
CONTROLLED = {
    "S-f32": dict(restart_threshold=(0.9, 0.9), tol_ratio=1e-3, stop_ratio=0.7),
    "S-bf16": dict(restart_threshold=(0.9, 0.9), tol_ratio=1e-3, stop_ratio=0.7),
    "T": dict(restart_threshold=(1.02, 1.02), tol_ratio=1e-3, stop_ratio=0.7),
    "R-lds": dict(restart_threshold=(0.85, 0.85), tol_ratio=1e-3, stop_ratio=0.7),
    "R-reg": dict(restart_threshold=(0.75, 0.75), tol_ratio=1e-3, stop_ratio=0.7),
}
# a first step 8 times too long and a gentle shrink factor: genuine shrinks at the start and again later in the window, none
# of the reference's step-underflow searches (tests/test_gpu_parity.py::_check_linesearch_counts) inside it
BACKTRACKING = dict(t_init_factor=8.0, eta=0.8)

# a plain-class handle whose device search parks itself (FOS_STOP_LS_STALL): on S-f32 with these parameters and weights the
# oracle's search of iteration STALL_K needs more shrinks than a batch has candidates (the reference's step underflow)
STALL = dict(name="stall", mode="fista", prox="l1", t_init_factor=4.0, eta=0.7)
STALL_WEIGHTS, STALL_K, BATCH = (0.10, 0.5), 6, 16

# weights of the two handles of a cell: (alpha1 as a fraction of max|A^T b|, alpha2), chosen with the data below so that a wrong
# transition moves the answer by 100 x TOL (test_a_wrong_transition_moves_the_answer); SIBLING_WEIGHTS: the other handles of a
# lockstep call
WEIGHTS = {"S-f32": ((0.02, 0.2), (0.01, 0.1)), "S-bf16": ((0.02, 0.2), (0.01, 0.1)), "T": ((0.05, 0.2), (0.02, 0.2)),
           "R-lds": ((0.01, 0.1), (0.003, 0.1)), "R-reg": ((0.02, 0.2), (0.005, 0.1))}
# the backtracking class: heavier weights, with which the searches shrink again late in the window
BT_WEIGHTS = ((0.10, 0.5), (0.04, 0.2))
SIBLING_WEIGHTS = ((0.2, 0.3), (0.14, 0.3), (0.07, 0.3), (0.03, 0.3))
# data: S - tests/_data.synth; T and R-reg - m >> n makes A^T A nearly a multiple of the identity and every solver converge in
# one step, so their columns share a common factor (rho) and are graded in scale (1 ... g): momentum then matters
SEED = {"S-f32": 11, "S-bf16": 11, "T": 13, "R-reg": 17}
GRADED = {"T": dict(rho=1.0, g=0.5), "R-reg": dict(rho=0.0, g=0.5)}


def families(cus):
    """name -> shape, storage, the replan flags of the routed problem (None: none) and the classes it runs."""
    return {
        # streaming fp32, the smallest shape fos_fista_run_fused serves, a partial last 4-row panel
        "S-f32": dict(m=8 * cus + 3, n=2048, dtype="f32", routed=dict(fused_mfma=True), classes=("plain", "controlled", "backtracking")),
        # the same stored as bf16: the YOUT_XQ forms of y_next, the bf16 candidate kernel
        "S-bf16": dict(m=8 * cus + 3, n=2048, dtype="bf16", routed=None, classes=("plain", "controlled", "backtracking")),
        # tall, not resident, inside fos_fista_run_chip's limits
        "T": dict(m=4608, n=8, dtype="f32", routed=dict(chip_resident=True), classes=("plain", "controlled")),
        # LDS-resident: the `tiny` golden, and the register-resident class
        "R-lds": dict(m=64, n=16, dtype="f32", routed=None, classes=("plain", "controlled")),
        "R-reg": dict(m=1000, n=5, dtype="f32", routed=None, classes=("plain", "controlled")),
    }


_S_PLAIN = ("run", "grad_update", "graddual_update", "run_history", "run_recorded", "run_multi4", "run_multi5",
            "run_multi_rhs", "run_multi_folds")
_S_CTRL = ("run", "grad_update", "graddual_update", "run_recorded", "run_multi4", "run_multi5", "run_multi_rhs", "run_multi_folds")
# (family, class) -> the forms it serves; every other form of the class's universe must refuse and leave the handle alone
SERVED = {
    ("S-f32", "plain"): _S_PLAIN + ("run_fused", "run_routed"),
    ("S-f32", "controlled"): _S_CTRL,
    ("S-f32", "backtracking"): BT_FORMS,
    # (the bf16 geometry of 2048 columns has no DUAL instantiation: run_history refuses, callers record through the split form)
    ("S-bf16", "plain"): tuple(f for f in _S_PLAIN if f != "run_history"),
    ("S-bf16", "controlled"): _S_CTRL,
    ("S-bf16", "backtracking"): BT_FORMS,
    # n <= 64: no matrix-core pair, no multi-vector kernel, no candidate pass
    ("T", "plain"): ("run", "grad_update", "graddual_update", "run_history", "run_recorded", "run_chip", "run_routed"),
    ("T", "controlled"): ("run", "grad_update", "graddual_update", "run_recorded", "run_chip", "run_routed"),
    ("R-lds", "plain"): ("run", "grad_update", "graddual_update", "run_history", "run_resident", "run_resident_rec"),
    ("R-lds", "controlled"): ("run", "grad_update", "graddual_update", "run_resident", "run_resident_rec"),
    # 1000 rows are also inside the chip loop's limits (from 512 rows on)
    ("R-reg", "plain"): ("run", "grad_update", "graddual_update", "run_history", "run_resident", "run_resident_rec", "run_chip"),
    ("R-reg", "controlled"): ("run", "grad_update", "graddual_update", "run_resident", "run_resident_rec", "run_chip"),
}


def weights(family, cls):
    return BT_WEIGHTS if cls == "backtracking" else WEIGHTS[family]


def universe(family, cls):
    """The forms that make sense for (family, class): the class's forms, the routed one only where the routed plan changes
    what run does (elsewhere it is the row `run`)."""
    if cls == "backtracking":
        return BT_FORMS
    return tuple(f for f in PLAIN_UNIVERSE if f != "run_routed" or f in SERVED[(family, cls)])


def unserved(family, cls):
    return tuple(f for f in universe(family, cls) if f not in SERVED[(family, cls)])


def class_params(family, cls, w=0):
    """The parameter sets of a class on a family, for the handle with weights WEIGHTS[family][w]."""
    if cls == "plain":
        return PLAIN
    if cls == "controlled":
        c = CONTROLLED[family]
        return (dict(name="restart", mode="fista", prox="l1", adaptive_restart=True, restart_threshold=c["restart_threshold"][w],
                     tol_ratio=c["tol_ratio"]),)
    return (dict(name="bt_fista", mode="fista", prox="l1", **BACKTRACKING), dict(name="bt_delta", mode="delta", prox="l1", delta=3.0, **BACKTRACKING))


def stop_params(family):
    """Controlled handle whose oracle stops on the ratio rule strictly inside a request of 5 iterations."""
    return dict(name="ratio_stop", mode="fista", prox="l1", tol_ratio=CONTROLLED[family]["stop_ratio"])


def pair_cells(family, cls):
    return [(X, Y) for X in SERVED[(family, cls)] for Y in SERVED[(family, cls)]]


def count_cells():
    """Cells per family: pairs x parameter sets x count patterns, inspector cells, sticky cells."""
    out = {}
    for (family, cls), forms in SERVED.items():
        n = len(forms) ** 2 * len(class_params(family, cls)) * len(COUNTS)
        if cls == "backtracking":
            n *= 2                        # ... and again with set_tau between the forms
            n += len(forms) * len(INSPECTORS) * len(class_params(family, cls))
        else:
            n += len(forms) * len(INSPECTORS)
        if cls == "controlled":
            n += len(forms) ** 2          # sticky: X stops, Y must not move
        if (family, cls) == ("S-f32", "plain"):
            n += (len(forms) + 2) ** 2    # sticky after a parked search: two forms in a row, the two device searches included
            n += 2                        # parked search -> resume -> host search -> either device search
        out[family] = out.get(family, 0) + n
    return out


# ---- planner constants restated (tests/test_fista_forms.py reads them from the source) ---------------------------------
RS_MAX_N, RS_MAX_M, RS_MAX_A, RS_CHUNK, RS_SMALL_M = 64, 4096, 10240, 8, 2048
CR_LDS_BUDGET = 150 * 1024
TALL_MAX_N = 64
FUSED_COLS, FUSED_MAX_N, FUSED_ROWS_PER_CU, FZ_OWN_MAX, FZ_ROWS = 2048, 8192, 8, 64, 4


def resident_fits(m, n):
    return 1 <= n <= RS_MAX_N and 1 <= m <= RS_MAX_M and m * (n | 1) <= RS_MAX_A


def register_resident(m, n):
    return resident_fits(m, n) and n <= RS_CHUNK and m <= RS_SMALL_M


def chip_serves(m, n, cus, dtype="f32"):
    nc = 8 if n <= 8 else 16
    cap = (CR_LDS_BUDGET - 1024) // ((nc + 4) * 4 + 4)
    return dtype == "f32" and n <= 16 and 512 <= m <= cap * cus


def chip_region(m, n, iters, dtype="f32"):
    """Where plain fos_fista_run takes the chip loop by itself (planner's region)."""
    return dtype == "f32" and m >= 512 and iters >= 8 and (m <= 131072 if n <= 8 else (n <= 16 and m <= 32768))


def fused_serves(m, n, cus, dtype="f32"):
    return (dtype == "f32" and n > TALL_MAX_N and not resident_fits(m, n) and n % FUSED_COLS == 0 and n <= FUSED_MAX_N and
            m >= FUSED_ROWS_PER_CU * cus and (n + cus - 1) // cus <= FZ_OWN_MAX)


# ---- data -----------------------------------------------------------------------------------------------------------
def make_data(family, cus, rounder=None):
    """(A, b, L, lam) in fp64 with A and b already rounded to what the device stores.  rounder(A) -> A as stored (bf16
    families: the GPU test passes torch's rounding; None: fp32).  L: a bound of ||A||_2^2 from 30 power iterations, times 1.1."""
    spec = families(cus)[family]
    if family == "R-lds":
        from tests import _data
        A, b, _ = _data.problem("tiny")
    elif family in GRADED:
        rng = np.random.default_rng(SEED[family])
        Z, z0 = rng.standard_normal((spec["m"], spec["n"])), rng.standard_normal(spec["m"])
        A = (Z + GRADED[family]["rho"] * z0[:, None]) * np.geomspace(1.0, GRADED[family]["g"], spec["n"])
        b = A @ rng.standard_normal(spec["n"]) + 0.5 * rng.standard_normal(spec["m"])
    else:
        from tests import _data
        A, b, _ = _data.synth(spec["m"], spec["n"], SEED[family])
    A = np.asarray(A, dtype=np.float32)
    A = (rounder(A) if rounder is not None else A).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    v = np.ones(A.shape[1]) / math.sqrt(A.shape[1])
    for _ in range(30):
        v = A.T @ (A @ v)
        v /= np.linalg.norm(v)
    L = 1.1 * float(np.linalg.norm(A @ v) ** 2)          # (a lower bound of ||A||_2^2 within a few per cent, times 1.1)
    lam = float(np.max(np.abs(A.T @ b)))
    return A, b, L, lam


def bf16_round_np(A):
    """Round-to-nearest-even of fp32 to bf16, in NumPy (the CPU tests' stand-in for torch's cast)."""
    u = np.asarray(A, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def tau_of(prm, L, a2):
    """The reference's step: 1 / (L + alpha2) where alpha2 is part of the smooth term (l1 prox), times t_init_factor."""
    Ls = L + (a2 if prm["prox"] == "l1" and a2 > 0 else 0.0)
    return prm.get("t_init_factor", 1.0) / Ls


# ---- the oracle, iteration by iteration -----------------------------------------------------------------------------
STOP_NONE, STOP_RATIO = 0, 2


def oracle_states(A, b, L, prm, a1, a2, iters, backtracking=False, tau_switch=None):
    """states[k], k = 0..iters, of oracle/fos_oracle.py's own loops: dict(x, k, t, beta, this, prev, x1, x2, restarts, stopped,
    tau, ls) after k iterations (a stopped run repeats its last state).  tau_switch = (k, tau): the step is set to tau before
    iteration k (fos_fista_set_tau between two forms)."""
    n = A.shape[1]
    out = []

    def rec(x, k, t, beta, this, prev, restarts, stopped, tau, ls):
        out.append(dict(x=x.copy(), k=k, t=t, beta=beta, this=this, prev=prev, x1=float(np.abs(x).sum()), x2=float(x @ x),
                        restarts=restarts, stopped=stopped, tau=tau, ls=ls))

    if prm["mode"] == "ista":
        assert not backtracking and prm["prox"] == "enet"
        tau = tau_of(prm, L, a2)
        _, log = orc.ista(np.zeros(n), lambda z: 0.5 * float(np.sum((A @ z - b) ** 2)), lambda z: A.T @ (A @ z - b),
                          lambda v, t: orc.prox_elastic_net(v, t, a1, a2), L, max_iter=iters, return_history=True)
        rec(log["x"][0], 0, 1.0, 0.0, 0.0, 0.0, 0, STOP_NONE, tau, None)
        for k in range(1, iters + 1):
            rec(log["x"][k], k, 1.0, 0.0, log["delta"][k - 1], log["delta"][k - 2] if k >= 2 else 0.0, 0, STOP_NONE, tau, None)
        return out
    prob = orc.FistaProblem(A, b, a1, a2)
    st = prob.init_state(L, prm.get("t_init_factor", 1.0))
    eta = prm.get("eta", ETA_DEFAULT)
    restarts, beta = 0, 0.0
    rec(st.x, 0, 1.0, 0.0, 0.0, 0.0, 0, STOP_NONE, st.tau, None)
    for k in range(iters):
        if st.stopped:
            out.append(dict(out[-1]))
            continue
        if tau_switch is not None and tau_switch[0] == k:
            st.tau = tau_switch[1]
        t_old = st.t
        if prm["mode"] == "delta":
            info = prob.step_delta(st, prm["delta"], backtracking=backtracking, eta=eta, tol_ratio=prm.get("tol_ratio", 0.0))
            beta = st.k / (st.k + 1.0 + prm["delta"])
        else:
            info = prob.step(st, backtracking=backtracking, eta=eta, tol_ratio=prm.get("tol_ratio", 0.0),
                             adaptive_restart=prm.get("adaptive_restart", False), restart_threshold=prm.get("restart_threshold", 1.0))
            if prm.get("adaptive_restart", False) and info["ratio"] > prm.get("restart_threshold", 1.0):
                restarts += 1
                beta = 0.0
            else:
                beta = (t_old - 1.0) / st.t
        rec(st.x, st.k, st.t, beta, info["move"], out[-1]["this"], restarts, STOP_RATIO if st.stopped else STOP_NONE, st.tau,
            prob.metrics.ls_iters[-1] if backtracking else None)
    return out


# ---- sensitivity: a 20-line FISTA / FISTA-delta / ISTA that takes a fault at one iteration ------------------------------
FAULTS = {"momentum_restarted": ("fista",), "beta_lags": ("fista", "delta"), "y_from_x_km2": ("fista", "delta"),
          "k_off_by_one": ("delta",), "tau_reverts": ("bt",)}


def faulty_run(A, b, L, prm, a1, a2, iters, fault=None, at=None, backtracking=False, shrinks=None):
    """x after `iters` iterations; `fault` strikes at iteration `at` (0-based: the first iteration of the next call).
    shrinks: a list that takes the shrink count of every search."""
    n = A.shape[1]
    enet = prm["prox"] == "enet"
    a2s = 0.0 if enet else a2
    tau = tau0 = tau_of(prm, L, a2)
    eta = prm.get("eta", ETA_DEFAULT)
    x, x_old, x_older = np.zeros(n), np.zeros(n), np.zeros(n)
    t, beta, beta_before = 1.0, 0.0, 0.0

    def smooth(z):
        r = A @ z - b
        return 0.5 * float(r @ r) + 0.5 * a2s * float(z @ z)

    for k in range(iters):
        hit = fault is not None and k == at
        if hit and fault == "momentum_restarted":
            t, beta = 1.0, 0.0
        bk = beta_before if hit and fault == "beta_lags" else beta
        y = x + bk * ((x_old - x_older) if hit and fault == "y_from_x_km2" else (x - x_old))
        if hit and fault == "tau_reverts":
            tau = tau0
        g = A.T @ (A @ y - b) + a2s * y
        count = 0
        while True:
            v = y - tau * g
            cand = np.sign(v) * np.maximum(np.abs(v) - tau * a1, 0.0) if a1 > 0 else v
            if enet:
                cand = cand / (1.0 + tau * a2)
            if not backtracking or smooth(cand) <= smooth(y) + ARMIJO_C * float(g @ (cand - y)):
                break
            tau *= eta
            count += 1
        if shrinks is not None:
            shrinks.append(count)
        x_older, x_old, x = x_old, x, cand
        beta_before = beta
        if prm["mode"] == "fista":
            ratio = np.linalg.norm(x - x_old) / np.linalg.norm(x_old - x_older) if np.any(x_old != x_older) else math.inf
            if prm.get("adaptive_restart", False) and ratio > prm.get("restart_threshold", 1.0):
                t, beta = 1.0, 0.0
            else:
                t_new = 0.5 * (1.0 + math.sqrt(1.0 + 4.0 * t * t))
                t, beta = t_new, (t - 1.0) / t_new
        elif prm["mode"] == "delta":
            kk = k + 1 + (1 if hit and fault == "k_off_by_one" else 0)
            beta = kk / (kk + 1.0 + prm["delta"])
    return x


def faults_of(prm, cls):
    kind = prm["mode"]
    out = [f for f, kinds in FAULTS.items() if kind in kinds]
    if cls == "backtracking":
        out.append("tau_reverts")
    return out


def switch_iterations():
    """The iterations at which a cell switches forms: after nx and after nx + ny."""
    return sorted({s for nx, ny in COUNTS for s in (nx, nx + ny)})
