"""Cells, moves and fp64 references of the tests that run every ordered pair of lockstep configurations on ONE problem handle
(a helper: no tests in here).  tests/test_handle_pairs.py checks the table on the CPU, tests/test_gpu_handle_pairs.py runs it.

fos_problem_set_loss, fos_problem_set_link_loss, fos_problem_set_multinomial, fos_row_weights_bind and fos_coord_bind end with
"no buffer depends on ...: nothing to invalidate"; fos_feature_groups_bind and fos_problem_replan re-bind or drop buffers beside
the bindings that stay.  All of them act on one handle whose workspace every lockstep call shares (cand.xp / q_part / bt_out,
multi.rbuf16 / slabs16, ws.b16 / link_part / grad_part, fg.u / nrm2, the borrowed b, row_weight and coord_* pointers, loss,
link_param and classes).  A CELL is a configuration of the handle plus one call on it; move(X, Y) is the shortest sequence of
binding calls a caller would make to get from X's configuration to Y's, ordered so that the library's refusal rules allow every
step.  The GPU file compares what a cell returns after any other cell, and after a replan, bit for bit with what it returns on a
fresh handle, whose own result is checked against the family's fp64 reference here.

One data set per (shape, storage type), shared by every cell: one seeded Gaussian design (tests/_data.synth) and one target per
loss - b with a tenth of gross outliers (tests/_link.huber_recipe) for the squared and Huber cells, labels of the planted model
in {0, 1} (tests/_logit.labels) and in {-1, +1} (tests/_link.hinge_recipe), class indices for C = 3 and C = 7
(tests/_multinomial.labels) - "counts" row weights (tests/_weighted.weights), penalty factors with exact zeros
(tests/_coord.factors) under the lower bound 0 - and the same factors with FREE_FACTOR in place of the zeros and no bound, the
configuration with factors that the duality-gap certificate serves -, and the "weights" group layout (tests/_fgroup.layout: seeded sizes 1..7, every
sixth group of weight 0).  The handle BORROWS b (fos.h: "the caller's: never freed here"), so a cell of another loss overwrites the
bound device vector in place; anything that cached a function of b would show.

The resampled calls (include/fos_resample.h) bind nothing - the multiplicities travel with the call - and share all of the above:
their cells sit on the existing configurations with the counts of tests/_resample.counts at the shape's rows (bootstrap with the
planted 15 and 0, or 0/1), the weighted references with the weights w * c_j and L per resample from the oracle's power iteration
on w * c_j.  The working set and the duality gap of the multinomial lockstep (include/fos_multinomial_ws.h) have two cells on the
multinomial configurations, against tests/_multinomial_ws.py.

Every run takes ITERS = 12 iterations with L of the reference passed to both sides: lambda_max(A^T A) from the oracle's power
iteration (of A^T W A with row weights), a quarter of it for the logistic and half for the multinomial loss.

Shapes, for the CU count the planner reports: "padded" 1003 x 37 (the device copy has 68 fp32 / 72 bf16 columns: the extra
zero group, the padded factor vectors, rows % 4 != 0) and tests/_menu_cv's "panels" (two row panels, the second short:
ws.link_part / ws.grad_part and the fold ids offset with the panel)."""
import collections
import functools
import glob
import os
import re

import numpy as np

from oracle import fos_oracle as orc
from tests import (_coord as cd, _data, _duality as du, _fgroup as fg, _forms, _group as gp, _link as lk, _logit as lg, _menu_cv as mcv,
                   _menu_multi as mm, _multinomial as mn, _multinomial_ws as mws, _power as pw, _resample as rsp, _weighted as wt,
                   _working_set as ws)
from tests._menu_product1 import CSRC, FISTA, PLAN, _body, _text

ITERS = 12
TOL = lg.TOL                              # the project's standing 1e-5 of the lockstep against the fp64 oracle
KINDS = ("f32", "bf16")
SHAPES = ("padded", "panels")
PADDED = (1003, 37)
WEIGHT_MAX = 3.0                          # tests/_weighted.weights("counts"): integers 0..3
MU = 0.5                                  # l1_ratio of the feature-group cells
# The planted model has 11 of 37 coefficients (tests/_data.synth's default leaves 2: nothing for a working set to grow into), and
# the seed is the one of 1 .. 8 at which every precondition of tests/test_handle_pairs.py holds for both storage types - the
# working set of both losses grows and ends certified, the controlled ladder has an early stop, a full run and a genuine restart:
# found on the references alone.
SEED = 6
DENSITY = 0.3
INCLUDE = os.path.join(os.path.dirname(CSRC), os.pardir, "include")


def shape(name, kind, cus=mm.GPU_CUS):
    if name == "padded":
        return PADDED
    c = mcv.shapes(kind, cus)["panels"]
    return c["m"], c["n"]


# ---- configurations ------------------------------------------------------------------------------------------------------------
# coord: "" (nothing bound), "bounds" (penalty factors with exact zeros under the lower bound 0) or "factors" (strictly positive
# penalty factors and no bound: what the certificate serves)
Config = collections.namedtuple("Config", "loss classes grouped weights coord groups", defaults=("squared", 0, False, False, "", False))
PLAIN = Config()
FREE_FACTOR = 0.5                         # what the exact zeros of the penalty factors become under "factors"
TARGET = {"squared": "b", "huber": "b", "logistic": "y01", "squared_hinge": "ysign"}
LOSS_IDS = {"squared": 0, "logistic": 1, "multinomial": 2, "huber": 3, "squared_hinge": 4}     # include/fos.h, fos_link_loss.h
SETTER = {"squared": "fos_problem_set_loss", "logistic": "fos_problem_set_loss", "multinomial": "fos_problem_set_multinomial",
          "huber": "fos_problem_set_link_loss", "squared_hinge": "fos_problem_set_link_loss"}


def target_key(cfg):
    return f"y{cfg.classes}" if cfg.loss == "multinomial" else TARGET[cfg.loss]


def plan_move(X, Y):
    """The steps from configuration X to Y as (entry point or "target" / "grouped", argument) pairs: only what differs, in the
    order the refusal rules of csrc/fos_plan.hip allow - feature groups come off before factors or the multinomial loss go on,
    factors come off before feature groups go on, the loss leaves multinomial before feature groups are bound.  Bindings that X
    and Y share stay bound; between "bounds" and "factors" fos_coord_bind is called once, with the vectors of Y (Ctx.apply takes
    them from Y's configuration: the step itself says bind or detach, which is all the refusal rules ask)."""
    steps = []
    if X.groups and not Y.groups:
        steps.append(("fos_feature_groups_bind", False))
    if X.coord and not Y.coord:
        steps.append(("fos_coord_bind", False))
    if target_key(X) != target_key(Y):
        steps.append(("target", target_key(Y)))
    if (X.loss, X.classes) != (Y.loss, Y.classes):
        steps.append((SETTER[Y.loss], (Y.loss, Y.classes)))
    if X.weights != Y.weights:
        steps.append(("fos_row_weights_bind", Y.weights))
    if Y.coord and X.coord != Y.coord:
        steps.append(("fos_coord_bind", True))
    if Y.groups and not X.groups:
        steps.append(("fos_feature_groups_bind", True))
    if X.grouped != Y.grouped:
        steps.append(("grouped", Y.grouped))
    return steps


class Refused(Exception):
    pass


class HostModel:
    """The refusal rules of the binding entry points, written from their guard texts in csrc/fos_plan.hip (GUARDS pins each to
    the source): what a step needs of the bindings that are in place when it is made.  The shape rules (b, no sharding, the
    matrix-core pair) hold for every handle of these tests and are not modelled."""

    def __init__(self, cfg=PLAIN):
        self.loss, self.coord, self.groups = cfg.loss, bool(cfg.coord), cfg.groups        # (factors with or without the bound: alike)

    def step(self, entry, arg):
        if entry == "fos_problem_set_multinomial" and self.groups:
            raise Refused("fos_problem_set_multinomial: feature groups (fos_feature_groups_bind) are bound")
        if entry == "fos_coord_bind" and arg and self.groups:
            raise Refused("fos_coord_bind: feature groups (fos_feature_groups_bind) are bound")
        if entry == "fos_feature_groups_bind" and arg:
            if self.coord:
                raise Refused("fos_feature_groups_bind: penalty factors or bounds (fos_coord_bind) are bound")
            if self.loss == "multinomial":
                raise Refused("fos_feature_groups_bind: a multinomial problem is not served")
        if entry in SETTER.values():
            self.loss = arg[0]
        elif entry == "fos_coord_bind":
            self.coord = bool(arg)
        elif entry == "fos_feature_groups_bind":
            self.groups = bool(arg)


# entry point -> (the condition of each guard the model knows, the start of its message), beside the shape rules every setter shares
GUARDS = {
    "fos_problem_set_multinomial": [(r"has_fgroups\(p\)", "fos_problem_set_multinomial: feature groups (fos_feature_groups_bind) are bound")],
    "fos_coord_bind": [(r"has_fgroups\(p\)", "fos_coord_bind: feature groups (fos_feature_groups_bind) are bound")],
    "fos_feature_groups_bind": [(r"has_coord\(p\)", "fos_feature_groups_bind: penalty factors or bounds (fos_coord_bind) are bound"),
                                (r"p->loss\s*==\s*FOS_LOSS_MULTINOMIAL", "fos_feature_groups_bind: a multinomial problem is not served")],
    "fos_problem_set_loss": [], "fos_problem_set_link_loss": [], "fos_row_weights_bind": [],
}
SHAPE_RULES = (r"!p->b", r"p->comm\s*\|\|\s*p->col_sharded", r"!pair_dd_multi_supported\(p\)")


def check_guards(plan=PLAN):
    """Every FOS_ERR_UNSUPPORTED of a binding entry point is a shape rule or a guard of HostModel: a new refusal rule fails here
    until the model (and with it the order of plan_move) knows it."""
    text = _text(plan)
    for entry, guards in GUARDS.items():
        body = _body(text, r"\bint\s+" + entry + r"\s*\([^)]*\)\s*(?=\{)")
        conds = re.findall(r"if\s*\(((?:[^()]|\([^()]*\))*)\)\s*return\s+fail\(FOS_ERR_UNSUPPORTED", body)
        left = [c for c in conds if not any(re.fullmatch(r"\s*" + s + r"\s*", c) for s in SHAPE_RULES)]
        assert len(left) == len(guards), (entry, left)
        for (cond, message), got in zip(guards, left):
            assert re.fullmatch(r"\s*" + cond + r"\s*", got), (entry, got)
            assert message in body, (entry, message)


# what sets a handle's configuration without being a step of a move, and why
NOT_A_MOVE = {
    "fos_problem_set_stream": "the stream the handle works on: Problem.ctx follows torch's current stream",
    "fos_problem_set_gbuf": "the caller's gradient buffer, bound once by Problem._bind",
    "fos_problem_set_comm": "row sharding: no lockstep feature of these cells serves a sharded handle",
    "fos_problem_set_comm_cols": "column sharding likewise",
    "fos_problem_set_fused_stamps": "a debugging hook of the one-launch persistent step",
    "fos_problem_replan": "no step of a move: part 3 of tests/test_gpu_handle_pairs.py replans with every cell's bindings in place",
}


def binding_entry_points(include=INCLUDE):
    """The entry points of include/*.h that bind or change a handle's configuration, by name."""
    names = set()
    for path in sorted(glob.glob(os.path.join(include, "*.h"))):
        with open(path) as fh:
            names |= set(re.findall(r"\bint\s+(fos_problem_set_\w+|fos_\w+_bind|fos_problem_replan)\s*\(", fh.read()))
    return names


# ---- data ------------------------------------------------------------------------------------------------------------------------
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=4)
def data(name, kind, cus=mm.GPU_CUS):
    """The data of a shape and storage type, computed once and never modified."""
    m, n = shape(name, kind, cus)
    A, b, xt = _data.synth(m, n, SEED, density=DENSITY)
    A32 = A.astype(np.float32)
    A64 = (_forms.bf16_round_np(A32) if kind == "bf16" else A32).astype(np.float64)
    rng = np.random.default_rng(20)                                  # tests/_link.huber_recipe: a tenth of gross outliers
    out = rng.choice(m, size=max(1, m // 10), replace=False)
    b = b.copy()
    b[out] += rng.choice([-1.0, 1.0], size=out.size) * 10.0 * np.std(b)
    b = b.astype(np.float32).astype(np.float64)
    s = A @ xt                                                       # tests/_link.hinge_recipe
    ysign = np.sign(s + 0.5 * np.std(s) * np.random.default_rng(SEED + 7).standard_normal(m))
    ysign[ysign == 0] = 1.0
    start, gw = fg.layout("weights", n, SEED)
    rngb = np.random.default_rng(600 + SEED)                         # tests/_cluster_planned.targets
    B = (b[:, None] * rngb.uniform(0.5, 1.5, size=5)[None, :] + 0.3 * rngb.standard_normal((m, 5))).astype(np.float32)
    ids = np.random.default_rng(800 + SEED).integers(0, 3, size=m)   # shuffled fold ids, no fold empty
    ids[:3] = np.arange(3)
    w = wt.as_stored(wt.weights("counts", m, SEED))
    assert w.max() <= WEIGHT_MAX and gw is not None and (gw == 0).any() and (gw > 0).any()
    v0 = np.random.default_rng(SEED + 1).standard_normal(n)
    L, Lw = float(orc.estimate_lipschitz(A64, v0=v0)), wt.estimate_lipschitz(A64, w, v0)
    p = cd.factors(n, SEED)
    return _frozen(dict(name=name, kind=kind, cus=cus, m=m, n=n, A32=A32, A=A64, b=b, threshold=float(np.float32(np.median(np.abs(b)))),
                        y01=lg.labels(A, xt, SEED), ysign=ysign, y3=mn.labels(A, 3, SEED), y7=mn.labels(A, 7, SEED), w=w,
                        p=p, pp=np.where(p == 0, FREE_FACTOR, p), lo=np.zeros(n), start=start, gw=gw, B=B, ids3=ids.astype(np.int64),
                        ids2=(ids % 2).astype(np.int64), L=L, Lw=Lw))


def L_of(d, cfg):
    return d["Lw" if cfg.weights else "L"] / {"logistic": 4.0, "multinomial": 2.0}.get(cfg.loss, 1.0)


def factors(d, cfg):
    """The penalty factors of the configuration: None, d["p"] with its exact zeros, or d["pp"] without."""
    return {"": None, "bounds": d["p"], "factors": d["pp"]}[cfg.coord]


def parts(d, cfg, rows=None):
    """What a reference of the configuration takes: A, the target, w, p, lo (None where not bound), on `rows` (a mask) or all."""
    A, t = d["A"], d[target_key(cfg)]
    w = d["w"] if cfg.weights else None
    if rows is not None:
        A, t, w = A[rows], t[rows], None if w is None else w[rows]
    return A, t, w, factors(d, cfg), (d["lo"] if cfg.coord == "bounds" else None)


def gradient0(d, cfg):
    """Minus the gradient of the data term at 0 (up to its sign per coordinate, which no weight depends on)."""
    A, t, w, _, _ = parts(d, cfg)
    ww = np.ones(d["m"]) if w is None else w
    r = {"squared": t, "logistic": t - 0.5, "huber": lk.psi(lk.HUBER, np.zeros(d["m"]), t, d["threshold"]), "squared_hinge": t}[cfg.loss]
    return A.T @ (ww * r)


def ladder(amax, count, first=0.5, last=0.02):
    """`count` weights from `first` to `last` of alpha_max, geometric, every third an elastic net."""
    ratio = (last / first) ** (1.0 / max(count - 1, 1))
    return [(amax * first * ratio ** i, 0.5 if i % 3 == 1 else 0.0) for i in range(count)]


def alphas(d, cfg, count):
    """`count` weights below alpha_max of the configuration (above it 0 is the solution), lasso and elastic net mixed."""
    if cfg.loss == "multinomial":
        A, y, w, _, _ = parts(d, cfg)
        return (gp.multinomial_weights(A, y, cfg.classes, count, w) if cfg.grouped else mn.weights(A, y, cfg.classes, count))
    g0 = gradient0(d, cfg)
    if cfg.groups:
        return ladder(fg.alpha_max(g0, d["start"], fg.weights_of(d["start"], d["gw"]), MU), count)
    if cfg.coord:
        p = factors(d, cfg)
        return ladder(float((np.abs(g0)[p > 0] / p[p > 0]).max()), count)
    return ladder(float(np.abs(g0).max()), count, *((0.03, 0.003) if cfg.loss == lk.HINGE else ()))   # (weaker: both hinge branches)


def fit(d, cfg, a1, a2, rows=None, **control):
    """The fp64 reference of one fit of the configuration after ITERS iterations from 0: a dict with x (n, or n x C) and, for
    the families with device control, what tests/_coord.run records."""
    A, t, w, p, lo = parts(d, cfg, rows)
    L = L_of(d, cfg)
    if cfg.loss == "multinomial":
        if cfg.grouped:
            return dict(x=gp.iterate(gp.GroupMultinomial(A, t, cfg.classes, a1, a2, w, p), L, ITERS)[0])
        return dict(x=mn.run(A, t, cfg.classes, a1, a2, L, ITERS, w=w, p=p, lo=lo))
    if cfg.loss in (lk.HUBER, lk.HINGE):
        assert not cfg.coord and not cfg.groups
        return dict(x=lk.run(cfg.loss, A, t, a1, a2, L, ITERS, c=d["threshold"] if cfg.loss == lk.HUBER else None, w=w)[0])
    if cfg.groups:
        return fg.run(A, t, a1, a2, L, ITERS, start=d["start"], gw=d["gw"], mu=MU, loss=cfg.loss, w=w, **control)
    return cd.run(A, t, a1, a2, L, ITERS, p=p, lo=lo, loss=cfg.loss, w=w, **control)


def data_term(d, cfg, X, rows=None):
    """(the data term of every column of X - of every class group for the multinomial loss -, the bound of its fp32 sum) on all
    rows or on `rows`."""
    A, t, w, _, _ = parts(d, cfg, rows)
    ww = np.ones(A.shape[0]) if w is None else w
    if cfg.loss == "multinomial":
        C = cfg.classes
        groups = [X[:, i:i + C] for i in range(0, X.shape[1], C)]
        return (np.array([mn.nll(A, G, t, w) for G in groups]), np.array([WEIGHT_MAX ** cfg.weights * mn.nll_tolerance(A, G) for G in groups]))
    if cfg.loss == "logistic":
        return wt.wnll(A, X, t, ww), wt.wnll_tolerance(A, X, ww)
    if cfg.loss in (lk.HUBER, lk.HINGE):
        c = d["threshold"] if cfg.loss == lk.HUBER else None
        return lk.data_term(cfg.loss, A, X, t, c, w), lk.loss_tolerance(cfg.loss, A, X, t, c, w)
    sse = wt.wsse(A, X, t, ww)                         # the squared sums (no 1/2), as fos_residual_batch answers
    sw = np.sqrt(ww)
    _, tol = _data.fp32_pass_tolerances_cols(sw[:, None] * A, X, sw * t, np.zeros_like(X), sse)
    return sse, tol


def penalties(d, cfg, X, a1, a2):
    """The separable penalties of the columns of X (of the class groups for the multinomial loss) with the factors as bound."""
    p = factors(d, cfg)[:, None] if cfg.coord else 1.0
    W = cfg.classes if cfg.loss == "multinomial" else 1
    l1 = (p * np.abs(X)).sum(axis=0).reshape(-1, W).sum(axis=1)
    return a1 * l1 + 0.5 * a2 * (p * X * X).sum(axis=0).reshape(-1, W).sum(axis=1)


def block(d, columns, seed):
    """A sparse seeded n x columns block of fp32 values (what an objective or a certificate is asked for), in fp64."""
    rng = np.random.default_rng(900 + seed)
    X = 0.1 * rng.standard_normal((d["n"], columns)) * (rng.random((d["n"], columns)) < 0.3)
    return X.astype(np.float32).astype(np.float64)


# ---- the device side -------------------------------------------------------------------------------------------------------------
class Ctx:
    """The device matrix and targets of a (shape, storage type), shared by every handle of its tests."""

    def __init__(self, fos, d):
        import torch
        self.fos, self.d, self.torch = fos, d, torch
        self.At = torch.as_tensor(np.array(d["A32"])).to(torch.bfloat16 if d["kind"] == "bf16" else torch.float32).cuda()
        self.targets = {k: torch.as_tensor(d[k].astype(np.float32)).cuda() for k in ("b", "y01", "ysign", "y3", "y7")}
        self.wbuf = torch.zeros((d["m"] + 3) // 4 * 4, dtype=torch.float32, device="cuda")      # Problem._setup's padding
        self.wbuf[:d["m"]] = torch.as_tensor(d["w"].astype(np.float32))
        self.B = torch.as_tensor(np.array(d["B"])).cuda()

    def fresh(self):
        """A plain squared-loss handle on a b of its own.  Bound through prepare_weighted and detached at once: only a handle
        that is served by the matrix-core pair alone gets the padding to 68 / 72 device columns that every binding needs at
        n <= 64, and no call has run on it."""
        P = self.fos.prepare_weighted(self.At, self.targets["b"].clone(), self.d["w"])
        P.set_sample_weight(None)
        return P

    def apply(self, P, steps, coord=""):
        """The steps of plan_move on the handle, with the Python attributes the front ends read.  coord: what a binding step of
        fos_coord_bind binds - the configuration's "bounds" or "factors"."""
        from fastoptsolver_amd import _lib
        d = self.d
        for entry, arg in steps:
            if entry == "target":
                with P.ctx():                              # on the handle's stream
                    P.b.copy_(self.targets[arg])
            elif entry == "grouped":
                P.set_grouped(arg)
            elif entry == "fos_row_weights_bind":
                P.set_sample_weight(self.wbuf[:d["m"]] if arg else None)
            elif entry == "fos_coord_bind":
                P.set_penalty(*(() if not arg else (np.array(d["pp"]),) if coord == "factors" else (np.array(d["p"]), np.array(d["lo"]), None)))
            elif entry == "fos_feature_groups_bind":
                P.set_feature_groups(*((np.diff(d["start"]), np.array(d["gw"]), MU) if arg else (None,)))
            else:
                loss, classes = arg
                if loss == "multinomial":
                    _lib.check(P.lib.fos_problem_set_multinomial(int(classes), P.h), entry)
                elif loss in (lk.HUBER, lk.HINGE):
                    _lib.check(P.lib.fos_problem_set_link_loss(LOSS_IDS[loss], d["threshold"] if loss == lk.HUBER else 0.0, P.h), entry)
                else:
                    _lib.check(P.lib.fos_problem_set_loss(P.h, LOSS_IDS[loss]), entry)
                if loss != "multinomial":
                    P.grouped = False
                P.loss, P.classes = loss, (classes or None)
                P.threshold = d["threshold"] if loss == lk.HUBER else None

    def move(self, P, X, Y):
        X, Y = (c.cfg if isinstance(c, Cell) else c for c in (X, Y))
        self.apply(P, plan_move(X, Y), Y.coord)

    def run(self, cell, P):
        """cell.call on the handle as host arrays, with the assertion that the cell was served: every answer of an entry point
        that may decline (fastoptsolver_amd._lib.served: the front ends of the plain squared loss then run one by one, or column
        by column, without a word) was a yes, and the entry points the cell names were asked."""
        from fastoptsolver_amd import _lib
        asked, served = [], _lib.served

        def spy(rc, what=""):
            ok = served(rc, what)
            asked.append((what, ok))
            return ok
        _lib.served = spy
        try:
            out = cell.call(self, P)
        finally:
            _lib.served = served
        assert all(ok for _, ok in asked), (cell.name, asked, P.lib.fos_last_error())
        assert set(cell.reaches + cell.serves) & MAY_DECLINE <= {what for what, _ in asked}, (cell.name, asked)
        return {k: _host(v) for k, v in out.items()}

    def getters(self, P):
        """What the library's getters report of the handle, as a Config-shaped tuple and the Huber parameter."""
        import ctypes as C
        lib, h = P.lib, P.h
        loss, link, classes, ng = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int32(-1)
        param, mix = C.c_double(-1.0), C.c_double(-1.0)
        w, pf, lo, hi = C.c_void_p(1), C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)
        assert lib.fos_problem_get_loss(h, C.byref(loss)) == 0 and lib.fos_problem_get_link_loss(C.byref(link), C.byref(param), h) == 0
        assert lib.fos_problem_get_classes(C.byref(classes), h) == 0 and lib.fos_row_weights_get(C.byref(w), h) == 0
        assert lib.fos_coord_get(C.byref(pf), C.byref(lo), C.byref(hi), h) == 0
        assert lib.fos_feature_groups_get(C.byref(ng), C.byref(mix), h) == 0
        return dict(loss=loss.value, link=link.value, param=param.value, classes=classes.value, weights=w.value,
                    coord=(pf.value, lo.value, hi.value), ngroups=ng.value, mix=mix.value)

    def check_getters(self, P, cfg, where):
        """The getters report the configuration just set, and the handle's own attributes agree."""
        d, g = self.d, self.getters(P)
        link = cfg.loss in (lk.HUBER, lk.HINGE)
        ngroups = len(d["start"]) - 1 + (1 if P.n_dev > P.n else 0)          # the padding columns form one more group
        want = dict(loss=LOSS_IDS[cfg.loss], link=LOSS_IDS[cfg.loss] if link else 0,
                    param=np.float64(d["threshold"]) if cfg.loss == lk.HUBER else 0.0, classes=cfg.classes,
                    weights=self.wbuf.data_ptr() if cfg.weights else None,
                    coord=(P._coord[0].data_ptr(), P._coord[1].data_ptr() if cfg.coord == "bounds" else None, None) if cfg.coord else (None, None, None),
                    ngroups=ngroups if cfg.groups else 0, mix=MU if cfg.groups else 0.0)
        assert g == want, (where, g, want)
        assert (P.loss, P.classes or 0, bool(P.grouped), P.sample_weight is not None, P.has_coord, P.has_feature_groups) == \
            tuple(cfg._replace(coord=bool(cfg.coord))), where


# ---- cells -----------------------------------------------------------------------------------------------------------------------
def _host(v):
    """A result leaf as an ndarray (device tensors come to the host; bit for bit)."""
    if hasattr(v, "detach"):
        return v.detach().cpu().numpy()
    return np.asarray(v)


def same_bits(a, b):
    """None where two results of a cell are bit for bit equal, else the first key that differs with the largest difference."""
    assert set(a) == set(b)
    for k in a:
        x, y = _host(a[k]), _host(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            return k, "shape", x.shape, y.shape
        if x.tobytes() != y.tobytes():
            return k, float(np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64))))
    return None


def _rel_ok(got, want, where):
    err = _data.rel(np.asarray(_host(got), dtype=np.float64), want)
    assert err < TOL, (where, err)


class Cell:
    """A configuration of the handle and one call on it.  reaches: the lockstep entry points the call goes through.
    sized_by_panels: whether a buffer of the call is sized by the number of row panels (the pairs run at "panels")."""
    reaches, serves, sized_by_panels = (), (), False

    def __init__(self, name, cfg):
        self.name, self.cfg = name, cfg

    def reference(self, d):
        raise NotImplementedError

    def precondition(self, d, ref):
        """What the reference must show so that the cell cannot pass vacuously (asserted at the padded shape on the CPU)."""

    def ref(self, d):
        return _reference(self.name, d["name"], d["kind"], d["cus"])


class Path(Cell):
    """The family's path call with `count` weights and return_info."""
    FRONT = {"squared": "fista_path", "logistic": "logistic_path", "huber": "huber_path", "squared_hinge": "hinge_path",
             "multinomial": "multinomial_path"}
    reaches = ("fos_fista_run_multi",)

    def __init__(self, name, cfg, count):
        super().__init__(name, cfg)
        self.count = count
        self.sized_by_panels = cfg.loss == "multinomial"

    def weights(self, d):
        return alphas(d, self.cfg, self.count)

    def call(self, c, P):
        xs, info = getattr(c.fos, self.FRONT[self.cfg.loss])(P, None, self.weights(c.d), max_iter=ITERS, L=L_of(c.d, self.cfg), return_info=True)
        return dict(x=c.torch.stack(list(xs)), info=np.array(info))

    def reference(self, d):
        refs = [fit(d, self.cfg, a1, a2) for a1, a2 in self.weights(d)]
        out = dict(x=np.stack([r["x"] for r in refs]))
        if self.cfg.groups:                                   # no group norm so close to its threshold that fp32 may decide otherwise
            out["closest"] = np.array([r["closest"] for r in refs])
            assert out["closest"].min() >= fg.CLOSE, out["closest"]
        return out

    def precondition(self, d, ref):
        X = ref["x"]
        flat = X.reshape(len(X), -1)
        assert all((x != 0).any() for x in flat) and (flat[0] == 0).any(), "the penalty must bite"
        if self.cfg.coord == "bounds":                        # the lower bound binds and an unpenalised coordinate is in the model
            A, t, w, p, _ = parts(d, self.cfg)
            unc = cd.run(A, t, *self.weights(d)[-1], L_of(d, self.cfg), ITERS, p=p, loss=self.cfg.loss, w=w)["x"]
            assert (unc < 0).any() and (X >= 0).all() and (X[:, d["p"] == 0] != 0).any()
        if self.cfg.groups:
            zero, _ = fg.zero_groups(X[0], d["start"])
            assert zero.any() and (~zero).any()
        if self.cfg.grouped:
            rows0 = np.abs(X[0]).sum(axis=1) == 0.0
            assert rows0.any() and (~rows0).any(), "the group penalty must bite"
        if self.cfg.loss == lk.HUBER:
            A, b, _, _, _ = parts(d, self.cfg)
            shares = [lk.clipped_share(A, x, b, d["threshold"]) for x in [np.zeros(d["n"])] + list(X)]
            assert all(0.05 <= s <= 0.95 for s in shares), shares

    def check(self, d, out):
        ref = self.ref(d)
        for i in range(self.count):
            _rel_ok(out["x"][i], ref["x"][i], (self.name, i))
        assert (out["info"] == [ITERS, 0]).all(), out["info"]


class Controlled(Path):
    """fista_path with adaptive restart and the ratio stop, decided per weight on the device: the weights of a ladder whose every
    decision tests/_coord.fp32_proof accepts on the reference alone, of which at least one stops early (a masked column of the
    block from then on) and one runs to the end."""
    CANDIDATES = 24
    MENU = (dict(adaptive_restart=True, restart_threshold=0.95, tol_ratio=0.5), cd.CONTROL_MENU[1], cd.CONTROL_MENU[0])

    def __init__(self, name):
        super().__init__(name, PLAIN, 0)

    def chosen(self, d):
        return _controlled(d["name"], d["kind"], d["cus"])

    def weights(self, d):
        return self.chosen(d)[1]

    def call(self, c, P):
        ctl, weights = self.chosen(c.d)
        xs, info = c.fos.fista_path(P, None, weights, max_iter=ITERS, L=c.d["L"], return_info=True, **ctl)
        return dict(x=c.torch.stack(list(xs)), info=np.array(info))

    def reference(self, d):
        ctl, weights = self.chosen(d)
        refs = [fit(d, PLAIN, a1, a2, **ctl) for a1, a2 in weights]
        assert all(cd.fp32_proof(r, ctl["restart_threshold"], ctl["tol_ratio"]) for r in refs)
        return dict(x=np.stack([r["x"] for r in refs]), info=np.array([(r["k"], r["stopped"]) for r in refs]),
                    restarts=np.array([cd.genuine_restarts(r, ctl["restart_threshold"]) for r in refs]))

    def precondition(self, d, ref):
        k, stopped = ref["info"][:, 0], ref["info"][:, 1]
        assert ((stopped == cd.STOP_RATIO) & (k < ITERS)).any() and (k == ITERS).any() and ref["restarts"].sum() >= 1

    def check(self, d, out):
        ref = self.ref(d)
        assert np.array_equal(out["info"], ref["info"]), (out["info"], ref["info"])
        for i in range(len(ref["x"])):
            _rel_ok(out["x"][i], ref["x"][i], (self.name, i))


@functools.lru_cache(maxsize=None)
def _controlled(name, kind, cus):
    """(control parameters, weights): the fp32-proof weights of the ladder (at most 16, at least five: the matrix-core lockstep
    takes a controlled call from three on) under the first entry of Controlled.MENU with which one of them stops early and one
    runs to the end; where no entry gives both (the panels shape is so well conditioned that every weight stops at once) under
    the first that gives five."""
    d = data(name, kind, cus)
    found = []
    for ctl in Controlled.MENU:
        keep, ks = [], []
        for a1, a2 in ladder(float(np.abs(gradient0(d, PLAIN)).max()), Controlled.CANDIDATES, 0.6, 0.001):
            r = fit(d, PLAIN, a1, a2, **ctl)
            if cd.fp32_proof(r, ctl["restart_threshold"], ctl["tol_ratio"]) and len(keep) < 16:
                keep.append((a1, a2))
                ks.append((r["k"], r["stopped"]))
        if len(keep) >= 5:
            found.append((ctl, keep))
            if any(k < ITERS and s == cd.STOP_RATIO for k, s in ks) and any(k == ITERS for k, _ in ks):
                return ctl, keep
    assert found, "no entry of Controlled.MENU gives five weights with fp32-proof decisions"
    return found[0]


class Single(Cell):
    """fista(A, b) with one target: the single-pass kernels and gbuf."""

    def call(self, c, P):
        a1, a2 = alphas(c.d, PLAIN, 2)[1]
        return dict(x=c.fos.fista(P, None, "elasticnet", a1, a2, max_iter=ITERS, L=c.d["L"]))

    def reference(self, d):
        return dict(x=fit(d, PLAIN, *alphas(d, PLAIN, 2)[1])["x"])

    def check(self, d, out):
        _rel_ok(out["x"], self.ref(d)["x"], self.name)


class Rhs(Cell):
    """fista(A, B) for a 2-D B of five targets (ws.b16), and the squared residuals of the fits against B in one further pass.
    fista itself keeps a handle that has a b of its own on the single-target path, so the cell enters at the driver fista(A, B)
    hands a 2-D B to."""
    reaches = ("fos_fista_run_multi_rhs", "fos_residual_batch_rhs")

    def call(self, c, P):
        from fastoptsolver_amd import iterative_solvers as its
        a1, a2 = alphas(c.d, PLAIN, 2)[1]
        lp = its._Loop(None, a1, a2, False, 0.5, 1.0, ITERS, 0.0, 0.0, False, 1.0)          # fista's own defaults
        X = its._solve_targets(P, c.B, lp, c.d["L"], None, None)
        return dict(x=X, rr=np.asarray(P.residual_batch_rhs(X, c.B)))

    def reference(self, d):
        a1, a2 = alphas(d, PLAIN, 2)[1]
        return dict(x=np.stack([orc.fista(d["A"], d["B"][:, j].astype(np.float64), "elasticnet", a1, a2, max_iter=ITERS, L=d["L"])
                                for j in range(5)], axis=1))

    def check(self, d, out):
        X, ref = np.asarray(_host(out["x"]), dtype=np.float64), self.ref(d)["x"]
        assert X.shape == ref.shape
        for j in range(5):
            _rel_ok(X[:, j], ref[:, j], (self.name, j))
        X32, B = X.astype(np.float32).astype(np.float64), d["B"].astype(np.float64)       # the sums on the device's own fits
        R = d["A"] @ X32 - B
        rr = (R * R).sum(axis=0)
        _, tol = _data.fp32_pass_tolerances_cols(d["A"], X32, B, np.zeros_like(X32), rr)
        assert out["rr"].shape == (5,) and (np.abs(out["rr"] - rr) <= tol).all(), (out["rr"], rr, tol)


class Lbfgs(Cell):
    """LBFGSSolver.fit(A, B) with three targets: the fp64 multi-point pass and its plan (dm).  As in Rhs, the cell enters at
    the driver fit hands a 2-D B to: fit keeps a handle with a b of its own on the single-target path."""
    serves = ("fos_lbfgs_minimize_multi",)

    def call(self, c, P):
        from fastoptsolver_amd.lbfgs import LBFGSSolver
        s = LBFGSSolver("ridge", 0.0, 1.0, max_iter=ITERS)._fit_targets(P, c.B[:, :3].contiguous())
        return dict(x=s.x_, nit=np.asarray(s.nit_), nfev=np.asarray(s.nfev_), f=np.asarray(s.final_obj_))

    def reference(self, d):
        fits = [orc.LBFGSSolver("ridge", 0.0, 1.0, max_iter=ITERS).fit(d["A"], d["B"][:, j].astype(np.float64)) for j in range(3)]
        return dict(x=np.stack([s.x_ for s in fits], axis=1))

    def check(self, d, out):
        X, ref = _host(out["x"]), self.ref(d)["x"]
        for j in range(3):
            _rel_ok(X[:, j], ref[:, j], (self.name, j))


class Power(Cell):
    """fos_power_iter past its first chunk of 16 steps: ws.vring and ws.lhist."""
    reaches = ("fos_power_iter",)
    STEPS = 20

    def v0(self, d):
        return np.random.default_rng(SEED + 3).standard_normal(d["n"]).astype(np.float32).astype(np.float64)

    def call(self, c, P):
        L, it, v = P.power_iter(self.v0(c.d), n_iter=self.STEPS, tol=0.0)
        return dict(L=np.float64(L), it=np.int64(it), v=v)

    def reference(self, d):
        v = self.v0(d) / np.linalg.norm(self.v0(d))
        for _ in range(self.STEPS):
            w = d["A"].T @ (d["A"] @ v)
            L = float(np.linalg.norm(w))
            v = w / L
        return dict(L=L, v=v)

    def check(self, d, out):
        ref = self.ref(d)
        assert int(out["it"]) == self.STEPS and abs(float(out["L"]) - ref["L"]) <= TOL * ref["L"], (out["L"], ref["L"])
        _rel_ok(out["v"], ref["v"], self.name)


class Lipschitz(Cell):
    """estimate_lipschitz on the weighted handle: one fos_gram_apply per step of the power iteration on A^T W A."""
    STEPS = 30

    def call(self, c, P):
        state = np.random.get_state()
        np.random.seed(SEED)                               # the front end draws its start vector from the global stream
        try:
            return dict(L=np.float64(c.fos.estimate_lipschitz(P, n_iter=self.STEPS, tol=0.0)))
        finally:
            np.random.set_state(state)

    def reference(self, d):
        return dict(L=wt.estimate_lipschitz(d["A"], d["w"], np.random.RandomState(SEED).randn(d["n"]), n_iter=self.STEPS, tol=0.0))

    def check(self, d, out):
        ref = self.ref(d)["L"]
        assert abs(float(out["L"]) - ref) <= TOL * ref, (out["L"], ref)


class Cv(Cell):
    """The family's CV call on explicit fold ids with return_coefs: the train form of product 1 on every panel, the held-out
    form (R not written) behind it, the refit."""
    FRONT = {"squared": "fista_cv", "logistic": "logistic_cv", "huber": "huber_cv", "squared_hinge": "hinge_cv"}
    reaches = ("fos_fista_run_multi_folds", "fos_residual_batch_folds")
    sized_by_panels = True

    def __init__(self, name, cfg, folds, count):
        super().__init__(name, cfg)
        self.folds, self.count = folds, count

    def call(self, c, P):
        res = getattr(c.fos, self.FRONT[self.cfg.loss])(P, None, alphas(c.d, self.cfg, self.count), folds=np.array(c.d[f"ids{self.folds}"]),
                                                       max_iter=ITERS, L=L_of(c.d, self.cfg), return_coefs=True)
        return dict(coefs=res.coefs, score=np.asarray(res[1]), mean=np.asarray(res[2]), best=np.int64(res.best), x=res.x,
                    info=np.array(res.info))

    def reference(self, d):
        ids, weights = d[f"ids{self.folds}"], alphas(d, self.cfg, self.count)
        coefs = np.stack([np.stack([fit(d, self.cfg, a1, a2, rows=ids != f)["x"] for a1, a2 in weights], axis=1)
                          for f in range(self.folds)], axis=1)                 # n x K x L
        return dict(coefs=coefs)

    def precondition(self, d, ref):
        assert (ref["coefs"] != 0).any(axis=0).all() and (ref["coefs"] == 0).any(), "the penalty must bite"
        if self.cfg.loss == lk.HINGE:                                          # tests/_link.hinge_recipe's rule, at every fit
            A, y, _, _, _ = parts(d, self.cfg)
            shares = [lk.active_share(A, ref["coefs"][:, f, a], y) for f in range(self.folds) for a in range(self.count)]
            assert all(0.1 <= s <= 0.9 for s in shares), shares

    def check(self, d, out):
        ref, ids = self.ref(d)["coefs"], d[f"ids{self.folds}"]
        coefs = np.asarray(_host(out["coefs"]), dtype=np.float64)
        assert coefs.shape == ref.shape
        for f in range(self.folds):
            held = ids == f
            for a in range(self.count):
                _rel_ok(coefs[:, f, a], ref[:, f, a], (self.name, f, a))
            # the held-out score against fp64 on the device's own fits, as stored in fp32
            X32 = coefs[:, f, :].astype(np.float32).astype(np.float64)
            want, tol = data_term(d, self.cfg, X32, held)
            den = float(d["w"][held].sum()) if self.cfg.weights else float(held.sum())
            got = out["score"][f] * den
            assert (np.abs(got - want) <= tol).all(), (self.name, f, got, want, tol)
        assert int(out["best"]) == int(np.argmin(out["mean"])) and (out["info"][..., 0] == ITERS).all()
        a1, a2 = alphas(d, self.cfg, self.count)[int(out["best"])]
        _rel_ok(out["x"], fit(d, self.cfg, a1, a2)["x"], (self.name, "refit"))


class Objective(Cell):
    """The family's objective of `members` members of a seeded block: fos_residual_batch with the loss's link and the partial
    sums it reserves (ws.link_part: twice the softmax size for a pointwise link)."""
    FRONT = {"logistic": "logistic_objective", "huber": "huber_objective", "squared_hinge": "hinge_objective",
             "multinomial": "multinomial_objective"}
    reaches = ("fos_residual_batch",)
    sized_by_panels = True

    def __init__(self, name, cfg, members):
        super().__init__(name, cfg)
        self.members = members

    def weight(self, d):
        return alphas(d, self.cfg, 2)[1]

    def block(self, d):
        W = self.cfg.classes or 1
        X = block(d, W * self.members, self.members)
        return X, (X.reshape(d["n"], self.members, W).transpose(0, 2, 1) if W > 1 else X)     # member-major columns, and n x C x k

    def call(self, c, P):
        return dict(value=np.asarray(getattr(c.fos, self.FRONT[self.cfg.loss])(self.block(c.d)[1], P, None, *self.weight(c.d))))

    def reference(self, d):
        X, _ = self.block(d)
        term, tol = data_term(d, self.cfg, X)
        return dict(value=term + penalties(d, self.cfg, X, *self.weight(d)), tol=tol)

    def check(self, d, out):
        ref = self.ref(d)
        assert out["value"].shape == ref["value"].shape and (np.abs(out["value"] - ref["value"]) <= ref["tol"]).all(), \
            (self.name, out["value"], ref["value"], ref["tol"])


class KktExcess(Cell):
    """kkt_excess of a seeded block of 16 columns: one fos_gradient_batch (ws.grad_part with several panels) and one
    fos_kkt_scan with an empty set."""
    reaches = ("fos_gradient_batch", "fos_kkt_scan")
    sized_by_panels = True

    def call(self, c, P):
        return dict(excess=c.fos.kkt_excess(P, c.torch.as_tensor(block(c.d, 16, 16)), alphas(c.d, self.cfg, 16)))

    def reference(self, d):
        A, t, w, _, _ = parts(d, self.cfg)
        X = block(d, 16, 16)
        G = ws.gradient(A, t, X, self.cfg.loss, w)
        a1 = np.array([a for a, _ in alphas(d, self.cfg, 16)])
        R = A @ X - t[:, None]
        # a coordinate of a gradient column is off by no more than the column's bound in the 2-norm (tests/_data); the excess
        # itself is stored in fp32
        g_tol, _ = _data.fp32_pass_tolerances_cols(A, X, t, G, (R * R).sum(axis=0))
        excess = (np.abs(G) / a1).max(axis=1)
        return dict(excess=excess, tol=float((g_tol / a1).max()) + 2.0 * float(np.finfo(np.float32).eps) * excess)

    def check(self, d, out):
        ref = self.ref(d)
        got = np.asarray(_host(out["excess"]), dtype=np.float64)
        assert got.shape == (d["n"],) and (np.abs(got - ref["excess"]) <= ref["tol"]).all(), \
            (self.name, np.abs(got - ref["excess"]).max(), ref["tol"].max())


class WorkingSet(Cell):
    """working_set_path on the handle: the KKT scans read fos_gradient_batch on the full problem, fos_gather_columns copies the
    set's columns, the rounds themselves run on handles of their own.  max_rounds rounds of ITERS iterations from the scan at 0;
    the reference (tests/_working_set.solve) must grow its set and end certified, every scan decision further than MARGIN from
    its threshold and the last excess value the growth step takes further than GAP from the first it leaves."""
    reaches = ("fos_gradient_batch", "fos_gather_columns", "fos_kkt_scan")
    sized_by_panels = True
    COUNT, KKT_TOL, MARGIN, GAP = 5, 1e-2, 1e-3, 1e-4

    def weights(self, d):
        return ladder(float(np.abs(gradient0(d, self.cfg)).max()), self.COUNT, 0.9, 0.3)

    def call(self, c, P):
        xs, infos = c.fos.working_set_path(P, None, self.weights(c.d), ITERS, L=L_of(c.d, self.cfg), kkt_tol=self.KKT_TOL,
                                           max_fraction=1.0, return_info=True)
        i = infos[0]
        return dict(x=c.torch.stack(list(xs)), rounds=np.int64(i.rounds), sizes=np.array(i.sizes), grads=np.int64(i.full_gradients),
                    fell_back=np.bool_(i.fell_back), worst=np.float64(i.worst_excess))

    def reference(self, d):
        A, t, w, _, _ = parts(d, self.cfg)
        margins, gaps = [], []
        scan = ws.scan

        def recording(G, alpha1, slack, in_ws, p=None):
            excess, viol = scan(G, alpha1, slack, in_ws, p)
            out = np.asarray(in_ws) == 0
            e = np.asarray(excess, dtype=np.float64)[out]
            margins.append(float(np.abs(e - (1.0 + slack)).min()) if out.any() else np.inf)
            want, top = int((np.asarray(in_ws) != 0).sum()), np.sort(e[e > 0])[::-1]      # grow = 2: the set doubles
            if slack > 0 and 0 < viol.size < want < top.size:                            # the growth step takes the `want` largest
                gaps.append(float(top[want - 1] - top[want]))
            return excess, viol
        ws.scan = recording
        try:
            X, info = self.solve(d, A, t, w)
        finally:
            ws.scan = scan
        assert min(margins) >= self.MARGIN and min(gaps + [np.inf]) >= self.GAP and not info["fell_back"], (margins, gaps, info)
        return dict(x=X.T, rounds=np.int64(info["rounds"]), sizes=np.array(info["sizes"]), grads=np.int64(info["full_gradients"]),
                    worst=np.float64(info["worst_excess"]), margin=np.float64(min(margins)), gap=np.float64(min(gaps + [np.inf])))

    def precondition(self, d, ref):
        assert ref["rounds"] >= 2 and ref["sizes"][-1] > ref["sizes"][0], ref["sizes"]                      # grown
        assert ref["worst"] <= 1.0 + self.KKT_TOL and ref["sizes"][-1] < d["n"], (ref["worst"], ref["sizes"])     # and certified

    def solve(self, d, A, t, w):
        if self.cfg.loss == lk.HUBER:
            return solve_link(A, t, d["threshold"], self.weights(d), L_of(d, self.cfg), self.KKT_TOL)
        return ws.solve(A, t, self.weights(d), ITERS, loss=self.cfg.loss, w=w, L=L_of(d, self.cfg), kkt_tol=self.KKT_TOL, max_fraction=1.0)

    def check(self, d, out):
        ref = self.ref(d)
        assert (int(out["rounds"]), list(out["sizes"]), int(out["grads"]), bool(out["fell_back"])) == \
            (int(ref["rounds"]), list(ref["sizes"]), int(ref["grads"]), False), (out, ref)
        for i in range(self.COUNT):
            _rel_ok(out["x"][i], ref["x"][i], (self.name, i))


def solve_link(A, b, c, weights, L, kkt_tol):
    """tests/_working_set.solve for the Huber loss (one group, from the scan at 0, no fall-back): the gradient of the data term is
    tests/_link.gradient and a round is tests/_link.run's loop from the set's current values."""
    n, nv = A.shape[1], len(weights)
    a1s = [a for a, _ in weights]
    X = np.zeros((n, nv))

    def check(slack, mask):
        return ws.scan(lk.gradient(lk.HUBER, A, X, b, c).T.astype(np.float32), a1s, slack, mask, np.ones(n))
    mask = np.zeros(n, dtype=np.uint8)
    excess, viol = check(0.0, mask)
    grads, sizes, worst = 1, [], float(excess.max())
    mask[viol] = 1
    while mask.any():
        idx = np.nonzero(mask)[0]
        sizes.append(int(idx.size))
        for j, (a1, a2) in enumerate(weights):
            prob = lk.LinkProblem(lk.HUBER, A[:, idx], b, a1, a2, c)
            st = prob.init_state(L)
            st.x, st.x_old, st.y = X[idx, j].copy(), X[idx, j].copy(), X[idx, j].copy()
            for _ in range(ITERS):
                prob.step(st)
            X[idx, j] = st.x
        excess, viol = check(kkt_tol, mask)
        grads, worst = grads + 1, float(excess.max())
        if viol.size == 0:
            break
        mask[viol] = 1
        want = int(idx.size)                                         # grow = 2
        if viol.size < want:
            order = np.argsort(-excess.astype(np.float64), kind="stable")[:want]
            mask[order[excess[order] > 0]] = 1
    return X, dict(rounds=len(sizes), sizes=sizes, full_gradients=grads, worst_excess=worst, fell_back=False)


class DualityGap(Cell):
    """The duality-gap certificate (fos_duality_gap) of the nv columns of a seeded block, one of them all zero, under the
    configuration's weights: the gradient block by the launches of fos_gradient_batch, product 1 once more in its plain storing
    form into multi.rbuf16, b and the row weights offset per panel, ws.dual_part sized by the panel count, ws.dual_col written by
    one launch and read by the next.  The lasso columns get a scale below 1 (an iterate that is not optimal), the elastic-net
    columns - every third - the scale 1 exactly: both arms of the scale and of the conjugate."""
    reaches = ("fos_duality_gap", "fos_gradient_batch")
    sized_by_panels = True
    ZERO = 0                                  # the all-zero column (a lasso column at every width)

    def __init__(self, name, cfg, nv):
        super().__init__(name, cfg)
        self.count = nv

    def points(self, d):
        X = block(d, self.count, self.count).copy()
        X[:, self.ZERO] = 0.0
        return X

    def call(self, c, P):
        weights = alphas(c.d, self.cfg, self.count)
        out64, G = P.duality_gap_block(c.torch.as_tensor(self.points(c.d)), [a for a, _ in weights], [a for _, a in weights])
        return dict(out=out64.reshape(4, 16), G=G)

    def _case(self, d):
        A, t, w, p, _ = parts(d, self.cfg)
        return A, t, (d["threshold"] if self.cfg.loss == lk.HUBER else None), w, p

    def reference(self, d):
        A, t, c, w, p = self._case(d)
        X = self.points(d)
        ref = du.certificate(self.cfg.loss, A, t, X, alphas(d, self.cfg, self.count), c, w, p)
        G = du.gradient(self.cfg.loss, A, X, t, c, w)
        # a gradient column is off by no more than the column's bound in the 2-norm, as in KktExcess (the pass on sqrt(w) A)
        sw = np.ones(d["m"]) if w is None else np.sqrt(w)
        g_tol, _ = _data.fp32_pass_tolerances_cols(sw[:, None] * A, X, sw * np.abs(t), G, np.ones(self.count))
        return dict(ref, G=G, g_tol=g_tol)

    def precondition(self, d, ref):
        s, live = ref["scale"], np.arange(self.count) != self.ZERO
        assert ((s > 0) & (s < 1)).any() and (s == 1).any(), s              # both arms of the scale, and with them of the conjugate
        # a gap made of rounding noise would let a wrong dual pass
        assert (ref["gap"][live] > 100.0 * du.TOL * ref["mag_gap"][live]).all(), ref["gap"] / ref["mag_gap"]
        assert all(np.isfinite(ref[k]).all() for k in ("primal", "dual", "gap", "scale"))
        if self.cfg.coord:
            assert self.cfg.coord == "factors" and (factors(d, self.cfg) > 0).all()      # an unpenalised coordinate: every scale 0

    def check(self, d, out):
        A, t, c, w, p = self._case(d)
        nv, n, ref = self.count, d["n"], self.ref(d)
        got, G = np.asarray(out["out"], dtype=np.float64), np.asarray(out["G"])
        assert got.shape == (4, 16) and G.shape[0] == nv and G.dtype == np.float32
        assert np.isfinite(got).all() and (got[:, nv:] == 0).all() and (G[:, n:] == 0).all(), (self.name, got[:, nv:])
        err = np.linalg.norm(G[:, :n].T.astype(np.float64) - ref["G"], axis=0)
        assert (err <= ref["g_tol"]).all(), (self.name, (err / ref["g_tol"]).max())
        weights = alphas(d, self.cfg, nv)
        on = du.certificate(self.cfg.loss, A, t, self.points(d), weights, c, w, p, G=G[:, :n])      # scale and conjugate from the returned G
        for row, key in enumerate(("primal", "dual", "gap")):
            assert (np.abs(got[row, :nv] - on[key]) <= du.TOL * on["mag_" + key]).all(), \
                (self.name, key, (np.abs(got[row, :nv] - on[key]) / on["mag_" + key]).max())
        assert np.abs(got[3, :nv] - du.scale_of(G[:, :n], p, weights)).max() <= 1e-12, (self.name, got[3, :nv])
        assert np.array_equal(got[2, :nv], got[0, :nv] - got[1, :nv])


class CertifiedPath(Cell):
    """certified_path on the handle: a certificate at 0, then rounds on handles of their own over gathered columns
    (fos_gather_columns), one fos_duality_gap per round on the full problem, and a scan of its gradient block (fos_kkt_scan).  The
    reference is tests/_duality.certified with the same L; every decision of it - the stop rule per column, the scans, the growth
    step - is further from its threshold than fp32 can move it (reference asserts so, at every shape it is computed for): the
    stop rule by STOP_MARGIN of the magnitude of the gap's terms, the scans and the growth step by the WorkingSet cell's MARGIN
    and GAP.  A tenth of the rows of b are gross outliers, so P* is 0.9 P(0) and the terms of a converged gap sum to 1.95 P(0) in
    magnitude: a bound of gap_tol P(0) lies gap_tol / 1.95 of that magnitude from a gap of 0, which is within STOP_MARGIN for
    certified_path's default 1e-4 and for 1e-3 alike.  GAP_TOL = 1e-2 is the first power of ten at which the rule can hold on this
    data, and the weights (a ladder from 0.3 to 0.05 of alpha_max) are the first of three ladders tried, on the reference alone,
    with which it does for both shapes and storage types: two rounds at the padded shape (30 columns, then all 37), one or two
    at the two-panel shape with the top-k branch of the growth step, smallest margins 3.9e-3 / 4.1e-3 / 9.0e-3."""
    reaches = ("fos_duality_gap", "fos_gradient_batch", "fos_gather_columns", "fos_kkt_scan")
    sized_by_panels = True
    COUNT, FRACTIONS, GAP_TOL, PATH_ITERS, ROUNDS = 5, (0.3, 0.05), 1e-2, ITERS, 20
    STOP_MARGIN = 100.0 * du.TOL

    def weights(self, d):
        return ladder(float(np.abs(gradient0(d, self.cfg)).max()), self.COUNT, *self.FRACTIONS)

    def call(self, c, P):
        xs, infos = c.fos.certified_path(P, None, self.weights(c.d), self.GAP_TOL, self.PATH_ITERS, max_rounds=self.ROUNDS, max_fraction=1.0,
                                         L=L_of(c.d, self.cfg), return_info=True)
        i = infos[0]
        return dict(x=c.torch.stack(list(xs)), rounds=np.int64(i.rounds), sizes=np.array(i.sizes), certificates=np.int64(i.certificates),
                    fell_back=np.bool_(i.fell_back), certified=np.array(i.certified), cert=np.stack([i.primal, i.dual, i.gap, i.scale]))

    def reference(self, d):
        A, t, w, p, _ = parts(d, self.cfg)
        X, info = du.certified(self.cfg.loss, A, t, self.weights(d), self.GAP_TOL, self.PATH_ITERS, w=w, p=p, L=L_of(d, self.cfg),
                               max_rounds=self.ROUNDS, max_fraction=1.0)
        assert info["stop_margins"].min() > self.STOP_MARGIN and info["scan_margins"].min() >= WorkingSet.MARGIN and \
            min(list(info["growth_gaps"]) + [np.inf]) >= WorkingSet.GAP, (info["stop_margins"], info["scan_margins"], info["growth_gaps"])
        return dict(x=X.T, rounds=np.int64(info["rounds"]), sizes=np.array(info["sizes"]), certificates=np.int64(info["certificates"]),
                    fell_back=np.bool_(info["fell_back"]), certified=info["certified"], gap=info["gap"], mag_gap=info["mag_gap"],
                    stop_margin=np.float64(info["stop_margins"].min()))

    def precondition(self, d, ref):
        assert ref["rounds"] >= 2 and ref["sizes"][-1] > ref["sizes"][0] and ref["certified"].all() and not ref["fell_back"], ref

    def check(self, d, out):
        ref = self.ref(d)
        assert (int(out["rounds"]), list(out["sizes"]), int(out["certificates"]), bool(out["fell_back"]), list(out["certified"])) == \
            (int(ref["rounds"]), list(ref["sizes"]), int(ref["certificates"]), bool(ref["fell_back"]), list(ref["certified"])), (out, ref)
        for i in range(self.COUNT):
            _rel_ok(out["x"][i], ref["x"][i], (self.name, i))
        assert (np.abs(out["cert"][2] - ref["gap"]) <= du.TOL * ref["mag_gap"]).all(), (out["cert"][2], ref["gap"])


# ---- the resampled lockstep (include/fos_resample.h) -----------------------------------------------------------------------------
# A resampled call binds nothing: the multiplicities travel with the call, so these cells use the configurations above and no new
# move.  Column j fits the problem with the row weights w * c_j; the references are the weighted references tests/_resample.py
# picks.  The counts are tests/_resample.counts at the shape's row count; L per resample is the oracle's power iteration on w * c_j.
def _divisor(cfg):
    return 4.0 if cfg.loss == "logistic" else 1.0


@functools.lru_cache(maxsize=None)
def _resampled_L(name, kind, cus, weighted, recipe, resamples):
    """lambda_max(A^T diag(w * c_r) A) per resample of rsp.counts(recipe, m, resamples, SEED), before the logistic quarter."""
    d = data(name, kind, cus)
    C = rsp.counts(recipe, d["m"], resamples, SEED)
    v0 = np.random.default_rng(SEED + 1).standard_normal(d["n"])
    return np.array([rsp.lipschitz(d["A"], rsp.effective(d["w"] if weighted else None, C[:, r]), v0) for r in range(resamples)])


def resampled_fit(d, cfg, weff, a1, a2, L, bounded=True):
    """The fp64 reference of one column of a resampled run: the configuration's fit with the row weights weff = w * c_j and the
    constant L of ITS data term, as a dict with x (and closest under feature groups).  bounded=False: the factors without the bound."""
    A, t, _, p, lo = parts(d, cfg)
    lo = lo if bounded else None
    if cfg.groups:
        return fg.run(A, t, a1, a2, L, ITERS, start=d["start"], gw=d["gw"], mu=MU, loss=cfg.loss, w=weff)
    if cfg.loss in (lk.HUBER, lk.HINGE):
        c = d["threshold"] if cfg.loss == lk.HUBER else None
        prob = lk.CoordLinkProblem(cfg.loss, A, t, a1, a2, c, weff).bind(p, lo, None) if cfg.coord else None
        return dict(x=rsp.run(cfg.loss, A, t, weff, a1, a2, L, ITERS, c=c, prob=prob)[0])
    if cfg.coord:
        return cd.run(A, t, a1, a2, L, ITERS, p=p, lo=lo, loss=cfg.loss, w=weff)
    return dict(x=rsp.run(cfg.loss, A, t, weff, a1, a2, L, ITERS)[0])


class ResampledPath(Cell):
    """resampled_path on `resamples` resamples x `weights` weights (count lockstep columns, resample-major), with return of the
    info and, with oob, the out-of-bag sums from one more pass (fos_gradient_batch_resampled, oob = 1)."""
    reaches = ("fos_fista_run_multi_resampled",)

    def __init__(self, name, cfg, recipe, resamples, weights, oob=False):
        super().__init__(name, cfg)
        self.recipe, self.resamples, self.nweights, self.oob = recipe, resamples, weights, oob
        self.count = resamples * weights
        assert self.count <= 16
        if oob:
            self.reaches = self.reaches + ("fos_gradient_batch_resampled",)
            self.sized_by_panels = True

    def counts(self, d):
        return rsp.counts(self.recipe, d["m"], self.resamples, SEED)

    def Ls(self, d):
        return _resampled_L(d["name"], d["kind"], d["cus"], self.cfg.weights, self.recipe, self.resamples)

    def weights(self, d):
        """The configuration's weights: fractions of alpha_max of all rows.  A 0/1 resample keeps half of the rows and with them
        about half of the gradient at 0, so its weights are halved - at the first weight of the ladder (half of alpha_max) the fit
        of a half would otherwise still be 0."""
        scale = 0.5 if self.recipe == "binary" else 1.0
        return [(scale * a1, a2) for a1, a2 in alphas(d, self.cfg, self.nweights)]

    def call(self, c, P):
        res = c.fos.resampled_path(P, self.weights(c.d), self.counts(c.d), ITERS, L=self.Ls(c.d), oob=self.oob)
        out = dict(x=res.coefs, info=np.array(res.info))
        return dict(out, oob=res.oob_loss, size=res.oob_size) if self.oob else out

    def reference(self, d):
        C, Ls, w = self.counts(d), self.Ls(d), (d["w"] if self.cfg.weights else None)
        refs = [[resampled_fit(d, self.cfg, rsp.effective(w, C[:, r]), a1, a2, Ls[r] / _divisor(self.cfg)) for a1, a2 in self.weights(d)]
                for r in range(self.resamples)]
        out = dict(x=np.stack([np.stack([f["x"] for f in row]) for row in refs]))           # resamples x weights x n
        if self.cfg.groups:                                   # no group norm so close to its threshold that fp32 may decide otherwise
            out["closest"] = np.array([[f["closest"] for f in row] for row in refs])
            assert out["closest"].min() >= fg.CLOSE, out["closest"]
        return out

    def precondition(self, d, ref):
        C, X = self.counts(d), ref["x"]
        flat = X.reshape(-1, d["n"])
        assert all((x != 0).any() for x in flat) and any((x == 0).any() for x in flat), "the penalty must bite"
        assert (C == 0).any(axis=0).all() and C.max() == (rsp.MAX_COUNT if self.recipe == "bootstrap" else 1)
        if self.cfg.weights:                                  # an exact-zero weight under a positive count, and a positive one under 0
            assert ((d["w"] == 0)[:, None] & (C > 0)).any() and ((d["w"] > 0)[:, None] & (C == 0)).any()
        if self.cfg.coord == "bounds":                        # the lower bound binds and an unpenalised coordinate is in the model
            w = d["w"] if self.cfg.weights else None
            free = [resampled_fit(d, self.cfg, rsp.effective(w, C[:, r]), *self.weights(d)[-1], self.Ls(d)[r] / _divisor(self.cfg), bounded=False)
                    for r in range(self.resamples)]
            assert any((f["x"] < 0).any() for f in free) and (X >= 0).all() and (X[..., d["p"] == 0] != 0).any()
        if self.cfg.groups:
            zero = [fg.zero_groups(x, d["start"])[0] for x in flat]
            assert all(z.any() and (~z).any() for z in zero)

    def check(self, d, out):
        ref = self.ref(d)
        X = np.asarray(_host(out["x"]), dtype=np.float64)
        assert X.shape == (d["n"], self.resamples, self.nweights)
        for r in range(self.resamples):
            for a in range(self.nweights):
                _rel_ok(X[:, r, a], ref["x"][r, a], (self.name, r, a))
        assert out["info"].shape == (self.resamples, self.nweights, 2) and (out["info"] == [ITERS, 0]).all(), out["info"]
        if self.oob:                                          # the sums against fp64 on the device's own fits, as stored in fp32
            A, t, w, _, _ = parts(d, self.cfg)
            left = self.counts(d) == 0
            size = left.sum(axis=0).astype(np.float64) if w is None else (w[:, None] * left).sum(axis=0)
            assert np.allclose(out["size"], size, rtol=1e-12, atol=0) and (size > 0).all()
            c = d["threshold"] if self.cfg.loss == lk.HUBER else None
            for r in range(self.resamples):
                X32 = X[:, r, :].astype(np.float32).astype(np.float64)
                Wo = np.repeat((left[:, r] * (1.0 if w is None else w))[:, None], self.nweights, axis=1)
                want, tol = rsp.data_term(self.cfg.loss, A, X32, t, Wo, c), rsp.loss_tolerance(self.cfg.loss, A, X32, t, Wo, c)
                assert (np.abs(out["oob"][r] - want) <= tol).all(), (self.name, r, out["oob"][r], want, tol)


class ResampledGradient(Cell):
    """fos_gradient_batch_resampled through the C ABI at the 16 columns of a seeded block with one zero column, bootstrap counts:
    G and loss16 in-bag, then loss16 out-of-bag with G = NULL (product 2 does not run).  With several panels the partial sums of
    every panel are copied behind each other into ws.grad_part before the fold."""
    reaches = ("fos_gradient_batch_resampled",)
    sized_by_panels = True
    ZERO = 3

    def counts(self, d):
        return rsp.counts("bootstrap", d["m"], 16, SEED)

    def points(self, d):
        """The seeded block times 4 (exact in fp32): at the block's own scale every margin 1 - y a.x of most columns is positive and
        the hinge has one branch; at this one at least a twentieth of the rows is on either (precondition: the Huber cells' rule)."""
        X = 4.0 * block(d, 16, 16)
        X[:, self.ZERO] = 0.0
        return X

    def call(self, c, P):
        from fastoptsolver_amd import _core, _lib, resample
        words = resample.pack_counts(c.torch.from_numpy(np.ascontiguousarray(self.counts(c.d))).to(P.device))
        Xf, nv = P._block16(c.torch.as_tensor(self.points(c.d)))
        G = c.torch.full((nv, P.n_dev), float("nan"), dtype=c.torch.float32, device=P.device)
        sums = []
        for oob in (0, 1):
            with P.ctx():
                _lib.check(P.lib.fos_gradient_batch_resampled(_core.ptr(Xf), nv, _core.ptr(words), oob, P.h, None if oob else _core.ptr(G),
                                                              _core.ptr(P.scratch)), "fos_gradient_batch_resampled")
            sums.append(P.scratch[:16].clone())
        return dict(G=G, inbag=sums[0], oob=sums[1])

    def _case(self, d):
        A, t, w, _, _ = parts(d, self.cfg)
        C = self.counts(d)
        return A, t, (d["threshold"] if self.cfg.loss == lk.HUBER else None), rsp.effective(None, C) * (1.0 if w is None else w[:, None]), \
            (C == 0) * (1.0 if w is None else w[:, None])

    def reference(self, d):
        A, t, c, W, Wo = self._case(d)
        X = self.points(d)
        G = rsp.gradient(self.cfg.loss, A, X, t, W, c)
        # a gradient column is off by no more than the column's bound in the 2-norm, as in KktExcess and DualityGap (the pass on
        # sqrt(w c_j) A: tests/_resample.gradient_tolerance is that bound with every column's own weights)
        return dict(G=G, g_tol=rsp.gradient_tolerance(A, X, t, W, G),
                    inbag=rsp.data_term(self.cfg.loss, A, X, t, W, c), inbag_tol=rsp.loss_tolerance(self.cfg.loss, A, X, t, W, c),
                    oob=rsp.data_term(self.cfg.loss, A, X, t, Wo, c), oob_tol=rsp.loss_tolerance(self.cfg.loss, A, X, t, Wo, c))

    def precondition(self, d, ref):
        C = self.counts(d)
        assert C.max() == rsp.MAX_COUNT and (C == 0).any(axis=0).all() and (self.points(d)[:, self.ZERO] == 0).all()
        assert (np.linalg.norm(ref["G"], axis=0) > 100.0 * ref["g_tol"]).all()              # no gradient of rounding noise
        assert (ref["inbag"] > 100.0 * ref["inbag_tol"]).all() and (ref["oob"] > 100.0 * ref["oob_tol"]).all()
        if self.cfg.loss == lk.HINGE:                         # both branches of the hinge at every non-zero column of the block
            A, t, _, _, _ = self._case(d)
            shares = [lk.active_share(A, x, t) for j, x in enumerate(self.points(d).T) if j != self.ZERO]
            assert all(0.05 <= s <= 0.95 for s in shares), shares

    def check(self, d, out):
        ref, n = self.ref(d), d["n"]
        G, inbag, oob = (np.asarray(out[k]) for k in ("G", "inbag", "oob"))
        assert G.shape[0] == 16 and G.dtype == np.float32 and np.isfinite(G).all() and (G[:, n:] == 0).all()      # nv = 16: no entry >= nv
        err = np.linalg.norm(G[:, :n].T.astype(np.float64) - ref["G"], axis=0)
        assert (err <= ref["g_tol"]).all(), (self.name, (err / ref["g_tol"]).max())
        for got, key in ((inbag, "inbag"), (oob, "oob")):
            assert got.shape == (16,) and (np.abs(got - ref[key]) <= ref[key + "_tol"]).all(), (self.name, key, got, ref[key], ref[key + "_tol"])


class ResampledLipschitz(Cell):
    """resampled_lipschitz on 18 resamples - a group of 16 bootstrap columns and one of two 0/1 columns -: one
    fos_gram_apply_resampled per step and group of the power iteration on A^T diag(w * c_r) A.  The front end draws its start
    vectors from the global legacy stream, which the cell seeds itself: a fresh handle and a shared one draw the same."""
    reaches = ("fos_gram_apply_resampled",)
    STEPS = 30

    def counts(self, d):
        return np.concatenate([rsp.counts("bootstrap", d["m"], 16, SEED), rsp.counts("binary", d["m"], 2, SEED)], axis=1)

    def call(self, c, P):
        state = np.random.get_state()
        np.random.seed(SEED)
        try:
            return dict(L=c.fos.resampled_lipschitz(P, self.counts(c.d), n_iter=self.STEPS, tol=0.0))
        finally:
            np.random.set_state(state)

    def reference(self, d):
        C, rs = self.counts(d), np.random.RandomState(SEED)
        v0 = [rs.randn(d["n"]) for _ in range(18)]
        return dict(L=np.array([wt.estimate_lipschitz(d["A"], rsp.effective(d["w"] if self.cfg.weights else None, C[:, r]), v0[r],
                                                       n_iter=self.STEPS, tol=0.0) for r in range(18)]))

    def precondition(self, d, ref):
        assert self.cfg.weights and ref["L"].shape == (18,) and ref["L"][:16].max() > ref["L"][16:].max() > 0      # a row drawn 15 times weighs 15 times

    def check(self, d, out):
        ref = self.ref(d)["L"]
        assert out["L"].shape == (18,) and out["L"].dtype == np.float64 and np.allclose(out["L"], ref, rtol=pw.TOL, atol=0), (out["L"], ref)


class ResampledControlled(Cell):
    """resampled_path with adaptive restart and the ratio stop per column, built like tests/_resample.controlled_case: RESAMPLES
    0/1 resamples under a ladder of WEIGHTS weights with L of the whole A (valid for 0/1 counts), ITERATIONS iterations at the most.
    Every (resample, weight) pair runs; those whose every decision in the fp64 reference tests/_coord.fp32_proof accepts - the
    rule of the Controlled cell - are compared: their stop iteration, stop code and iterate."""
    reaches = ("fos_fista_run_multi_resampled",)
    RESAMPLES, WEIGHTS, ITERATIONS = 2, 8, 36
    MENU = Controlled.MENU + rsp.CONTROL_MENU

    def __init__(self, name):
        super().__init__(name, PLAIN)

    def counts(self, d):
        return rsp.counts("binary", d["m"], self.RESAMPLES, SEED)

    def weights(self, d):
        return ladder(float(np.abs(gradient0(d, PLAIN)).max()), self.WEIGHTS, 0.3, 0.01)

    def chosen(self, d):
        return _resampled_controlled(d["name"], d["kind"], d["cus"])

    def call(self, c, P):
        ctl = self.chosen(c.d)[0]
        res = c.fos.resampled_path(P, self.weights(c.d), self.counts(c.d), self.ITERATIONS, L=c.d["L"], **ctl)
        return dict(x=res.coefs, info=np.array(res.info))

    def runs(self, d, ctl):
        C = self.counts(d)
        return {(r, a): cd.run(d["A"], d["b"], a1, a2, d["L"], self.ITERATIONS, w=C[:, r].astype(np.float64), **ctl)
                for r in range(self.RESAMPLES) for a, (a1, a2) in enumerate(self.weights(d))}

    def reference(self, d):
        ctl, kept = self.chosen(d)
        pairs = sorted(kept)
        return dict(pairs=np.array(pairs), x=np.stack([kept[p]["x"] for p in pairs]), info=np.array([(kept[p]["k"], kept[p]["stopped"]) for p in pairs]),
                    restarts=np.array([cd.genuine_restarts(kept[p], ctl["restart_threshold"]) for p in pairs]))

    def precondition(self, d, ref):
        k, stopped = ref["info"][:, 0], ref["info"][:, 1]
        assert 2 * len(ref["pairs"]) >= self.RESAMPLES * self.WEIGHTS, len(ref["pairs"])       # at least half of the pairs remain
        assert ((stopped == cd.STOP_RATIO) & (k < self.ITERATIONS)).any() and (k == self.ITERATIONS).any() and ref["restarts"].sum() >= 1

    def check(self, d, out):
        ref = self.ref(d)
        X = np.asarray(_host(out["x"]), dtype=np.float64)
        assert X.shape == (d["n"], self.RESAMPLES, self.WEIGHTS) and out["info"].shape == (self.RESAMPLES, self.WEIGHTS, 2)
        for (r, a), x, info in zip(ref["pairs"], ref["x"], ref["info"]):
            assert tuple(out["info"][r, a]) == tuple(info), (self.name, r, a, out["info"][r, a], info)
            _rel_ok(X[:, r, a], x, (self.name, r, a))


@functools.lru_cache(maxsize=None)
def _resampled_controlled(name, kind, cus):
    """(control parameters, {(resample, weight): the reference run} of the fp32-proof pairs) under the first entry of
    ResampledControlled.MENU with which at least half of the pairs are fp32-proof and one of them stops early, one runs to the end
    and one restarts on a finite ratio; where no entry gives all three (the panels shape is so well conditioned that every pair
    stops at once) under the first that keeps half.  Decided on the reference alone."""
    d, cell = data(name, kind, cus), ALL_CELLS["resampled_controlled"]
    found = []
    for ctl in cell.MENU:
        kept = {p: r for p, r in cell.runs(d, ctl).items() if cd.fp32_proof(r, ctl["restart_threshold"], ctl["tol_ratio"])}
        if 2 * len(kept) >= cell.RESAMPLES * cell.WEIGHTS:
            found.append((ctl, kept))
            refs = list(kept.values())
            if any(r["k"] < cell.ITERATIONS and r["stopped"] == cd.STOP_RATIO for r in refs) and any(r["k"] == cell.ITERATIONS for r in refs) \
                    and sum(cd.genuine_restarts(r, ctl["restart_threshold"]) for r in refs) >= 1:
                return ctl, kept
    assert found, "no entry of ResampledControlled.MENU keeps half of the pairs"
    return found[0]


# ---- the working set and the duality gap of the multinomial lockstep (include/fos_multinomial_ws.h) ----------------------------------
class MultinomialGap(Cell):
    """multinomial_duality_gap's device call (fos_multinomial_duality_gap: the certificate of `count` fits of a seeded block, one of
    them zero, with the gradient block of the same pass) and multinomial_kkt_excess (one fos_multinomial_gradient_batch and one
    fos_multinomial_kkt_scan with an empty set), against tests/_multinomial_ws.certificate and .scan."""
    reaches = ("fos_multinomial_gradient_batch", "fos_multinomial_kkt_scan", "fos_multinomial_duality_gap")
    sized_by_panels = True
    ZERO = 0

    def __init__(self, name, cfg, count):
        super().__init__(name, cfg)
        self.count = count
        assert count * cfg.classes <= 16

    def fits(self, d):
        C = self.cfg.classes
        X = block(d, C * self.count, C * self.count + 1)
        fits = [X[:, s * C:(s + 1) * C].copy() for s in range(self.count)]
        fits[self.ZERO][:] = 0.0
        return fits

    def call(self, c, P):
        weights = alphas(c.d, self.cfg, self.count)
        fits = self.fits(c.d)
        out64, G = P.multinomial_duality_gap_block(c.torch.as_tensor(mws.block(fits).astype(np.float32)).cuda(),
                                                   [a for a, _ in weights], [a for _, a in weights])
        return dict(out=out64.reshape(4, 16), G=G, excess=c.fos.multinomial_kkt_excess(P, fits, weights))

    def reference(self, d):
        A, y, w, p, _ = parts(d, self.cfg)
        C, fits, weights = self.cfg.classes, self.fits(d), alphas(d, self.cfg, self.count)
        ref = mws.certificate(A, y, C, fits, weights, self.cfg.grouped, w, p)
        G = mws.gradient_block(A, y, C, fits, w)                                       # (count C) x n
        # sigma - onehot(y) moves by at most half the largest error of the fit's C logits: a class column of the gradient is off by
        # no more than the largest bound of fos_gradient_batch among the fit's columns (|t| <= 1 in b's place), as in KktExcess
        col_tol, _ = _data.fp32_pass_tolerances_cols(A, mws.block(fits), np.ones(d["m"]), G.T, np.ones(C * self.count))
        g_tol = np.repeat(col_tol.reshape(self.count, C).max(axis=1), C)
        excess = np.zeros(d["n"])
        for s, (a1, _) in enumerate(weights):
            e, _, _ = mws.scan(G[s * C:(s + 1) * C].astype(np.float32), C, self.cfg.grouped, [a1], 0.0, np.zeros(d["n"]), p)
            excess = np.maximum(excess, e.astype(np.float64))
        a1s = np.repeat([a for a, _ in weights], C)
        return dict(ref, G=G, g_tol=g_tol, excess=excess,
                    excess_tol=(np.sqrt(C) if self.cfg.grouped else 1.0) * float((g_tol / a1s).max()) + 2.0 * float(np.finfo(np.float32).eps) * excess)

    def precondition(self, d, ref):
        s, live = ref["scale"], np.arange(self.count) != self.ZERO
        assert ((s > 0) & (s < 1)).any() and (s == 1).any(), s
        assert (ref["gap"][live] > 100.0 * mws.TOL * ref["mag_gap"][live]).all(), ref["gap"] / ref["mag_gap"]
        assert all(np.isfinite(ref[k]).all() for k in ("primal", "dual", "gap", "scale", "excess")) and (ref["excess"] > 0).all()

    def check(self, d, out):
        A, y, w, p, _ = parts(d, self.cfg)
        C, n, nv, ref = self.cfg.classes, d["n"], self.cfg.classes * self.count, self.ref(d)
        got, G = np.asarray(out["out"], dtype=np.float64), np.asarray(out["G"])
        used = np.arange(self.count) * C
        off = np.setdiff1d(np.arange(16), used)
        assert got.shape == (4, 16) and np.isfinite(got).all() and (got[:, off] == 0).all() and G.shape[0] == nv and (G[:, n:] == 0).all()
        err = np.linalg.norm(G[:, :n].T.astype(np.float64) - ref["G"].T, axis=0)
        assert (err <= ref["g_tol"]).all(), (self.name, (err / ref["g_tol"]).max())
        weights = alphas(d, self.cfg, self.count)
        on = mws.certificate(A, y, C, self.fits(d), weights, self.cfg.grouped, w, p, G=G[:, :n])      # scale and conjugate from the returned G
        for row, key in enumerate(("primal", "dual", "gap")):
            assert (np.abs(got[row, used] - on[key]) <= mws.TOL * on["mag_" + key]).all(), \
                (self.name, key, (np.abs(got[row, used] - on[key]) / on["mag_" + key]).max())
        assert np.abs(got[3, used] - on["scale"]).max() <= 1e-12 and np.array_equal(got[2, used], got[0, used] - got[1, used])
        ex = np.asarray(_host(out["excess"]), dtype=np.float64)
        assert ex.shape == (n,) and (np.abs(ex - ref["excess"]) <= ref["excess_tol"]).all(), (self.name, np.abs(ex - ref["excess"]).max())


class MultinomialWorkingSet(Cell):
    """multinomial_working_set_path on the handle, one group of floor(16 / C) weights: the scans read
    fos_multinomial_gradient_batch and fos_multinomial_kkt_scan on the full problem, fos_gather_columns copies the set's columns,
    the rounds run on handles of their own.  The reference is tests/_multinomial_ws.solve with the same L; as in WorkingSet it must
    grow its set and end certified, every scan decision further than MARGIN (relative) from its threshold and every growth step
    further than GAP.  The first set is every fifth coordinate (`initial`, no scan at X = 0) and the violators of round 1 join in
    round 2: from the scan at 0 no ladder between 0.9 and 0.1 of alpha_max grows a set on this data within ITERS iterations a round
    short of taking all 37 columns (tried on the reference alone: 0.9 .. 0.5, 0.7 .. 0.3, 0.6 .. 0.2, 0.5 .. 0.15 certify their
    first set, 0.4 .. 0.1 ends with every column); with the first set given, the first ladder tried doubles it and certifies."""
    reaches = ("fos_multinomial_gradient_batch", "fos_multinomial_kkt_scan", "fos_gather_columns")
    sized_by_panels = True
    KKT_TOL, FRACTIONS, EVERY = WorkingSet.KKT_TOL, (0.9, 0.5), 5

    def initial(self, d):
        return np.arange(0, d["n"], self.EVERY)

    def weights(self, d):
        A, y, w, p, _ = parts(d, self.cfg)
        amax = mws.alpha_max(A, y, self.cfg.classes, self.cfg.grouped, w, p)
        return [(amax * f, 0.0) for f in np.geomspace(*self.FRACTIONS, 16 // self.cfg.classes)]

    def call(self, c, P):
        xs, infos = c.fos.multinomial_working_set_path(P, None, self.weights(c.d), max_iter=ITERS, L=L_of(c.d, self.cfg), kkt_tol=self.KKT_TOL,
                                                       max_fraction=1.0, initial=self.initial(c.d).tolist(), return_info=True)
        assert len(infos) == 1
        i = infos[0]
        return dict(x=c.torch.stack([c.torch.as_tensor(x) for x in xs]), rounds=np.int64(i.rounds), sizes=np.array(i.sizes),
                    grads=np.int64(i.full_gradients), fell_back=np.bool_(i.fell_back), worst=np.float64(i.worst_excess))

    def reference(self, d):
        A, y, w, _, _ = parts(d, self.cfg)
        fits, info = mws.solve(A, y, self.cfg.classes, self.weights(d), self.cfg.grouped, ITERS, L_of(d, self.cfg), w=w, kkt_tol=self.KKT_TOL,
                               max_fraction=1.0, initial=self.initial(d))
        assert info["scan_margins"].min() >= WorkingSet.MARGIN and min(list(info["growth_gaps"]) + [np.inf]) >= WorkingSet.GAP and \
            not info["fell_back"], info
        return dict(x=np.stack(fits), rounds=np.int64(info["rounds"]), sizes=np.array(info["sizes"]), grads=np.int64(info["full_gradients"]),
                    worst=np.float64(info["worst_excess"]), margin=np.float64(info["scan_margins"].min()))

    def precondition(self, d, ref):
        assert ref["rounds"] >= 2 and ref["sizes"][-1] > ref["sizes"][0], ref["sizes"]                      # grown
        assert ref["worst"] <= 1.0 + self.KKT_TOL and ref["sizes"][-1] < d["n"], (ref["worst"], ref["sizes"])     # and certified

    def check(self, d, out):
        ref = self.ref(d)
        assert (int(out["rounds"]), list(out["sizes"]), int(out["grads"]), bool(out["fell_back"])) == \
            (int(ref["rounds"]), list(ref["sizes"]), int(ref["grads"]), False), (out, ref)
        for i in range(len(ref["x"])):
            _rel_ok(out["x"][i], ref["x"][i], (self.name, i))


W, COORD, GROUPS = PLAIN._replace(weights=True), PLAIN._replace(coord="bounds"), PLAIN._replace(groups=True)
FACTORS =PLAIN._replace(coord="factors")
LOGIT, HUBER, HINGE_W = PLAIN._replace(loss="logistic"), PLAIN._replace(loss="huber"), W._replace(loss="squared_hinge")
M3, M7G = PLAIN._replace(loss="multinomial", classes=3), PLAIN._replace(loss="multinomial", classes=7, grouped=True)

CELLS = collections.OrderedDict((c.name, c) for c in (
    Path("path16", PLAIN, 16), Path("path3", PLAIN, 3), Rhs("rhs5", PLAIN), Single("single", PLAIN), Cv("cv", PLAIN, 3, 4),
    Lbfgs("lbfgs3", PLAIN), Power("power", PLAIN),
    Path("weights_path5", W, 5), Lipschitz("weights_lipschitz", W),
    Path("factors_path16", COORD, 16),
    Path("groups_path3", GROUPS, 3), Cv("groups_cv", GROUPS, 3, 2),
    Path("logistic_path16", LOGIT, 16), Objective("logistic_objective5", LOGIT, 5),
    Cv("logistic_weights_factors_cv", LOGIT._replace(weights=True, coord="bounds"), 2, 3),
    Path("huber_path5", HUBER, 5), Objective("huber_objective16", HUBER, 16),
    Cv("hinge_weights_cv", HINGE_W, 2, 3),
    Path("multinomial3_path5", M3, 5), Objective("multinomial3_objective5", M3, 5),
    Path("multinomial7_grouped_path2", M7G, 2),
    WorkingSet("working_set", PLAIN), WorkingSet("working_set_huber", HUBER), KktExcess("kkt_excess", PLAIN),
    Controlled("controlled"),
    DualityGap("gap16", PLAIN, 16), DualityGap("gap3", PLAIN, 3), DualityGap("weights_gap5", W, 5), DualityGap("logistic_gap16", LOGIT, 16),
    DualityGap("huber_gap5", HUBER, 5), DualityGap("hinge_weights_gap5", HINGE_W, 5), DualityGap("positive_factors_gap16", FACTORS, 16),
    CertifiedPath("certified_path", PLAIN),
    ResampledPath("resampled_path5", PLAIN, "bootstrap", 5, 1, oob=True),
    ResampledPath("resampled_logistic_weights_path16", LOGIT._replace(weights=True), "binary", 4, 4),
    ResampledPath("resampled_huber_bounds_path3", HUBER._replace(coord="bounds"), "bootstrap", 3, 1),
    ResampledPath("resampled_groups_path3", GROUPS, "bootstrap", 3, 1),
    ResampledGradient("resampled_gradient16", HINGE_W), ResampledLipschitz("resampled_lipschitz", W),
    ResampledControlled("resampled_controlled"),
    MultinomialGap("multinomial3_gap5", M3, 5), MultinomialWorkingSet("multinomial7_grouped_working_set", M7G),
))
LOCKSTEP_ENTRY_POINTS = ("fos_fista_run_multi", "fos_fista_run_multi_rhs", "fos_fista_run_multi_folds", "fos_residual_batch",
                         "fos_residual_batch_rhs", "fos_residual_batch_folds", "fos_gradient_batch", "fos_gather_columns",
                         "fos_kkt_scan", "fos_power_iter", "fos_duality_gap",
                         "fos_fista_run_multi_resampled", "fos_gradient_batch_resampled", "fos_gram_apply_resampled",
                         "fos_multinomial_gradient_batch", "fos_multinomial_kkt_scan", "fos_multinomial_duality_gap")
# Every other `int fos_*(` of include/*.h that takes no part in the table, and why: an entry point a new header declares is a lockstep
# entry point with a cell, a binding entry point (binding_entry_points: a step of a move or a row of NOT_A_MOVE) or a row here -
# tests/test_handle_pairs.py fails until it is one of the three.
_EXCUSED = (
    ("no handle is involved: the version, the communicator, the proximal maps and the vector helpers of the L-BFGS loop",
     "fos_abi_version fos_comm_unique_id fos_comm_create fos_comm_mesh_create fos_comm_mesh_connect fos_comm_check fos_comm_destroy "
     "fos_comm_info fos_comm_mesh_info fos_comm_allreduce fos_prox_l1 fos_prox_l1_vec fos_prox_elastic_net fos_prox_elastic_net_vec "
     "fos_lbfgs_two_loop fos_lbfgs_two_loop_dd fos_lbfgs_direction_cols fos_lbfgs_direction_dd fos_vec_stats fos_vec_axpby "
     "fos_vec_stats_f64 fos_vec_axpby_f64 fos_vec_stats_dd fos_vec_axpby_dd fos_stream_read_probe"),
    ("creation and destruction: Ctx.fresh and the front ends make and drop every handle and state machine of the table",
     "fos_problem_create fos_problem_destroy fos_fista_create fos_fista_destroy"),
    ("a getter: Ctx.check_getters reads it after every move, and the plan before and after a refusal",
     "fos_problem_get_loss fos_problem_get_link_loss fos_problem_get_classes fos_row_weights_get fos_coord_get fos_feature_groups_get "
     "fos_problem_plan fos_fista_status_get fos_fista_get_x"),
    ("tuning and profiling of a handle's plan: no run form", "fos_problem_tune fos_problem_tune_dd fos_problem_profile "
     "fos_problem_profile_read"),
    ("a state machine's own parameters, set by the front ends before every run of a cell", "fos_fista_reset fos_fista_set_tau fos_fista_set_precise "
     "fos_fista_set_gbuf64"),
    ("a single-vector run form or step: the Single cell runs fos_fista_run beside the lockstep cells, tests/test_gpu_fista_forms.py and "
     "tests/test_gpu_armijo.py cover the forms pair by pair",
     "fos_fista_run fos_fista_run_resident fos_fista_run_history fos_fista_run_fused fos_fista_run_chip fos_fista_grad fos_fista_grad_dual "
     "fos_fista_update fos_fista_trial fos_fista_trial_batch fos_fista_run_backtracking fos_fista_run_recorded fos_fista_resume_after_stall "
     "fos_gemv_pair fos_gemv_pair_f64 fos_gemv_pair_dd fos_residual_objective"),
    ("the L-BFGS optimiser: the Lbfgs cell serves fos_lbfgs_minimize_multi (it may decline: Cell.serves), tests/test_gpu_lbfgs_driver.py and "
     "tests/test_gpu_lbfgs_multi.py cover the rest", "fos_lbfgs_minimize fos_lbfgs_minimize_multi fos_gemv_pair_dd_multi"),
    ("the Gram operator of the weighted power iteration: the weights_lipschitz cell calls it at every step (estimate_lipschitz), "
     "tests/test_gpu_weighted.py and tests/test_gpu_cluster_planned.py compare it with fp64", "fos_gram_apply"),
    ("batches of small independent problems on handles of their own: tests/test_gpu_batch.py", "fos_fista_run_batch fos_power_iter_batch"),
)
NOT_LOCKSTEP = {name: reason for reason, names in _EXCUSED for name in names.split()}


def declared_entry_points(include=INCLUDE):
    """Every `int fos_*(` that include/*.h declares, by name."""
    names = set()
    for path in sorted(glob.glob(os.path.join(include, "*.h"))):
        with open(path) as fh:
            names |= set(re.findall(r"\bint\s+(fos_\w+)\s*\(", fh.read()))
    return names


def check_entry_points(include=INCLUDE, cells=None):
    """Every entry point the headers declare is a lockstep entry point that a cell reaches, a binding entry point or a row of
    NOT_LOCKSTEP - exactly one of the three -, and every name of the two lists is declared: a new header fails here until its
    entry points have cells (or a stated reason), and a cell that drops an entry point from its reaches fails too."""
    cells = CELLS if cells is None else cells
    reached = {e for c in cells.values() for e in c.reaches}
    assert reached == set(LOCKSTEP_ENTRY_POINTS), sorted(set(LOCKSTEP_ENTRY_POINTS) ^ reached)
    declared, binding = declared_entry_points(include), binding_entry_points(include)
    assert reached <= declared, sorted(reached - declared)
    assert set(NOT_LOCKSTEP) <= declared, sorted(set(NOT_LOCKSTEP) - declared)
    assert all(reason.strip() for reason in NOT_LOCKSTEP.values())
    for a, b in ((reached, binding), (reached, set(NOT_LOCKSTEP)), (binding, set(NOT_LOCKSTEP))):
        assert a.isdisjoint(b), sorted(a & b)
    left = declared - reached - binding - set(NOT_LOCKSTEP)
    assert not left, f"declared in include/*.h, reached by no cell and not excused: {sorted(left)}"
MAY_DECLINE = {"fos_fista_run_multi", "fos_fista_run_multi_rhs", "fos_fista_run_multi_folds", "fos_residual_batch_rhs",
               "fos_residual_batch_folds", "fos_lbfgs_minimize_multi"}
PAIRS = [(x, y) for x in CELLS for y in CELLS if x != y]
PANEL_PAIRS = [(x, y) for x, y in PAIRS if CELLS[x].sized_by_panels or CELLS[y].sized_by_panels]
# the same call at another width on one handle: (wide, narrow) per configuration; C = 7 with two fits fills 14 columns, C = 3 with
# five fits 15
_NARROW = [Path("factors_path3", COORD, 3), Path("logistic_path3", LOGIT, 3), Path("multinomial7_path2", M7G._replace(grouped=False), 2),
           ResampledPath("resampled_path16", PLAIN, "bootstrap", 8, 2, oob=True)]          # (the wide twin of resampled_path5)
ALL_CELLS = dict(CELLS, **{c.name: c for c in _NARROW})
WIDTHS = {"plain": ("path16", "path3"), "factors": ("factors_path16", "factors_path3"), "logistic": ("logistic_path16", "logistic_path3"),
          "multinomial": ("multinomial7_path2", "multinomial3_path5"), "gap": ("gap16", "gap3"),
          "resampled": ("resampled_path16", "resampled_path5")}


@functools.lru_cache(maxsize=None)
def _reference(cell, name, kind, cus):
    """The fp64 reference of a cell, computed once and never modified."""
    return _frozen(ALL_CELLS[cell].reference(data(name, kind, cus)))


# ---- what the certificate refuses --------------------------------------------------------------------------------------------------
# (the condition of each guard of fos_duality_gap, a word of its message, whether a configuration of the table meets it), beside the
# shape rules every lockstep entry point shares
DUALITY_GUARDS = (
    (r"p->loss\s*==\s*FOS_LOSS_MULTINOMIAL", "fos_duality_gap: a multinomial problem is not served", lambda cfg: cfg.loss == "multinomial"),
    (r"p->coord_lo\s*\|\|\s*p->coord_hi", "fos_duality_gap: box bounds (fos_coord_bind) are bound", lambda cfg: cfg.coord == "bounds"),
    (r"has_fgroups\(p\)", "fos_duality_gap: feature groups (fos_feature_groups_bind) are bound", lambda cfg: cfg.groups),
)
FOS_ERR_UNSUPPORTED = -4


def refusal(cfg):
    """The text fos_duality_gap refuses the configuration with (its first guard that applies), or None where it is served."""
    return next((message for _, message, applies in DUALITY_GUARDS if applies(cfg)), None)


# one cell per refusing configuration of the table: the first that has it
REFUSED = collections.OrderedDict()
for _c in ALL_CELLS.values():
    if refusal(_c.cfg) and _c.cfg not in [r.cfg for r in REFUSED.values()]:
        REFUSED[_c.name] = _c


def check_duality_guards(fista=FISTA):
    """Every FOS_ERR_UNSUPPORTED of fos_duality_gap is a shape rule or a row of DUALITY_GUARDS, in the order of the source; every
    configuration of the table that a row refuses has a cell in REFUSED and every certificate cell has a configuration none does:
    a new guard fails here until it has a row."""
    body = _body(_text(fista), r"\bint\s+fos_duality_gap\s*\([^)]*\)\s*(?=\{)")
    conds = re.findall(r"if\s*\(((?:[^()]|\([^()]*\))*)\)\s*return\s+fail\(FOS_ERR_UNSUPPORTED", body)
    left = [c for c in conds if not any(re.fullmatch(r"\s*" + s + r"\s*", c) for s in SHAPE_RULES)]
    assert len(left) == len(DUALITY_GUARDS), left
    for (cond, message, _), got in zip(DUALITY_GUARDS, left):
        assert re.fullmatch(r"\s*" + cond + r"\s*", got), got
        assert message in body, message
    assert list(REFUSED) == ["factors_path16", "groups_path3", "logistic_weights_factors_cv", "multinomial3_path5",
                             "multinomial7_grouped_path2", "resampled_huber_bounds_path3", "multinomial7_path2"], list(REFUSED)
    assert {refusal(c.cfg) for c in REFUSED.values()} == {message for _, message, _ in DUALITY_GUARDS}
    for c in ALL_CELLS.values():
        if "fos_duality_gap" in c.reaches:
            assert refusal(c.cfg) is None, c.name
