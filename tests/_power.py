"""Case menu and fp64 reference of the power iteration (a helper: no tests in here), beside tests/_menu_cv.py and tests/_coord.py.

estimate_lipschitz (ref:45-60) exists in several implementations - the LDS-resident kernel, the batch kernel, the streaming
host loop with its 16-step chunks, the weighted host loop, the column-sharded host loop - each with its own copy of the
break rule |L_k - L_{k-1}| < tol.  tests/test_power_reference.py checks this menu on the CPU, tests/test_gpu_power.py runs
every entry on every route against `trajectory` below.

Reference.  `sequence` is oracle.estimate_lipschitz restated to return the whole sequence L_1..L_k, the step k at which it broke
and v after that step; `trajectory` is the same loop without the rule, keeping every iterate.  Both run in fp64 on the stored A
(rounded to bf16 for bf16 storage) from v0 as the device receives it (fp32).

Matrices.  A = scale * U diag(s) V^T from seeded orthonormal factors with s = (1, ratio, ratio/2, ratio/4, ...), rounded to the
storage type; the rounded matrix is the truth.  v0 = 3 (V_1 + mix V_2 + 1e-3 noise): with ratio = 0.95 and mix = 1.1 the
differences d_k = |L_k - L_{k-1}| fall strictly and slowly over the first 30 steps (by about 0.8 per step), which a random
Gaussian matrix does not give.  Shapes of rank one (one row, one column) converge in one step: d_1 = L, d_2 = 0 up to
rounding; their stop menu is step 1 and step 2.

Stop menu.  An entry is (name, n_iter, tol, step): tol is the geometric mean of the reference's d_{step-1} and d_step, so the
rule fires at `step`; `never` entries have tol = 0 and compare L and v after exactly n_iter steps.  An entry is valid only if
the reference meets  |d_k - tol| > 2 * TOL * L_k  for every k up to and including the break step: a run whose L_k are within
TOL (relative) of the reference's then decides the same at every step.  tol = 0 entries need no margin: |x| < 0 is false for
every x.  The margin is checked on the CPU for every entry of every case (tests/test_power_reference.py); an entry that fails
it is mended here (spectrum, mix), never dropped at run time."""
import functools
import zlib

import numpy as np

from tests import _menu, _menu_cv, _weighted

TOL = 1e-5                           # the project's standing tolerance: on L, on v (relative 2-norm), and in the margin
EPS32 = float(np.finfo(np.float32).eps)
CHUNK = 16                           # iterations the streaming loop enqueues per read-back (csrc/fos_plan.hip fos_power_iter)
STEPS = (1, 5, 16, 17, 20)           # break steps: huge tol, inside the first chunk, its last step, the first of the next, later
NEVER = (1, 2, 16, 17, 21)           # n_iter of the tol = 0 entries
RANK1_STEPS = (1, 2)
HORIZON = 32                         # steps of the reference trajectory
RATIO, MIX = 0.95, 1.1
SCALE = 40.0                         # L about 1600

# resident.hpp
RS_MAX_N, RS_MAX_M, RS_MAX_A, RS_CHUNK = 64, 4096, 10240, 8


def resident_fits(m, n):
    return 1 <= n <= RS_MAX_N and 1 <= m <= RS_MAX_M and m * (n | 1) <= RS_MAX_A


def seed(*key):
    return zlib.crc32(repr(key).encode())


def round_to(A, dtype):
    """A (fp64) as the device stores it, back in fp64."""
    A32 = np.asarray(A, dtype=np.float32)
    if dtype == "f32":
        return A32.astype(np.float64)
    u = A32.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16          # round to nearest even on the upper 16 bits
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def designed(m, n, dtype, key, ratio=RATIO, mix=MIX, scale=SCALE, row_scale=None):
    """(stored A in fp64, v0 in fp32) with the designed spectrum.  row_scale (m values, 0 allowed): the spectrum is that of
    diag(row_scale) A - the weighted route, where the reference runs on sqrt(w) * A; rows with row_scale 0 are noise."""
    rng = np.random.default_rng(seed(key, m, n, dtype))
    live = np.ones(m, dtype=bool) if row_scale is None else row_scale > 0
    ml = int(live.sum())
    r = min(ml, n)
    U = np.linalg.qr(rng.standard_normal((ml, r)))[0]
    V = np.linalg.qr(rng.standard_normal((n, r)))[0]
    s = np.ones(r)
    if r > 1:
        s[1:] = ratio * 0.5 ** np.arange(r - 1)
    A = rng.standard_normal((m, n))
    A[live] = scale * (U * s) @ V.T
    if row_scale is not None:
        A[live] /= row_scale[live, None]
    v0 = V[:, 0] + (mix * V[:, 1] if r > 1 else 0.0) + 1e-3 * rng.standard_normal(n) / np.sqrt(n)
    return round_to(A, dtype), (3.0 * v0).astype(np.float32)


def sequence(A, v0, n_iter=100, tol=1e-6):
    """oracle.estimate_lipschitz with everything it knows: (L_1..L_k as an array, k, v after step k)."""
    A = np.asarray(A, dtype=np.float64)
    v = np.array(v0, dtype=np.float64)
    v = v / np.linalg.norm(v)
    last, Ls = 0.0, []
    for _ in range(n_iter):
        w = A.T @ (A @ v)
        L = float(np.linalg.norm(w))
        with np.errstate(invalid="ignore", divide="ignore"):
            v = w / L
        Ls.append(L)
        if abs(L - last) < tol:
            break
        last = L
    return np.array(Ls), len(Ls), v


def trajectory(A, v0, steps=HORIZON):
    """(L_1..L_steps, [v_1..v_steps]) of the loop without the break rule."""
    A = np.asarray(A, dtype=np.float64)
    v = np.array(v0, dtype=np.float64)
    v = v / np.linalg.norm(v)
    Ls, Vs = [], []
    for _ in range(steps):
        w = A.T @ (A @ v)
        L = float(np.linalg.norm(w))
        v = w / L
        Ls.append(L)
        Vs.append(v)
    return np.array(Ls), Vs


def diffs(Ls):
    """d_k = |L_k - L_{k-1}| with L_0 = 0 (d[k - 1] is d_k)."""
    return np.abs(np.diff(np.concatenate([[0.0], Ls])))


def tol_for(Ls, step):
    """The tol that makes the rule fire at `step`: between d_{step-1} and d_step (geometric mean); anything above d_1 for step 1.
    A d_step that is rounding noise (rank one: d_2 = 0) counts as 1e-6 L^2 / d_{step-1}, which puts tol at 1e-3 L."""
    d = diffs(Ls)
    if step == 1:
        return 4.0 * d[0]
    L = Ls[step - 1]
    lo = d[step - 1] if d[step - 1] > 1e-9 * L else 1e-6 * L * L / d[step - 2]
    return float(np.sqrt(d[step - 2] * lo))


def margin(Ls, tol, step):
    """min over k <= step of |d_k - tol| / L_k: has to exceed 2 * TOL."""
    d = diffs(Ls)[:step]
    return float(np.min(np.abs(d - tol) / Ls[:step]))


def stop_menu(Ls, rank1=False):
    """[(name, n_iter, tol, step)] of one case."""
    out = [(f"stop{k}", max(k + 7, 2 * CHUNK + 3), tol_for(Ls, k), k) for k in (RANK1_STEPS if rank1 else STEPS)]
    out += [(f"never{k}", k, 0.0, k) for k in NEVER]
    return out


def unsafe(Ls, entry):
    """None, or why the entry is not a valid one: it does not fire where it says, or the margin condition fails."""
    name, n_iter, tol, step = entry
    if step > n_iter:
        return f"{name}: step {step} beyond n_iter {n_iter}"
    d = diffs(Ls)
    fired = next((k + 1 for k in range(n_iter) if d[k] < tol), n_iter)
    if fired != step:
        return f"{name}: the reference fires at step {fired}, not {step}"
    if tol > 0.0 and not margin(Ls, tol, step) > 2.0 * TOL:
        return f"{name}: margin {margin(Ls, tol, step):.3g} is not above 2 * TOL = {2 * TOL:.1g}"
    return None


# ---- the cases ---------------------------------------------------------------------------------------------------------
# layout: compact; strided (lda = n + 4, the padding NaN); offset (a contiguous view one element into a NaN-filled buffer);
# ragged (lda = n + 1); host (a host array handed to prepare(pad=True))
def _c(name, route, dtype, m, n, layout="compact", **kw):
    c = dict(name=name, route=route, dtype=dtype, m=m, n=n, layout=layout, rank1=min(m, n) == 1)
    c.update(kw)
    return c


def _resident(dtype):
    return [
        _c("lds_full", "resident", dtype, 157, 64),             # row stride 65: 10205 of 10240 floats
        _c("one_col", "resident", dtype, 4096, 1),              # RS_MAX_M
        _c("m2048", "resident", dtype, 2048, 5),                # 2048 * 5 = 10240 exactly
        _c("m3413", "resident", dtype, 3413, 2),                # 3413 * 3 = 10239
        _c("one_row", "resident", dtype, 1, 37),
        _c("chunk", "resident", dtype, 301, RS_CHUNK, "offset"),            # one block reduction, misaligned view
        _c("chunk_plus", "resident", dtype, 300, RS_CHUNK + 1, "strided"),  # a second one of a single column, lda > n
    ]


RESIDENT = _resident("f32") + _resident("bf16")

# one representative plan per table of tests/_menu.py; `plan`: what plan() has to say (threads, chunks, rows where named)
STREAMING = [
    _c("menu_f32", "streaming", "f32", 300, 1024, no_resident=True,
       plan=dict(path=0, tall=0, colblock=0, resident=0, geo=_menu.MENU[_menu.first_fit(_menu.MENU, "f32", 1024)][1:4])),
    _c("menu_bf16", "streaming", "bf16", 200, 1536, no_resident=True,
       plan=dict(path=0, tall=0, colblock=0, resident=0, geo=_menu.MENU[_menu.first_fit(_menu.MENU, "bf16", 1536)][1:4])),
    _c("tall_thread", "streaming", "f32", 20001, 7, no_resident=True, plan=dict(path=0, tall=1, colblock=0, resident=0)),
    _c("tall_lanes", "streaming", "f32", 1001, 100, no_resident=True,
       plan=dict(path=0, tall=1, colblock=0, resident=0, geo=(256, 32, 0))),
    _c("wide", "streaming", "f32", 96, 20000, plan=dict(path=0, tall=0, colblock=0, resident=0, geo=(512, 16, 1))),
    _c("wide_blocks", "streaming", "f32", 3, 32772, plan=dict(path=0, colblock=1, resident=0)),
    _c("two_pass", "streaming", "f32", 513, 1023, "ragged", plan=dict(path=1, resident=0)),
    _c("padded", "streaming", "f32", 200, 1030, "host", n_dev=1032, plan=dict(path=0, tall=0, colblock=0, resident=0)),
]


def normalize_classes(cases=None):
    """The trip classes of power_normalize_kernel's 1024-stride loops the streaming cases reach (device width n_dev)."""
    out = set()
    for c in STREAMING if cases is None else cases:
        n = c.get("n_dev", c["n"])
        if n < 64:
            out.add("below_a_wave")
        if 1025 <= n <= 2047:
            out.add("partial_second_trip")
        if n % 1024 == 0:
            out.add("whole_trips")
    return out


NORMALIZE_CLASSES = {"below_a_wave", "partial_second_trip", "whole_trips"}


def _weighted_cases():
    out = []
    for dtype in ("f32", "bf16"):
        for (name, s), kind in zip(_menu_cv.shapes(dtype, 256).items(), ("counts", "spread")):
            if name in ("one_tile", "edges"):
                out.append(_c(name, "weighted", dtype, s["m"], s["n"], "host", weights=kind))
    return out


WEIGHTED = _weighted_cases()

# the narrowest width a column-sharded problem is served at: one chunk above the chunk-per-lane rows (tests/_menu._cb_cases)
COLS = [_c("cols", "cols", "f32", 161, _menu.TLR_MAX_N["f32"] + _menu.EPC["f32"])]

ALL = RESIDENT + STREAMING + WEIGHTED + COLS


def case_id(c):
    return f"{c['route']}-{c['name']}-{c['dtype']}"


def weights_of(c):
    """The fp64 weights of a weighted case as the device stores them (fp32), or None."""
    if "weights" not in c:
        return None
    return _weighted.as_stored(_weighted.weights(c["weights"], c["m"], seed(c["name"]) % 1000))


@functools.lru_cache(maxsize=None)
def _built(cid, scale):
    c = next(x for x in ALL if case_id(x) == cid)
    w = weights_of(c)
    A, v0 = designed(c["m"], c["n"], c["dtype"], cid, scale=scale, row_scale=None if w is None else np.sqrt(w))
    B = A if w is None else np.sqrt(w)[:, None] * A
    Ls, Vs = trajectory(B, v0)
    for a in (A, v0, Ls, *Vs):
        a.setflags(write=False)
    return A, v0, Ls, Vs


def build(c, scale=SCALE):
    """(stored A fp64, v0 fp32, L_1..L_HORIZON, [v_1..]) of a case, computed once and shared (read-only).  The trajectory of a
    weighted case is that of sqrt(w) * A."""
    return _built(case_id(c), float(scale))


def menu(c):
    return stop_menu(build(c)[2], c["rank1"])


# ---- the batch: the resident shapes in one call, one tol ----------------------------------------------------------------
BATCH_TOL = 0.05
BATCH_N_ITER = 2 * CHUNK + 3
BATCH_LDV = 80                        # larger than every n
_BATCH_STEPS = {"lds_full": 16, "one_col": 2, "m2048": 5, "m3413": 17, "one_row": 2, "chunk": 20, "chunk_plus": 9}


@functools.lru_cache(maxsize=None)
def batch_scale(cid):
    """The scale at which member `cid` breaks at its own step under BATCH_TOL: d_k is linear in scale^2."""
    c = next(x for x in RESIDENT if case_id(x) == cid)
    if c["rank1"]:
        return 10.0                   # d_1 = L = 100, d_2 = 0: step 2, with a margin of BATCH_TOL / L = 5e-4
    return SCALE * float(np.sqrt(BATCH_TOL / tol_for(build(c)[2], _BATCH_STEPS[c["name"]])))


def batch_members(dtype):
    """[(case, step under BATCH_TOL, scale)] of one batch call; the last member repeats the first (same a_offset)."""
    ms = [(c, _BATCH_STEPS[c["name"]], batch_scale(case_id(c))) for c in RESIDENT if c["dtype"] == dtype]
    return ms + [ms[0]]


BATCH_ENTRIES = [("stops", BATCH_N_ITER, BATCH_TOL), ("never17", CHUNK + 1, 0.0)]
