"""Inputs of the L-BFGS driver tests (a helper: no tests in here).

Every case is a small least-squares problem on which the oracle's L-BFGS (oracle/fos_oracle.py::lbfgs_minimize, SciPy's
unbounded L-BFGS-B) takes a known route: a given exit, line searches of a given length, a ring of pairs that wraps.
tests/test_lbfgs_driver_cases.py runs the oracle on every case on the CPU, twice - the second time with the rows of A and b
permuted, i.e. with every sum over the rows taken in another order - and requires the same (nit, nfev, task) and iterates
equal to 1e-8: a case on which the route depends on the summation order cannot be compared with a device run and does not get
in.  The same test asserts the coverage the cases are there for.  tests/test_gpu_lbfgs_driver.py runs the native drivers on
them.

A case: name, kind ("f32" / "bf16" storage of A), m, n, cols (log10 range of the column scales of A), a2, bscale (b is
multiplied by it), max_iter, tol, x0 (None: zero start, else the seed of a start point), nonfinite (None, or how the data is
spoiled: "nan_b", "nan_A", "inf_b")."""
import numpy as np

from oracle import fos_oracle as orc

TASKS = ("CONVERGENCE: NORM_OF_PROJECTED_GRADIENT_<=_PGTOL", "CONVERGENCE: REL_REDUCTION_OF_F_<=_FACTR*EPSMCH",
         "STOP: TOTAL NO. OF ITERATIONS REACHED LIMIT", "ABNORMAL_TERMINATION_IN_LNSRCH")


def _c(name, kind, m, n, cols=(-1, 1), a2=1e-3, bscale=1.0, max_iter=12, tol=1e-6, x0=None, nonfinite=None, zero_b=False):
    return dict(name=name, kind=kind, m=m, n=n, cols=cols, a2=a2, bscale=bscale, max_iter=max_iter, tol=tol, x0=x0,
                nonfinite=nonfinite, zero_b=zero_b)


# length classes: n < 2048 divisible by 4 (div64), not divisible (ragged33, ragged515), the switch to the whole-chip
# direction (n2047, n2048, n2049), ragged above 4096 (ragged4101); bf16 storage on div64 and n2048
CASES = [
    # ---- exits -------------------------------------------------------------------------------------------------------
    _c("div64-zero", "f32", 300, 64, zero_b=True),                                   # task 0 at nit = 0
    _c("div64-tol", "f32", 300, 64, tol=3.0, max_iter=40),                          # task 0 at nit > 0
    _c("div64-conv", "f32", 300, 64, cols=(0, 0), a2=5.0, max_iter=60),            # task 1
    _c("div64-limit", "f32", 300, 64, max_iter=3),                                  # task 2
    _c("div64-b1e20", "f32", 300, 64, bscale=1e20),                                 # task 3 from finite data
    _c("div64-iter0", "f32", 300, 64, cols=(-2, 2), a2=1e-4, max_iter=0),
    _c("div64-iter1", "f32", 300, 64, cols=(-2, 2), a2=1e-4, max_iter=1),
    # ---- long line searches and the ring, per length class -----------------------------------------------------------------
    _c("div64-b1e4", "f32", 300, 64, bscale=1e4),
    _c("div64-b1e8", "f32", 300, 64, bscale=1e8),
    _c("div64-ring", "f32", 300, 64, cols=(-2, 2), a2=1e-4, max_iter=30),
    _c("div64-bf16-b1e8", "bf16", 300, 64, bscale=1e8),
    _c("div64-start", "f32", 300, 64, x0=11, max_iter=15),                          # non-zero start point (raw ABI)
    _c("ragged33-b1e4", "f32", 200, 33, bscale=1e4),
    _c("ragged33-b1e8", "f32", 200, 33, bscale=1e8),
    _c("ragged33-ring", "f32", 200, 33, cols=(-1.5, 1.5), max_iter=25),
    _c("ragged515-b1e8", "f32", 800, 515, bscale=1e8),
    _c("ragged515-b1e4", "f32", 800, 515, bscale=1e4),
    _c("ragged515-b1e20", "f32", 800, 515, bscale=1e20),
    _c("n2047-b1e4", "f32", 500, 2047, bscale=1e4, max_iter=8),
    _c("n2047-b1e8", "f32", 500, 2047, bscale=1e8, max_iter=6),
    _c("n2048-b1e4", "f32", 500, 2048, bscale=1e4, max_iter=8),
    _c("n2048-b1e8", "f32", 500, 2048, bscale=1e8, max_iter=6),
    _c("n2048-bf16-b1e4", "bf16", 500, 2048, bscale=1e4, max_iter=8),
    _c("n2048-ring", "f32", 500, 2048, a2=1e-4, max_iter=16),
    _c("n2048-b1e20", "f32", 500, 2048, bscale=1e20),
    _c("n2049-b1e4", "f32", 500, 2049, bscale=1e4, max_iter=8),
    _c("n2049-b1e8", "f32", 500, 2049, bscale=1e8, max_iter=6),
    _c("ragged4101-b1e4", "f32", 250, 4101, bscale=1e4, max_iter=8),
    _c("ragged4101-b1e8", "f32", 250, 4101, bscale=1e8, max_iter=6),
    # ---- non-finite data: bounded by MAXLS = 20 evaluations ------------------------------------------------------------------
    _c("div64-nan-b", "f32", 300, 64, nonfinite="nan_b"),
    _c("div64-nan-A", "f32", 300, 64, nonfinite="nan_A"),
    _c("div64-inf-b", "f32", 300, 64, nonfinite="inf_b"),
    _c("n2048-nan-b", "f32", 500, 2048, nonfinite="nan_b"),
]
BY_NAME = {c["name"]: c for c in CASES}

LENGTH_CLASSES = {"div": lambda c: c["n"] < 2048 and c["n"] % 4 == 0 and c["kind"] == "f32",
                  "ragged": lambda c: c["n"] < 2048 and c["n"] % 4 != 0,
                  "n2047": lambda c: c["n"] == 2047, "n2048": lambda c: c["n"] == 2048 and c["kind"] == "f32",
                  "n2049": lambda c: c["n"] == 2049, "ragged>4096": lambda c: c["n"] > 4096 and c["n"] % 4 != 0,
                  "bf16": lambda c: c["kind"] == "bf16"}


def _round_storage(A, kind):
    """A as the device stores it, in fp64."""
    A32 = A.astype(np.float32)
    if kind == "bf16":
        import torch
        return torch.from_numpy(A32).to(torch.bfloat16).to(torch.float64).numpy(), A32
    return A32.astype(np.float64), A32


def data(c):
    """(A32: what is handed to the library (fp32; bf16 cases are rounded by it), A64: A as stored, b32, x0 (fp64 or None))."""
    seed = sum(ord(ch) for ch in c["name"].split("-")[0]) + 1000 * c["m"] + c["n"]
    rng = np.random.default_rng(seed)
    m, n = c["m"], c["n"]
    A = rng.standard_normal((m, n)) * np.logspace(c["cols"][0], c["cols"][1], n)
    A64, A32 = _round_storage(A, c["kind"])
    xt = np.zeros(n)
    idx = rng.choice(n, max(1, n // 20), replace=False)
    xt[idx] = rng.standard_normal(idx.size)
    b = (A64 @ xt + 0.1 * rng.standard_normal(m)) * c["bscale"]
    if c["zero_b"]:
        b[:] = 0.0
    b32 = b.astype(np.float32)
    assert np.isfinite(b32).all()
    if c["nonfinite"] == "nan_b":
        b32[m // 3] = np.nan
    elif c["nonfinite"] == "inf_b":
        b32[m // 3] = np.inf
    elif c["nonfinite"] == "nan_A":
        A32 = A32.copy()
        A32[m // 2, n // 2] = np.nan
        A64 = A64.copy()
        A64[m // 2, n // 2] = np.nan
    x0 = None if c["x0"] is None else np.random.default_rng(c["x0"]).standard_normal(n) * 0.05
    return A32, A64, b32, x0


def oracle(c, A64, b32, x0=None, perm=None):
    """The oracle's run: dict(nit, nfev, task (index into TASKS), x, f, iterates, evals (fg evaluations of every line search
    that ended in an iterate))."""
    b = b32.astype(np.float64)
    A = A64
    if perm is not None:
        A, b = A64[perm], b[perm]
    count = [0]
    evals, iterates = [], []
    last = [1]

    def fg(x):
        count[0] += 1
        with np.errstate(all="ignore"):
            g, rr = orc.gram_gradient(A, x, b, c["a2"])
            return 0.5 * rr + 0.5 * c["a2"] * float(x @ x), g

    def cb(xk):
        iterates.append(xk)
        evals.append(count[0] - last[0])
        last[0] = count[0]

    start = np.zeros(c["n"]) if x0 is None else x0
    with np.errstate(all="ignore"):
        r = orc.lbfgs_minimize(fg, start, maxiter=c["max_iter"], pgtol=c["tol"], callback=cb)
    return dict(nit=r["nit"], nfev=r["nfev"], task=TASKS.index(r["task"]), x=r["x"], f=r["f"], iterates=iterates, evals=evals)


# ---- lockstep groups: columns of one B that take different exits in one call ------------------------------------------------
def group(m, n, nv, seed, kind="f32"):
    """(A32, A64, B32 (m x nv), roles): column 0 ordinary, 1 zero, 2 scaled 1e8; with 16 columns also 3 scaled 1e20, 4 scaled
    1e4, 5 and 9 a duplicated pair, the rest ordinary with growing noise."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n)) * np.logspace(-1, 1, n)
    A64, A32 = _round_storage(A, kind)
    B = np.empty((m, nv))
    for j in range(nv):
        xt = np.zeros(n)
        idx = rng.choice(n, max(1, n // 20), replace=False)
        xt[idx] = rng.standard_normal(idx.size)
        B[:, j] = A64 @ xt + 0.1 * (1 + j % 4) * rng.standard_normal(m)
    roles = ["ordinary"] * nv
    B[:, 1], roles[1] = 0.0, "zero"
    B[:, 2] *= 1e8
    roles[2] = "1e8"
    if nv >= 16:
        B[:, 3] *= 1e20
        roles[3] = "1e20"
        B[:, 4] *= 1e4
        roles[4] = "1e4"
        B[:, 9] = B[:, 5]
        roles[5] = roles[9] = "twin"
    return A32, A64, B.astype(np.float32), roles


GROUPS = {"group3-n512": dict(m=600, n=512, nv=3, seed=31), "group16-n512": dict(m=600, n=512, nv=16, seed=32),
          "group3-n2052": dict(m=500, n=2052, nv=3, seed=33), "group16-n2052": dict(m=500, n=2052, nv=16, seed=34)}
GROUP_A2, GROUP_MAX_ITER, GROUP_TOL = 1e-3, 10, 1e-6
