"""Probes of the packed gradient pass (csrc/gemv_packed.hpp; ensure_packed and launch_pass_packed in csrc/fos_plan.hip) - a
helper: no tests in here, beside tests/_forms.py and tests/_armijo.py.

The pass claims A = P + D bit for bit: P the 28-bit copy with an in-window placeholder for every element outside the window,
D the exception list (+true, -placeholder) applied by pk_bprime_kernel (b' = b - D y) before and pk_dtr_kernel (slab 0 += D^T r)
after the streaming loop.  A norm over the whole gradient cannot see a below-window element served as its placeholder, so this
file holds PROBES - a (b, y, alpha2) for Problem.gemv_pair whose answer is known element by element - with the MATRICES whose
exception positions and counts are stated, the CHECKS with their derived bounds, and a NumPy MODEL of the three launches that
takes a named fault.  tests/test_packed_probes.py proves the bounds on the model and shows every fault caught;
tests/test_gpu_packed_probes.py runs the same checks on the device.

row probe i      y = 0, b = -e_i: r = e_i, g = row i of A.  In-window elements bit for bit (one slab holds a non-zero, every
                 other term is a * 0); an exception through two fp32 roundings (check_row).
column probe j   b = None, y = s e_j, s a power of two: r = s * column j exactly, rr = s^2 sum A_ij^2 (check_col).
sum probes       on `heavy`, whose values are dyadic with few bits: every partial sum of every order is exact in fp32
                 (asserted here), so g and rr are compared bit for bit with the fp64 value (sum_probe_b, sum_probe_y).
"""
import math

import numpy as np

from tests.test_packed_format import CPT, MAX_EXCEPTIONS, pack, decode, window

U = 2.0 ** -24                    # unit roundoff of fp32
TOL = 1e-5                        # the project's parity tolerance (tests/test_gpu_parity.py)
F32 = np.finfo(np.float32)
SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-30, -1e-30, F32.tiny, 1e30, -1e30, F32.max, 300.0, -5000.0], dtype=np.float32)


def threads_of(n):
    """The geometry ensure_packed lays the copy out for."""
    return 512 if n <= 8192 else 1024


def sampled_rows(m, n):
    """The rows whose exponents ensure_packed counts for the window (a hipMemcpy2D of every stride-th row)."""
    srows = min(m, max(1, (4 << 20) // n))
    return np.arange(srows) * (m // srows)


def exceptions(A, e0=None):
    """(out mask, placeholder bits, e0) of pk::in_window / pk::placeholder - also for a matrix the packer refuses."""
    bits = np.ascontiguousarray(A, dtype=np.float32).view(np.uint32)
    ex = (bits >> 23) & 0xFF
    if e0 is None:
        e0 = window(bits)
    out = (ex < e0) | (ex > e0 + 15)
    ph = (bits & np.uint32(0x807FFFFF)) | (np.where(ex < e0, e0, e0 + 15).astype(np.uint32) << 23)
    return out, ph, e0


class Case:
    """A matrix with what the checks need: the exception mask, the placeholders (as floats), the fp64 copy and, where the
    packer takes it, pack()'s output.  planted: the (row, col) put there on purpose."""

    def __init__(self, name, A, planted=(), packs=True):
        self.name, self.A = name, np.ascontiguousarray(A, dtype=np.float32)
        self.m, self.n = self.A.shape
        self.threads = threads_of(self.n)
        self.planted = sorted(set(planted))
        self.out, ph, self.e0 = exceptions(self.A)
        self.pv = ph.view(np.float32)
        self.packed = pack(self.A, self.threads)
        assert (self.packed is not None) == packs, (name, "packs" if packs else "is refused", int(self.out.sum()), self.A.size)
        if packs:
            rows, cols = self.packed[1], self.packed[2]
            assert self.packed[5] == self.e0 and np.array_equal(np.flatnonzero(self.out), rows * self.n + cols)
        self.share = float(self.out.sum()) / self.A.size
        self._A64 = self._reach = None

    @property
    def A64(self):
        if self._A64 is None:
            self._A64 = self.A.astype(np.float64)
        return self._A64

    @property
    def reach(self):
        """The largest magnitude by which element (i, k) can multiply a residual on its way into g_k: |A_ik|, and for an
        exception |pv| + |tv - pv| <= |tv| + 2 |pv| (its placeholder in the pass, its correction in D^T r)."""
        if self._reach is None:
            self._reach = np.where(self.out, np.abs(self.A64) + 2.0 * np.abs(self.pv.astype(np.float64)), np.abs(self.A64))
        return self._reach

    def exception_rows(self):
        return sorted({r for r, _ in self.planted})

    def exception_cols(self):
        return sorted({c for _, c in self.planted})


# ---- matrices -------------------------------------------------------------------------------------------------------------
T16 = 2                           # the thread of `edges` whose 16 columns all hold a special value, in one row


def edges(m, n):
    """standard_normal with every value of SPECIALS planted, one planted element per column (so every column has a scale s):
    all 16 positions of thread T16 in the middle row (16 exceptions of one thread and one row: the slot hand-out of
    pack_rows_kernel and the host's re-sort); the first and last column of thread 0 and the first and last column of the last
    live thread (beside the dead ones where n < 16 * threads) in the first row; the last row; and the last row but one, which
    with the last row falls into the clamped tail of a burst wherever a workgroup's row count is no multiple of R."""
    assert n % CPT == 0 and n >= 5 * CPT
    rng = np.random.default_rng(1000 + 31 * m + n)
    A = rng.standard_normal((m, n)).astype(np.float32)
    tl = n // CPT - 1
    mid, last, tail = m // 2, m - 1, max(m - 2, 0)
    put = [(mid, CPT * T16 + e, v) for e, v in enumerate(np.resize(SPECIALS, CPT))]
    put += [(0, 0, 0.0), (0, CPT - 1, 1e30), (0, CPT * tl, -1e-40), (0, n - 1, 300.0)]
    put += [(last, 1, -5000.0), (last, CPT + 1, F32.max), (last, CPT * tl + 7, -0.0), (last, n - 2, F32.tiny)]
    put += [(tail, 3 * CPT + 1, 1e-30), (tail, n - 3, -1e30), (tail, CPT * tl + 1, 1e-40)]
    assert len({c for _, c, _ in put}) == len(put)
    # (a matrix of few elements would be refused with all 27: the cap leaves (1, 16384) 16 exceptions, so it gets the first 12 -
    # every value once, in thread T16 - and keeps 4 for what standard_normal itself puts outside the window)
    put = put[:max(0, min(len(put), int(MAX_EXCEPTIONS * m * n) - 4))]
    for r, c, v in put:
        A[r, c] = v
    case = Case(f"edges{m}x{n}", A, [(r, c) for r, c, _ in put])
    assert all(case.out[r, c] for r, c in case.planted)
    case.probe_rows = list(range(m)) if m <= 37 else sorted({0, m // 3, mid, tail, last})
    case.probe_cols = sorted(set(case.exception_cols()) | set(range(CPT * T16, CPT * T16 + CPT)) | {0, n - 1})
    return case


HEAVY_SHAPE = (260, 4112)
HEAVY_ROW, HEAVY_COL, CLEAN_ROW, CLEAN_COL = 100, 2000, 7, 3000
HEAVY_FULL_THREADS = (10, 11)     # the two threads of HEAVY_ROW whose 16 columns are all exceptions


def heavy(extra=0):
    """Dyadic values for the sum probes, window 128 .. 143 (values 2 .. < 2^17): +-8 everywhere (binade 130), +-2 and +-4 in a
    block of columns of their own and 2^15 on 400 scattered elements (they pin the window: without the first the window
    130 .. 145 would hold as much, without the second 126 .. 141), and as exceptions 0 (placeholder 2 - as large as the
    values around it), +-1 (placeholder +-2) and +-2^17 (placeholder +-2^16):
      HEAVY_ROW   200 exceptions (150 zeros, 40 of +-1, 10 of +-2^17), 16 of them filling thread 10 and 16 thread 11;
      HEAVY_COL   130 exceptions among the 260 rows (92 zeros, 30 of +-1, 8 of +-2^17 - in rows where the second sum probe's
                  residual is small, or their products alone would leave 24 bits);
      600 + extra more, each in a column of its own, outside HEAVY_ROW's exception columns (they would break the 8-bit
      granularity of the second probe's residual); CLEAN_ROW and CLEAN_COL hold none.
    extra = 0: 930 exceptions, 0.87e-3 of m * n - packed.  extra = 360: 1.2e-3 - refused."""
    m, n = HEAVY_SHAPE
    rng = np.random.default_rng(7)
    A = (8.0 * rng.choice([-1.0, 1.0], size=(m, n))).astype(np.float32)
    block = np.arange(3500, 3900)
    A[:, block] = (rng.choice([2.0, 4.0], size=(m, block.size)) * rng.choice([-1.0, 1.0], size=(m, block.size))).astype(np.float32)
    big = np.float32(2.0 ** 17)
    # HEAVY_ROW
    free = np.setdiff1d(np.arange(n), np.concatenate([np.arange(160, 192), [HEAVY_COL, CLEAN_COL], block]))
    J = np.sort(np.concatenate([np.arange(160, 192), rng.choice(free, 168, replace=False)]))
    kinds = rng.permutation(np.array([0.0] * 150 + [1.0, -1.0] * 20 + [big, -big] * 5, dtype=np.float32))
    A[HEAVY_ROW, J] = kinds
    planted = [(HEAVY_ROW, int(c)) for c in J]
    # the second sum probe's y (sum_probe_y): +-1 and +-2 on J, the 10 products with +-2^17 cancelling in pairs
    y = np.zeros(n)
    y[J] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=J.size)
    above = J[np.abs(kinds) == big]
    y[above] = np.sign(kinds[np.abs(kinds) == big]) * np.resize([1.0, -1.0], above.size)
    # 400 x 2^15 and the scattered exceptions: columns of their own, outside J, the block and the reserved ones
    rows_free = np.setdiff1d(np.arange(m), [HEAVY_ROW, CLEAN_ROW])
    cols_free = rng.permutation(np.setdiff1d(np.arange(n), np.concatenate([J, [HEAVY_COL, CLEAN_COL], block])))
    pins, scat = cols_free[:400], cols_free[400:1000 + extra]
    A[rng.choice(rows_free, pins.size), pins] = np.float32(2.0 ** 15)
    srows = rng.choice(rows_free, scat.size)
    A[srows, scat] = np.resize(np.array([0.0, 1.0, big, 0.0, -1.0, -big], dtype=np.float32), scat.size)
    planted += [(int(r), int(c)) for r, c in zip(srows, scat)]
    # HEAVY_COL: its +-2^17 go where |r| of the second probe is smallest and not zero
    r2 = A[:, J].astype(np.float64) @ y[J]
    order = [int(i) for i in np.argsort(np.abs(r2), kind="stable") if i not in (HEAVY_ROW, CLEAN_ROW) and r2[i] != 0.0]
    rows_big = order[:8]
    rest = rng.permutation(np.setdiff1d(rows_free, rows_big))[:122]
    A[rows_big, HEAVY_COL] = np.resize([big, -big], 8)
    A[rest, HEAVY_COL] = rng.permutation(np.array([0.0] * 92 + [1.0, -1.0] * 15, dtype=np.float32))
    planted += [(int(r), HEAVY_COL) for r in list(rows_big) + list(rest)]
    case = Case("heavy" if not extra else "heavy_over_cap", A, planted, packs=not extra)
    assert case.e0 == 128 and int(case.out.sum()) == len(case.planted) == 930 + extra
    assert int(case.out[HEAVY_ROW].sum()) == 200 and int(case.out[:, HEAVY_COL].sum()) == 130 > 2 * 64
    for t in HEAVY_FULL_THREADS:
        assert case.out[HEAVY_ROW, CPT * t:CPT * t + CPT].all()
    assert not case.out[CLEAN_ROW].any() and not case.out[:, CLEAN_COL].any()
    tv = case.A[case.out]
    assert (tv == 0).any() and (np.abs(tv) == 1).any() and (np.abs(tv) == big).any()      # zeros, below and above the window
    if extra:
        assert 1.19e-3 < case.share < 1.25e-3
    else:
        assert 0.8e-3 <= case.share <= MAX_EXCEPTIONS
    case.y_probe = y
    case.probe_rows = sorted({0, CLEAN_ROW, HEAVY_ROW, rows_big[0], int(srows[2]), m - 1})
    case.probe_cols = sorted(set(range(CPT * HEAVY_FULL_THREADS[0], CPT * HEAVY_FULL_THREADS[0] + CPT)) |
                             {0, n - 1, HEAVY_COL, CLEAN_COL, int(pins[0]), int(scat[2]), int(scat[1])})
    return case


def scaled(name):
    """`low` and `high`: the two ends of the window's range.  Every value is finite; denormals (low) and the top binades
    (high) are exceptions."""
    k, e0 = {"low": (-112, 2), "high": (124, 238)}[name]
    A = (np.random.default_rng(0).standard_normal(HEAVY_SHAPE) * 2.0 ** k).astype(np.float32)
    assert np.isfinite(A).all()
    case = Case(name, A)
    assert case.e0 == e0 and 1.0e-4 < case.share < 1.4e-4, (case.e0, case.share)
    rows, cols = np.nonzero(case.out)
    case.planted = [(int(rows[q]), int(cols[q])) for q in np.linspace(0, len(rows) - 1, 12).astype(int)]
    case.probe_rows = sorted(set(case.exception_rows()) | {0, case.m // 3, case.m - 1})
    case.probe_cols = sorted(set(case.exception_cols()) | set(range(CPT * T16, CPT * T16 + CPT)) | {0, case.n - 1})
    return case


UNSAMPLED_SHAPE = (515, 16384)


def unsampled():
    """Row 1 carries 7000 elements times 2^40 - 0.83e-3 of m * n - and is not among the rows the window is chosen from."""
    m, n = UNSAMPLED_SHAPE
    rng = np.random.default_rng(5)
    A = rng.standard_normal((m, n)).astype(np.float32)
    cols = np.sort(rng.choice(n, 7000, replace=False))
    A[1, cols] *= np.float32(2.0 ** 40)
    case = Case("unsampled", A, [(1, int(cols[0])), (1, int(cols[-1])), (1, int(cols[3500]))])
    rows = sampled_rows(m, n)
    assert 1 not in rows and 0 in rows and 2 in rows
    assert window(case.A[rows].view(np.uint32)) == case.e0          # the sample gives the window of the whole matrix
    assert int(case.out[1].sum()) >= 7000 and 0.9e-3 < case.share < MAX_EXCEPTIONS
    case.probe_rows, case.probe_cols = [0, 1, 2], [int(cols[3500])]
    return case


_CASES = {}


def case(name):
    """The matrices by name, built once: edges<m>x<n>, heavy, heavy_over_cap, low, high, unsampled."""
    if name not in _CASES:
        if name.startswith("edges"):
            m, n = name[5:].split("x")
            _CASES[name] = edges(int(m), int(n))
        else:
            _CASES[name] = {"heavy": heavy, "heavy_over_cap": lambda: heavy(360), "low": lambda: scaled("low"),
                            "high": lambda: scaled("high"), "unsampled": unsampled}[name]()
    return _CASES[name]


# ---- probes ---------------------------------------------------------------------------------------------------------------
def row_probe(case, i):
    """(b, y, alpha2): r = e_i."""
    b = np.zeros(case.m, dtype=np.float32)
    b[i] = -1.0
    return b, np.zeros(case.n, dtype=np.float32), 0.0


def check_row(case, i, g):
    """g of row probe i.  In-window: the bits of A_ij.  An exception (true value tv, placeholder pv): the slab of row i's
    workgroup holds pv, slab 0 receives (float)(slab0 + (tv - pv)) - one fp32 rounding of a quantity no larger than
    |tv| + |pv| - and the slab sum is the second, of a quantity no larger than |tv| (1 + 2^-23): at most
    2 * 2^-24 * (|tv| + |pv|) from tv.  A zero comes back as 0.0: pv - pv.  -> the worst error / bound."""
    g = np.asarray(g, dtype=np.float32)
    row, out = case.A[i], case.out[i]
    same = g.view(np.uint32) == row.view(np.uint32)
    assert same[~out].all(), (case.name, i, "in-window elements", np.flatnonzero(~same & ~out)[:8])
    tv, pv = row[out].astype(np.float64), case.pv[i][out].astype(np.float64)
    err, bound = np.abs(g[out].astype(np.float64) - tv), 2.0 * U * (np.abs(tv) + np.abs(pv))
    assert (err <= bound).all(), (case.name, i, "exceptions", np.flatnonzero(out)[err > bound][:8], (err / bound).max())
    assert (g[out][tv == 0.0] == 0.0).all(), (case.name, i, "a zero came back as", g[out][tv == 0.0])
    return float((err / bound).max()) if err.size else 0.0


def col_scale(case, j):
    """The power of two s of column probe j, inside 2^-120 .. 2^120: the one that brings the column's largest element into
    [1, 2) (the residual is then of order one and the gradient of the order of A), raised as far as its smallest non-zero needs
    to stay a normal number; every product s A_ij is then a normal fp32 number (asserted), so it is exact.  1 for a zero column."""
    col = np.abs(case.A64[:, j])
    nz = col[col > 0]
    if nz.size == 0:
        return 1.0
    k = max(-math.floor(math.log2(nz.max())), math.ceil(-126 - math.log2(nz.min())))
    k = int(min(120, max(-120, k)))
    s = 2.0 ** k
    assert 2.0 ** -126 <= nz.min() * s and nz.max() * s < 2.0 ** 127, (case.name, j, k)
    return s


def col_probe(case, j):
    y = np.zeros(case.n, dtype=np.float32)
    y[j] = col_scale(case, j)
    return None, y, 0.0


def check_col(case, j, g, rr):
    """g and rr of column probe j.  In-window element: P_i . y is s A_ij plus zeros - exact - and rr sums the fp64 squares,
    exact too, in some order: rel = m * 2^-52.  Exception (tv, pv): b'_i = (float)(-s (tv - pv)) is the one fp32 rounding of
    b', at most u s |tv - pv| with u = 2^-24; r_i = s pv - b'_i the one of s, at most u |r_i| <= u (1 + u) (s |tv| + u s |tv - pv|):
        |r_i - s tv| <= d_i = u s (|tv - pv| + |tv|) (1 + 2^-20)       (the factor: second-order terms and the fp64 roundings)
    and rr moves by at most sum_i (2 s |tv| d_i + d_i^2).  Wherever the reference leaves no room for an overflow (below), g is
    finite and within TOL of the oracle in norm, after the sum_i |A_ik| d_i that the exception rows' residuals may carry into
    g_k has been taken off every element's error."""
    s = col_scale(case, j)
    col, out = case.A64[:, j], case.out[:, j]
    rr_ref = math.fsum((s * col) ** 2)
    tv, pv = col[out], case.pv[:, j][out].astype(np.float64)
    d = U * s * (np.abs(tv - pv) + np.abs(tv)) * (1.0 + 2.0 ** -20)
    bound = case.m * 2.0 ** -52 * rr_ref + float(np.sum(2.0 * s * np.abs(tv) * d + d * d))
    assert abs(rr - rr_ref) <= bound, (case.name, j, "rr", rr, rr_ref, abs(rr - rr_ref) / bound)
    with np.errstate(over="ignore", invalid="ignore"):
        g_ref = case.A64.T @ (s * col)
        # d_i reaches g_k times |A_ik|: with 1e-40 and 1e30 in one row of `edges` that is 1e28 in a gradient of 1e12, from a
        # residual that is right to 2^-24 of s |pv|.  The raw pass has no such term, a norm-wise bound (u |A_i| |y|) dwarfs it.
        slack = np.zeros(case.n)
        slack[:] = np.abs(case.A64[out]).T @ d if out.any() else 0.0
        # Where g has to be finite - decided by the reference alone, never by g: every product that reaches g_k is a_ik r_i with
        # |a_ik| <= |A_ik| (in-window), or pv r_i and (tv - pv) r_i of an exception, |.| <= |pv| and |tv| + |pv|; while the sum
        # of their magnitudes stays below the largest fp32 number no partial sum, in any order, can overflow.
        r_abs = np.abs(s * col)
        r_abs[out] += d
        room = case.reach.T @ r_abs < 0.99 * float(F32.max)
    g64 = np.asarray(g, dtype=np.float64)
    assert np.isfinite(g64[room]).all(), (case.name, j, "g is not finite in", np.flatnonzero(room & ~np.isfinite(g64))[:8])
    fin = room
    if fin.any() and np.linalg.norm(g_ref[fin]) > 0:
        over = np.maximum(np.abs(g64[fin] - g_ref[fin]) - slack[fin], 0.0)
        rel = float(np.linalg.norm(over) / np.linalg.norm(g_ref[fin]))
        assert rel < TOL, (case.name, j, "g", rel)
    return abs(rr - rr_ref) / bound if bound > 0 else 0.0


def _lowbit(x):
    """Lowest set bit of every non-zero of x (fp64), inf for a zero."""
    mant, ex = np.frexp(np.asarray(x, dtype=np.float64))
    M = np.abs(mant * 2.0 ** 53).astype(np.int64)
    low = (M & -M).astype(np.float64) * 2.0 ** (ex.astype(np.float64) - 53.0)
    return np.where(M == 0, np.inf, low)


def assert_exact_sums(terms, what):
    """terms [k, c]: every partial sum of a column, in any order, is a multiple of the lowest set bit of any term and no
    larger than sum |terms|; it is an fp32 number if that span is at most 24 bits."""
    total, low = np.abs(terms).sum(axis=0), _lowbit(terms).min(axis=0)
    ok = (total < 2.0 ** 24 * low) | (total == 0)
    assert ok.all(), (what, np.flatnonzero(~ok)[:8], (total / low)[~ok][:8])


def _pd_terms(case, v, axis):
    """The products the three launches sum along `axis` against the vector v: P v, and +tv v and -pv v of every exception."""
    Pm = np.where(case.out, case.pv.astype(np.float64), case.A64)
    tvm, pvm = np.where(case.out, case.A64, 0.0), np.where(case.out, case.pv.astype(np.float64), 0.0)
    w = v[:, None] if axis == 0 else v[None, :]
    stack = np.concatenate([Pm * w, tvm * w, pvm * w], axis=0 if axis == 0 else 1)
    return stack if axis == 0 else stack.T


def sum_probe_b(case):
    """y = 0 and a small-integer b: r = -b, g = -A^T b, exact in every order.  -> (b, y, alpha2), g as fp32."""
    rng = np.random.default_rng(21)
    b = rng.integers(-2, 3, case.m).astype(np.float32)
    b[CLEAN_ROW], b[HEAVY_ROW] = 2.0, -1.0
    r = -b.astype(np.float64)
    assert_exact_sums(_pd_terms(case, r, 0), "sum probe b: g")
    g = case.A64.T @ r
    assert np.array_equal(g.astype(np.float32).astype(np.float64), g)
    return (b, np.zeros(case.n, dtype=np.float32), 0.0), g.astype(np.float32)


def sum_probe_y(case):
    """b = None and the small-integer y of heavy() on HEAVY_ROW's 200 exception columns: r = A y (through b' of a row with 200
    exceptions), g = A^T r (through D^T r of a column with 130), rr = |r|^2 - exact in every order.
    -> (b, y, alpha2), g as fp32, rr."""
    y = case.y_probe
    assert np.array_equal(np.flatnonzero(y), np.flatnonzero(case.out[HEAVY_ROW])) and np.abs(y).max() <= 2
    assert_exact_sums(_pd_terms(case, y, 1), "sum probe y: r")
    r = case.A64 @ y
    assert r[HEAVY_ROW] != 0 and np.count_nonzero(r[case.out[:, HEAVY_COL]]) > 64
    assert_exact_sums(_pd_terms(case, r, 0), "sum probe y: g")
    g, rr = case.A64.T @ r, float(r @ r)
    assert np.array_equal(g.astype(np.float32).astype(np.float64), g) and float(np.sum(r * r)) < 2.0 ** 53
    return (None, y.astype(np.float32), 0.0), g.astype(np.float32), rr


def check_bits(case, what, g, g_ref, rr=None, rr_ref=None):
    g = np.asarray(g, dtype=np.float32)
    diff = np.flatnonzero(g != g_ref)               # (values: +0.0 and -0.0 are the same sum)
    assert diff.size == 0, (case.name, what, "g differs in", diff.size, "columns", diff[:8], g[diff[:4]], g_ref[diff[:4]])
    if rr_ref is not None:
        assert rr == rr_ref, (case.name, what, "rr", rr, rr_ref)


# ---- the model ------------------------------------------------------------------------------------------------------------
FAULTS = ("d_dropped_below", "d_dropped", "placeholder_at_the_wrong_end", "nibbles_swapped", "d_bytes_exchanged",
          "lowest_nibble_wrong", "csc_past_64_dropped", "csr_last_dropped", "bprime_y_is_x_cur")
# faults that touch only below-window elements or the lowest binades of the window: the old norm check cannot see them
QUIET_FAULTS = ("d_dropped_below", "lowest_nibble_wrong")


class Model:
    """The three launches in NumPy on the mirror's packed bytes: decode, b' = b - D y in fp64 rounded once, r = P y - b',
    slab w = P_w^T r_w for `nslab` blocks of rows, slab 0 += D^T r in fp64 rounded once, g = the fp32 sum of the slabs.  Row and
    column dots are formed in fp64 and rounded once - exact for the probes, whose dots have one non-zero term or are exact in
    every order.  fault: one of FAULTS, built into the decode or the lists."""

    def __init__(self, case, fault=None, nslab=4):
        assert fault is None or fault in FAULTS
        P, rows, cols, tv, pv, e0 = case.packed
        self.case, self.fault, self.nslab = case, fault, nslab
        P = P.copy()
        if fault == "nibbles_swapped":
            nibs = P[:, 3 * case.threads * 16:]
            nibs[:] = (nibs >> 4) | ((nibs & 0x0F) << 4)
        bits = decode(P, case.threads, case.n, e0).copy()
        if fault == "d_bytes_exchanged":
            d = bits[:, 3::4]
            bits[:, 3::4] = (d & np.uint32(0xFFFF0000)) | ((d & np.uint32(0xFF)) << 8) | ((d >> 8) & np.uint32(0xFF))
        if fault == "lowest_nibble_wrong":                   # the two lowest binades of the window decoded as the next two
            low = ((bits >> 23) & 0xFF) < e0 + 2
            bits[low] += np.uint32(2 << 23)
        if fault == "placeholder_at_the_wrong_end":
            ex = (tv >> 23) & 0xFF
            bits[rows, cols] = (tv & np.uint32(0x807FFFFF)) | (np.where(ex < e0, e0 + 15, e0).astype(np.uint32) << 23)
        self.P64 = bits.view(np.float32).astype(np.float64)
        keep = np.ones(len(rows), dtype=bool)
        if fault == "d_dropped":
            keep[:] = False
        elif fault == "d_dropped_below":
            keep = ((tv >> 23) & 0xFF) > e0
        self.rows, self.cols = rows[keep], cols[keep]
        self.d = tv[keep].view(np.float32).astype(np.float64) - pv[keep].view(np.float32).astype(np.float64)
        # (pack() lists the exceptions row by row, columns ascending: the CSR order; a stable sort by column is the CSC order)
        self.in_csr = np.ones(len(self.rows), dtype=bool)
        if fault == "csr_last_dropped" and len(self.rows):
            self.in_csr = np.append(self.rows[1:] == self.rows[:-1], False)
        self.in_csc = np.ones(len(self.rows), dtype=bool)
        if fault == "csc_past_64_dropped" and len(self.rows):
            order = np.argsort(self.cols, kind="stable")
            c = self.cols[order]
            first = np.searchsorted(c, c, side="left")
            self.in_csc[order] = np.arange(len(c)) - first < 64

    def run(self, b, y=None, alpha2=0.0, x_cur=None, x_prev=None, beta=0.0):
        """-> (g fp32, rr).  y explicit, or the momentum form y = x_cur + beta (x_cur - x_prev), rounded once."""
        case = self.case
        with np.errstate(over="ignore", invalid="ignore"):
            if y is None:
                y_b = y = (x_cur + beta * (x_cur - x_prev)).astype(np.float32).astype(np.float64)
                if self.fault == "bprime_y_is_x_cur":
                    y_b = np.asarray(x_cur, dtype=np.float32).astype(np.float64)
            else:
                y_b = y = np.asarray(y, dtype=np.float32).astype(np.float64)
            b64 = np.zeros(case.m) if b is None else np.asarray(b, dtype=np.float64)
            k = self.in_csr
            dy = np.bincount(self.rows[k], weights=self.d[k] * y_b[self.cols[k]], minlength=case.m)
            bp = (b64 - dy).astype(np.float32) if len(self.rows) else b64.astype(np.float32)
            r = ((self.P64 @ y).astype(np.float32) - bp).astype(np.float32).astype(np.float64)
            edges_ = np.linspace(0, case.m, min(self.nslab, case.m) + 1).astype(int)
            slabs = [(self.P64[lo:hi].T @ r[lo:hi]).astype(np.float32) for lo, hi in zip(edges_[:-1], edges_[1:])]
            k = self.in_csc
            dtr = np.bincount(self.cols[k], weights=self.d[k] * r[self.rows[k]], minlength=case.n)
            hit = np.bincount(self.cols[k], minlength=case.n) > 0
            slabs[0] = np.where(hit, (slabs[0].astype(np.float64) + dtr).astype(np.float32), slabs[0])
            g = slabs[0]
            for s in slabs[1:]:
                g = (g + s).astype(np.float32)
            if alpha2:
                g = (g.astype(np.float64) + alpha2 * y).astype(np.float32)
            return g, float(np.sum(r * r))

    def probe(self, probe):
        b, y, alpha2 = probe
        return self.run(b, y, alpha2)


def momentum_probe(case, j):
    """Column probe j in the momentum form: x_cur = 0, x_prev = -2 s e_j, beta = 1/2 give y = s e_j exactly - and 0 where y is
    taken as x_cur."""
    s = col_scale(case, j)
    x_prev = np.zeros(case.n)
    x_prev[j] = -2.0 * s
    return dict(x_cur=np.zeros(case.n), x_prev=x_prev, beta=0.5)


def all_checks(case, run, run_momentum=None):
    """Every probe of a matrix through run((b, y, alpha2)) -> (g, rr): the rows and columns its builder lists, the sum probes on
    `heavy`, and with run_momentum(x_cur=, x_prev=, beta=) -> (g, rr) the column probes of exception columns in the momentum
    form.  -> the worst error / bound of the row and of the column checks."""
    worst_row = max([check_row(case, i, run(row_probe(case, i))[0]) for i in case.probe_rows] + [0.0])
    worst_col = 0.0
    for j in case.probe_cols:
        g, rr = run(col_probe(case, j))
        worst_col = max(worst_col, check_col(case, j, g, rr))
    if case.name.startswith("heavy"):
        probe, g_ref = sum_probe_b(case)
        check_bits(case, "sum probe b", run(probe)[0], g_ref)
        probe, g_ref, rr_ref = sum_probe_y(case)
        g, rr = run(probe)
        check_bits(case, "sum probe y", g, g_ref, rr, rr_ref)
    if run_momentum is not None:
        for j in [j for j in case.probe_cols if case.out[:, j].any()][:4]:
            g, rr = run_momentum(**momentum_probe(case, j))
            check_col(case, j, g, rr)
    return worst_row, worst_col


# ---- the data of tests/test_gpu_packed_forms.py -----------------------------------------------------------------------------
FORMS_FAMILY = "S-f32"
PLANT_LO, PLANT_HI = 16.0, 256.0  # magnitudes of the planted entries (the first pair tried: no larger one was needed)


def fista_with_pass(A, b, L, a1, a2, iters, P=None, bprime_from_x_cur=False):
    """Plain FISTA (l1 prox, alpha2 in the smooth term, step 1 / (L + alpha2)) in fp64 whose gradient is formed as the three
    launches form it: r = P y - (b - D y_b) with D = A - P, g = P^T r + D^T r = A^T r.  y_b = y gives A^T (A y - b) whatever P
    is; bprime_from_x_cur takes y_b = x_cur, the fault "bprime_y_is_x_cur" of the model."""
    D = None if P is None else A - P
    tau = 1.0 / (L + a2)
    x, x_old, t, beta = np.zeros(A.shape[1]), np.zeros(A.shape[1]), 1.0, 0.0
    for _ in range(iters):
        y = x + beta * (x - x_old)
        r = A @ y - b
        if bprime_from_x_cur:
            r -= D @ (y - x)
        v = y - tau * (A.T @ r + a2 * y)
        x_old, x = x, np.sign(v) * np.maximum(np.abs(v) - tau * a1, 0.0)
        t_new = 0.5 * (1.0 + math.sqrt(1.0 + 4.0 * t * t))
        t, beta = t_new, (t - 1.0) / t_new
    return x


def forms_data(cus):
    """(A, b, L, lam) as tests/_forms.make_data("S-f32") makes them, on a heavy-tailed A: 6e-4 of the entries replaced by
    +-uniform(PLANT_LO, PLANT_HI) and 2e-4 by 0.0; b = A x_true + noise, L and lam are recomputed for the new A the way
    make_data does (tests/_data.synth: the same x_true, the same noise)."""
    from tests import _data, _forms as F
    spec = F.families(cus)[FORMS_FAMILY]
    A0, b0, xt = _data.synth(spec["m"], spec["n"], F.SEED[FORMS_FAMILY])
    rng = np.random.default_rng(101)
    A = A0.astype(np.float32)
    idx = rng.choice(A.size, int(8e-4 * A.size), replace=False)
    nbig = int(6e-4 * A.size)
    A.ravel()[idx[:nbig]] = (rng.uniform(PLANT_LO, PLANT_HI, nbig) * rng.choice([-1.0, 1.0], nbig)).astype(np.float32)
    A.ravel()[idx[nbig:]] = 0.0
    A = A.astype(np.float64)
    b = (b0 + (A - A0) @ xt).astype(np.float32).astype(np.float64)
    v = np.ones(A.shape[1]) / math.sqrt(A.shape[1])
    for _ in range(30):
        v = A.T @ (A @ v)
        v /= np.linalg.norm(v)
    L = 1.1 * float(np.linalg.norm(A @ v) ** 2)
    lam = float(np.max(np.abs(A.T @ b)))
    return A, b, L, lam
