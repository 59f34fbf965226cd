"""Coverage table of the L-BFGS kernels (a helper: no tests in here), beside tests/_menu.py and tests/_menu_multi.py.

One row per launchable instantiation of a __global__ of csrc/lbfgs_kernels.hpp, with the public entry point that reaches it
and the cases that are run on it.  tests/test_kernel_menu_lbfgs.py keeps the set of rows equal to what the four .hip files
launch and checks the constants below against the source; tests/test_gpu_kernel_menu_lbfgs.py runs the rows whose check is a
kernel check, tests/test_gpu_lbfgs_driver.py the rows that only a driver reaches (check "driver" / "lockstep").

kernel                          instantiations            reached through
lbfgs_two_loop_kernel           <float|double, 1|2|4|0>   fos_lbfgs_two_loop / _dd: NQ from n <= 4096 / 8192 / 16384 when n % 4 == 0
                                                          and every pointer is 16-byte (float) / 32-byte (double) aligned, else 0
lbfgs_gram_kernel, _combine_    -                         fos_lbfgs_direction_dd
vec_stats_kernel                <float,float> <double,float> <double,double>   fos_vec_stats / _f64 / _dd
vec_axpby_kernel                -                         fos_vec_axpby
vec_axpby_f64_kernel            <float> <double>          fos_vec_axpby_f64 / _dd
add_l2_kernel                   <float> <double>          fos_gemv_pair / fos_gemv_pair_f64 (alpha2 != 0)
vec_norms_kernel                -                         fos_residual_objective
cast_f64_f32_kernel             -                         fos_fista_grad_dual on a precise handle (no dual pass: x_k is rounded)
stamp_kernel, lbfgs_first_trial_kernel, lbfgs_store_pair_kernel                fos_lbfgs_minimize (no entry point of their own)
*_multi_kernel                  two_loop <1> <0>          fos_lbfgs_minimize_multi

A kernel-check case is a dict; its keys depend on the check:
  two_loop    n, off (elements every operand is shifted by inside its allocation: 1 breaks the alignment), cfgs (list of
              (hist, cap, head))
  direction   n, cfgs, gd (gd_out given), tail (extra NaN doubles behind `work`)
  stats       n
  axpby       n
  pass        m, n
A driver row names the driver cases (tests/_lbfgs_cases.py) that launch it."""
LB_THREADS = 1024
LB_MAXHIST = 64
BUCKETS = ((4096, 1), (8192, 2), (16384, 4))      # n <= limit -> NQ chunks of q per thread in registers
ALIGN = {"float": 16, "double": 32}               # bytes; below it the generic form (NQ = 0) runs
VL_MAXH, VL_COLS, VL_THREADS, VL_PSTRIDE, VL_MAXPARTS = 10, 128, 256, 256, 64
CHIP_MIN_N = 2048                                 # both drivers: whole-chip direction from here on, two-loop below
AX_BLOCK, AX_CAP = 256, 1024                      # grid_1d(n, 256, 1024) of the element-wise kernels
DRIVER_M = 10                                     # pairs both drivers keep
BIG = 70001                                       # "above 70000": ragged, 547 chunks of the Gram kernel, 69 strides of 1024

HISTS = (0, 1, 2, 9, 10, 11, 33, 64)
# Lengths up to TINY keep at most min(n, 2) pairs: once the pairs span the space (hist >= n) the first sweep cancels q to
# rounding noise and the direction is a difference of nearly equal terms - a comparison there measures the conditioning of
# the inputs, not the kernel.
TINY = 4


def two_loop_nq(n, aligned):
    """NQ of the instantiation fos_lbfgs_two_loop / _dd launch."""
    if n % 4 or not aligned:
        return 0
    for limit, nq in BUCKETS:
        if n <= limit:
            return nq
    return 0


def direction_parts(n):
    """Workgroups of lbfgs_gram_kernel = partial Gram matrices (vl_parts)."""
    return min(-(-n // VL_COLS), VL_MAXPARTS)


def direction_work(n):
    return direction_parts(n) * VL_PSTRIDE


def axpby_grid(n):
    return min(-(-n // AX_BLOCK), AX_CAP)


def driver_direction(n):
    """What a driver launches for the direction at length n: "chip" or the two-loop NQ."""
    return "chip" if n >= CHIP_MIN_N else (1 if n % 4 == 0 else 0)


def ring_cfgs(hist, with_slack=True):
    """(hist, cap, head) for one history length: cap = hist and cap > hist, head at 0, in the middle and at cap - 1 (the
    live window wraps whenever head + hist > cap)."""
    if hist == 0:
        return [(0, 0, 0), (0, 10, 7)]
    out = [(hist, hist, 0), (hist, hist, hist // 2), (hist, hist, hist - 1)]
    if with_slack:
        cap = hist + max(1, hist // 4)
        out += [(hist, cap, 0), (hist, cap, cap // 2), (hist, cap, cap - 1)]
    return out


def _two_loop_lengths():
    """Per NQ: (n, off).  Bucket edges from BUCKETS: the limit, one chunk past it (the next bucket), one chunk short; one
    ragged length per bucket (generic form); offset-by-one views of aligned lengths (generic form)."""
    (b1, _), (b2, _), (b4, _) = BUCKETS
    per = {1: [(4, 0), (b1 - 4, 0), (b1, 0), (LB_THREADS * 4 - 4, 0)],
           2: [(b1 + 4, 0), (b2, 0)],
           4: [(b2 + 4, 0), (b4, 0)],
           0: [(1, 0), (3, 0), (b1 - 3, 0), (b2 - 3, 0), (b4 - 3, 0), (b4 + 4, 0), (BIG, 0), (b1, 1), (b2, 1), (b4, 1)]}
    per[1] = sorted(set(per[1]))
    return per


def _spread(lengths, seed):
    """Every history length of HISTS on every row, every ring form somewhere: case i takes the forms i, i + k, ... of the
    full list, so a row of k cases covers the list once."""
    forms = [c for h in HISTS for c in ring_cfgs(h)]
    tiny = [(n, off) for n, off in lengths if n <= TINY]
    rest = [(n, off) for n, off in lengths if n > TINY]
    k = len(rest)
    out = [dict(n=n, off=off, cfgs=[c for h in range(min(n, 2) + 1) for c in ring_cfgs(h)]) for n, off in tiny]
    for i, (n, off) in enumerate(rest):
        cfgs = forms[(i + seed) % k::k]
        if n > 20000:                                   # 64 pairs of 70001 doubles: keep the long case to three forms
            cfgs = [(10, 10, 9), (33, 41, 40), (64, 64, 32)]
        out.append(dict(n=n, off=off, cfgs=cfgs))
    return out


def _direction_cases(flip):
    """Lengths around one and two chunks of the Gram kernel (VL_COLS), around one workgroup of the combine kernel
    (VL_THREADS), at VL_MAXPARTS chunks exactly and just above (the first length where a workgroup loops), and long ones.
    Every history length 0..VL_MAXH at every length, ring forms taken in turn.  gd_out given / NULL and `work` exact / with a
    NaN tail alternate over the lengths; `flip` swaps both, so the two rows together run every length in both forms."""
    full = VL_COLS * VL_MAXPARTS
    lengths = [1, VL_COLS - 1, VL_COLS, VL_COLS + 1, VL_THREADS - 1, VL_THREADS, VL_THREADS + 1, full - 1, full, full + 1,
               2 * full + 1, BIG]
    out = []
    for i, n in enumerate(lengths):
        cfgs = []
        for h in range(min(n, VL_MAXH) + 1 if n <= TINY else VL_MAXH + 1):
            forms = ring_cfgs(h)
            cfgs.append(forms[(i + h) % len(forms)])
        out.append(dict(n=n, cfgs=cfgs, gd=(i % 2 == 0) != flip, tail=300 if (i % 3 == 0) != flip else 0))
    return out


STATS_LENGTHS = (1, 63, 64, LB_THREADS - 1, LB_THREADS, LB_THREADS + 1, BIG)
AXPBY_LENGTHS = (1, AX_BLOCK - 1, AX_BLOCK + 1, AX_BLOCK * AX_CAP, AX_BLOCK * AX_CAP + 3, 3 * AX_BLOCK * AX_CAP + 77)


def build():
    rows = []

    def add(kernel, targs, entry, check, cases, unreachable=None):
        rows.append(dict(kernel=kernel, targs=tuple(targs), entry=entry, check=check, cases=[] if unreachable else cases,
                         unreachable=unreachable))

    for vt, entry in (("float", "fos_lbfgs_two_loop"), ("double", "fos_lbfgs_two_loop_dd")):
        for j, (nq, lengths) in enumerate(sorted(_two_loop_lengths().items())):
            add("lbfgs_two_loop_kernel", (vt, str(nq)), entry, "two_loop", _spread(lengths, j))
    add("lbfgs_gram_kernel", (), "fos_lbfgs_direction_dd", "direction", _direction_cases(False))
    add("lbfgs_combine_kernel", (), "fos_lbfgs_direction_dd", "direction", _direction_cases(True))
    for targs, entry in ((("float", "float"), "fos_vec_stats"), (("double", "float"), "fos_vec_stats_f64"),
                         (("double", "double"), "fos_vec_stats_dd")):
        add("vec_stats_kernel", targs, entry, "stats", [dict(n=n) for n in STATS_LENGTHS])
    add("vec_axpby_kernel", (), "fos_vec_axpby", "axpby", [dict(n=n) for n in AXPBY_LENGTHS])
    add("vec_axpby_f64_kernel", ("float",), "fos_vec_axpby_f64", "axpby", [dict(n=n) for n in AXPBY_LENGTHS])
    add("vec_axpby_f64_kernel", ("double",), "fos_vec_axpby_dd", "axpby", [dict(n=n) for n in AXPBY_LENGTHS])
    shapes = [dict(m=37, n=132), dict(m=300, n=AX_BLOCK * 4 + 4), dict(m=5, n=20000)]
    add("add_l2_kernel", ("float",), "fos_gemv_pair", "pass", shapes)
    add("add_l2_kernel", ("double",), "fos_gemv_pair_f64", "pass", shapes)
    add("vec_norms_kernel", (), "fos_residual_objective", "pass", shapes)
    add("cast_f64_f32_kernel", (), "fos_fista_grad_dual", "pass", shapes)
    # kernels without an entry point of their own: the driver cases (tests/_lbfgs_cases.py) that launch them
    add("stamp_kernel", (), "fos_lbfgs_minimize", "driver", ["ragged33-b1e4"])                # fg_ms given, no stamping pass
    add("lbfgs_first_trial_kernel", (), "fos_lbfgs_minimize", "driver", ["div64-b1e4", "n2048-b1e8"])
    add("lbfgs_store_pair_kernel", (), "fos_lbfgs_minimize", "driver", ["div64-ring", "n2049-b1e4"])
    add("lbfgs_two_loop_multi_kernel", ("1",), "fos_lbfgs_minimize_multi", "lockstep", ["group16-n512", "group3-n512"])
    add("lbfgs_two_loop_multi_kernel", ("0",), "fos_lbfgs_minimize_multi", "lockstep", [],
        unreachable="fos_lbfgs_minimize_multi needs the single-pass plan (pair_dd_multi_supported: path 0), which takes rows "
                    "of 16 bytes only: n % 4 == 0 on every problem it serves, so the n % 4 != 0 branch never runs")
    for k in ("lbfgs_gram_multi_kernel", "lbfgs_combine_multi_kernel"):
        add(k, (), "fos_lbfgs_minimize_multi", "lockstep", ["group16-n2052", "group3-n2052"])
    for k in ("lbfgs_first_trial_multi_kernel", "lbfgs_step_multi_kernel", "lbfgs_store_pair_multi_kernel",
              "vec_stats_multi_kernel"):
        add(k, (), "fos_lbfgs_minimize_multi", "lockstep", ["group16-n512", "group16-n2052", "group3-n512", "group3-n2052"])
    return rows


ROWS = build()


def cell(row):
    return (row["kernel"], row["targs"])


def cells(rows=None):
    return {cell(r) for r in (ROWS if rows is None else rows)}


def row_id(row):
    return row["kernel"].replace("_kernel", "") + "".join("-" + t for t in row["targs"])


def axpby_inputs(n, seed, ytype="double"):
    """(a, x, b, y) of full-mantissa numbers.  Odd elements are independent draws of one magnitude; in the even ones b*y
    cancels a*x down to 2^-1 .. 2^-12 of the products (a line-search step back towards x_old), so the rounding of each
    product is worth several ulps of the sum: a contracted b*y + (a*x) (one rounding less) differs there from the separately
    rounded result nearly always (tests/test_kernel_menu_lbfgs.py measures the share with exact rational arithmetic)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * (1.0 + rng.random(n))
    y = rng.standard_normal(n) * (1.0 + rng.random(n))
    even = np.arange(0, n, 2)
    y[even] = (0.7310585786300049 / 1.3591409142295225) * x[even] * (1.0 + rng.standard_normal(even.size) * 2.0 ** -(1 + even // 2 % 12))
    if ytype == "float":
        y = y.astype(np.float32).astype(np.float64)
    return 0.7310585786300049, x, -1.3591409142295225, y
