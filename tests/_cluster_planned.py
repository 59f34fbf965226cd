"""Shapes, recipes and reference glue of the tests that run the two-product features of the matrix-core lockstep on
cluster-planned problems (a helper: no tests in here, and no GPU code).

plan_multi_mfma (csrc/fos_plan.hip) lays a cluster-planned problem out for the one-read form: multi.gram_splits is the number of
clusters and slabs16 is [clusters][16][n].  Every feature (several right-hand sides, fold masks, the logistic and multinomial
losses, row weights, penalty factors and bounds, the group penalty, feature groups, the working-set gradient batch) runs the
two-product form on that layout through two_product_splits (csrc/fos_fista.hip), which works the row splits out again.
tests/test_gpu_cluster_planned.py runs them there; tests/test_cluster_planned.py checks the arithmetic below against the source
and sweeps the refusal of two_product_splits over the CU counts.

The data of a shape is ONE seeded Gaussian design (tests/_data.synth) with the families' own recipes on top of it: labels
(tests/_logit.labels, tests/_multinomial.labels), "counts" row weights (tests/_weighted.weights), penalty factors and bounds
(tests/_coord.factors / bounds), the cross64 group layout (tests/_fgroup.layout), weights below alpha_max of every family.  The
constant of the data term is a bound and no estimate: the families' power iterations take 200 fp64 products with a 270 MB
matrix, the bound none.  For an m x n matrix of independent standard normal entries the largest singular value is at most
sqrt(m) + sqrt(n) + t with probability 1 - 2 exp(-t^2 / 2) (Davidson & Szarek), so L = LIPSCHITZ_SAFETY (sqrt(m) + sqrt(n))^2
bounds lambda_max(A^T A) (t >= 6.6 at these shapes); both sides take the same L, so the comparison does not depend on it
being tight.  With weights w_i <= WEIGHT_MAX the weighted constant is at most WEIGHT_MAX times it."""
import functools
import math
import re

import numpy as np

from oracle import fos_oracle as orc
from tests import _coord as cd, _data, _duality as du, _fgroup as fg, _logit as lg, _menu_multi as mm, _weighted as wt
from tests._menu_product1 import FISTA, PLAN, _body, _text

ITERS = 12
TOL = lg.TOL
FORMS_TOL = 1e-6                          # the one-read form against the two-product form (test_fista_path_one_read_cluster_pass)
LIPSCHITZ_SAFETY = 1.1
WEIGHT_MAX = 3.0                          # tests/_weighted.weights("counts"): integers 0..3

# (m, n, what runs there): the smallest shapes the cluster form is served at on 256 CUs (test_fista_path_one_read_cluster_pass)
SHAPES = {
    "cs4": (8200, 4096),                  # full strips, ragged last row panel
    "cs8": (4200, 5000),                  # members without a column, a strip ending inside a 1024-column block
    "cs16": (2100, 16384),                # two cells only
}
EXPECTED_CS = {"cs4": 4, "cs8": 8, "cs16": 16}


# ---- the split arithmetic of plan_multi_mfma, restated (tests/test_cluster_planned.py pins it to the source) -----------------------
GRAM_ROWS = 256                           # a row split of product 2 holds at least this many panel rows


def two_product_layout(m, n, cus, dtype="f32"):
    """dict(panel_rows, strips, splits, rows_per_split, gram_splits) of the two-product form: what plan_multi_mfma computes for
    every problem and two_product_splits computes again on a cluster-planned one."""
    panel_rows = min(mm.PANEL_ROWS_PER_CU * cus, -(-m // 256) * 256)
    strips = -(-n // mm.TILE_COLS[dtype])
    splits = max(1, -(-2 * cus // strips))
    splits = min(splits, max(1, panel_rows // GRAM_ROWS))
    rows_per_split = -(-(-(-panel_rows // splits)) // mm.TILE_ROWS) * mm.TILE_ROWS
    return dict(panel_rows=panel_rows, strips=strips, splits=splits, rows_per_split=rows_per_split,
                gram_splits=-(-panel_rows // rows_per_split))


def clusters(m, n, cus):
    """Slab sets of the cluster layout (multi.gram_splits of a cluster-planned problem), 0 where the form is not served."""
    cs = mm.cluster_size(m, n, cus)
    return cus // cs if cs else 0


def min_cluster_rows(n, cus):
    """The fewest rows at which plan_multi_mfma serves the cluster form for n columns on `cus` CUs (None: at no row count)."""
    need = -(-n // mm.CP_W)
    cs = 0 if need <= 2 else 4 if need <= 4 else 8 if need <= 8 else 16 if need <= 16 else 0
    if cus % 8 or not cs or (cus // 8) % cs:
        return None
    return (cus // cs) * mm.CP_ROWS * mm.CP_MIN_PANELS


def refused(m, n, cus):
    """Whether two_product_splits refuses a feature on the cluster-planned m x n fp32 problem: fewer slab sets than row splits."""
    c = clusters(m, n, cus)
    return bool(c) and two_product_layout(m, n, cus)["gram_splits"] > c


def check_source(plan=PLAN, fista=FISTA):
    """The restatement above against csrc/fos_plan.hip and csrc/fos_fista.hip: every expression and constant it copies."""
    tp = _body(_text(plan), r"int\s+plan_multi_mfma\s*\(\s*fos_problem\s*\*\s*p\s*\)\s*(?=\{)")
    assert re.search(r"const\s+int64_t\s+rows\s*=\s*%d\s*\*\s*\(int64_t\)\s*p->ncu\s*;\s*p->multi\.panel_rows\s*=\s*std::min<int64_t>\(rows,\s*"
                     r"\(p->m\s*\+\s*255\)\s*/\s*256\s*\*\s*256\)" % mm.PANEL_ROWS_PER_CU, tp)
    assert re.search(r"strips\s*=\s*\(p->n\s*\+\s*\(is_bf16\s*\?\s*fos::GQ_COLS\s*:\s*fos::GB_COLS\)\s*-\s*1\)\s*/\s*"
                     r"\(is_bf16\s*\?\s*fos::GQ_COLS\s*:\s*fos::GB_COLS\)", tp)
    assert re.search(r"splits\s*=\s*std::max<int64_t>\(1,\s*\(2\s*\*\s*\(int64_t\)\s*p->ncu\s*\+\s*strips\s*-\s*1\)\s*/\s*strips\)", tp)
    assert re.search(r"splits\s*=\s*std::min<int64_t>\(splits,\s*std::max<int64_t>\(1,\s*p->multi\.panel_rows\s*/\s*%d\)\)" % GRAM_ROWS, tp)
    assert re.search(r"p->multi\.gram_rows_per_split\s*=\s*\(\(p->multi\.panel_rows\s*\+\s*splits\s*-\s*1\)\s*/\s*splits\s*\+\s*fos::GB_ROWS\s*-\s*1\)"
                     r"\s*/\s*fos::GB_ROWS\s*\*\s*fos::GB_ROWS", tp)
    split_count = (r"\(int\)\(\(p->multi\.panel_rows\s*\+\s*p->multi\.gram_rows_per_split\s*-\s*1\)\s*/\s*p->multi\.gram_rows_per_split\)")
    assert re.search(r"p->multi\.gram_splits\s*=\s*" + split_count, tp)
    assert re.search(r"if\s*\(p->multi\.cp_cs\)\s*p->multi\.gram_splits\s*=\s*p->multi\.cp_clusters\s*;", tp)
    assert re.search(r"p->multi\.cp_clusters\s*=\s*p->ncu\s*/\s*cs\s*;", tp)
    assert re.search(r"p->multi\.slabs16\.reserve\(\(size_t\)p->multi\.gram_splits\s*\*\s*fos::BT_NV\s*\*\s*p->n\)", tp)
    tf = _body(_text(fista), r"static\s+int\s+two_product_splits\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"if\s*\(p->multi\.cp_cs\)\s*\{\s*\*g_splits\s*=\s*" + split_count + r"\s*;\s*if\s*\(\*g_splits\s*>\s*p->multi\.gram_splits\)\s*"
                     r"return\s+fail\(FOS_ERR_UNSUPPORTED", tf)


# ---- data ------------------------------------------------------------------------------------------------------------------------
def lipschitz_bound(m, n):
    return LIPSCHITZ_SAFETY * (math.sqrt(m) + math.sqrt(n)) ** 2


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=3)
def data(name):
    """The data of a shape, computed once and never modified: A32 (what goes to the device), A (the same in fp64), b, y (labels),
    w ("counts" weights as stored), p (penalty factors as stored), L (squared loss; a quarter for the logistic, half for the
    multinomial loss, WEIGHT_MAX times it with the weights)."""
    m, n = SHAPES[name]
    seed = 5 + n
    A, b, xt = _data.synth(m, n, seed)
    A32 = A.astype(np.float32)
    A64 = A32.astype(np.float64)
    y = lg.labels(A, xt, seed)
    del A
    w = wt.as_stored(wt.weights("counts", m, seed))
    assert w.max() <= WEIGHT_MAX
    return _frozen(dict(name=name, m=m, n=n, seed=seed, A32=A32, A=A64, b=b.astype(np.float32).astype(np.float64), y=y, w=w,
                        p=cd.factors(n, seed), L=lipschitz_bound(m, n)))


def L_of(d, loss="squared", weighted=False):
    return d["L"] * (WEIGHT_MAX if weighted else 1.0) / {"squared": 1.0, "logistic": 4.0, "multinomial": 2.0}[loss]


def target(d, loss):
    return d["y"] if loss == "logistic" else d["b"]


def alphas(d, loss="squared", weighted=False, count=3):
    """tests/_weighted.alphas: below alpha_max of the (weighted) problem."""
    ones = d["w"] if weighted else np.ones(d["m"])
    return wt.alphas(d["A"], target(d, loss), ones, loss, count)


def plain_alphas(d, count=6):
    """The weights of the plain squared-loss path (more than four, so that the matrix-core lockstep takes them): the ladder of
    test_fista_path_one_read_cluster_pass."""
    lam = float(np.max(np.abs(d["A"].T @ d["b"])))
    return [(lam * 0.4 * 0.7 ** i, 0.5 if i % 3 == 1 else 0.0) for i in range(count)]


def targets(d, count):
    """An m x count block of right-hand sides: b scaled and shifted by seeded noise, as the device stores it (fp32)."""
    rng = np.random.default_rng(600 + d["seed"])
    B = d["b"][:, None] * rng.uniform(0.5, 1.5, size=count)[None, :] + 0.3 * rng.standard_normal((d["m"], count))
    return B.astype(np.float32)


def picks(count):
    """First, middle and last of `count`."""
    return sorted({0, count // 2, count - 1})


def fold_ids(m, K, seed):
    """Shuffled fold ids 0..K-1 (every fold non-empty)."""
    ids = np.random.default_rng(800 + seed).integers(0, K, size=m)
    ids[:K] = np.arange(K)
    return ids.astype(np.int64)


@functools.lru_cache(maxsize=None)
def bounds(name, loss, weighted=False):
    """tests/_coord.bounds from the unbounded fit of the case at its strongest penalty, so that they bind."""
    d = data(name)
    a1, a2 = alphas(d, loss, weighted)[0]
    x_unc = cd.run(d["A"], target(d, loss), a1, a2, L_of(d, loss, weighted), ITERS, p=d["p"], loss=loss,
                   w=d["w"] if weighted else None)["x"]
    lo, hi = cd.bounds(x_unc, d["seed"])
    return x_unc, lo, hi


def coord_reference(name, loss, a1, a2, *, weighted=False, rows=None):
    """tests/_coord.run on the case with its factors and bounds; rows: a boolean mask of the training rows."""
    d = data(name)
    _, lo, hi = bounds(name, loss, weighted)
    A, b, w = d["A"], target(d, loss), d["w"] if weighted else None
    if rows is not None:
        A, b, w = A[rows], b[rows], None if w is None else w[rows]
    return cd.run(A, b, a1, a2, L_of(d, loss, weighted), ITERS, p=d["p"], lo=lo, hi=hi, loss=loss, w=w)


def group_layout(n):
    """tests/_fgroup's cross64 layout: a group over columns 60..69 across the first 64-column update block, and groups of 8 from
    column 70 on, every eighth of which crosses a later block boundary (70 + 8 k is never a multiple of 64)."""
    start, gw = fg.layout("cross64", n)
    crossing = [(s, e) for s, e in zip(start[:-1], start[1:]) if s // 64 != (e - 1) // 64]
    assert len(crossing) > n // 128
    return start, gw


# tests/_fgroup.FRACTIONS with the middle weight at a quarter of alpha_max instead of a fifth: at a fifth one group of the cs8
# reference comes within 1.1e-5 of its threshold (tests/_fgroup.CLOSE is 1e-4), where the device may fall on either side; with
# these no group of either shape and mixing comes closer than 1.5e-4 (decided on the reference alone)
GROUP_FRACTIONS = ((0.5, 0.0), (0.25, 0.5), (0.08, 0.0))


def group_alphas(d, start, gw, mu):
    amax = fg.alpha_max(d["A"].T @ d["b"], start, fg.weights_of(start, gw), mu)
    return [(f * amax, a2) for f, a2 in GROUP_FRACTIONS]


# ---- the duality-gap certificate -------------------------------------------------------------------------------------------------
CERT_COLUMNS = 16
CERT_ZERO = 0                             # the all-zero column
CERT_ITERATES = (2, 3, 5)                 # the columns of the plain path's iterates: lasso columns (see certificate_case)
CERT_CELLS = {"gap": ("squared", False), "weighted_logistic_gap": ("logistic", True)}


@functools.lru_cache(maxsize=None)
def certificate_case(name, cell):
    """What a certificate cell is asked for on the shape, computed once and never modified: dict(loss, t, w, X - n x 16, as the
    device takes it: fp32 values in fp64 -, alphas).  Column 0 is all zero, columns 2, 3 and 5 are the iterates of the plain path's
    reference (the oracle's FISTA on b with the first, middle and last of plain_alphas), the others a seeded sparse block scaled so
    that A x is of order 1.  The iterates sit in lasso columns: the first of them, in the elastic-net column 1, is so close to
    that column's own optimum (a gap of 8.8e-4 of its terms' magnitude on cs4) that the gap would not stand clear of rounding.  The weights are a ladder from a half to a fiftieth of the configuration's alpha_max, every third an
    elastic net: the certificate of a lasso column has a scale below 1, that of an elastic-net column the scale 1."""
    d = data(name)
    loss, weighted = CERT_CELLS[cell]
    t, w = target(d, loss), (d["w"] if weighted else None)
    rng = np.random.default_rng(950 + d["seed"])
    X = 0.05 * rng.standard_normal((d["n"], CERT_COLUMNS)) * (rng.random((d["n"], CERT_COLUMNS)) < 0.1)
    X[:, CERT_ZERO] = 0.0
    weights = plain_alphas(d)
    for col, i in zip(CERT_ITERATES, picks(len(weights))):
        X[:, col] = orc.fista(d["A"], d["b"], "elasticnet", *weights[i], max_iter=ITERS, L=d["L"])
    amax = float(np.abs(du.gradient(loss, d["A"], np.zeros((d["n"], 1)), t, None, w)).max())
    ratio = (0.02 / 0.5) ** (1.0 / (CERT_COLUMNS - 1))
    alphas = [(amax * 0.5 * ratio ** i, 0.5 if i % 3 == 1 else 0.0) for i in range(CERT_COLUMNS)]
    return _frozen(dict(loss=loss, t=t, w=w, X=X.astype(np.float32).astype(np.float64), alphas=alphas))


def check_certificate_case(name, cell, G=None):
    """The preconditions of a certificate cell on its fp64 certificate: a scale inside (0, 1) and the scale 1, every value finite,
    and the gap of every non-zero column far above what the fp32 passes can move it by - a gap made of rounding noise would let a
    wrong dual pass.  G: the fp64 gradient block, n x 16, where it is at hand.  Returns the certificate."""
    d, cs = data(name), certificate_case(name, cell)
    ref = du.certificate(cs["loss"], d["A"], cs["t"], cs["X"], cs["alphas"], None, cs["w"], G=None if G is None else G.T)
    s, live = ref["scale"], np.arange(CERT_COLUMNS) != CERT_ZERO
    assert ((s > 0) & (s < 1)).any() and (s == 1).any(), s
    assert all(np.isfinite(ref[k]).all() for k in ("primal", "dual", "gap", "scale"))
    assert (ref["gap"][live] > 100.0 * du.TOL * ref["mag_gap"][live]).all(), ref["gap"] / ref["mag_gap"]
    assert (cs["X"][:, CERT_ZERO] == 0).all() and (cs["X"][:, 1:] != 0).any(axis=0).all()
    return ref


@functools.lru_cache(maxsize=None)
def certificate_gradient(name, cell):
    """(the fp64 gradient block of a certificate cell, n x 16, the bound of a column of the device's in the 2-norm - that of
    fos_gradient_batch, the pass on sqrt(w) A), computed once with the preconditions of the case."""
    d, cs = data(name), certificate_case(name, cell)
    G = du.gradient(cs["loss"], d["A"], cs["X"], cs["t"], None, cs["w"])
    check_certificate_case(name, cell, G)
    sw = np.ones(d["m"]) if cs["w"] is None else np.sqrt(cs["w"])
    g_tol, _ = _data.fp32_pass_tolerances_cols(sw[:, None] * d["A"], cs["X"], sw * np.abs(cs["t"]), G, np.ones(CERT_COLUMNS))
    G.setflags(write=False)
    return G, g_tol


# ---- the resampled lockstep (include/fos_resample.h) -------------------------------------------------------------------------------
# A resampled call is kept off the one-read cluster pass by one term of run_multi_mfma (use_cluster ... && !counts) and works the
# row splits out again by a line of its own; fos_gradient_batch_resampled and fos_gram_apply_resampled call two_product_splits
# themselves.  Column j fits the problem with the row weights w * c_j, so the references are tests/_resample.py's (the weighted
# references).  The step: lambda_max(A^T diag(w c_j) A) <= max_i (w_i c_ij) lambda_max(A^T A), so L_j = max_i c_ij times the
# bound of the whole A (times WEIGHT_MAX under the "counts" weights) - passed to both sides.
# cell -> (loss, row weights, recipe of the counts, resamples = lockstep columns)
RESAMPLE_CELLS = {"resampled_path": ("squared", False, "bootstrap", 5), "resampled_weighted_logistic_path": ("logistic", True, "binary", 3),
                  "resampled_gradient": ("squared", False, "bootstrap", 16), "resampled_gram": ("squared", True, "binary", 16)}
RESAMPLE_PLAIN = "resampled_as_the_plain_path"          # part 2: one 0/1 resample under the plain path's own weights and step


@functools.lru_cache(maxsize=None)
def resample_counts(name, recipe, nv):
    """m x nv int64 multiplicities.  binary: a random half of the rows (0 / 1); bootstrap: m draws of the m rows with replacement
    per column, as they fall (no planted 15: the largest count sets the step).  Never a column of zeros."""
    m = SHAPES[name][0]
    rng = np.random.default_rng(9300 + 31 * nv + m)
    if recipe == "binary":
        c = (rng.random((m, nv)) < 0.5).astype(np.int64)
        c[0] = 1
    else:
        assert recipe == "bootstrap"
        c = np.stack([np.bincount(rng.integers(0, m, size=m), minlength=m) for _ in range(nv)], axis=1).astype(np.int64)
    assert c.min() == 0 and 1 <= c.max() <= 15 and (c.sum(axis=0) > 0).all()
    c.setflags(write=False)
    return c


def resample_weights(d, cell, C):
    """The m x nv weights of the references: w * c_j."""
    weighted = RESAMPLE_CELLS[cell][1] if cell in RESAMPLE_CELLS else False
    return C.astype(np.float64) * (d["w"][:, None] if weighted else 1.0)


def resample_case(name, cell):
    """dict(loss, weighted, counts, L - per resample, before the logistic quarter, as resampled_path takes it -, alphas) of a path
    cell.  The squared cell takes the third weight of the plain ladder, the weighted logistic one the middle weight of its family
    (a tenth of alpha_max of all rows: a fifth of that of half of them)."""
    d = data(name)
    if cell == RESAMPLE_PLAIN:
        C = resample_counts(name, "binary", 1)
        return dict(loss="squared", weighted=False, counts=C, L=np.full(1, d["L"]), alphas=plain_alphas(d))
    loss, weighted, recipe, nv = RESAMPLE_CELLS[cell]
    C = resample_counts(name, recipe, nv)
    L = C.max(axis=0) * d["L"] * (WEIGHT_MAX if weighted else 1.0)
    weights = [alphas(d, loss, weighted)[1] if loss == "logistic" else plain_alphas(d)[2]]
    return dict(loss=loss, weighted=weighted, counts=C, L=L, alphas=weights)


def resample_reference(name, cell, r, a=0):
    """The fp64 fit of resample r at weight a of a path cell after ITERS iterations (tests/_resample.run on the weights w * c_r)."""
    from tests import _resample as rsp
    d, cs = data(name), resample_case(name, cell)
    w = rsp.effective(d["w"] if cs["weighted"] else None, cs["counts"][:, r])
    a1, a2 = cs["alphas"][a]
    return rsp.run(cs["loss"], d["A"], target(d, cs["loss"]), w, a1, a2, cs["L"][r] / rsp.divisor(cs["loss"]), ITERS)[0]


def resample_block(d):
    """The n x 16 block the gradient and Gram cells are asked for (fp32 values): tests/test_gpu_cluster_planned.Batches' recipe
    scaled so that A x is of order 1, with one all-zero column."""
    rng = np.random.default_rng(930 + d["seed"])
    X = 0.05 * rng.standard_normal((d["n"], 16)) * (rng.random((d["n"], 16)) < 0.1)
    X[:, 1] = 0.0
    return X.astype(np.float32)


# The controlled resampled run: two 0/1 resamples under the 16 weights of the controlled case - 32 (resample, weight) cells, two
# lockstep groups -, of which the cells stay whose every decision in the fp64 reference is fp32-proof (tests/_coord.fp32_proof;
# a cell whose fit is still 0 decides on nothing and goes too) and stands MIN_CONTROL_MARGIN clear of its thresholds, as the
# controlled case below does.  L is the bound of the whole A, valid for 0/1 counts; on half of the rows it is about twice the
# resample's own constant, the steps are short and no ratio falls below CONTROL's tolerance of 0.5 within 12 iterations (scanned on
# the reference alone over thresholds 0.95 / 1 and tolerances 0.5 .. 0.8: at 0.5 every cell of cs4 runs to the end, from 0.7 on
# every cell of both shapes stops by iteration 5).  At 0.6 both shapes have early stops, full runs and genuine restarts.
RESAMPLE_CONTROL_RESAMPLES = 2
RESAMPLE_CONTROL = dict(adaptive_restart=True, restart_threshold=0.95, tol_ratio=0.6)


@functools.lru_cache(maxsize=None)
def resample_control_case(name):
    """(counts m x 2, the 16 weights, {(r, a): the reference run (tests/_coord.run's dict without its problem)} of the kept cells)."""
    d = data(name)
    C = resample_counts(name, "binary", RESAMPLE_CONTROL_RESAMPLES)
    weights = control_alphas(d)
    kept = {}
    for r in range(RESAMPLE_CONTROL_RESAMPLES):
        for a, (a1, a2) in enumerate(weights):
            ref = cd.run(d["A"], d["b"], a1, a2, d["L"], CONTROL_ITERS, w=C[:, r].astype(np.float64), **RESAMPLE_CONTROL)
            ref.pop("prob")
            thresholds = RESAMPLE_CONTROL["restart_threshold"], RESAMPLE_CONTROL["tol_ratio"]
            if cd.fp32_proof(ref, *thresholds) and cd.decision_margin(ref, *thresholds) >= MIN_CONTROL_MARGIN:
                kept[(r, a)] = ref
    return C, weights, kept


def check_resample_control(kept):
    """At least half of the 32 cells stay, and among them one stops early, one runs to the end and one restarts on a finite ratio."""
    refs = list(kept.values())
    assert 2 * len(refs) >= RESAMPLE_CONTROL_RESAMPLES * CONTROL_WEIGHTS, len(refs)
    assert any(r["stopped"] == cd.STOP_RATIO and r["k"] < CONTROL_ITERS for r in refs), "no kept cell stops early"
    assert any(r["stopped"] == cd.STOP_NONE and r["k"] == CONTROL_ITERS for r in refs), "no kept cell runs to the end"
    assert sum(cd.genuine_restarts(r, RESAMPLE_CONTROL["restart_threshold"]) for r in refs) >= 1, "no genuine restart"


# ---- the device-controlled case ------------------------------------------------------------------------------------------------
# test_fista_path_lockstep_with_restart_and_ratio_stop's second recipe with the restart threshold moved from 0.9 to 0.95: at 0.9 the
# cs4 run has a ratio 4.1e-4 from the ratio tolerance (weight 4, iteration 11: 0.49959 against 0.5), which no fp32 run is bound to
# decide as fp64 does; at 0.95 every decision of both shapes is fp32-proof (scanned over thresholds 0.9 / 0.95 / 1 and tolerances
# 0.4 .. 0.58 on the oracle alone).
CONTROL = dict(adaptive_restart=True, restart_threshold=0.95, tol_ratio=0.5)
CONTROL_ITERS = 12
MIN_CONTROL_MARGIN = 3.5e-3
CONTROL_MORE = 2                          # iterations of the further call on the same handles (the oracle's decisions there: margin 9e-3)
CONTROL_WEIGHTS = 16


def control_alphas(d):
    """16 weights, the ladder of test_fista_path_lockstep_with_restart_and_ratio_stop."""
    lam = float(np.max(np.abs(d["A"].T @ d["b"])))
    return [(lam * 0.5 * 0.6 ** i, 0.3 if i % 3 == 2 else 0.0) for i in range(CONTROL_WEIGHTS)]


def control_references(name):
    """The oracle's controlled run of every weight (tests/_coord.run without factors and bounds: the oracle's own FistaProblem
    stepped by its own `step`), as dicts of x, k, stopped, ratios, moves."""
    d = data(name)
    return [cd.run(d["A"], d["b"], a1, a2, d["L"], CONTROL_ITERS, **CONTROL) for a1, a2 in control_alphas(d)]


def control_margin(refs):
    """The smallest distance of a finite step ratio of the run from the restart threshold and from the ratio tolerance.

    Every decision must be fp32-proof (tests/_coord.fp32_proof): further from its threshold than MARGIN = 1e-3 and than
    2 eps32 ||x|| / move, which is what the parity bar (TOL = 1e-5 on the iterate) lets a ratio of two steps move when the
    steps themselves carry fp32 rounding.

    Computed once on the CPU for the chosen case: 3.52e-3 on cs4 (iterations run per weight 8 8 8 8 8 12 12 2 2 2 2 2 2 2 2 2) and
    5.51e-3 on cs8 (12 x 7, then 2 x 9); the smallest is 3.52e-3, against a bar of 1e-3.  tests/test_gpu_cluster_planned.py asserts
    MIN_CONTROL_MARGIN on the run it compares with."""
    return min(cd.decision_margin(r, CONTROL["restart_threshold"], CONTROL["tol_ratio"]) for r in refs)


def check_control(refs):
    """The preconditions of the controlled case, on the oracle's run alone."""
    ks = [r["k"] for r in refs]
    assert min(ks) < CONTROL_ITERS and any(r["stopped"] == cd.STOP_RATIO for r in refs), ("no weight stops early", ks)
    assert any(r["stopped"] == cd.STOP_NONE and r["k"] == CONTROL_ITERS for r in refs), ("no weight runs to the end", ks)
    assert sum(cd.genuine_restarts(r, CONTROL["restart_threshold"]) for r in refs) >= 1, "no genuine restart"
    for i, r in enumerate(refs):
        assert cd.fp32_proof(r, CONTROL["restart_threshold"], CONTROL["tol_ratio"]), (i, r["ratios"])
