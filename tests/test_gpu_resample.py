"""GPU: resampled fits in the lockstep (include/fos_resample.h, fastoptsolver_amd/resample.py) - the resample link kernel per
element, the gradient, data term, out-of-bag sums and the Gram operator against fp64, the bitwise anchors against the existing run
forms, path parity on every loss with every composition, the per-resample power iteration, stability selection end to end, the
out-of-bag loss, handle hygiene and the refusals.

Column j of a resampled pass is the problem with the row weights w * c_j: every reference is the existing weighted reference of
tests/_weighted.py / tests/_link.py (tests/_resample.py picks it), on the bf16-rounded A for bf16 storage, with L from the
oracle's power iteration passed to both sides.  Tolerances are those of the corresponding checks of tests/test_gpu_link.py,
tests/test_gpu_weighted.py and tests/test_gpu_power.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _data, _fgroup as fg, _link as lk, _resample as rsp

pytestmark = pytest.mark.gpu

TOL, ITERS = rsp.TOL, rsp.ITERS
KINDS = ("f32", "bf16")
LOSSES = rsp.LOSSES
F32 = np.float32
UNSUPPORTED = -4


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def _device(kind, A64):
    return torch.as_tensor(A64.astype(np.float32)).to(torch.bfloat16 if kind == "bf16" else torch.float32).cuda()


def _handle(fos, loss, kind, A64, b, c, w=None):
    """The handle of the loss on (A, b), with the sample weights w.  An unweighted squared problem of at most 64 columns has no
    matrix-core pair (tests/test_gpu_duality.py): it is bound with unit weights, which pads it as a logistic problem is padded;
    a wider one is padded to the granularity of its storage type (68 bf16 columns are no multiple of 8)."""
    At = _device(kind, A64) if isinstance(A64, np.ndarray) else A64
    if loss == rsp.HUBER:
        return fos.prepare_huber(At, b, c, sample_weight=w)
    if loss == rsp.HINGE:
        return fos.prepare_hinge(At, b, sample_weight=w)
    if w is None and (loss == rsp.LOGISTIC or At.shape[1] > 64):
        return fos.prepare(At, b, pad=True, loss=loss)
    return fos.prepare_weighted(At, b, np.ones(At.shape[0]) if w is None else w, loss=loss)


def _words(P, counts):
    from fastoptsolver_amd import resample
    return resample.pack_counts(torch.from_numpy(np.ascontiguousarray(counts)).to(P.device))


def _gradient(P, X, words, oob=False):
    """(G as an nv x n_dev float32 ndarray or None, the 16 doubles of loss16) of fos_gradient_batch_resampled."""
    from fastoptsolver_amd import _core, _lib
    Xf, nv = P._block16(torch.as_tensor(X))
    G = torch.full((nv, P.n_dev), float("nan"), dtype=torch.float32, device=P.device)
    with P.ctx():
        _lib.check(P.lib.fos_gradient_batch_resampled(_core.ptr(Xf), nv, _core.ptr(words), int(oob), P.h, None if oob else _core.ptr(G),
                                                      _core.ptr(P.scratch)), "fos_gradient_batch_resampled")
    return (None if oob else G.cpu().numpy()), P.scratch[:16].cpu().numpy().copy()


def _gram(P, X, words):
    from fastoptsolver_amd import resample
    return resample._gram_apply(P, torch.as_tensor(X), words)


def _states(P, params, **kw):
    """One state machine per (tau, alpha1, alpha2)."""
    from fastoptsolver_amd import _core
    hs = []
    for tau, a1, a2 in params:
        st = _core.Fista(P)
        st.reset(tau, a1, a2, **kw)
        hs.append(st)
    return hs


def _run_resampled(hs, words, iters):
    from fastoptsolver_amd import _core
    arr = (C.c_void_p * len(hs))(*[h.h for h in hs])
    with hs[0].prob.ctx():
        return hs[0].lib.fos_fista_run_multi_resampled(arr, len(hs), int(iters), _core.ptr(words))


def _xs(hs):
    return [st.x_tensor().cpu().numpy() for st in hs]


def _W(counts, w):
    """The m x nv weights of the reference: w * c_j."""
    return counts.astype(np.float64) * (1.0 if w is None else w[:, None])


# ---- 1. the link per element, through a diagonal A ----------------------------------------------------------------------------
M_D, N_D, C_D = 259, 260, 0.5


@functools.lru_cache(maxsize=None)
def _diagonal(loss):
    """(s, b, Z): A = diag(s) (259 x 260, powers of two), and the 259 x 16 panel Z = A X the kernel must see, with planted rows:
    the kinks and their fp32 neighbours of Huber and the hinge, z = 0 and the saturated ends of the logistic loss."""
    rng = np.random.default_rng(31)
    s = rng.choice([0.5, 1.0, 2.0], M_D).astype(F32)
    s[:16] = 1.0
    Z = (2.0 * rng.standard_normal((M_D, 16))).astype(F32)
    one = F32(1)
    if loss == rsp.HUBER:
        b = rng.standard_normal(M_D).astype(F32)
        b[:6] = [0.25, -0.25, 1.5, 0.0, 0.0, 0.0]
        planted = [C_D, -C_D, 0.0, 1e30, np.nextafter(F32(C_D), one), np.nextafter(F32(C_D), F32(0))]
        for i, r in enumerate(planted):                                   # r = z - b exactly
            Z[i, :] = F32(r) + b[i] if abs(r) < 4 else F32(r)
            assert F32(Z[i, 0] - b[i]) == F32(r)
    elif loss == rsp.HINGE:
        b = rng.choice([-1.0, 1.0], M_D).astype(F32)
        for i, t in enumerate([one, np.nextafter(one, F32(2)), np.nextafter(one, F32(0)), F32(-1e15)]):      # the margin t = b z
            Z[i, :] = b[i] * t
    elif loss == rsp.LOGISTIC:
        b = rng.choice([0.0, 1.0, 0.25], M_D).astype(F32)
        for i, z in enumerate([0.0, 30.0, -30.0, 100.0, -100.0]):
            Z[i, :] = z
    else:                                                                  # squared, and the Gram form (b unused)
        b = rng.standard_normal(M_D).astype(F32)
        Z[0, :] = b[0]                                                     # r = 0
    for a in (s, b, Z):
        a.setflags(write=False)
    return s, b, Z


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("nv", rsp.NVS)
@pytest.mark.parametrize("loss", ("gram",) + LOSSES)
def test_the_link_per_element_through_a_diagonal_matrix(fos, loss, nv, weighted):
    """R of every LOSS x MODE x WEIGHT instantiation against the kernel's fp32 expressions in numpy, bit for bit: G[j, i] = s_i
    R_ij is one non-zero product per sum.
    The logistic pair has no bitwise restatement in numpy: its expf and log1pf are another implementation than the device's
    (measured on an MI355X: 8 % of the elements of sigma(z) - b differ, by an ulp of sigma).  There sigma(z) - b is taken from the
    device's own established form of the same device function - product 1's logistic epilogue on a handle with unit weights, read
    back exactly through the same diagonal A - and what this kernel adds, the weight first and the count second, is still done in
    numpy fp32 and compared bit for bit; numpy's own sigma must agree within 4 eps32 of sigma's range."""
    s, b, Z = _diagonal(loss)
    A = np.zeros((M_D, N_D), dtype=F32)
    A[np.arange(M_D), np.arange(M_D)] = s
    w = None
    if weighted:
        w = np.random.default_rng(9).uniform(0.25, 4.0, M_D).astype(F32)
        w[::17] = 0.0
        w[3] = 2.0                                                       # an exact product with the 1e30 row
    base = rsp.SQUARED if loss == "gram" else loss
    wd = None if w is None else w.astype(np.float64)
    if base in (rsp.HUBER, rsp.HINGE) or w is not None:
        P = _handle(fos, base, "f32", torch.as_tensor(A).cuda(), b.astype(np.float64), C_D, wd)
    else:
        P = fos.prepare(torch.as_tensor(A).cuda(), b.astype(np.float64), loss=base)
    assert (P.sample_weight is not None) == weighted
    Cn = rsp.counts("bootstrap", M_D, nv)
    assert {0, 1, 2, rsp.MAX_COUNT} <= set(np.unique(Cn))
    words = _words(P, Cn)
    X = np.zeros((N_D, nv), dtype=F32)
    X[:M_D] = Z[:, :nv] / s[:, None]                                     # exact: s is a power of two
    v, l = rsp.link32(loss, Z[:, :nv], None if loss == "gram" else b, w, Cn, False, C_D)
    want = np.zeros((nv, P.n_dev), dtype=F32)
    want[:, :M_D] = (v * s[:, None]).T
    if loss == "gram":
        G = _gram(P, X, words).t().contiguous().cpu().numpy()
        assert G.shape == (nv, N_D) and np.array_equal(G, want[:, :N_D]), np.argwhere(G != want[:, :N_D])[:8]
        return
    G, loss16 = _gradient(P, X, words)
    if loss == rsp.LOGISTIC:
        scale = s[:, None] * Cn.astype(F32) * (F32(1) if w is None else w[:, None])
        assert np.all(np.abs(G[:, :M_D].T - want[:, :M_D].T) <= 4 * np.finfo(F32).eps * scale), "numpy's sigma and the device's"
        print(f"logistic nv={nv} weighted={weighted}: {int((G != want).sum())} of {G.size} elements differ from numpy's fp32 exp")
        P1 = fos.prepare_weighted(torch.as_tensor(A).cuda(), b.astype(np.float64), np.ones(M_D), loss=rsp.LOGISTIC)
        v1 = P1.gradient_block(torch.as_tensor(X).cuda()).cpu().numpy()[:, :M_D].T / s[:, None]      # sigma(z) - b of the device, exactly
        v = v1.astype(F32) if w is None else v1.astype(F32) * w[:, None]
        want[:, :M_D] = ((v * Cn.astype(F32)).astype(F32) * s[:, None]).T
    diff = np.argwhere(G != want)
    assert G.shape == want.shape and np.array_equal(G, want), diff[:8]
    assert (loss16[nv:] == 0).all()                                      # the columns >= nv contribute 0
    Ad, Xd, bd = A.astype(np.float64), X.astype(np.float64), b.astype(np.float64)
    for oob in (False, True):
        if oob:
            none, got = _gradient(P, X, words, oob=True)
            assert none is None and (got[nv:] == 0).all()
            _, l = rsp.link32(loss, Z[:, :nv], b, w, Cn, True, C_D)
            W = (Cn == 0) * (1.0 if wd is None else wd[:, None])
        else:
            got, W = loss16, _W(Cn, wd)
        fp32_terms = l.astype(np.float64).sum(axis=0)
        exact, bound = rsp.data_term(loss, Ad, Xd, bd, W, C_D), rsp.loss_tolerance(loss, Ad, Xd, bd, W, C_D)
        print(f"{loss} nv={nv} weighted={weighted} oob={oob}: sums err/tol {(np.abs(got[:nv] - exact) / bound).max():.3f}")
        assert np.all(np.abs(got[:nv] - exact) <= bound), (got, exact, bound)
        if loss != rsp.LOGISTIC:         # the terms are the same fp32 numbers: their fp64 sums differ by the order of 259 additions
            assert np.all(np.abs(got[:nv] - fp32_terms) <= 259 * np.finfo(np.float64).eps * fp32_terms), (got, fp32_terms)


# ---- 2. gradient, data term, out-of-bag sums and the Gram operator against fp64 ----------------------------------------------------
CELLS = ((1, "bootstrap", True), (5, "binary", False), (16, "bootstrap", False), (16, "ones", True))      # (nv, counts, weighted)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(rsp.SHAPES))
@pytest.mark.parametrize("loss", LOSSES)
def test_gradient_sums_and_gram_against_fp64(fos, loss, name, kind):
    m, n = rsp.SHAPES[name]
    A64, b, c, _, _ = rsp.recipe(loss, kind, m, n)
    handles = {}
    for nv, recipe, weighted in CELLS:
        w = rsp.row_weights(m) if weighted else None
        if weighted not in handles:
            handles[weighted] = _handle(fos, loss, kind, A64, b, c, w)
        P = handles[weighted]
        Cn = rsp.counts(recipe, m, nv)
        words = _words(P, Cn)
        X = (0.3 * np.random.default_rng(m + nv).standard_normal((n, nv))).astype(F32)
        X[:, 0] = 0.0
        Xd = X.astype(np.float64)
        W = _W(Cn, w)
        G, loss16 = _gradient(P, X, words)
        G = G.astype(np.float64)[:, :n].T
        G_ref = rsp.gradient(loss, A64, Xd, b, W, c)
        err, g_tol = np.linalg.norm(G - G_ref, axis=0), rsp.gradient_tolerance(A64, Xd, b, W, G_ref)
        ref, tol = rsp.data_term(loss, A64, Xd, b, W, c), rsp.loss_tolerance(loss, A64, Xd, b, W, c)
        print(f"{loss} {name} {kind} nv={nv} {recipe} weighted={weighted}: gradient err/tol {(err / g_tol).max():.3f} "
              f"sums err/tol {(np.abs(loss16[:nv] - ref) / tol).max():.3f}")
        assert (err <= g_tol).all(), (err, g_tol)
        assert np.isfinite(loss16).all() and (np.abs(loss16[:nv] - ref) <= tol).all() and (loss16[nv:] == 0).all(), (loss16, ref, tol)
        Wo = (Cn == 0) * (1.0 if w is None else w[:, None])
        _, oob16 = _gradient(P, X, words, oob=True)
        ref, tol = rsp.data_term(loss, A64, Xd, b, Wo, c), rsp.loss_tolerance(loss, A64, Xd, b, Wo, c)
        assert (np.abs(oob16[:nv] - ref) <= tol).all() and (oob16[nv:] == 0).all(), (oob16, ref, tol)
        if recipe == "ones":
            assert (oob16 == 0).all()
        got = _np(_gram(P, X, words))
        ref = A64.T @ (W * (A64 @ Xd))
        err, g_tol = np.linalg.norm(got - ref, axis=0), rsp.gram_tolerance(A64, Xd, W, ref)
        print(f"   gram err/tol {(err / np.maximum(g_tol, 1e-300)).max():.3f}")
        assert got.shape == (n, nv) and (err <= g_tol).all(), (err, g_tol)


# ---- 3. the bitwise anchors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["edges", "panels"])
@pytest.mark.parametrize("loss", (rsp.HUBER, rsp.HINGE))
def test_anchors_against_the_existing_run_forms(fos, loss, name, kind):
    """c = 1 reproduces the pointwise link bit for bit, c = 0 its fold mask, and an integer count is a sample weight: the panel R
    holds the same values and everything after it is the same launches.  Derived, not measured."""
    from fastoptsolver_amd import _core
    m, n = rsp.SHAPES[name]
    A64, b, c, L, alphas = rsp.recipe(loss, kind, m, n)
    At = _device(kind, A64)
    P = _handle(fos, loss, kind, At, b, c)
    nv = 5
    many = [(a1 * 0.9 ** (j // 3), a2) for j in range(nv) for a1, a2 in [alphas[j % 3]]]
    params = [(1.0 / (L + a2), a1, a2) for a1, a2 in many]
    # all-ones counts: fos_fista_run_multi on the same handle
    a, r = _states(P, params), _states(P, params)
    assert _run_resampled(a, _words(P, np.ones((m, nv), dtype=np.int64)), ITERS) == 0 and _core.run_multi(r, ITERS)
    for x, y in zip(_xs(a), _xs(r)):
        assert np.array_equal(x, y) and np.count_nonzero(x) > 0
    # the complement of a fold assignment: fos_fista_run_multi_folds
    ids = np.random.default_rng(5).integers(0, 3, m).astype(np.uint8)
    held = [0, 1, 2, -1, 1]
    Cf = np.stack([(ids != h).astype(np.int64) for h in held], axis=1)
    a, r = _states(P, params), _states(P, params)
    assert _run_resampled(a, _words(P, Cf), ITERS) == 0 and _core.run_multi_folds(r, _core.fold_ids_tensor(ids, P.device), held, ITERS)
    for x, y in zip(_xs(a), _xs(r)):
        assert np.array_equal(x, y) and np.count_nonzero(x) > 0
    # one column of integer counts: a handle with those sample weights (the step leaves room for lambda_max up to 16 L)
    c1 = rsp.counts("bootstrap", m, 1)
    assert c1.max() == rsp.MAX_COUNT
    Pw = _handle(fos, loss, kind, At, b, c, c1[:, 0].astype(np.float64))
    one = [(1.0 / (16.0 * L), many[1][0], many[1][1])]
    a, r = _states(P, one), _states(Pw, one)
    assert _run_resampled(a, _words(P, c1), ITERS) == 0 and _core.run_multi(r, ITERS)
    assert np.array_equal(_xs(a)[0], _xs(r)[0]) and np.count_nonzero(_xs(a)[0]) > 0


# ---- 4. unit counts on squared and logistic handles ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["edges", "panels"])
@pytest.mark.parametrize("loss", (rsp.SQUARED, rsp.LOGISTIC))
def test_unit_counts_are_the_unit_weight_lockstep(fos, loss, name, kind):
    from fastoptsolver_amd import _core
    m, n = rsp.SHAPES[name]
    A64, b, c, L, alphas = rsp.recipe(loss, kind, m, n)
    Ld = L / rsp.divisor(loss)
    At = _device(kind, A64)
    P1 = fos.prepare_weighted(At, b, np.ones(m), loss=loss)
    Pu = fos.prepare(At, b, pad=True, loss=loss)
    params = [(1.0 / (Ld + a2), a1, a2) for a1, a2 in alphas]
    ones = np.ones((m, len(alphas)), dtype=np.int64)
    weighted, on_weighted, on_plain = _states(P1, params), _states(P1, params), _states(Pu, params)
    assert _core.run_multi(weighted, ITERS)
    assert _run_resampled(on_weighted, _words(P1, ones), ITERS) == 0 and _run_resampled(on_plain, _words(Pu, ones), ITERS) == 0
    xw, xa, xb = _xs(weighted), _xs(on_weighted), _xs(on_plain)
    for j, (a1, a2) in enumerate(alphas):
        x_ref, _ = rsp.run(loss, A64, b, np.ones(m), a1, a2, Ld, ITERS)
        errs = [_data.rel(x[j], x_ref) for x in (xw, xa, xb)]
        print(f"{loss} {name} {kind} alpha=({a1:.3g}, {a2}): rel err weighted lockstep {errs[0]:.2e}, resampled on it {errs[1]:.2e}, on the "
              f"unweighted handle {errs[2]:.2e}; bitwise equal to the weighted lockstep: {np.array_equal(xa[j], xw[j])}, {np.array_equal(xb[j], xw[j])}")
        assert np.linalg.norm(x_ref) > 0 and max(errs) < TOL, errs


# ---- 5. path parity --------------------------------------------------------------------------------------------------------------
def _v0(n, r):
    return np.random.default_rng(1000 + r).standard_normal(n)


@functools.lru_cache(maxsize=None)
def _path_case(loss, kind, name, B, weighted):
    """(counts m x B - bootstrap, one row per column at 15 -, L per resample from the oracle's power iteration on w * c_r)."""
    m, n = rsp.SHAPES[name]
    A64 = rsp.recipe(loss, kind, m, n)[0]
    w = rsp.row_weights(m) if weighted else None
    Cn = rsp.counts("bootstrap", m, B, seed=2)
    Ls = np.array([rsp.lipschitz(A64, rsp.effective(w, Cn[:, r]), _v0(n, r)) for r in range(B)])
    return Cn, Ls


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("loss", LOSSES)
def test_path_matches_the_reference(fos, loss, kind, weighted):
    """Six bootstrap resamples x three weights: 18 pairs, a full group and a partial one; every fit against its reference."""
    m, n = rsp.SHAPES["edges"]
    A64, b, c, _, alphas = rsp.recipe(loss, kind, m, n)
    B = 6
    w = rsp.row_weights(m) if weighted else None
    Cn, Ls = _path_case(loss, kind, "edges", B, weighted)
    P = _handle(fos, loss, kind, A64, b, c, w)
    res = fos.resampled_path(P, list(alphas), Cn, ITERS, L=Ls)
    coefs = _np(res.coefs)
    assert coefs.shape == (n, B, 3) and res.oob_loss is None and np.array_equal(res.L, Ls) and res.alphas == [tuple(a) for a in alphas]
    assert res.info == [[(ITERS, 0)] * 3] * B and fos.get_metrics()["grad_num_calls"] == 2 * ITERS
    worst = 0.0
    for r in range(B):
        for a, (a1, a2) in enumerate(alphas):
            x_ref, _ = rsp.run(loss, A64, b, rsp.effective(w, Cn[:, r]), a1, a2, Ls[r] / rsp.divisor(loss), ITERS, c=c)
            err = _data.rel(coefs[:, r, a], x_ref)
            worst = max(worst, err)
            assert np.linalg.norm(x_ref) > 0 and err < TOL, (r, a, err)
    print(f"{loss} {kind} weighted={weighted}: worst rel err of 18 fits {worst:.3e}")


@pytest.mark.parametrize("delta", [None, 3.0], ids=["fista", "delta"])
@pytest.mark.parametrize("cell", [(rsp.SQUARED, "f32"), (rsp.LOGISTIC, "bf16"), (rsp.HUBER, "bf16"), (rsp.HINGE, "f32")], ids=lambda c: "-".join(c))
def test_path_at_two_panels(fos, cell, delta):
    """70001 rows are two row panels: the words of the second are offset by the first's rows."""
    loss, kind = cell
    m, n = rsp.SHAPES["panels"]
    A64, b, c, _, alphas = rsp.recipe(loss, kind, m, n)
    Cn, Ls = _path_case(loss, kind, "panels", 2, False)
    P = _handle(fos, loss, kind, A64, b, c)
    res = fos.resampled_path(P, list(alphas), Cn, ITERS, L=Ls, delta=delta)
    coefs = _np(res.coefs)
    for r, a in ((0, 0), (1, 1), (1, 2)):
        a1, a2 = alphas[a]
        x_ref, _ = rsp.run(loss, A64, b, Cn[:, r].astype(np.float64), a1, a2, Ls[r] / rsp.divisor(loss), ITERS, c=c, delta=delta)
        err = _data.rel(coefs[:, r, a], x_ref)
        print(f"{loss} {kind} delta={delta} resample {r} alpha=({a1:.3g}, {a2}) rel err {err:.3e}")
        assert np.linalg.norm(x_ref) > 0 and err < TOL, (r, a, err)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("loss", LOSSES)
def test_device_control_per_column(fos, loss, kind):
    m, n = rsp.SHAPES["edges"]
    A64, b, c, L, alphas = rsp.recipe(loss, kind, m, n)
    ctl, Cn, keep, refs = rsp.controlled_case(loss, kind)
    print(ctl, "cells", keep, "reference iterations", [k for _, k in refs])
    P = _handle(fos, loss, kind, A64, b, c)
    res = fos.resampled_path(P, list(alphas), Cn, rsp.CONTROL_ITERS, L=L, **ctl)
    coefs = _np(res.coefs)
    for (r, a), (x_ref, k_ref) in zip(keep, refs):
        assert res.info[r][a] == (k_ref, 2 if k_ref < rsp.CONTROL_ITERS else 0), (r, a, res.info[r][a], k_ref)    # FOS_STOP_RATIO
        assert _data.rel(coefs[:, r, a], x_ref) < TOL, (r, a)


@pytest.mark.parametrize("loss", (rsp.HUBER, rsp.HINGE))
def test_penalty_factors_bounds_and_feature_groups_compose(fos, loss):
    m, n = rsp.SHAPES["edges"]
    A64, b, c, _, alphas = rsp.recipe(loss, "f32", m, n)
    Cn, Ls = _path_case(loss, "f32", "edges", 6, False)
    Cn, Ls = Cn[:, :2], Ls[:2]
    a1 = alphas[1][0]
    pf = np.random.default_rng(4).uniform(0.5, 2.0, n).astype(F32).astype(np.float64)
    pf[-1] = 0.0
    lo = np.zeros(n)
    P = _handle(fos, loss, "f32", A64, b, c)
    P.set_penalty(pf, lower=0.0)
    coefs = _np(fos.resampled_path(P, [(a1, 0.0)], Cn, ITERS, L=Ls).coefs)
    for r in range(2):
        wr = Cn[:, r].astype(np.float64)
        ref = lk.CoordLinkProblem(loss, A64, b, a1, 0.0, c, wr).bind(pf, lo, None)
        x_ref, _ = rsp.run(loss, A64, b, wr, a1, 0.0, Ls[r], ITERS, prob=ref)
        free, _ = rsp.run(loss, A64, b, wr, a1, 0.0, Ls[r], ITERS, prob=lk.CoordLinkProblem(loss, A64, b, a1, 0.0, c, wr).bind(pf))
        assert (free < 0).any() and (coefs[:, r, 0] >= 0).all() and _data.rel(coefs[:, r, 0], x_ref) < TOL, (r, _data.rel(coefs[:, r, 0], x_ref))
    P = _handle(fos, loss, "f32", A64, b, c)
    start, gw = fg.layout("small", n, seed=2)
    P.set_feature_groups(np.repeat(np.arange(len(start) - 1), np.diff(start)), gw, 0.5)
    for r in range(2):
        wr = Cn[:, r].astype(np.float64)
        g0 = -rsp.gradient(loss, A64, np.zeros((n, 1)), b, wr[:, None], c)[:, 0]
        amax = fg.alpha_max(g0, np.asarray(start), fg.weights_of(start, gw), 0.5)
        x = _np(fos.resampled_path(P, [(0.2 * amax, 0.0)], Cn[:, r:r + 1], ITERS, L=Ls[r:r + 1]).coefs)[:, 0, 0]
        ref = fg._fgroup_class(lk.LinkProblem)(loss, A64, b, 0.2 * amax, 0.0, c, wr).bind(start, gw, 0.5)
        x_ref, _ = rsp.run(loss, A64, b, wr, 0.2 * amax, 0.0, Ls[r], ITERS, prob=ref)
        zero, _ = fg.zero_groups(x_ref, np.asarray(start))
        assert zero.any() and (~zero).any() and _data.rel(x, x_ref) < TOL, (r, _data.rel(x, x_ref))
        assert np.array_equal(fg.zero_groups(x, np.asarray(start))[0], zero)


# ---- 6. the power iteration per resample -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("kind", KINDS)
def test_resampled_lipschitz_is_the_power_iteration_per_resample(fos, kind, weighted):
    """18 resamples - a group of 16 and one of 2 - bootstrap and 0/1 mixed; the start vectors are the draws of the global stream.
    The tolerance is tests/test_gpu_power.py's for the weighted route (tests/_power.TOL, relative)."""
    from tests import _power as pw
    m, n = rsp.SHAPES["edges"]
    A64, b, _, L_whole, _ = rsp.recipe(rsp.SQUARED, kind, m, n)
    w = rsp.row_weights(m) if weighted else None
    Cn = np.concatenate([rsp.counts("bootstrap", m, 16, seed=1), rsp.counts("binary", m, 2, seed=1)], axis=1)
    P = _handle(fos, rsp.SQUARED, kind, A64, b, None, w)
    np.random.seed(11)
    got = fos.resampled_lipschitz(P, Cn)
    after = np.random.randn()
    np.random.seed(11)
    v0 = [np.random.randn(n) for _ in range(18)]
    assert after == np.random.randn()                                      # one draw of n normals per resample, in order
    ref = np.array([rsp.lipschitz(A64, rsp.effective(w, Cn[:, r]), v0[r]) for r in range(18)])
    print(f"{kind} weighted={weighted}: worst rel err {np.abs(got / ref - 1).max():.2e}; whole A {L_whole:.1f}, resamples {ref.min():.1f} .. {ref.max():.1f}")
    assert got.shape == (18,) and got.dtype == np.float64 and np.allclose(got, ref, rtol=pw.TOL, atol=0)
    if not weighted:
        top = float(np.linalg.eigvalsh(A64.T @ A64)[-1])
        assert (ref[:16] > top).any() and (ref[16:] < top).all()           # a bootstrap column exceeds the whole A; a subsample never does


# ---- 7. stability selection end to end ----------------------------------------------------------------------------------------------
def test_stability_selection_end_to_end(fos):
    d = rsp.stability_case()
    nonzero, near = rsp.stability_reference()
    m, n = rsp.ST_SHAPE
    P = fos.prepare(torch.as_tensor(d["A"].astype(F32)).cuda(), d["b"])
    res = fos.stability_selection(P, list(d["alphas"]), n_pairs=rsp.ST_PAIRS, fraction=0.5, threshold=0.6, seed=0, max_iter=rsp.ST_ITERS,
                                  L=d["L"])
    assert res.frequency.shape == (len(d["alphas"]), n) and np.array_equal(res.max_frequency, res.frequency.max(axis=0))
    coefs = _np(fos.resampled_path(P, list(d["alphas"]), d["counts"], rsp.ST_ITERS, L=d["L"]).coefs)        # the same fits, cell by cell
    got = np.transpose(coefs != 0, (1, 2, 0))
    assert np.array_equal(fos.selection_frequencies(coefs), res.frequency)
    decided = ~near
    print(f"left out {int(near.sum())} of {near.size} cells; differing decided cells {int((got != nonzero)[decided].sum())}, "
          f"differing cells near the threshold {int((got != nonzero)[near].sum())}")
    assert near.mean() <= rsp.ST_LEFT_OUT and np.array_equal(got[decided], nonzero[decided])
    # the frequencies equal the reference's wherever no left-out cell enters them
    ref_freq, clean = nonzero.mean(axis=0), ~near.any(axis=0)
    assert np.array_equal(res.frequency[clean], ref_freq[clean])
    assert set(d["support"]) <= set(res.selected.tolist()) and np.array_equal(res.selected, np.flatnonzero(res.max_frequency >= 0.6))
    off = np.setdiff1d(np.arange(n), d["support"])
    assert ((res.frequency[-1, off] > 0) & (res.frequency[-1, off] < 1)).any()


# ---- 8. the out-of-bag loss -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("loss", LOSSES)
def test_out_of_bag_loss(fos, loss, weighted):
    m, n = rsp.SHAPES["edges"]
    A64, b, c, _, alphas = rsp.recipe(loss, "f32", m, n)
    w = rsp.row_weights(m) if weighted else None
    Cn, Ls = _path_case(loss, "f32", "edges", 6, weighted)
    P = _handle(fos, loss, "f32", A64, b, c, w)
    res = fos.resampled_path(P, list(alphas), Cn, ITERS, L=Ls, oob=True)
    out = Cn == 0
    size = out.sum(axis=0).astype(np.float64) if w is None else (w[:, None] * out).sum(axis=0)
    assert res.oob_loss.shape == (6, 3) and res.oob_size.shape == (6,) and np.allclose(res.oob_size, size, rtol=1e-12, atol=0) and (size > 0).all()
    coefs = _np(res.coefs)
    for r in range(6):
        X32 = coefs[:, r, :].astype(F32).astype(np.float64)                # the pass over A reads x in fp32
        Wo = np.repeat((out[:, r] * (1.0 if w is None else w))[:, None], 3, axis=1)
        ref, tol = rsp.data_term(loss, A64, X32, b, Wo, c), rsp.loss_tolerance(loss, A64, X32, b, Wo, c)
        assert np.isfinite(res.oob_loss[r]).all() and (np.abs(res.oob_loss[r] - ref) <= tol).all(), (r, res.oob_loss[r], ref, tol)
        mean_ref = rsp.loss_terms(loss, A64, X32, b, c)[out[:, r]]
        if w is None:                                                      # the reference's mean loss on the rows with count 0
            assert np.all(np.abs(res.oob_loss[r] / res.oob_size[r] - mean_ref.mean(axis=0)) <= tol / size[r])


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("cell", [(rsp.SQUARED, "f32"), (rsp.LOGISTIC, "bf16")], ids=lambda c: "-".join(c))
def test_out_of_bag_loss_at_two_panels(fos, cell, weighted):
    """resampled_path(..., oob=True) on 70001 rows: the out-of-bag form of the link reads counts, b and the weights of the second
    panel at + row0, and its partial sums are copied behind the first panel's (ws.grad_part) before the fold."""
    loss, kind = cell
    m, n = rsp.SHAPES["panels"]
    A64, b, c, _, alphas = rsp.recipe(loss, kind, m, n)
    w = rsp.row_weights(m) if weighted else None
    Cn, Ls = _path_case(loss, kind, "panels", 2, weighted)
    P = _handle(fos, loss, kind, A64, b, c, w)
    first = 256 * P.plan()["cus"]                                          # the rows of the first panel
    out = Cn == 0
    live = out if w is None else out & (w > 0)[:, None]
    assert m > first and live[:first].any(axis=0).all() and live[first:].any(axis=0).all()
    res = fos.resampled_path(P, list(alphas), Cn, ITERS, L=Ls, oob=True)
    size = out.sum(axis=0).astype(np.float64) if w is None else (w[:, None] * out).sum(axis=0)
    assert res.oob_loss.shape == (2, 3) and np.allclose(res.oob_size, size, rtol=1e-12, atol=0) and (size > 0).all()
    coefs = _np(res.coefs)
    for r in range(2):
        X32 = coefs[:, r, :].astype(F32).astype(np.float64)                # the pass over A reads x in fp32
        assert np.count_nonzero(X32, axis=0).all()
        Wo = np.repeat((out[:, r] * (1.0 if w is None else w))[:, None], 3, axis=1)
        ref, tol = rsp.data_term(loss, A64, X32, b, Wo, c), rsp.loss_tolerance(loss, A64, X32, b, Wo, c)
        second = rsp.data_term(loss, A64[first:], X32, b[first:], Wo[first:], c)
        print(f"{loss} {kind} weighted={weighted} resample {r}: oob sums err/tol {(np.abs(res.oob_loss[r] - ref) / tol).max():.3f}, "
              f"the second panel's share / tol {(second / tol).min():.1f}")
        assert (second > 10.0 * tol).all()                                 # a sum that lost or misplaced the second panel is out of bounds
        assert np.isfinite(res.oob_loss[r]).all() and (np.abs(res.oob_loss[r] - ref) <= tol).all(), (r, res.oob_loss[r], ref, tol)


# ---- 9. handle hygiene ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", (rsp.SQUARED, rsp.HUBER))
def test_a_handle_that_ran_resampled_serves_the_other_forms_as_a_fresh_one(fos, loss):
    from fastoptsolver_amd import _core
    m, n = rsp.SHAPES["panels"]
    A64, b, c, L, alphas = rsp.recipe(loss, "f32", m, n)
    At = _device("f32", A64)
    params = [(1.0 / (16.0 * L + a2), a1, a2) for a1, a2 in alphas]
    Cn = rsp.counts("bootstrap", m, 3, seed=2)

    def plain(P):
        hs = _states(P, params)
        assert _core.run_multi(hs, ITERS)
        return _xs(hs)

    def resampled(P):
        hs = _states(P, params)
        assert _run_resampled(hs, _words(P, Cn), ITERS) == 0
        return _xs(hs)

    fresh_plain, fresh_resampled = plain(_handle(fos, loss, "f32", At, b, c)), resampled(_handle(fos, loss, "f32", At, b, c))
    P = _handle(fos, loss, "f32", At, b, c)
    first, second = resampled(P), plain(P)
    assert all(np.array_equal(x, y) for x, y in zip(first, fresh_resampled)) and all(np.array_equal(x, y) for x, y in zip(second, fresh_plain))
    Q = _handle(fos, loss, "f32", At, b, c)
    first, second = plain(Q), resampled(Q)
    assert all(np.array_equal(x, y) for x, y in zip(first, fresh_plain)) and all(np.array_equal(x, y) for x, y in zip(second, fresh_resampled))
    assert any(not np.array_equal(x, y) for x, y in zip(fresh_plain, fresh_resampled)) and all(np.count_nonzero(x) for x in fresh_plain)
    # the same state machines go on in another form: plain after resampled on the handles themselves
    hs = _states(P, params)
    assert _run_resampled(hs, _words(P, Cn), 10) == 0 and _core.run_multi(hs, 5)
    assert all(int(st.status().k) == 15 for st in hs)


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------------
def _snapshot(hs):
    out = []
    for st in hs:
        s = st.status()
        out.append((st.x_tensor().clone(), tuple(getattr(s, k) for k, _ in s._fields_)))
    return out


def _same(a, b):
    return all(torch.equal(x, y) and s == t for (x, s), (y, t) in zip(a, b))


def test_refusals_leave_the_handles_untouched(fos):
    from fastoptsolver_amd import _core, _lib, distributed
    m, n = rsp.SHAPES["edges"]
    A64, b, _, L, alphas = rsp.recipe(rsp.SQUARED, "f32", m, n)
    At = _device("f32", A64)
    params = [(1.0 / L, a1, 0.0) for a1, _ in alphas[:2]]
    Cn = rsp.counts("binary", m, 2)

    def refused(P, hs, what, run=True, grad=True, gram=True):
        words, X = _words(P, Cn), np.zeros((P.n, 2), dtype=F32)
        before = _snapshot(hs)
        if run:
            assert _run_resampled(hs, words, 5) == UNSUPPORTED
            msg = P.lib.fos_last_error().decode()
            assert "fos_fista_run_multi_resampled" in msg and what in msg, msg
            assert _run_resampled(hs, words, 0) == UNSUPPORTED                # before the return of a call of no iterations
        if grad:
            with pytest.raises(_lib.FosError, match="fos_gradient_batch_resampled"):
                _gradient(P, X, words)
        if gram:
            with pytest.raises(_lib.FosError, match="fos_gram_apply_resampled"):
                _gram(P, X, words)
        assert _same(before, _snapshot(hs))

    # a multinomial problem
    y3 = np.random.default_rng(1).integers(0, 3, m)
    y3[:3] = [0, 1, 2]
    Pm = fos.prepare_multinomial(At, y3)
    hs = _states(Pm, [(1.0 / L, 0.1, 0.0)] * 3)
    assert _core.run_multi(hs, 3)
    refused(Pm, hs, "multinomial")
    with pytest.raises(_lib.FosError, match="multinomial problem is not served"):
        fos.resampled_path(Pm, [(0.1, 0.0)], Cn, 5, L=L)
    with pytest.raises(_lib.FosError, match="multinomial problem is not served"):
        fos.stability_selection(Pm, [(0.1, 0.0)], n_pairs=1, max_iter=5, L=L)
    with pytest.raises(_lib.FosError, match="multinomial problem is not served"):
        fos.resampled_lipschitz(Pm, Cn)
    # a problem without b: the loss-free operator serves it
    Pn = fos.prepare(At)
    hs = _states(Pn, params)
    refused(Pn, hs, "needs b", gram=False)
    assert _gram(Pn, np.zeros((n, 2), dtype=F32), _words(Pn, Cn)).shape == (n, 2)
    with pytest.raises(_lib.FosError, match="needs b"):
        fos.resampled_path(Pn, [(0.1, 0.0)], Cn, 5, L=L)
    # a shape without the matrix-core pair: a plain squared handle of at most 64 columns
    Ps = fos.prepare(At[:, :40].contiguous(), b)
    hs = _states(Ps, params)
    refused(Ps, hs, "matrix-core pair")
    with pytest.raises(_lib.FosError, match="matrix-core pair"):
        fos.resampled_path(Ps, [(0.1, 0.0)], Cn, 5, L=L)
    # a row-sharded and a column-sharded problem (one-rank communicators)
    comm = distributed.Comm.solo()
    Pr = fos.prepare(At, b)
    Pr.set_comm(comm)
    refused(Pr, _states(Pr, params), "sharded")
    wide = torch.as_tensor(np.random.default_rng(2).standard_normal((m, 260)).astype(F32)).cuda()     # column sharding needs the streaming layout
    Pc = fos.prepare(wide, b)
    Pc.set_comm_cols(comm)
    refused(Pc, _states(Pc, params), "sharded")
    # handles under the group penalty across columns, the gradient-norm rule, the fp64 split gradient
    P = fos.prepare_weighted(At, b, np.ones(m))
    words = _words(P, Cn)
    for what, make in (("group penalty", lambda: _states(P, params, group=2)),
                       ("gradient-norm", lambda: _states(P, params, tol_grad=1e-3)),
                       ("fp64 split gradient", lambda: [st.set_precise(True) or st for st in _states(P, params)])):
        hs = make()
        before = _snapshot(hs)
        for iters in (5, 0):
            assert _run_resampled(hs, words, iters) == UNSUPPORTED, what
            msg = P.lib.fos_last_error().decode()
            assert "fos_fista_run_multi_resampled" in msg and what in msg, msg
        assert _same(before, _snapshot(hs))
    # a controlled run of two families is the shared refusal of the lockstep
    mixed = _states(P, params[:1], tol_ratio=0.1) + _states(P, params[1:], tol_ratio=0.1, mode=_lib.MODE_DELTA, delta=3.0)
    assert _run_resampled(mixed, words, 5) == UNSUPPORTED and "one family" in P.lib.fos_last_error().decode()
    # ... and the same handle serves
    ok = _states(P, params)
    assert _run_resampled(ok, words, 5) == 0 and all(int(st.status().k) == 5 for st in ok)
