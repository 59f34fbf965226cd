"""GPU: the Huber and squared-hinge losses in the lockstep - the pointwise link kernel per element, fos_gradient_batch and
fos_residual_batch on such a problem, huber_path / hinge_path, their CV, objectives and working-set solve.

Every fit must equal the fp64 reference of tests/_link.py (the oracle's FistaProblem with the gradient replaced: the same
momentum, restart and stop rules) within 1e-5 relative, on the bf16-rounded A for bf16 storage; L = lambda_max(A^T W A) comes from
the oracle's power iteration and is passed to both sides.  Loss sums are compared against fp64 on the kernel's OWN x rounded to
fp32 within tests/_link.loss_tolerance.  The link kernel's arithmetic is specified per element, so through a diagonal A its
output is compared with the same fp32 expressions in numpy EXACTLY, and with a threshold no residual reaches huber_path is
bitwise fista_path on a handle with unit row weights."""
import functools

import numpy as np
import pytest
import torch

from tests import _data, _fgroup as fg, _link as lk, _working_set as ws

pytestmark = pytest.mark.gpu

TOL, ITERS = lk.TOL, lk.ITERS
KINDS = ("f32", "bf16")
LOSSES = (lk.HUBER, lk.HINGE)
SHAPES = {"one_tile": (257, 37), "edges": (1003, 68), "rb2": (33000, 68), "panels": (70001, 68)}
F32 = np.float32


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def _bf16(A32):
    return torch.as_tensor(A32).to(torch.bfloat16).to(torch.float64).numpy()


def _device(kind, A64):
    return torch.as_tensor(A64.astype(np.float32)).to(torch.bfloat16 if kind == "bf16" else torch.float32).cuda()


@functools.lru_cache(maxsize=None)
def _recipe(loss, kind, m, n):
    """(A as the device stores it in fp64, b or labels, c or None, L, the three weights): once per shape, never modified.  The
    branch mix is asserted on the fp32 matrix (bf16 rounding moves no share by more than a few rows)."""
    rnd = _bf16 if kind == "bf16" else None
    if loss == lk.HUBER:
        A64, b, c, L, alphas = lk.huber_recipe(m, n, round_a=rnd, check=kind == "f32")
    else:
        A64, b, L, alphas = lk.hinge_recipe(m, n, 3 * m + n, round_a=rnd, check=kind == "f32")
        c = None
    for a in (A64, b):
        a.setflags(write=False)
    return A64, b, c, L, alphas


def _handle(fos, loss, kind, A64, b, c, **kw):
    At = _device(kind, A64) if isinstance(A64, np.ndarray) else A64
    return fos.prepare_huber(At, b, c, **kw) if loss == lk.HUBER else fos.prepare_hinge(At, b, **kw)


def _path(fos, loss):
    return fos.huber_path if loss == lk.HUBER else fos.hinge_path


@functools.lru_cache(maxsize=None)
def _ref(loss, kind, m, n, a1, a2, iters, delta, rows=None, wkey=None, **kw):
    """(x, iterations) of the reference; rows: (fold, K, split) -> the fit on the other rows; wkey: the weights of `_weights`."""
    A64, b, c, L, _ = _recipe(loss, kind, m, n)
    w = None if wkey is None else _weights(m, wkey)
    if wkey is not None:
        L = lk.lipschitz(A64, 1, w)
    if rows is not None:
        keep = _ids(m, rows[1], rows[2]) != rows[0]
        A64, b, w = A64[keep], b[keep], None if w is None else w[keep]
    x, k = lk.run(loss, A64, b, a1, a2, L, iters, c=c, w=w, delta=delta, **kw)
    x.setflags(write=False)
    return x, k


@functools.lru_cache(maxsize=None)
def _weights(m, key):
    rng = np.random.default_rng(77)
    if key == "01":
        w = (rng.random(m) < 0.7).astype(np.float64)
    else:
        w = rng.uniform(0.25, 4.0, m).astype(np.float32).astype(np.float64)
        w[rng.choice(m, m // 20, replace=False)] = 0.0
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _ids(m, K, split):
    ids = (np.arange(m) * K // m) if split == "contiguous" else np.random.default_rng(5).integers(0, K, m)
    ids = ids.astype(np.uint8)
    ids.setflags(write=False)
    return ids


# ---- 1. the link per element, through a diagonal A ----------------------------------------------------------------------------
M_D, N_D, C_D = 259, 260, 0.5


@functools.lru_cache(maxsize=None)
def _diagonal(loss):
    """(s, b, Z): A = diag(s) (259 x 260, powers of two), and the 259 x 16 panel Z = A X the kernel must see, with planted rows."""
    rng = np.random.default_rng(31)
    s = rng.choice([0.5, 1.0, 2.0], M_D).astype(F32)
    s[:16] = 1.0
    Z = rng.standard_normal((M_D, 16)).astype(F32)
    if loss == lk.HUBER:
        b = rng.standard_normal(M_D).astype(F32)
        b[:8] = [0.25, -0.25, 1.5, 0.0, 0.0, 0.0, 0.0, 0.0]
        planted = [C_D, -C_D, 0.0, 1e30, -1e30, np.nextafter(F32(C_D), F32(1)), -np.nextafter(F32(C_D), F32(1)), np.nextafter(F32(C_D), F32(0))]
        for i, r in enumerate(planted):                                   # r = z - b exactly: b and r share the binade or b = 0
            Z[i, :] = F32(r) + b[i] if abs(r) < 4 else F32(r)
            if abs(r) >= 4:
                b[i] = 0.0
            assert F32(Z[i, 0] - b[i]) == F32(r)
    else:
        b = rng.choice([-1.0, 1.0], M_D).astype(F32)
        b[:8] = [1, -1, 1, -1, 1, -1, 1, -1]
        one = F32(1)
        planted = [one, one, np.nextafter(one, F32(2)), np.nextafter(one, F32(2)), np.nextafter(one, F32(0)), np.nextafter(one, F32(0)),
                   F32(-1e15), F32(-1e15)]
        for i, t in enumerate(planted):                                   # margin t = b z
            Z[i, :] = b[i] * t
    b[8:16] = b[:8]                                                       # the planted values again, in some columns only
    Z[8:16] = np.where(rng.random((8, 16)) < 0.5, Z[:8], Z[8:16])
    for a in (s, b, Z):
        a.setflags(write=False)
    return s, b, Z


def _link32(loss, Z, b, w, c=C_D):
    """The kernel's per-element expressions in numpy fp32, in its order: (v, l), both times w."""
    b = b[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        if loss == lk.HUBER:
            r = Z - b
            v = np.minimum(np.maximum(r, F32(-c)), F32(c))
            l = np.where(np.abs(r) <= F32(c), (F32(0.5) * r) * r, F32(c) * np.abs(r) - F32(0.5) * F32(c) * F32(c))
        else:
            u = np.maximum(F32(0), F32(1) - b * Z)
            v = -b * u
            l = (F32(0.5) * u) * u
    assert v.dtype == F32 and l.dtype == F32
    if w is not None:
        v, l = v * w[:, None], l * w[:, None]
    return v.astype(F32), l.astype(F32)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("nv", [1, 5, 16])
@pytest.mark.parametrize("loss", LOSSES)
def test_the_link_per_element_through_a_diagonal_matrix(fos, loss, nv, weighted):
    s, b, Z = _diagonal(loss)
    A = np.zeros((M_D, N_D), dtype=F32)
    A[np.arange(M_D), np.arange(M_D)] = s
    w = None
    if weighted:
        w = np.random.default_rng(9).uniform(0.25, 4.0, M_D).astype(F32)
        w[::17] = 0.0
        w[3], w[4] = 2.0, 0.5                                            # exact products with the 1e30 rows
    P = _handle(fos, loss, "f32", torch.as_tensor(A).cuda(), b.astype(np.float64), C_D, sample_weight=w)
    X = np.zeros((N_D, nv), dtype=F32)
    X[:M_D] = Z[:, :nv] / s[:, None]                                     # exact: s is a power of two
    G, loss16 = P.gradient_block(torch.as_tensor(X).cuda(), want_loss=True)
    tail = P.scratch[nv:16].cpu().numpy()
    G = G.cpu().numpy()
    v, l = _link32(loss, Z[:, :nv], b, w)
    want = np.zeros((nv, P.n_dev), dtype=F32)
    want[:, :M_D] = (v * s[:, None]).T                                   # G[j, i] = s_i v_ij: one non-zero product per sum
    assert G.shape == want.shape and np.array_equal(G, want), np.argwhere(G != want)[:8]
    assert (tail == 0).all()                                             # the columns >= nv contribute 0
    ref = l.astype(np.float64).sum(axis=0)
    got = np.asarray(loss16)
    # the terms are the same fp32 numbers; their fp64 sums differ by the order of at most 259 additions of non-negative terms
    assert np.all(np.abs(got - ref) <= 259 * np.finfo(np.float64).eps * ref), (got, ref)
    Xd = X.astype(np.float64)
    bound = lk.loss_tolerance(loss, A.astype(np.float64), Xd, b.astype(np.float64), C_D, w)
    exact = lk.data_term(loss, A.astype(np.float64), Xd, b.astype(np.float64), C_D, w)
    assert np.all(np.abs(got - exact) <= bound), (got, exact, bound)
    assert np.allclose(P.residual_batch(torch.as_tensor(X).cuda(), use_b=True), got, rtol=1e-14, atol=0)


# ---- 2. generic A: gradient and sums against fp64 -------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("m", [257, 1003])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("loss", LOSSES)
def test_gradient_and_sums_against_fp64(fos, loss, kind, m, weighted):
    n, nv = 68, 7
    A64, b, c, L, alphas = _recipe(loss, kind, m, n)
    w = _weights(m, "frac") if weighted else None
    P = _handle(fos, loss, kind, A64, b, c, sample_weight=w)
    X = (0.3 * np.random.default_rng(m).standard_normal((n, nv))).astype(F32)
    X[:, 0] = 0.0
    Xd = X.astype(np.float64)
    G, loss16 = P.gradient_block(torch.as_tensor(X).cuda(), want_loss=True)
    G = _np(G)[:, :n].T
    G_ref = lk.gradient(loss, A64, Xd, b, c, w)
    sw = np.ones(m) if w is None else np.sqrt(w)
    # psi is 1-Lipschitz in z: the residual bound of the squared pass holds for it, on the rows scaled by sqrt(w) as the
    # weighted squared pass is judged (tests/test_gpu_working_set.py)
    g_tol, _ = _data.fp32_pass_tolerances_cols(sw[:, None] * A64, Xd, sw * np.abs(b), G_ref, np.ones(nv))
    err = np.linalg.norm(G - G_ref, axis=0)
    print(f"{loss} {kind} m={m} weighted={weighted}: gradient err/tol {(err / g_tol).max():.3f}")
    assert (err <= g_tol).all(), (err, g_tol)
    ref, tol = lk.data_term(loss, A64, Xd, b, c, w), lk.loss_tolerance(loss, A64, Xd, b, c, w)
    for got in (np.asarray(loss16), np.asarray(P.residual_batch(torch.as_tensor(X).cuda(), use_b=True))):
        print(f"   sums err/tol {(np.abs(got - ref) / tol).max():.3f}")
        assert np.isfinite(got).all() and (np.abs(got - ref) <= tol).all(), (got, ref, tol)
    ids = _ids(m, 3, "random")
    held = [j % 3 for j in range(nv)]
    got = np.asarray(P.residual_batch_folds(torch.as_tensor(X).cuda(), fos._core.fold_ids_tensor(ids, P.device), held))
    for j in range(nv):
        te = ids == held[j]
        wj = None if w is None else w[te]
        rj = lk.data_term(loss, A64[te], Xd[:, j], b[te], c, wj)
        tj = lk.loss_tolerance(loss, A64[te], Xd[:, j:j + 1], b[te], c, wj)[0]
        assert abs(got[j] - rj) <= tj, (j, got[j], rj, tj)


# ---- 3. one lockstep iteration from a given X0 with 16 different steps ----------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "weighted", "train_mask"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("loss", LOSSES)
def test_one_iteration_is_a_gradient_step(fos, loss, kind, form):
    from fastoptsolver_amd import _core
    m, n = SHAPES["edges"]
    A64, b, c, L, _ = _recipe(loss, kind, m, n)
    w = _weights(m, "frac") if form == "weighted" else None
    P = _handle(fos, loss, kind, A64, b, c, sample_weight=w)
    X0 = (0.2 * np.random.default_rng(3).standard_normal((n, 16))).astype(F32).astype(np.float64)
    taus = [(0.3 + 0.05 * j) / L for j in range(16)]
    hs = []
    for j in range(16):
        st = _core.Fista(P)
        st.reset(taus[j], 0.0, 0.0, x0=X0[:, j])
        hs.append(st)
    ids, held = _ids(m, 4, "random"), [j % 5 - 1 for j in range(16)]       # -1: a column that keeps every row
    if form == "train_mask":
        assert _core.run_multi_folds(hs, _core.fold_ids_tensor(ids, P.device), held, 1)
    else:
        assert _core.run_multi(hs, 1)
    for j, st in enumerate(hs):
        keep = ids != held[j] if form == "train_mask" else np.ones(m, bool)
        g_ref = lk.gradient(loss, A64[keep], X0[:, j], b[keep], c, None if w is None else w[keep])
        g = (X0[:, j] - _np(st.x_tensor())) / taus[j]
        assert _data.rel(g, g_ref) < TOL, (j, _data.rel(g, g_ref))


# ---- 4. path parity ------------------------------------------------------------------------------------------------------------
def _many(alphas, count):
    return [(a1 * 0.93 ** (j // 3), a2) for j in range(count) for a1, a2 in [alphas[j % 3]]]


@pytest.mark.parametrize("delta", [None, 3.0], ids=["fista", "delta"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("loss", LOSSES)
def test_path_matches_the_reference(fos, loss, name, kind, delta):
    m, n = SHAPES[name]
    A64, b, c, L, alphas = _recipe(loss, kind, m, n)
    count = 18                                                            # a full group and a partial one of two columns
    many = _many(alphas, count)
    P = _handle(fos, loss, kind, A64, b, c)
    assert P.n == n and P.n_dev >= 68
    xs, info = _path(fos, loss)(P, None, many, max_iter=ITERS, L=L, delta=delta, return_info=True)
    assert len(xs) == count and info == [(ITERS, 0)] * count, info
    assert fos.get_metrics()["grad_num_calls"] == 2 * ITERS
    for j in (0, 1, 2, count - 1):                                        # the three kinds of weight, and the partial group
        a1, a2 = many[j]
        x_ref, _ = _ref(loss, kind, m, n, a1, a2, ITERS, delta)
        err = _data.rel(_np(xs[j]), x_ref)
        print(f"{loss} {name} {kind} delta={delta} alpha=({a1:.3g}, {a2}) rel err {err:.3e} nnz {int(np.count_nonzero(x_ref))}")
        assert np.linalg.norm(x_ref) > 0 and err < TOL, (a1, a2, err)


# ---- 5. controlled runs -----------------------------------------------------------------------------------------------------------
CONTROL_MENU = (dict(adaptive_restart=True, restart_threshold=1.0, tol_ratio=0.1), dict(adaptive_restart=True, restart_threshold=0.9, tol_ratio=0.2))


@functools.lru_cache(maxsize=None)
def _controlled(loss, kind):
    """(control, weights, reference (x, iterations) per weight) of the controlled check on 1003 x 68: the first entry of
    CONTROL_MENU under which at least three of nine weights have fp32-proof restart and stop decisions on the reference
    (tests/_coord.fp32_proof: the device decides on fp32 step norms, so a ratio within rounding of its threshold is no case), some
    stopping early and not all at the same iteration.  Decided on the reference alone."""
    from tests import _coord as cd
    m, n = SHAPES["edges"]
    A64, b, c, L, alphas = _recipe(loss, kind, m, n)
    for ctl in CONTROL_MENU:
        keep, refs = [], []
        for a1, a2 in _many(alphas, 9):
            tr = {}
            x, k = lk.run(loss, A64, b, a1, a2, L, 60, c=c, trace=tr, **ctl)
            if cd.fp32_proof(tr, ctl["restart_threshold"], ctl["tol_ratio"]):
                keep.append((a1, a2))
                refs.append((x, k))
        ks = [k for _, k in refs]
        if len(keep) >= 3 and min(ks) < 60 and len(set(ks)) >= 2:
            return ctl, keep, refs
    raise AssertionError("no entry of CONTROL_MENU gives the case three controlled runs with fp32-proof decisions")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("loss", LOSSES)
def test_device_control_per_column(fos, loss, kind):
    m, n = SHAPES["edges"]
    iters = 60
    A64, b, c, L, _ = _recipe(loss, kind, m, n)
    ctl, many, refs = _controlled(loss, kind)
    print(ctl, "reference iterations", [k for _, k in refs])
    xs, info = _path(fos, loss)(_device(kind, A64), b, many, *([c] if loss == lk.HUBER else []), max_iter=iters, L=L, return_info=True, **ctl)
    print("device", info)
    for (x_ref, k_ref), x, (k, code) in zip(refs, xs, info):
        assert (k, code) == (k_ref, 2 if k_ref < iters else 0), (k, code, k_ref)       # FOS_STOP_RATIO where the reference stopped
        assert _data.rel(_np(x), x_ref) < TOL


# ---- 6. the bitwise anchor ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["edges", "panels"])
def test_huber_with_an_unreachable_threshold_is_bitwise_the_weighted_squared_path(fos, name, kind):
    """clip(r, -3e38, 3e38) = r and r * 1.0f = r: the panel R holds the same bits and everything after it is the same launches.
    Derived, not measured: a failure means the link's arithmetic order is wrong."""
    m, n = SHAPES[name]
    A64, b, _, L, alphas = _recipe(lk.HUBER, kind, m, n)
    At = _device(kind, A64)
    many = _many(alphas, 5)
    xs = fos.huber_path(At, b, many, 3e38, max_iter=ITERS, L=L)
    ys = fos.fista_path(fos.prepare_weighted(At, b, np.ones(m)), None, many, max_iter=ITERS, L=L)
    for x, y in zip(xs, ys):
        assert torch.equal(torch.as_tensor(x), torch.as_tensor(y)) and float(torch.as_tensor(x).abs().sum()) > 0


# ---- 7. compositions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("loss", LOSSES)
def test_row_weights(fos, loss, kind):
    m, n = SHAPES["edges"]
    A64, b, c, _, alphas = _recipe(loss, kind, m, n)
    for key in ("01", "frac"):
        w = _weights(m, key)
        L = lk.lipschitz(A64, 1, w)
        P = _handle(fos, loss, kind, A64, b, c, sample_weight=w)
        xs = _path(fos, loss)(P, None, alphas, max_iter=ITERS, L=L)
        for (a1, a2), x in zip(alphas, xs):
            x_ref, _ = _ref(loss, kind, m, n, a1, a2, ITERS, None, wkey=key)
            assert _data.rel(_np(x), x_ref) < TOL, (key, a1, _data.rel(_np(x), x_ref))
        if key == "01":                                                   # 0/1 weights: the fit on the kept rows
            keep = w > 0
            x_kept, _ = lk.run(loss, A64[keep], b[keep], *alphas[0], L, c=c)
            assert _data.rel(_np(xs[0]), x_kept) < TOL


@pytest.mark.parametrize("loss", LOSSES)
def test_intercept_bounds_and_feature_groups(fos, loss):
    m, n = SHAPES["edges"]
    A64, b, c, _, alphas = _recipe(loss, "f32", m, n)
    A1 = np.concatenate([A64[:, :n - 1], np.ones((m, 1))], axis=1)         # the last column becomes the intercept
    if loss == lk.HUBER:
        b = b + 1.5
    L = lk.lipschitz(A1, 1)
    a1 = alphas[1][0]
    pf = np.ones(n)
    pf[-1] = 0.0
    # an unpenalised constant column
    P = _handle(fos, loss, "f32", A1, b, c)
    P.set_penalty(pf)
    x = _np(_path(fos, loss)(P, None, [(a1, 0.0)], max_iter=ITERS, L=L)[0])
    x_ref, _ = lk.run(loss, A1, b, a1, 0.0, L, prob=lk.CoordLinkProblem(loss, A1, b, a1, 0.0, c).bind(pf))
    assert _data.rel(x, x_ref) < TOL and x_ref[-1] != 0.0
    # the non-negativity bound
    lo = np.zeros(n)
    P.set_penalty(pf, lower=0.0)
    x = _np(_path(fos, loss)(P, None, [(a1, 0.0)], max_iter=ITERS, L=L)[0])
    x_ref, _ = lk.run(loss, A1, b, a1, 0.0, L, prob=lk.CoordLinkProblem(loss, A1, b, a1, 0.0, c).bind(pf, lo, None))
    free = lk.run(loss, A1, b, a1, 0.0, L, prob=lk.CoordLinkProblem(loss, A1, b, a1, 0.0, c).bind(pf))[0]
    assert (free[:-1] < 0).any() and (x[:-1] >= 0).all() and _data.rel(x, x_ref) < TOL
    # feature groups: the group prox of tests/_fgroup.py on the new gradient
    P = _handle(fos, loss, "f32", A1, b, c)
    start, gw = fg.layout("small", n, seed=2)
    P.set_feature_groups(np.repeat(np.arange(len(start) - 1), np.diff(start)), gw, 0.5)
    amax = fg.alpha_max(-lk.gradient(loss, A1, np.zeros(n), b, c), np.asarray(start), fg.weights_of(start, gw), 0.5)
    x = _np(_path(fos, loss)(P, None, [(0.2 * amax, 0.0)], max_iter=ITERS, L=L)[0])
    ref = fg._fgroup_class(lk.LinkProblem)(loss, A1, b, 0.2 * amax, 0.0, c).bind(start, gw, 0.5)
    x_ref, _ = lk.run(loss, A1, b, 0.2 * amax, 0.0, L, prob=ref)
    zero, full = fg.zero_groups(x_ref, np.asarray(start))
    assert zero.any() and (~zero).any() and _data.rel(x, x_ref) < TOL, _data.rel(x, x_ref)
    assert np.array_equal(fg.zero_groups(x, np.asarray(start))[0], zero)


# ---- 8. cross-validation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["int_folds", "ids_weighted_panels"])
@pytest.mark.parametrize("loss", LOSSES)
def test_cv(fos, loss, case):
    kind = "f32"
    m, n = SHAPES["edges"] if case == "int_folds" else SHAPES["panels"]
    K, split, wkey = (4, "contiguous", None) if case == "int_folds" else (3, "random", "frac")       # random ids cross the panel boundary
    A64, b, c, L, alphas = _recipe(loss, kind, m, n)
    alphas = alphas[:2] if case != "int_folds" else alphas
    w = None if wkey is None else _weights(m, wkey)
    if w is not None:
        L = lk.lipschitz(A64, 1, w)
    ids = _ids(m, K, split)
    P = _handle(fos, loss, kind, A64, b, c, sample_weight=w)
    cv = fos.huber_cv if loss == lk.HUBER else fos.hinge_cv
    res = cv(P, None, alphas, K if case == "int_folds" else ids, max_iter=ITERS, L=L, return_coefs=True)
    coefs = _np(res.coefs)
    assert type(res).__name__ == ("HuberCVResult" if loss == lk.HUBER else "HingeCVResult")
    assert coefs.shape == (n, K, len(alphas)) and res.loss.shape == (K, len(alphas)) and res.loss.dtype == np.float64
    for f in range(K):
        te = ids == f
        for a, (a1, a2) in enumerate(alphas):
            x_ref, _ = _ref(loss, kind, m, n, a1, a2, ITERS, None, rows=(f, K, split), wkey=wkey)
            assert _data.rel(coefs[:, f, a], x_ref) < TOL, (f, a, _data.rel(coefs[:, f, a], x_ref))
        X32 = coefs[:, f, :].astype(np.float32).astype(np.float64)          # the pass over A reads x in fp32
        wt = None if w is None else w[te]
        ref = lk.data_term(loss, A64[te], X32, b[te], c, wt)
        tol = lk.loss_tolerance(loss, A64[te], X32, b[te], c, wt)
        got = res.loss[f] * (float(te.sum()) if w is None else float(w[te].sum()))
        assert np.isfinite(got).all() and (np.abs(got - ref) <= tol).all(), (f, got, ref, tol)
    assert np.allclose(res.mean_loss, res.loss.mean(axis=0), rtol=1e-14) and res.best == int(np.argmin(res.mean_loss))
    assert res.info == [[(ITERS, 0)] * len(alphas)] * K
    x_ref, _ = _ref(loss, kind, m, n, *alphas[res.best], ITERS, None, wkey=wkey)
    assert _data.rel(_np(res.x), x_ref) < TOL


# ---- 9. objectives -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES)
def test_objectives(fos, loss):
    m, n = SHAPES["panels"]
    A64, b, c, L, alphas = _recipe(loss, "f32", m, n)
    P = _handle(fos, loss, "f32", A64, b, c)
    X = (0.2 * np.random.default_rng(8).standard_normal((n, 19))).astype(F32).astype(np.float64)
    obj = (lambda x, a1, a2: fos.huber_objective(x, P, None, a1, a2)) if loss == lk.HUBER else (lambda x, a1, a2: fos.hinge_objective(x, P, None, a1, a2))
    a1, a2 = alphas[1]
    tol = lk.loss_tolerance(loss, A64, X, b, c)
    ref = lk.objective(loss, A64, X, b, a1, a2, c)
    one = obj(X[:, 0], a1, a2)
    many = obj(X, a1, a2)
    assert isinstance(one, float) and abs(one - ref[0]) <= tol[0] + 1e-12 * abs(ref[0])
    assert many.shape == (19,) and many.dtype == np.float64 and (np.abs(many - ref) <= tol + 1e-12 * np.abs(ref)).all()
    if loss == lk.HUBER:
        assert fos.huber_objective(X[:, 0], P, None, a1, a2, threshold=c) == one
        with pytest.raises(ValueError, match="threshold"):
            fos.huber_objective(X[:, 0], P, None, a1, a2, threshold=2 * c)
        with pytest.raises(ValueError, match="threshold"):
            fos.huber_path(P, None, [(a1, a2)], 2 * c, max_iter=2, L=L)
        assert P.threshold == c and P.loss == "huber"
    else:
        assert P.threshold is None and P.loss == "squared_hinge"


# ---- 10. the working-set solve ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planted(loss):
    """The planted-support case of tests/_working_set.py with this loss's b: gross outliers for Huber, the signs for the hinge."""
    base = ws.case("squared", False, False, "f32")
    A, b = base["A"], base["b"].copy()
    c = None
    if loss == lk.HUBER:
        rng = np.random.default_rng(20)
        out = rng.choice(ws.M, ws.M // 10, replace=False)
        b[out] += rng.choice([-1.0, 1.0], out.size) * 10.0 * np.std(b)
        b = b.astype(F32).astype(np.float64)
        c = float(F32(np.median(np.abs(b))))
    else:
        b = np.where(b >= 0, 1.0, -1.0)
    amax = float(np.abs(lk.gradient(loss, A, np.zeros(ws.N), b, c)).max())
    alphas = tuple((f * amax, 0.0) for f in np.geomspace(0.9, 0.35, 4))
    L = lk.lipschitz(A, 1)
    Xstar = np.stack([lk.run(loss, A, b, a1, a2, L, 4000, c=c)[0] for a1, a2 in alphas], axis=1)
    return A, b, c, L, alphas, Xstar


@pytest.mark.parametrize("loss", LOSSES)
def test_working_set_path(fos, loss):
    A, b, c, L, alphas, Xstar = _planted(loss)
    kkt_tol = 1e-4
    P = _handle(fos, loss, "f32", A, b, c)
    xs, infos = fos.working_set_path(P, None, list(alphas), ws.ITERS, L=L, return_info=True)
    X = np.stack([_np(x) for x in xs], axis=1)
    info = infos[0]
    assert len(infos) == 1 and not info.fell_back and info.rounds >= 1 and info.sizes[0] <= 0.5 * ws.N
    assert info.worst_excess <= 1.0 + kkt_tol
    Xfull = np.stack([_np(x) for x in _path(fos, loss)(P, None, list(alphas), max_iter=ws.ITERS, L=L)], axis=1)
    nrm = np.linalg.norm(Xstar, axis=0)
    d_ws, d_full = np.linalg.norm(X - Xstar, axis=0) / nrm, np.linalg.norm(Xfull - Xstar, axis=0) / nrm
    print(f"{loss}: rounds {info.rounds} sizes {info.sizes} worst excess {info.worst_excess:.5f} distance ws {d_ws.max():.2e} full {d_full.max():.2e}")
    assert (nrm > 0).all() and (d_ws <= np.maximum(2.0 * d_full, 1e-5)).all(), (d_ws, d_full)
    ex = _np(fos.kkt_excess(P, xs, list(alphas)))
    off = (X == 0).all(axis=1)
    assert ex.shape == (ws.N,) and ex[off].max() <= 1.0 + kkt_tol
    assert abs(fos.alpha_max(P) - alphas[0][0] / 0.9) <= 1e-5 * alphas[0][0]
