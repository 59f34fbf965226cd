"""GPU: the duality-gap certificate (fos_duality_gap, duality_gap) and the gap-stopped path (certified_path) against the fp64
reference of tests/_duality.py.

1. Per element, through a diagonal A of powers of two (tests/test_gpu_link.py's recipe): z is exact, the row pass is fp64 per
   element, so primal, dual and gap equal the reference to 1e-12 of the magnitude of their terms and the scale equals scale_of on
   the returned G to 1e-12, with planted rows (the Huber threshold and its neighbours, the hinge margin 1, logistic z = +-40, zero
   weights) and planted coordinates (|G| = tau, |G| = 2 tau, p = 0 with and without a gradient, alpha1 = alpha2 = 0, alpha2 > 0).
2. End to end on the shapes of tests/test_gpu_link.py, at FISTA iterates of the reference whose place on the way to the minimum
   tests/test_duality_reference.py asserts: each of primal, dual, gap within 1e-5 - the project's fp32 parity bound - of the sum of
   the magnitudes of its reference terms (data term, penalty, conjugate); the reference forms scale and conjugate from the
   returned G, which is bitwise the block of gradient_block.
3. The refusals, with the handle unchanged.
4. certified_path on the planted-support recipe of tests/_working_set.py: by properties (every column certified, a budget that is
   not met reported), and against the fp64 restatement of its loop (tests/_duality.certified) - rounds, set sizes, certificates,
   fell_back and certified exactly, solutions and gap within 1e-5 - on cases whose every decision tests/test_duality_reference.py
   shows to be out of fp32's reach: squared weighted, Huber, weighted squared hinge, logistic with positive penalty factors, bf16,
   a grown set beyond max_fraction * n (fell_back, three certificates), a round without a violator whose set runs again, the warm
   start X0 (every second round, the fall-back), 20 weights as groups of 16 and 4.  gap_tol is 1e-3 in all of them: at
   certified_path's default 1e-4 no seed of the recipe meets the margins (tests/_duality.py, next to CERTIFIED_CASES).  The top-k
   branch of the growth step is reached by no case at this shape (every grown set is all 256 columns by violators alone); the
   certified_path cell of tests/_handle_pairs.py reaches it at the two-panel shape.  110 tests in 8 s on the MI355X (102 in 8 s
   before the eight cases; the slowest of them 0.28 s).  Under the temporary edits that tests/test_gpu_handle_pairs.py lists, the
   eight cases fail with dual_scale_kernel skipped (all) and with the row weights also in product 1 (the four weighted ones)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _data, _duality as du, _working_set as ws

pytestmark = pytest.mark.gpu

UNSUPPORTED = -4
F32 = np.float32
EXACT, TOL = 1e-12, du.TOL


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def _device(kind, A64):
    return torch.as_tensor(np.asarray(A64).astype(np.float32)).to(torch.bfloat16 if kind == "bf16" else torch.float32).cuda()


def _handle(fos, loss, kind, A64, b, c=None, w=None, p=None):
    At = _device(kind, A64)
    if loss in (du.HUBER, du.HINGE):
        P = fos.prepare_huber(At, b, c, sample_weight=w) if loss == du.HUBER else fos.prepare_hinge(At, b, sample_weight=w)
        if p is not None:
            P.set_penalty(p)
        return P
    if p is not None:
        return fos.prepare_penalized(At, b, penalty_factor=p, loss=loss, sample_weight=w)
    if w is not None:
        return fos.prepare_weighted(At, b, w, loss=loss)
    if loss == du.SQUARED and At.shape[1] <= 64:
        # A plain squared handle of at most 64 columns runs the row-per-thread kernel and has no matrix-core pair:
        # fos_gradient_batch refuses it, and so does the certificate (test_refusals_leave_the_handle_alone).  The plain cell of
        # such a shape runs on the handle that serves the same problem there: unit row weights.
        return fos.prepare_weighted(At, b, np.ones(At.shape[0]), loss=loss)
    return fos.prepare(At, b, pad=True, loss=loss)       # padded as the other kinds are: the matrix-core pair serves the shape


def _certify(P, X, alphas):
    """(out64 as a 4 x 16 float64 array, G as nv x n_dev float32) of one fos_duality_gap call."""
    out64, G = P.duality_gap_block(torch.as_tensor(X).cuda(), [a for a, _ in alphas], [a for _, a in alphas])
    return out64.cpu().numpy().reshape(4, 16), G.cpu().numpy()


def _compare(out, ref, nv, tol, what):
    assert np.isfinite(out).all(), (what, out)
    assert (out[:, nv:] == 0).all(), (what, out[:, nv:])                  # the columns >= nv
    worst = {}
    for row, key in enumerate(("primal", "dual", "gap")):
        err, mag = np.abs(out[row, :nv] - ref[key]), ref["mag_" + key]
        worst[key] = float(np.where(err > 0, err / np.where(mag > 0, mag, 1.0), 0.0).max())     # all terms 0 (s = 0): exactly 0 expected
        assert (err[mag == 0] == 0).all(), (what, key, out[row, :nv], ref[key])
    worst["scale"] = float(np.abs(out[3, :nv] - ref["scale"]).max())
    print(f"{what}: err / magnitude primal {worst['primal']:.2e} dual {worst['dual']:.2e} gap {worst['gap']:.2e}; scale {worst['scale']:.2e}; "
          f"scales {np.round(out[3, :nv], 4).tolist()}")
    assert worst["scale"] <= EXACT, (what, out[3, :nv], ref["scale"])
    for key in ("primal", "dual", "gap"):
        assert worst[key] <= tol, (what, key, worst[key])
    assert np.array_equal(out[2, :nv], out[0, :nv] - out[1, :nv])          # gap = primal - dual, in fp64
    return worst


# ---- 1. per element, through a diagonal A ---------------------------------------------------------------------------------------
M_D, N_D, C_D = 259, 260, 0.5
FREE_ROW = 20                            # the coordinate that the "free" plant leaves unpenalised: a row with a generic gradient


@functools.lru_cache(maxsize=None)
def _diagonal(loss):
    """(s, b, Z): A = diag(s) (259 x 260, powers of two; column 259 is zero) and the 259 x 16 panel Z = A X, with planted rows."""
    rng = np.random.default_rng(41 + du.LOSSES.index(loss))
    s = rng.choice([0.5, 1.0, 2.0], M_D).astype(F32)
    Z = rng.standard_normal((M_D, 16)).astype(F32)
    up, down = np.nextafter(F32(C_D), F32(1)), np.nextafter(F32(C_D), F32(0))
    if loss == du.LOGISTIC:
        b = (rng.random(M_D) < 0.5).astype(F32)
        b[:4] = [0, 1, 0, 1]
        Z[:4] = np.asarray([40.0, 40.0, -40.0, -40.0], dtype=F32)[:, None]                    # sigma saturates: q or 1 - q is 0
    elif loss == du.HINGE:
        b = rng.choice([-1.0, 1.0], M_D).astype(F32)
        one = F32(1)
        for i, t in enumerate([one, one, np.nextafter(one, F32(2)), np.nextafter(one, F32(0)), F32(3), F32(3)]):     # the margin b z
            Z[i] = b[i] * t
        Z[FREE_ROW] = -b[FREE_ROW] * np.abs(Z[FREE_ROW])                    # a margin below 1 in every column: a gradient there
    else:
        b = rng.standard_normal(M_D).astype(F32)
        b[:6] = [0.25, -0.25, 0.25, -0.25, -0.25, 0.0]
        for i, r in enumerate([C_D, -C_D, up, -up, down, 0.0]):            # r = z - b exactly: b and r share the binade, or are 0
            Z[i] = F32(r) + b[i]
            assert F32(Z[i, 0] - b[i]) == F32(r)
    Z[8:14] = np.where(rng.random((6, 16)) < 0.5, Z[:6], Z[8:14])          # the planted values again, in some columns only
    b[8:14] = b[:6]
    for a in (s, b, Z):
        a.setflags(write=False)
    return s, b, Z


@pytest.mark.parametrize("plant", ["bind", "free"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("nv", [1, 5, 16])
@pytest.mark.parametrize("loss", du.LOSSES)
def test_the_certificate_per_element_through_a_diagonal_matrix(fos, loss, nv, weighted, plant):
    s, b, Z = _diagonal(loss)
    A = np.zeros((M_D, N_D), dtype=F32)
    A[np.arange(M_D), np.arange(M_D)] = s
    w = None
    if weighted:
        w = np.random.default_rng(9).choice([0.5, 1.0, 2.0, 4.0], M_D).astype(F32)
        w[::17] = 0.0                                                     # row 0 among them: a planted row with weight 0
    # factors that are powers of two, so that tau = alpha1 p and |G| / p are exact; column 259 of A is zero: p = 0 against G = 0
    p = np.random.default_rng(10).choice([0.5, 1.0, 2.0], N_D).astype(F32)
    p[N_D - 1] = 0.0
    if plant == "free":
        p[FREE_ROW] = 0.0                                                 # p = 0 against G != 0: s = 0 in every column
    A64, b64, c = A.astype(np.float64), b.astype(np.float64), C_D if loss == du.HUBER else None
    P = _handle(fos, loss, "f32", A64, b64, c, w, p.astype(np.float64))
    X = np.zeros((N_D, nv), dtype=F32)
    X[:M_D] = Z[:, :nv] / s[:, None]                                     # exact: s is a power of two
    G0 = P.gradient_block(torch.as_tensor(X).cuda()).cpu().numpy()
    assert (G0[:, N_D - 1] == 0).all() and (G0[:, FREE_ROW] != 0).all()
    # the weights, planted on the gradient: gmax_j = max_k |G_jk| / p_k over the penalised coordinates, exact in fp64
    pen = p > 0
    gmax = (np.abs(G0[:, :N_D][:, pen]).astype(np.float64) / p[pen].astype(np.float64)).max(axis=1)
    assert (gmax > 0).all()
    plan = [lambda g: (g, 0.0),              # |G| = tau exactly on the binding coordinate: s stays 1
            lambda g: (g / 2.0, 0.0),        # |G| = 2 tau there: s = 1/2
            lambda g: (0.0, 0.0),            # no penalty at all: tau = rho = 0 against a gradient, s = 0
            lambda g: (g / 4.0, g / 8.0),    # a ridge on every penalised coordinate: s = 1 and a conjugate term
            lambda g: (0.3 * g, 0.0)]        # a generic scale
    alphas = [plan[j % 5](gmax[j]) for j in range(nv)]
    out, G = _certify(P, X, alphas)
    assert np.array_equal(G, G0)
    ref = du.certificate(loss, A64, b64, X.astype(np.float64), alphas, c, None if w is None else w.astype(np.float64), p, G=G)
    if plant == "free":
        assert (out[3, :nv] == 0.0).all()
    else:
        want = [1.0, 0.5, 0.0, 1.0][: min(nv, 4)]
        assert out[3, : len(want)].tolist() == want, out[3, :nv]
        if nv > 4:
            assert 0.29 < out[3, 4] < 0.31
    _compare(out, ref, nv, EXACT, f"diagonal {loss} nv={nv} weighted={weighted} {plant}")
    if loss == du.LOGISTIC and plant == "free":
        assert (out[1, :nv] == 0.0).all()                                # s = 0: q is the label, the entropy exactly 0 - and no NaN
    again, _ = _certify(P, X, alphas)
    assert again.tobytes() == out.tobytes()


# ---- 2. end to end --------------------------------------------------------------------------------------------------------------
E2E = [(loss, form, shape, "f32") for shape in du.SHAPES for loss in du.LOSSES for form in du.FORMS] + \
      [(loss, form, "edges", "bf16") for loss in du.LOSSES for form in du.FORMS]
POINT = (4, 0, 1, 2, 3)                  # column j takes the iterate COUNTS[POINT[j % 5]]: the converged one first


def _columns(cs, nv):
    """The nv columns of a call: iterates of the case under its own weights, the lasso at the same alpha1, a heavier elastic net
    and a lighter lasso, in turn."""
    a1, a2 = cs["alpha"]
    ridge = a2 if a2 > 0 else a1 / 10.0
    variants = [(a1, a2), (a1, 0.0), (2.0 * a1, ridge), (0.5 * a1, 0.0)]
    X = np.stack([cs["X"][:, POINT[j % 5]] for j in range(nv)], axis=1)
    return X, [variants[j % 4] for j in range(nv)]


@pytest.mark.parametrize("loss,form,shape,kind", E2E, ids=["-".join(e) for e in E2E])
def test_certificate_end_to_end(fos, loss, form, shape, kind):
    cs = du.case(loss, form, shape, kind)
    P = _handle(fos, loss, kind, cs["A"], cs["b"], cs["c"], cs["w"], cs["p"])
    n = cs["A"].shape[1]
    for nv in (1, 5, 16):
        X, alphas = _columns(cs, nv)
        Xd = torch.as_tensor(X.astype(F32)).cuda()
        out, G = _certify(P, X.astype(F32), alphas)
        assert np.array_equal(G, P.gradient_block(Xd).cpu().numpy())     # bitwise the block of gradient_block
        ref = du.certificate(loss, cs["A"], cs["b"], X, alphas, cs["c"], cs["w"], cs["p"], G=G[:, :n])
        _compare(out, ref, nv, TOL, f"{loss} {form} {shape} {kind} nv={nv}")
        again, G2 = _certify(P, X.astype(F32), alphas)
        assert again.tobytes() == out.tobytes() and np.array_equal(G, G2)
        if nv == 16:                     # the public call: the same numbers per pair
            got = fos.duality_gap(P, X, alphas)
            assert isinstance(got, fos.DualityGap) and all(v.dtype == np.float64 and v.shape == (16,) for v in got)
            assert np.array_equal(np.stack(got), out)
    # the converged point under its own weights: a gap at the resolution of the pass, not above it
    rel = out[2, 0] / cs["p0"]
    print(f"   converged point: device gap / P(0) = {rel:.2e}")
    assert abs(out[2, 0]) <= TOL * ref["mag_gap"][0]


def test_more_than_sixteen_columns_go_sixteen_per_call(fos):
    cs = du.case(du.SQUARED, "plain", "edges")
    P = _handle(fos, du.SQUARED, "f32", cs["A"], cs["b"])
    X, alphas = _columns(cs, 16)
    X, alphas = np.concatenate([X, X[:, :3]], axis=1), alphas + alphas[:3]
    got = fos.duality_gap(P, [X[:, j] for j in range(19)], alphas)
    first, _ = _certify(P, X[:, :16].astype(F32), alphas[:16])
    last, _ = _certify(P, X[:, 16:].astype(F32), alphas[16:])
    assert np.array_equal(np.stack(got), np.concatenate([first, last[:, :3]], axis=1))
    with pytest.raises(ValueError):
        fos.duality_gap(P, X, alphas[:5])


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone(fos):
    m, n = 67, 200
    rng = np.random.default_rng(3)
    A64 = rng.standard_normal((m, n)).astype(F32).astype(np.float64)
    b = rng.standard_normal(m).astype(F32).astype(np.float64)
    At = _device("f32", A64)
    X = torch.zeros(n, 16, device="cuda")
    G = torch.full((16, n), 9.0, device="cuda")
    out64 = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
    a = (C.c_double * 2)(0.5, 0.25)
    alphas, L = [(0.5, 0.0), (0.1, 0.05)], float(np.linalg.norm(A64, 2) ** 2)      # a given L: the paths estimate it from a random start

    def refused(P, word, answer):
        before, plan = answer(), P.plan()
        rc = P.lib.fos_duality_gap(C.c_void_p(X.data_ptr()), 2, a, a, P.h, C.c_void_p(G.data_ptr()), C.c_void_p(out64.data_ptr()))
        msg = P.lib.fos_last_error().decode()
        assert rc == UNSUPPORTED and "fos_duality_gap" in msg and word in msg, (rc, msg)
        assert P.plan() == plan
        after = answer()
        assert all(torch.equal(x, y) for x, y in zip(before, after))     # the handle answers as before

    for P in (fos.prepare_penalized(At, b, lower=0.0), fos.prepare_penalized(At, b, upper=0.0)):
        refused(P, "bounds", lambda P=P: fos.fista_path(P, None, alphas, max_iter=5, L=L))
    P = fos.prepare_grouped(At, b, [100, 100])
    refused(P, "feature groups", lambda: fos.fista_path(P, None, alphas, max_iter=5, L=L))
    P = fos.prepare_multinomial(At, np.arange(m) % 3)
    refused(P, "multinomial", lambda: fos.multinomial_path(P, None, alphas, max_iter=5, L=L))
    P = fos.prepare(At)                  # no b: no path runs on it either; what it does serve answers as before
    refused(P, "needs b", lambda: [P.gram_apply(torch.ones(n, 2, device="cuda"))])
    P = fos.prepare(torch.zeros(100, 4, device="cuda"), torch.zeros(100))          # a plain squared handle of at most 64 columns
    refused(P, "matrix-core pair", lambda: fos.fista_path(P, None, alphas, max_iter=5, L=1.0))
    torch.cuda.synchronize()
    assert bool((G == 9.0).all()) and bool((out64 == 7.0).all())         # nothing was launched
    for bad in (fos.prepare_penalized(At, b, lower=0.0), fos.prepare_grouped(At, b, [100, 100]), fos.prepare_multinomial(At, np.arange(m) % 3),
                fos.prepare(At)):
        with pytest.raises(ValueError):
            fos.duality_gap(bad, np.zeros((n, 2)), alphas)
        with pytest.raises(ValueError):
            fos.certified_path(bad, None, alphas)


# ---- 4. certified_path ----------------------------------------------------------------------------------------------------------
def _ws_handle(fos, c, loss):
    return fos.prepare(_device("f32", c["A"]), c["b"], loss=loss)


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_certified_path_certifies_every_column(fos, loss):
    c = ws.case(loss, False, False, "f32")
    P = _ws_handle(fos, c, loss)
    alphas, L = list(c["alphas"]), c["L"]
    before = fos.working_set_path(P, None, alphas, 60, L=L)
    xs, infos = fos.certified_path(P, None, alphas, du.GAP_TOL, du.PATH_ITERS, max_rounds=du.PATH_ROUNDS, L=L, return_info=True)
    info = infos[0]
    print(f"{loss}: {info}")
    assert len(xs) == 16 and len(infos) == 1 and isinstance(info, fos.GapInfo)
    assert info.certified.dtype == bool and info.certified.all() and not info.fell_back
    assert 1 <= info.rounds <= du.PATH_ROUNDS and len(info.sizes) == info.rounds and info.certificates == info.rounds + 1
    assert info.sizes[0] <= 0.5 * ws.N
    # the fp64 gap of every returned x: within the bound, plus the resolution of the device's certificate
    X = np.stack([_np(x) for x in xs], axis=1)
    ref = du.certificate(loss, c["A"], c["b"], X, alphas)
    p0 = du.certificate(loss, c["A"], c["b"], np.zeros_like(X), alphas)["primal"]
    print(f"   fp64 gap / P(0) max {(ref['gap'] / p0).max():.2e}; device gap / P(0) max {(info.gap / p0).max():.2e}")
    assert (ref["gap"] <= du.GAP_TOL * p0 + TOL * ref["mag_gap"]).all(), ref["gap"] / p0
    assert (np.abs(info.gap - ref["gap"]) <= TOL * ref["mag_gap"]).all() and (info.gap <= du.GAP_TOL * p0 * (1 + TOL)).all()
    # the public certificate of the same solutions is the path's last one
    got = fos.duality_gap(P, xs, alphas)
    assert np.array_equal(got.gap, info.gap) and np.array_equal(got.scale, info.scale)
    # working_set_path on the same handle returns the bytes it returned before
    after = fos.working_set_path(P, None, alphas, 60, L=L)
    assert all(torch.equal(x, y) for x, y in zip(before, after))


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_a_tight_budget_is_reported_not_certified(fos, loss):
    c = ws.case(loss, False, False, "f32")
    P = _ws_handle(fos, c, loss)
    alphas, L = list(c["alphas"]), c["L"]
    xs, infos = fos.certified_path(P, None, alphas, 1e-10, 3, max_rounds=1, L=L, return_info=True)
    info = infos[0]
    print(f"{loss} tight: {info}")
    assert info.rounds == 1 and info.fell_back and info.certificates == 3
    assert not info.certified.any()
    p0 = du.certificate(loss, c["A"], c["b"], np.zeros((ws.N, 16)), alphas)["primal"]
    assert np.isfinite(info.gap).all() and (info.gap > 1e-10 * p0).all()   # the gap that was not met is reported
    X = np.stack([_np(x) for x in xs], axis=1)
    ref = du.certificate(loss, c["A"], c["b"], X, alphas)
    assert (np.abs(info.gap - ref["gap"]) <= TOL * ref["mag_gap"]).all()
    # a list of plain arrays goes in and comes out, 20 weights as a group of 16 and a group of 4
    if loss == "squared":
        zs, infos = fos.certified_path(np.array(c["A"]), np.array(c["b"]), alphas + alphas[:4], du.GAP_TOL, du.PATH_ITERS, L=L, return_info=True)
        assert len(zs) == 20 and len(infos) == 2 and all(isinstance(z, np.ndarray) and z.shape == (ws.N,) for z in zs)
        assert all(i.certified.all() for i in infos) and infos[1].certified.shape == (4,)


@pytest.mark.parametrize("name", list(du.CERTIFIED_CASES))
def test_certified_path_against_its_fp64_loop(fos, name):
    args, gap_tol, iters, max_fraction, count = du.CERTIFIED_CASES[name]
    cs, weights = du.path_case(*args), du.certified_weights(name)
    P = _handle(fos, cs["loss"], args[1], cs["A"], cs["b"], cs["c"], cs["w"], cs["p"])
    xs, infos = fos.certified_path(P, None, weights, gap_tol, iters, max_rounds=du.PATH_ROUNDS, max_fraction=max_fraction, L=cs["L"],
                                   return_info=True)
    groups = du.certified_reference(name)
    assert len(xs) == count and len(infos) == len(groups)
    first = 0
    for info, (X, ref) in zip(infos, groups):
        nv = X.shape[1]
        got = (info.rounds, list(info.sizes), info.certificates, bool(info.fell_back), info.certified.tolist())
        want = (ref["rounds"], ref["sizes"], ref["certificates"], ref["fell_back"], ref["certified"].tolist())
        errs = [_data.rel(_np(xs[first + j]), X[:, j]) for j in range(nv)]
        gap_err = np.abs(info.gap - ref["gap"]) / ref["mag_gap"]
        print(f"{name}: {got[:4]}; solutions {max(errs):.2e}, gap / magnitude {gap_err.max():.2e}")
        assert got == want, (got, want)
        assert max(errs) <= TOL, errs
        assert (gap_err <= TOL).all(), gap_err
        first += nv
