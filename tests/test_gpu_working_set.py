"""GPU: the working-set solve - fos_gather_columns, fos_gradient_batch, fos_kkt_scan and working_set_path / kkt_excess / alpha_max.

The gather is compared bitwise with A[:, idx] (exact zero padding, a poisoned guard band after every row and after the last row),
the gradient with the fp64 gradient of tests/_working_set.py under the bound the fos_gram_apply check of
tests/test_gpu_weighted.py takes (_data.fp32_pass_tolerances_cols: the same pair of products), the scan with the NumPy scan exactly,
and the path end to end with the fp64 minimiser, its KKT conditions and fista_path / logistic_path on the same handle."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _data, _weighted as wt, _working_set as ws

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED = -1, -4
KINDS = ("f32", "bf16")
EPS32 = float(np.finfo(np.float32).eps)
GRAD_EPS = 8.0 * EPS32                   # the resolution of the fp32 gradient pass (tests/_armijo.py GRAD_EPS["f32"])
KKT_TOL = 1e-4                           # working_set_path's default
PARITY = 1e-5                            # the project's parity bar


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def _tdtype(kind):
    return torch.bfloat16 if kind == "bf16" else torch.float32


def _device(kind, A64, lda=None):
    """A64 (values the element type holds exactly) on the device; lda: the row stride of the buffer it is a view of."""
    t = torch.as_tensor(np.asarray(A64, dtype=np.float32)).to(_tdtype(kind)).cuda()
    if lda is None or lda == t.shape[1]:
        return t
    base = torch.full((t.shape[0], lda), 7.0, dtype=t.dtype, device="cuda")
    base[:, : t.shape[1]] = t
    return base[:, : t.shape[1]]


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- fos_gather_columns -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matrix(kind, m, n):
    A = ws.stored(np.random.default_rng(100 * m + n).standard_normal((m, n)), kind)
    A[0, 0] = -0.0                                               # a sign bit alone must survive
    A.setflags(write=False)
    return A


def _index_sets(n, n_ws):
    rng = np.random.default_rng(n + n_ws)
    if n_ws == 1:
        return [np.array([0]), np.array([n - 1])]
    if n_ws == n:
        return [np.arange(n)]
    inner = np.sort(rng.choice(np.arange(1, n - 1), size=n_ws - 2, replace=False))
    return [np.concatenate([[0], inner, [n - 1]])]               # column 0 and column n - 1 are gathered


@pytest.mark.parametrize("n_ws", [1, 63, 64, 65, "n"])
@pytest.mark.parametrize("n,lda", [(128, 128), (200, 208)])
@pytest.mark.parametrize("m", [1, 67, 300])
@pytest.mark.parametrize("kind", KINDS)
def test_gather_is_bitwise_with_zero_padding_and_an_untouched_guard_band(fos, kind, m, n, lda, n_ws):
    n_ws = n if n_ws == "n" else n_ws
    A64 = _matrix(kind, m, n)
    At = _device(kind, A64, lda)
    P = fos.prepare(At, np.zeros(m))
    assert P.A.data_ptr() == At.data_ptr() and P.n_dev == n and (m == 1 or P.lda == lda)          # borrowed as it is
    n_ws_pad = (n_ws + 7) // 8 * 8 + 8                            # always a block of padding columns
    lda_ws = n_ws_pad + 8                                         # ... and a guard band after every row end
    for idx in _index_sets(n, n_ws):
        buf = torch.full((m * lda_ws + 64,), 3.0, dtype=_tdtype(kind), device="cuda")            # 64 more elements after the last row
        _bits(buf).fill_(0x7BAD if kind == "bf16" else 0x7FC0BAAD)
        want = buf.clone()
        rows = want[: m * lda_ws].view(m, lda_ws)
        rows[:, :n_ws] = At[:, torch.as_tensor(idx, device="cuda")]
        rows[:, n_ws:n_ws_pad] = 0
        out = buf[: m * lda_ws].view(m, lda_ws)[:, :n_ws_pad]
        got = P.gather_columns(torch.as_tensor(idx), n_ws_pad, out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == buf.data_ptr()
        assert torch.equal(_bits(buf), _bits(want)), (kind, m, n, n_ws)
        assert not _bits(buf[: m * lda_ws].view(m, lda_ws)[:, n_ws:n_ws_pad]).any()               # +0.0 exactly
    # the default output: a fresh m x (n_ws rounded up to 8) tensor
    got = P.gather_columns(torch.as_tensor(idx, device="cuda"))
    assert got.shape == (m, (n_ws + 7) // 8 * 8) and torch.equal(_bits(got[:, :n_ws].contiguous()), _bits(At[:, torch.as_tensor(idx, device="cuda")].contiguous()))
    assert not _bits(got[:, n_ws:].contiguous()).any()


def test_gather_refuses_bad_scalars_and_bad_indices(fos):
    m, n = 67, 128
    P = fos.prepare(_device("f32", _matrix("f32", m, n)), np.zeros(m))
    buf = torch.full((m * 144 + 8,), 5.0, device="cuda")
    idx = torch.arange(64, dtype=torch.int32, device="cuda")

    def call(n_ws=64, off=0, lda_ws=72, n_ws_pad=64, i=idx, p=None):
        return P.lib.fos_gather_columns(C.c_void_p(i.data_ptr()) if i is not None else None, n_ws, C.c_void_p(buf.data_ptr() + off), lda_ws,
                                        n_ws_pad, P.h if p is None else p)
    for kw in (dict(n_ws=0), dict(n_ws=-1), dict(n_ws=n + 1, n_ws_pad=136, lda_ws=136), dict(n_ws_pad=56), dict(n_ws_pad=68, lda_ws=80),
               dict(lda_ws=56), dict(lda_ws=76), dict(off=4), dict(off=8)):
        assert call(**kw) == ARG, kw
        assert "fos_gather_columns" in P.lib.fos_last_error().decode()
    torch.cuda.synchronize()
    assert bool((buf == 5.0).all())                               # nothing was launched
    assert call() == 0
    for bad in ([3, 3], [5, 2], [-1, 4], [0, n], []):
        with pytest.raises(ValueError):
            P.gather_columns(torch.as_tensor(bad, dtype=torch.int64))


# ---- fos_gradient_batch -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grad_case(kind, loss, weighted, m, n):
    c = ws.case(loss, weighted, False, kind, seed=m + n, m=m, n=n)
    return c["A"], c["b"], (wt.as_stored(c["w"]) if weighted else None)


@pytest.mark.parametrize("nv", [1, 5, 16])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("m,n", [(300, 128), (67, 200)])
@pytest.mark.parametrize("kind", KINDS)
def test_gradient_batch_against_fp64(fos, kind, m, n, loss, weighted, nv):
    """The bound is the one of test_gram_apply (tests/test_gpu_weighted.py): 2e-6 ||G|| + ||sqrt(w) A|| * 4 eps32 || |sqrt(w) A| |X| +
    sqrt(w) |B| ||, with B what product 1 subtracts - b for the squared loss; for the logistic loss the residual sigma(z) - y is formed
    from z with |sigma'| <= 1/4 and both terms are at most 1, so B = 1 covers it.  loss16 takes the bounds the residual checks of
    that file take: rr_tol of the same function, tests/_weighted.wnll_tolerance for the log-loss."""
    A64, b, w = _grad_case(kind, loss, weighted, m, n)
    P = fos.prepare_weighted(_device(kind, A64), b, w, loss=loss) if weighted else fos.prepare(_device(kind, A64), b, loss=loss)
    X32 = (0.2 * np.random.default_rng(m + nv).standard_normal((n, nv))).astype(np.float32).astype(np.float64)
    G, loss16 = P.gradient_block(torch.as_tensor(X32), want_loss=True)
    assert G.shape == (nv, P.n_dev) and G.dtype == torch.float32
    got = _np(G).T[:n]
    assert torch.equal(P.gradient_batch(torch.as_tensor(X32)), G.t()[:n])                          # the public layout, the same bits
    ref = ws.gradient(A64, b, X32, loss, w)
    sw = np.ones(m) if w is None else np.sqrt(w)
    As = sw[:, None] * A64
    B = sw * (np.abs(b) if loss == "squared" else 1.0)
    rr_ref = ws.data_term(A64, b, X32, loss, w)
    g_tol, rr_tol = _data.fp32_pass_tolerances_cols(As, X32, B, ref, rr_ref)
    err = np.linalg.norm(got - ref, axis=0)
    l_tol = rr_tol if loss == "squared" else wt.wnll_tolerance(A64, X32, np.ones(m) if w is None else w)
    l_err = np.abs(np.asarray(loss16) - rr_ref)
    print(f"{kind} {m}x{n} {loss} weighted={weighted} nv={nv} gradient err/tol {(err / g_tol).max():.3f} loss err/tol {(l_err / l_tol).max():.3f}")
    assert (err <= g_tol).all(), (err, g_tol)
    assert (l_err <= l_tol).all(), (l_err, l_tol)
    # the sums fos_residual_batch(use_b = 1) gives: the same residuals, summed in fp64 (another order at most)
    assert np.allclose(P.residual_batch(torch.as_tensor(X32)), loss16, rtol=1e-9, atol=0.0)


def test_gradient_batch_refuses_what_it_does_not_serve_and_leaves_the_handle_alone(fos):
    from fastoptsolver_amd.distributed import Comm
    m, n = 67, 200
    A64, b, _ = _grad_case("f32", "squared", False, m, n)
    At = _device("f32", A64)
    X = torch.zeros(n, 16, device="cuda")
    G = torch.full((16, n), 9.0, device="cuda")

    def refused(P, word):
        plan = P.plan()
        rc = P.lib.fos_gradient_batch(C.c_void_p(X.data_ptr()), 2, P.h, C.c_void_p(G.data_ptr()), None)
        msg = P.lib.fos_last_error().decode()
        assert rc == UNSUPPORTED and "fos_gradient_batch" in msg and word in msg, (rc, msg)
        assert P.plan() == plan
    refused(fos.prepare_multinomial(At, np.arange(m) % 3), "multinomial")
    refused(fos.prepare(At), "needs b")
    sharded = fos.prepare(At, b)
    sharded.set_comm(Comm.solo())
    refused(sharded, "sharded")
    refused(fos.prepare(torch.zeros(100, 4, device="cuda"), torch.zeros(100)), "matrix-core pair")
    torch.cuda.synchronize()
    assert bool((G == 9.0).all())                                 # nothing was launched
    # the scan's refusals: bounds, feature groups, the multinomial loss
    ex, vi, cnt = torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    in_ws = torch.zeros(n, dtype=torch.uint8, device="cuda")
    a1 = (C.c_double * 1)(0.5)
    for P, word in ((fos.prepare_penalized(At, b, lower=0.0), "bounds"), (fos.prepare_penalized(At, b, upper=0.0), "bounds"),
                    (fos.prepare_grouped(At, b, [100, 100]), "feature groups"), (fos.prepare_multinomial(At, np.arange(m) % 3), "multinomial")):
        rc = P.lib.fos_kkt_scan(C.c_void_p(G.data_ptr()), 1, a1, 0.0, C.c_void_p(in_ws.data_ptr()), P.h, C.c_void_p(ex.data_ptr()),
                                C.c_void_p(vi.data_ptr()), C.c_void_p(cnt.data_ptr()))
        msg = P.lib.fos_last_error().decode()
        assert rc == UNSUPPORTED and "fos_kkt_scan" in msg and word in msg, (rc, msg)
    # ... and the Python layer's, before any device work
    for bad in (fos.prepare_penalized(At, b, lower=0.0), fos.prepare_grouped(At, b, [100, 100]), fos.prepare_multinomial(At, np.arange(m) % 3),
                sharded, fos.prepare(At)):
        with pytest.raises(ValueError):
            fos.working_set_path(bad, None, [(0.5, 0.0)])
    with pytest.raises(ValueError, match="alpha1 = 0"):
        fos.working_set_path(fos.prepare(At, b), None, [(0.5, 0.0), (0.0, 0.1)])


# ---- fos_kkt_scan -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scan_handle(n):
    import fastoptsolver_amd as f
    p = (10.0 ** np.random.default_rng(n).uniform(-1.0, 1.0, size=n)).astype(np.float32).astype(np.float64)
    p[np.random.default_rng(n + 1).random(n) < 0.05] = 0.0
    p[[0, n - 1]] = 0.0
    p.setflags(write=False)
    return f.prepare_penalized(torch.zeros(8, n, device="cuda"), np.zeros(8), penalty_factor=p), f.prepare(torch.zeros(8, n, device="cuda"), np.zeros(8)), p


@pytest.mark.parametrize("sets", ["empty", "full", "random"])
@pytest.mark.parametrize("nv", [1, 16])
@pytest.mark.parametrize("n", [128, 200, 16384])
def test_scan_equals_the_numpy_scan_exactly(fos, n, nv, sets):
    Pp, Pu, p = _scan_handle(n)
    rng = np.random.default_rng(n + nv)
    G = rng.standard_normal((nv, n)).astype(np.float32)             # continuous draws: no comparison is a tie
    G[:, 5] = 0.0                                                    # a zero gradient: 0 excess whatever the factor
    a1 = rng.uniform(0.3, 3.0, size=nv)
    in_ws = {"empty": np.zeros(n, dtype=np.uint8), "full": np.ones(n, dtype=np.uint8), "random": (rng.random(n) < 0.4).astype(np.uint8) * 3}[sets]
    Gd, md = torch.as_tensor(G).cuda(), torch.as_tensor(in_ws).cuda()
    for P, pf in ((Pp, p), (Pu, None)):
        for slack in (0.0, KKT_TOL):
            e_ref, v_ref = ws.scan(G, a1, slack, in_ws, pf)
            d = np.asarray(a1)[:, None] * (np.ones(n) if pf is None else pf)[None, :] * (1.0 + slack)
            a = np.abs(G).astype(np.float64)
            assert ((a != d) | (a == 0.0)).all()                    # the precondition: no tie (0 > 0 is false in any arithmetic)
            e1, v1 = P.kkt_scan(Gd, a1, slack, md)
            e2, v2 = P.kkt_scan(Gd, a1, slack, md)
            assert e1.dtype == torch.float32 and v1.dtype == torch.int32
            assert np.array_equal(e1.cpu().numpy().view(np.uint32), e_ref.view(np.uint32)), (n, nv, sets, slack)
            assert np.array_equal(v1.cpu().numpy(), v_ref)
            assert torch.equal(e1.view(torch.int32), e2.view(torch.int32)) and torch.equal(v1, v2)   # two runs: the same bytes
            if sets == "full":
                assert v1.numel() == 0 and not e1.any()
            elif pf is not None and sets == "empty":
                assert np.isinf(e_ref[0]) and v_ref[0] == 0 and v_ref[-1] == n - 1 and e_ref[5] == 0.0
    if sets == "empty" and n > 1024:
        v = ws.scan(G, a1, 0.0, in_ws, None)[1]                      # violators in the first and in the last trip of the workgroup
        assert v[0] < 1024 and v[-1] >= n - 1024 and len(v) > 64


# ---- end to end ---------------------------------------------------------------------------------------------------------------
E2E = [(loss, full, kind) for loss in ("squared", "logistic") for full in (False, True) for kind in KINDS]
E2E_IDS = [f"{loss}{'-weights-factors' if full else ''}-{kind}" for loss, full, kind in E2E]


def _handle(fos, c, loss, kind):
    At = _device(kind, c["A"])
    if c["p"] is not None or c["w"] is not None:
        return fos.prepare_penalized(At, c["b"], penalty_factor=c["p"], loss=loss, sample_weight=c["w"])
    return fos.prepare(At, c["b"], loss=loss)


@functools.lru_cache(maxsize=None)
def _minimiser(loss, full, kind, **case_kw):
    """The fp64 minimiser of the full problem on the stored A: the reference working-set solve run to convergence (validated on
    the CPU against the full-problem reference and the KKT conditions to 1e-8)."""
    c = ws.case(loss, full, full, kind, **case_kw)
    X, info = ws.solve(c["A"], c["b"], c["alphas"], 4 * ws.ITERS, p=c["p"], loss=loss, w=c["w"], max_fraction=1.0)
    assert not info["fell_back"]
    X.setflags(write=False)
    return X


def _certificate(c, loss, X):
    """(a): per weight, the largest |g_i| / (alpha1 p_i) over the penalised coordinates with x_i = 0, g the fp64 gradient of the data
    term at the returned X on the stored A, minus the resolution of the fp32 pass, GRAD_EPS (|A|^T W |r|)_i / (alpha1 p_i)."""
    A, n = c["A"], c["A"].shape[1]
    p = np.ones(n) if c["p"] is None else c["p"]
    w = np.ones(A.shape[0]) if c["w"] is None else c["w"]
    G = ws.gradient(A, c["b"], X, loss, c["w"])
    Z = A @ X
    R = (ws.lg.sigmoid(Z) if loss == "logistic" else Z) - c["b"][:, None]
    res = GRAD_EPS * (np.abs(A).T @ (w[:, None] * np.abs(R)))
    out = []
    for j, (a1, _) in enumerate(c["alphas"]):
        off = (X[:, j] == 0) & (p > 0)
        out.append(float(((np.abs(G[off, j]) - res[off, j]) / (a1 * p[off])).max()))
    return np.asarray(out)


@pytest.mark.parametrize("loss,full,kind", E2E, ids=E2E_IDS)
def test_path_end_to_end(fos, loss, full, kind):
    c = ws.case(loss, full, full, kind)
    P = _handle(fos, c, loss, kind)
    alphas, L = list(c["alphas"]), c["L"]
    xs, infos = fos.working_set_path(P, None, alphas, ws.ITERS, L=L, return_info=True)
    X = np.stack([_np(x) for x in xs], axis=1)
    info = infos[0]
    assert len(infos) == 1 and not info.fell_back and 1 <= info.rounds and info.sizes[0] <= 0.5 * ws.N
    assert info.full_gradients == info.rounds + 1 and info.worst_excess <= 1.0 + KKT_TOL
    # (a) the certificate, recomputed in fp64 on the host
    cert = _certificate(c, loss, X)
    # (b) the distance to the fp64 minimiser against that of the full path on the same handle, same max_iter and L
    Xstar = _minimiser(loss, full, kind)
    path = fos.logistic_path if loss == "logistic" else fos.fista_path
    Xfull = np.stack([_np(x) for x in path(P, None, alphas, max_iter=ws.ITERS, L=L)], axis=1)
    nrm = np.linalg.norm(Xstar, axis=0)
    d_ws, d_full = np.linalg.norm(X - Xstar, axis=0) / nrm, np.linalg.norm(Xfull - Xstar, axis=0) / nrm
    print(f"{loss} full={full} {kind}: rounds {info.rounds} sizes {info.sizes} gradients {info.full_gradients} worst excess {info.worst_excess:.4f} "
          f"certificate max {cert.max():.6f} distance ws max {d_ws.max():.2e} full path max {d_full.max():.2e}")
    assert (cert <= 1.0 + KKT_TOL).all(), cert
    assert (d_ws <= np.maximum(2.0 * d_full, PARITY)).all(), (d_ws, d_full)
    # the public certificate of the same X: the device's own excess off the support is the scan's
    ex = _np(fos.kkt_excess(P, xs, alphas))
    off = (X == 0).all(axis=1) & ((c["p"] > 0) if c["p"] is not None else True)
    assert ex.shape == (ws.N,) and ex[off].max() <= 1.0 + KKT_TOL


@pytest.mark.parametrize("loss,full,kind", E2E, ids=E2E_IDS)
def test_all_columns_as_the_initial_set_is_the_full_path(fos, loss, full, kind):
    """(c): n = 256 is a multiple of 64 and lda = n, so the gathered matrix is a copy of A with A's shape and alignment and the
    planner gives both handles the same plan: bit for bit."""
    c = ws.case(loss, full, full, kind)
    P = _handle(fos, c, loss, kind)
    alphas, L = list(c["alphas"]), c["L"]
    xs, infos = fos.working_set_path(P, None, alphas, 60, L=L, initial=np.arange(ws.N), max_fraction=1.0, return_info=True)
    path = fos.logistic_path if loss == "logistic" else fos.fista_path
    ys = path(P, None, alphas, max_iter=60, L=L)
    assert infos[0].rounds == 1 and infos[0].sizes == [ws.N] and not infos[0].fell_back and infos[0].full_gradients == 1
    for j, (x, y) in enumerate(zip(xs, ys)):
        assert torch.equal(x, y), (j, float((x - y).abs().max()))


@pytest.mark.parametrize("kind", KINDS)
def test_the_planted_case_grows_and_is_certified(fos, kind):
    """(d)"""
    c = ws.case("squared", False, False, kind, **ws.GROWTH)
    P = _handle(fos, c, "squared", kind)
    xs, infos = fos.working_set_path(P, None, list(c["alphas"]), ws.ITERS, L=c["L"], return_info=True)
    info, X = infos[0], np.stack([_np(x) for x in xs], axis=1)
    print(f"growth {kind}: {info}")
    assert info.rounds >= 2 and not info.fell_back and info.sizes[1] > info.sizes[0] and info.worst_excess <= 1.0 + KKT_TOL
    assert (_certificate(c, "squared", X) <= 1.0 + KKT_TOL).all()
    Xstar = _minimiser("squared", False, kind, **ws.GROWTH)
    assert (np.linalg.norm(X - Xstar, axis=0) <= 1e-4 * np.linalg.norm(Xstar, axis=0)).all()      # the same minimiser, not a parity claim
    one = fos.working_set_path(P, None, list(c["alphas"]), ws.ITERS, L=c["L"], max_rounds=1, return_info=True)[1][0]
    assert one.fell_back and one.rounds == 1                      # round 1 left violators: never returned uncertified


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_the_fall_back_is_the_full_solver_and_says_so(fos, loss):
    """(e)"""
    c = ws.case(loss, False, False, "f32")
    P = _handle(fos, c, loss, "f32")
    alphas, L = list(c["alphas"]), c["L"]
    xs, infos = fos.working_set_path(P, None, alphas, 60, L=L, max_fraction=ws.FALLBACK_FRACTION, return_info=True)
    ys = (fos.logistic_path if loss == "logistic" else fos.fista_path)(P, None, alphas, max_iter=60, L=L)
    assert infos[0].fell_back and infos[0].rounds == 0 and infos[0].sizes == [] and infos[0].full_gradients == 2
    assert all(torch.equal(x, y) for x, y in zip(xs, ys))
    if loss == "squared":             # 20 weights are a group of 16 and a group of 4; arrays go in and come out
        zs, infos = fos.working_set_path(np.array(c["A"]), np.array(c["b"]), alphas + alphas[:4], ws.ITERS, L=L, return_info=True)
        assert len(zs) == 20 and len(infos) == 2 and all(isinstance(z, np.ndarray) and z.shape == (ws.N,) for z in zs)
        assert all(not i.fell_back and i.worst_excess <= 1.0 + KKT_TOL for i in infos) and infos[1].sizes[0] <= infos[0].sizes[0]
        assert (_certificate(dict(c, alphas=tuple(alphas + alphas[:4])), loss, np.stack(zs, axis=1)) <= 1.0 + KKT_TOL).all()


@pytest.mark.parametrize("full", [False, True], ids=["plain", "weights-factors"])
@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_alpha_max(fos, loss, full):
    """Every coordinate is penalised here (positive factors): with an unpenalised one X = 0 is not a solution at any weight."""
    c = ws.case(loss, full, False, "f32")
    p = (10.0 ** np.random.default_rng(3).uniform(-0.5, 0.5, size=ws.N)).astype(np.float32).astype(np.float64) if full else None
    P = _handle(fos, dict(c, p=p), loss, "f32")
    amax, ref = fos.alpha_max(P), ws.alpha_max(c["A"], c["b"], p, loss, c["w"])
    print(f"alpha_max {loss} full={full}: device {amax!r} reference {ref!r}")
    assert abs(amax - ref) <= 1e-5 * ref
    above, info = fos.working_set_path(P, None, [(1.001 * amax, 0.0), (1.001 * amax, 0.5)], 50, L=c["L"], return_info=True)
    below = fos.working_set_path(P, None, [(0.999 * amax, 0.0), (0.999 * amax, 0.5)], 50, L=c["L"])
    assert not any(_np(x).any() for x in above)                   # exactly zero
    assert all(_np(x).any() for x in below)
    assert info[0].rounds == 0 and info[0].sizes == [] and not info[0].fell_back and info[0].worst_excess <= 1.0
    path = fos.logistic_path if loss == "logistic" else fos.fista_path
    assert not any(_np(x).any() for x in path(P, None, [(1.001 * amax, 0.0)], max_iter=50, L=c["L"]))
    assert all(_np(x).any() for x in path(P, None, [(0.999 * amax, 0.0)], max_iter=50, L=c["L"]))
