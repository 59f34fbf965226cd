"""GPU: the working set and the duality gap of the multinomial lockstep (include/fos_multinomial_ws.h,
fastoptsolver_amd/multinomial_ws.py) against the fp64 reference of tests/_multinomial_ws.py.

1. fos_multinomial_gradient_batch: the class gradients and loss16 within 1e-5 - the project's fp32 parity bound - of the sum of the
   magnitudes of their reference terms, C = 2, 3, 7, 16 (8, 5, 2 and 1 segments; columns 15 and 14 - 15 idle at C = 3 and 7), plain
   and weighted with zero weights, bf16 on one shape; loss16 is fos_residual_batch's value; columns >= nv are not read.
2. fos_multinomial_kkt_scan: the violators exactly (on inputs whose every decision stands SCAN_MARGIN clear), excess within one
   unit in the last place, two runs the same bytes; n = 37 and 2053 user columns, l1 and grouped, exact-zero factors, a non-empty
   set, a segment with alpha1 = 0.
3. fos_multinomial_duality_gap at iterates of the reference: primal, dual, gap within 1e-5 of their magnitudes, the scale to
   1e-12, G bitwise the gradient entry point's, two calls the same 64 doubles, zeros off s*C and beyond nv, gap >= -1e-5 mag.
4. The anchor: C = 2, X = (x, 0), alpha2 = 0, l1 equals fos_duality_gap on the logistic handle of the same A with b = [y = 0].
5. The two paths against the fp64 restatement of their loops - rounds, sizes, fell_back and certificates exactly, X within 1e-5.
6. multinomial_path on a handle gives the same bytes before and after a gradient, a scan and a certificate on it, also at the
   smallest cluster-planned width.
7. The refusals, C and Python, with nothing launched and the handle unchanged; the FOS_ERR_ARG rows of the per-segment weights."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _cluster_planned as cp, _multinomial as mn, _multinomial_ws as mw

pytestmark = pytest.mark.gpu

UNSUPPORTED, ARG = -4, -1
F32 = np.float32
EXACT, TOL = 1e-12, mw.TOL


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


def _handle(fos, cs, kind="f32"):
    return fos.prepare_multinomial(_device(kind, cs["A"]), cs["y"], cs["C"], sample_weight=cs["w"], penalty_factor=cs["p"],
                                   grouped=cs["grouped"])


def _fits(cs, count):
    """`count` fits of a case: its iterates in turn, the converged one first, rounded to fp32."""
    order = (4, 0, 1, 2, 3)
    return [cs["fits"][order[j % 5]] for j in range(count)]


def _weights(cs, count):
    a1, a2 = cs["alpha"]
    ridge = a2 if a2 > 0 else a1 / 10.0
    variants = [(a1, a2), (a1, 0.0), (2.0 * a1, ridge), (0.5 * a1, 0.0)]
    return [variants[j % 4] for j in range(count)]


# ---- 1. the gradient ------------------------------------------------------------------------------------------------------------
GRAD = [(Cn, weighted, shape, "f32") for shape in mw.SHAPES for Cn in mw.CLASSES for weighted in (False, True)] + \
       [(3, False, "edges", "bf16"), (7, True, "edges", "bf16")]


@pytest.mark.parametrize("Cn,weighted,shape,kind", GRAD, ids=[f"C{c}-{'weighted' if w else 'plain'}-{s}-{k}" for c, w, s, k in GRAD])
def test_gradient_and_loss_against_fp64(fos, Cn, weighted, shape, kind):
    cs = mw.case(Cn, False, "weighted" if weighted else "lasso", shape, kind)
    P = _handle(fos, cs, kind)
    A, y, w, n = cs["A"], cs["y"], cs["w"], cs["A"].shape[1]
    nseg = 16 // Cn
    fits = _fits(cs, nseg)
    X = mw.block(fits).astype(F32)
    G, loss = P.multinomial_gradient_block(torch.as_tensor(X), want_loss=True)
    assert G.shape == (nseg * Cn, P.n_dev) and G.dtype == torch.float32 and len(loss) == nseg
    got = _np(G)
    assert (got[:, n:] == 0).all()                                           # the padding columns of A are zero
    ref = mw.gradient_block(A, y, Cn, fits, w)
    ww = np.ones(A.shape[0]) if w is None else w
    mag = np.concatenate([(np.abs(A).T @ (ww[:, None] * np.abs(mn.softmax(A @ Xf) - mn.onehot(y, Cn)))).T for Xf in fits], axis=0)
    g_err = float((np.abs(got[:, :n] - ref) / mag).max())
    l_ref = mw.loss_sums(A, y, fits, w)                                      # every term is >= 0: the sum is its own magnitude
    l_err = float((np.abs(np.asarray(loss) - l_ref) / l_ref).max())
    print(f"C={Cn} weighted={weighted} {shape} {kind}: gradient err / magnitude {g_err:.2e}, loss {l_err:.2e}")
    assert g_err <= TOL and l_err <= TOL
    # loss16 is fos_residual_batch's value (the same launches) and the other entries are 0
    assert P.residual_batch(torch.as_tensor(X))[::Cn] == loss
    assert all(v == 0.0 for j, v in enumerate(P.scratch[:16].cpu().tolist()) if j % Cn or j >= nseg * Cn)
    # columns >= nv of X are not read, rows >= nv of G not written
    nv = nseg * Cn
    Xf = torch.full((P.n_dev, 16), float("nan"), device="cuda")
    Xf[:, :nv] = 0.0
    Xf[:n, :nv] = torch.as_tensor(X).cuda()
    Gb = torch.full((16, P.n_dev), 9.0, device="cuda")
    rc = P.lib.fos_multinomial_gradient_batch(C.c_void_p(Xf.data_ptr()), nv, P.h, C.c_void_p(Gb.data_ptr()), None)
    assert rc == 0 and torch.equal(Gb[:nv], G) and bool((Gb[nv:] == 9.0).all())


# ---- 2. the scan ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scan_handle(n, Cn):
    import fastoptsolver_amd as f
    p = (10.0 ** np.random.default_rng(n).uniform(-1.0, 1.0, size=n)).astype(F32).astype(np.float64)
    p[np.random.default_rng(n + 1).random(n) < 0.05] = 0.0
    p[[0, n - 1]] = 0.0
    p.setflags(write=False)
    y = np.arange(8) % Cn
    return (f.prepare_multinomial(torch.zeros(8, n, device="cuda"), y, Cn, penalty_factor=p),
            f.prepare_multinomial(torch.zeros(8, n, device="cuda"), y, Cn), p)


@pytest.mark.parametrize("grouped", [False, True], ids=["l1", "grouped"])
@pytest.mark.parametrize("Cn", [2, 3, 7, 16])
@pytest.mark.parametrize("n", [37, 2053])
def test_scan_takes_the_decisions_of_the_stated_arithmetic(fos, n, Cn, grouped):
    Pp, Pu, p = _scan_handle(n, Cn)
    nd, nseg = Pp.n_dev, 16 // Cn
    assert nd == Pu.n_dev and nd % 1024 != 0 and (n < 1024 or nd > 2048)
    rng = np.random.default_rng(n + Cn)
    a1 = rng.uniform(0.3, 3.0, size=nseg)
    if nseg > 1:
        a1[1] = 0.0                                                          # a segment with alpha1 = 0
    in_ws = np.zeros(nd, dtype=np.uint8)
    in_ws[rng.random(nd) < 0.3] = 3
    in_ws[[0, 7]] = 0
    md = torch.as_tensor(in_ws).cuda()
    for P, pf in ((Pp, p), (Pu, None)):
        pd = np.ones(nd)
        if pf is not None:
            pd[:n] = pf
        for slack in (0.0, 1e-4):
            G = np.zeros((nseg * Cn, nd), dtype=F32)
            G[:, :n] = rng.standard_normal((nseg * Cn, n)).astype(F32)
            G[:, 5] = 0.0                                                    # a zero gradient: 0 excess whatever the factor
            for _ in range(20):                                              # decisions within 2 SCAN_MARGIN of a threshold move away
                close = np.zeros(nd, dtype=bool)
                for s in range(nseg):
                    Gs = G[s * Cn:(s + 1) * Cn].astype(np.float64)
                    v = np.sqrt((Gs * Gs).sum(axis=0)) if grouped else np.abs(Gs).max(axis=0)
                    thr = a1[s] * pd * (1.0 + slack)
                    close |= (thr > 0) & (np.abs(v / np.where(thr > 0, thr, 1.0) - 1.0) < 2.0 * mw.SCAN_MARGIN)
                if not close.any():
                    break
                G[:, close] *= F32(1.05)
            e_ref, v_ref, margin = mw.scan(G, Cn, grouped, a1, slack, in_ws, pd)
            assert margin > mw.SCAN_MARGIN, margin
            Gd = torch.as_tensor(G).cuda()
            e1, v1 = P.multinomial_kkt_scan(Gd, a1, slack, md, grouped)
            e2, v2 = P.multinomial_kkt_scan(Gd, a1, slack, md, grouped)
            assert e1.dtype == torch.float32 and v1.dtype == torch.int32 and e1.shape == (nd,)
            assert np.array_equal(v1.cpu().numpy(), v_ref), (n, Cn, grouped, slack)
            got = e1.cpu().numpy()
            assert np.array_equal(np.isinf(got), np.isinf(e_ref)) and (got >= 0).all()
            fin = np.isfinite(e_ref)
            ulps = np.abs(got[fin].view(np.int32).astype(np.int64) - e_ref[fin].view(np.int32).astype(np.int64))
            assert ulps.max() <= 1, ulps.max()                               # both sides round an fp64 value once
            assert torch.equal(e1.view(torch.int32), e2.view(torch.int32)) and torch.equal(v1, v2)
            assert (got[in_ws != 0] == 0).all() and got[5] == 0.0
            if pf is not None:
                assert np.isinf(got[0]) and 0 in v_ref                       # an unpenalised coordinate with a gradient
            if nseg > 1:
                assert np.isinf(got[7]) and 7 in v_ref                       # alpha1 = 0 against a gradient


# ---- 3. the certificate ---------------------------------------------------------------------------------------------------------
CERT = [(Cn, g, form, "edges", "f32") for Cn in mw.CLASSES for g in (False, True) for form in ("lasso", "enet")] + \
       [(Cn, g, form, "one_tile", "f32") for Cn, g in ((3, False), (7, True)) for form in ("weighted", "penalised", "free")] + \
       [(2, False, "enet", "panels", "f32"), (3, True, "lasso", "panels", "f32"), (16, False, "weighted", "panels", "f32"),
        (7, True, "penalised", "panels", "f32"), (3, True, "enet", "edges", "bf16"), (3, False, "lasso", "edges", "bf16")]


def _certify(P, X, alphas, grouped=None):
    out64, G = P.multinomial_duality_gap_block(torch.as_tensor(X).cuda(), [a for a, _ in alphas], [a for _, a in alphas], grouped)
    return out64.cpu().numpy().reshape(4, 16), G.cpu().numpy()


def _compare(out, ref, Cn, nseg, tol, what):
    assert np.isfinite(out).all(), (what, out)
    used = np.arange(nseg) * Cn
    off = np.setdiff1d(np.arange(16), used)
    assert (out[:, off] == 0).all(), (what, out[:, off])                      # entries off s*C and segments >= nv / C
    got = out[:, used]
    worst = {}
    for row, key in enumerate(("primal", "dual", "gap")):
        err, mag = np.abs(got[row] - ref[key]), ref["mag_" + key]
        worst[key] = float(np.where(err > 0, err / np.where(mag > 0, mag, 1.0), 0.0).max())
        assert (err[mag == 0] == 0).all(), (what, key)
    worst["scale"] = float(np.abs(got[3] - ref["scale"]).max())
    print(f"{what}: err / magnitude primal {worst['primal']:.2e} dual {worst['dual']:.2e} gap {worst['gap']:.2e}; scale {worst['scale']:.2e}; "
          f"scales {np.round(got[3], 4).tolist()}")
    assert worst["scale"] <= EXACT, (what, got[3], ref["scale"])
    for key in ("primal", "dual", "gap"):
        assert worst[key] <= tol, (what, key, worst[key])
    assert np.array_equal(got[2], got[0] - got[1])                            # gap = primal - dual, in fp64
    assert (got[2] >= -tol * ref["mag_gap"]).all(), (what, got[2])
    return got


@pytest.mark.parametrize("Cn,grouped,form,shape,kind", CERT, ids=[f"C{c}-{'grouped' if g else 'l1'}-{f}-{s}-{k}" for c, g, f, s, k in CERT])
def test_certificate_against_fp64(fos, Cn, grouped, form, shape, kind):
    cs = mw.case(Cn, grouped, form, shape, kind)
    P = _handle(fos, cs, kind)
    n, per = cs["A"].shape[1], 16 // Cn
    fits, alphas = _fits(cs, 5), _weights(cs, 5)
    parts = []
    for first in range(0, 5, per):
        group, weights = fits[first:first + per], alphas[first:first + per]
        X = mw.block(group).astype(F32)
        out, G = _certify(P, X, weights)
        assert np.array_equal(G, P.multinomial_gradient_block(torch.as_tensor(X)).cpu().numpy())      # bitwise the gradient entry point's
        ref = mw.certificate(cs["A"], cs["y"], Cn, group, weights, grouped, cs["w"], cs["p"], G=G[:, :n])
        parts.append(_compare(out, ref, Cn, len(group), TOL, f"C={Cn} grouped={grouped} {form} {shape} {kind} fits {first}.."))
        again, G2 = _certify(P, X, weights)
        assert again.tobytes() == out.tobytes() and np.array_equal(G, G2)
    if form == "free":                                                        # an unpenalised coordinate with a gradient: s = 0 at every
        assert (np.concatenate(parts, axis=1)[3, 1:] == 0.0).all()            # fit on the way, reported and not hidden
    got = fos.multinomial_duality_gap(P, fits, alphas)                        # the public call: the same numbers per fit
    assert isinstance(got, fos.DualityGap) and all(v.dtype == np.float64 and v.shape == (5,) for v in got)
    assert np.array_equal(np.stack(got), np.concatenate(parts, axis=1))
    block = np.stack(fits, axis=2)                                            # and an n x C x k block is the list
    assert all(np.array_equal(a, b) for a, b in zip(fos.multinomial_duality_gap(P, block, alphas), got))
    with pytest.raises(ValueError):
        fos.multinomial_duality_gap(P, fits, alphas[:3])


def test_alpha_max_and_kkt_excess(fos):
    for grouped in (False, True):
        cs = mw.case(3, grouped, "penalised", "edges")
        P = _handle(fos, cs)
        amax = mw.alpha_max(cs["A"], cs["y"], 3, grouped, cs["w"], cs["p"])
        assert abs(fos.multinomial_alpha_max(P) - amax) <= TOL * amax
        fits, alphas = _fits(cs, 7), _weights(cs, 7)
        ex = _np(fos.multinomial_kkt_excess(P, fits, alphas))
        want = np.zeros(ex.shape)
        for X, (a1, _) in zip(fits, alphas):
            e, _, _ = mw.scan(mw.gradient_block(cs["A"], cs["y"], 3, [X], cs["w"]).astype(F32), 3, grouped, [a1], 0.0, np.zeros(ex.size), cs["p"])
            want = np.maximum(want, e)
        assert ex.shape == (cs["A"].shape[1],) and np.abs(ex - want).max() <= 1e-3 * want.max()
        # at the converged fit under its own weight the zero rows are optimal
        zero = np.abs(fits[0]).sum(axis=1) == 0
        ex0 = _np(fos.multinomial_kkt_excess(P, [fits[0]], alphas[:1]))
        assert zero.any() and ex0[zero].max() <= 1.0 + 1e-3


# ---- 4. the anchor --------------------------------------------------------------------------------------------------------------
def test_two_classes_with_a_zero_column_are_the_logistic_certificate(fos):
    cs = mw.case(2, False, "lasso", "edges")
    A, y, n = cs["A"], cs["y"], cs["A"].shape[1]
    At = _device("f32", A)
    Pm = fos.prepare_multinomial(At, y, 2)
    Pl = fos.prepare(At, (y == 0).astype(np.float64), loss="logistic")
    a1 = cs["alpha"][0]
    xs = [X[:, 0] - X[:, 1] for X in cs["fits"]]                              # (x, 0) has the logits (a.x, 0)
    xs = [x.astype(F32).astype(np.float64) for x in xs]
    fits = [np.stack([x, np.zeros(n)], axis=1) for x in xs]
    alphas = [(a1, 0.0), (2.0 * a1, 0.0), (0.5 * a1, 0.0), (a1, 0.0), (0.25 * a1, 0.0)]
    out, G = _certify(Pm, mw.block(fits).astype(F32), alphas)
    lo64, Gl = Pl.duality_gap_block(torch.as_tensor(np.stack(xs, axis=1).astype(F32)).cuda(), [a for a, _ in alphas], [0.0] * 5)
    lo = lo64.cpu().numpy().reshape(4, 16)
    ref = mw.certificate(A, y, 2, fits, alphas, False, G=G[:, :n])
    worst = {}
    for row, key in enumerate(("primal", "dual", "gap")):
        worst[key] = float((np.abs(out[row, 0:10:2] - lo[row, :5]) / ref["mag_" + key]).max())
    worst["scale"] = float(np.abs(out[3, 0:10:2] - lo[3, :5]).max())
    print(f"anchor: multinomial C = 2 against logistic, err / magnitude {worst}; scales {out[3, 0:10:2].tolist()}")
    assert all(worst[k] <= TOL for k in ("primal", "dual", "gap")) and worst["scale"] <= TOL
    assert (out[3, 0:10:2] < 1.0).any() and (out[3, 0:10:2] == 1.0).any()     # both kinds of scale are among them
    # G = (g, -g): the same data term
    Gl = Gl.cpu().numpy()
    mag = np.abs(Gl).max()
    assert np.abs(G[0:10:2] - Gl[:5]).max() <= TOL * mag and np.abs(G[1:10:2] + Gl[:5]).max() <= TOL * mag


# ---- 5. the paths ---------------------------------------------------------------------------------------------------------------
def _path_handle(fos, cs):
    return fos.prepare_multinomial(_device("f32", cs["A"]), cs["y"], cs["C"], grouped=cs["grouped"])


@pytest.mark.parametrize("name", list(mw.WS_CASES))
def test_working_set_path_against_its_fp64_loop(fos, name):
    grouped, args, loop = mw.WS_CASES[name]
    cs = mw.path_case(grouped, *args)
    P = _path_handle(fos, cs)
    kw = dict(loop)
    if "initial" in kw:
        kw["initial"] = list(kw["initial"])
    xs, infos = fos.multinomial_working_set_path(P, None, list(cs["alphas"]), max_iter=mw.WS_ITERS, L=cs["L"], return_info=True, **kw)
    groups = mw.ws_reference(name)
    assert len(xs) == mw.PATH_WEIGHTS and len(infos) == len(groups) == 2
    first = 0
    for info, (fits, ref) in zip(infos, groups):
        assert isinstance(info, fos.WorkingSetInfo)
        got = (info.rounds, list(info.sizes), info.full_gradients, bool(info.fell_back))
        want = (ref["rounds"], ref["sizes"], ref["full_gradients"], ref["fell_back"])
        errs = [mn.rel(xs[first + j], fits[j]) for j in range(len(fits))]
        print(f"{name}: {got}; solutions {max(errs):.2e}; worst excess {info.worst_excess:.4f} (reference {ref['worst_excess']:.4f})")
        assert got == want, (got, want)
        assert max(errs) <= TOL, errs
        assert all(_np(x).shape == (cs["A"].shape[1], cs["C"]) for x in xs)
        if not info.fell_back:
            assert info.worst_excess <= 1.0 + 1e-4
        if grouped:                                                           # a row is in the model for every class or for none
            assert all((((_np(x) != 0).all(axis=1)) | ((_np(x) == 0).all(axis=1))).all() for x in xs[first:first + len(fits)])
        first += len(fits)


@pytest.mark.parametrize("name", list(mw.CERT_CASES))
def test_certified_path_against_its_fp64_loop(fos, name):
    grouped, args, gap_tol, iters, loop = mw.CERT_CASES[name]
    cs = mw.path_case(grouped, *args)
    P = _path_handle(fos, cs)
    xs, infos = fos.multinomial_certified_path(P, None, list(cs["alphas"]), None, gap_tol, iters, L=cs["L"], return_info=True, **loop)
    groups = mw.cert_reference(name)
    assert len(xs) == mw.PATH_WEIGHTS and len(infos) == len(groups) == 2
    first = 0
    for info, (fits, ref) in zip(infos, groups):
        assert isinstance(info, fos.GapInfo)
        got = (info.rounds, list(info.sizes), info.certificates, bool(info.fell_back), info.certified.tolist())
        want = (ref["rounds"], ref["sizes"], ref["certificates"], ref["fell_back"], ref["certified"].tolist())
        errs = [mn.rel(xs[first + j], fits[j]) for j in range(len(fits))]
        gap_err = np.abs(info.gap - ref["gap"]) / ref["mag_gap"]
        print(f"{name}: {got[:4]}; solutions {max(errs):.2e}, gap / magnitude {gap_err.max():.2e}")
        assert got == want, (got, want)
        assert max(errs) <= TOL, errs
        assert (gap_err <= TOL).all(), gap_err
        assert info.gap.shape == (len(fits),) and info.scale.shape == (len(fits),)
        first += len(fits)
    # the public certificate of the returned fits is the path's last one
    cert = fos.multinomial_duality_gap(P, xs, list(cs["alphas"]))
    assert np.array_equal(cert.gap, np.concatenate([i.gap for i in infos]))


# ---- 6. the handle is untouched --------------------------------------------------------------------------------------------------
def _touch(fos, P, Cn, alphas):
    """A gradient, a scan and a certificate on P."""
    X = torch.zeros(P.n_dev, Cn, device="cuda")
    X[::7, 1] = 0.01
    G = P.multinomial_gradient_block(X)
    P.multinomial_kkt_scan(G, [alphas[0][0]], 0.0, torch.zeros(P.n_dev, dtype=torch.uint8, device="cuda"))
    out64, G2 = P.multinomial_duality_gap_block(X, [alphas[0][0]], [alphas[0][1]])
    assert torch.equal(G, G2)
    return out64.cpu().numpy().reshape(4, 16), G


@pytest.mark.parametrize("grouped", [False, True], ids=["l1", "grouped"])
def test_multinomial_path_answers_the_same_bytes_after_the_new_calls(fos, grouped):
    cs = mw.case(3, grouped, "weighted", "edges")
    P = _handle(fos, cs)
    alphas, L = _weights(cs, 6), cs["L"]
    before, plan = fos.multinomial_path(P, None, alphas, max_iter=5, L=L), P.plan()
    _touch(fos, P, 3, alphas)
    after = fos.multinomial_path(P, None, alphas, max_iter=5, L=L)
    assert P.plan() == plan and P.grouped == grouped
    assert all(torch.equal(torch.as_tensor(x), torch.as_tensor(y)) for x, y in zip(before, after))
    # and first on a fresh handle: the same certificate, the same path after it
    P2 = _handle(fos, cs)
    first = _touch(fos, P2, 3, alphas)
    assert first[0].tobytes() == _touch(fos, P, 3, alphas)[0].tobytes()
    assert all(torch.equal(torch.as_tensor(x), torch.as_tensor(y)) for x, y in zip(before, fos.multinomial_path(P2, None, alphas, max_iter=5, L=L)))


def test_the_same_at_the_smallest_cluster_planned_width(fos):
    d = cp.data("cs4")                                                        # 8200 x 4096: the cluster form is planned, two products run
    Cn = 3
    y = mn.labels(d["A"], Cn, d["seed"])
    At = torch.from_numpy(d["A32"].copy()).cuda()
    alphas, L = mn.weights(d["A"], y, Cn, 2), cp.L_of(d, "multinomial")

    def handle(cluster):
        P = fos.prepare_multinomial(At, y, Cn)
        P.replan(cluster=cluster)
        return P

    Pc, Pt = handle(True), handle(False)
    before = fos.multinomial_path(Pc, None, alphas, max_iter=3, L=L)
    plan = Pc.plan()
    out_c, G_c = _touch(fos, Pc, Cn, alphas)
    after = fos.multinomial_path(Pc, None, alphas, max_iter=3, L=L)
    assert Pc.plan() == plan
    assert all(torch.equal(torch.as_tensor(x), torch.as_tensor(y_)) for x, y_ in zip(before, after))
    # the two layouts give the same bytes, and the fp64 reference agrees
    out_t, G_t = _touch(fos, Pt, Cn, alphas)
    assert out_c.tobytes() == out_t.tobytes() and torch.equal(G_c, G_t)
    X = np.zeros((d["n"], Cn))
    X[::7, 1] = np.float64(F32(0.01))
    ref = mw.certificate(d["A"], y, Cn, [X], alphas[:1], False, G=G_c.cpu().numpy()[:, :d["n"]])
    _compare(out_c, ref, Cn, 1, TOL, "cluster-planned cs4")
    # the calls first on a fresh cluster-planned handle, then the path
    Pn = handle(True)
    out_n, _ = _touch(fos, Pn, Cn, alphas)
    assert out_n.tobytes() == out_c.tobytes()
    assert all(torch.equal(torch.as_tensor(x), torch.as_tensor(y_)) for x, y_ in zip(before, fos.multinomial_path(Pn, None, alphas, max_iter=3, L=L)))


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone(fos):
    from fastoptsolver_amd.distributed import Comm
    m, n = 67, 200
    rng = np.random.default_rng(3)
    A64 = rng.standard_normal((m, n)).astype(F32).astype(np.float64)
    b = rng.standard_normal(m).astype(F32).astype(np.float64)
    y = np.arange(m) % 3
    At = _device("f32", A64)
    X = torch.zeros(n, 16, device="cuda")
    G = torch.full((16, n), 9.0, device="cuda")
    out64 = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
    ex = torch.full((n,), 5.0, device="cuda")
    vi, cnt = torch.full((n,), 4, dtype=torch.int32, device="cuda"), torch.full((1,), 4, dtype=torch.int32, device="cuda")
    in_ws = torch.zeros(n, dtype=torch.uint8, device="cuda")
    a = (C.c_double * 2)(0.5, 0.25)
    alphas, L = [(0.5, 0.0), (0.1, 0.05)], float(np.linalg.norm(A64, 2) ** 2)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def calls(P, nv):
        return {"fos_multinomial_gradient_batch": lambda: P.lib.fos_multinomial_gradient_batch(ptr(X), nv, P.h, ptr(G), None),
                "fos_multinomial_kkt_scan": lambda: P.lib.fos_multinomial_kkt_scan(ptr(G), nv, 0, a, 0.0, ptr(in_ws), P.h, ptr(ex), ptr(vi), ptr(cnt)),
                "fos_multinomial_duality_gap": lambda: P.lib.fos_multinomial_duality_gap(ptr(X), nv, 1, a, a, P.h, ptr(G), ptr(out64))}

    def refused(P, word, answer, nv=6, only=None):
        before, plan = answer(), P.plan()
        for name, call in calls(P, nv).items():
            if only is not None and name not in only:
                continue
            rc = call()
            msg = P.lib.fos_last_error().decode()
            assert rc == UNSUPPORTED and name in msg and word in msg, (name, rc, msg)
        assert P.plan() == plan
        assert all(torch.equal(torch.as_tensor(x), torch.as_tensor(z)) for x, z in zip(before, answer()))     # the handle answers as before

    for P, path in ((fos.prepare(At, b, pad=True), fos.fista_path), (fos.prepare(At, (b > 0).astype(np.float64), loss="logistic"), fos.logistic_path)):
        refused(P, "not multinomial", lambda P=P, path=path: path(P, None, alphas, max_iter=5, L=L))
    P = fos.prepare_multinomial(At, y, 3)
    refused(P, "multiple", lambda: fos.multinomial_path(P, None, alphas, max_iter=5, L=L / 2), nv=4)
    for P in (fos.prepare_multinomial(At, y, 3, lower=0.0), fos.prepare_multinomial(At, y, 3, upper=0.0)):
        refused(P, "bounds", lambda P=P: fos.multinomial_path(P, None, alphas, max_iter=5, L=L / 2),
                only=("fos_multinomial_kkt_scan", "fos_multinomial_duality_gap"))
    # (fos_problem_set_comm refuses a multinomial problem, so the sharded refusal of the C entry points has no handle to meet; the
    # Python layer reads the host attribute, below)
    sharded = fos.prepare_multinomial(At, y, 3)
    sharded.comm = Comm.solo()
    # the per-segment weights: FOS_ERR_ARG once the class count is read, before any HIP call
    P = fos.prepare_multinomial(At, y, 3)
    for bad in (-1e-300, float("nan"), float("inf")):
        w = (C.c_double * 2)(0.5, bad)
        for name, call in (("fos_multinomial_kkt_scan", lambda: P.lib.fos_multinomial_kkt_scan(ptr(G), 6, 0, w, 0.0, ptr(in_ws), P.h, ptr(ex), ptr(vi), ptr(cnt))),
                           ("fos_multinomial_duality_gap", lambda: P.lib.fos_multinomial_duality_gap(ptr(X), 6, 0, w, a, P.h, ptr(G), ptr(out64))),
                           ("fos_multinomial_duality_gap", lambda: P.lib.fos_multinomial_duality_gap(ptr(X), 6, 0, a, w, P.h, ptr(G), ptr(out64)))):
            assert call() == ARG
            msg = P.lib.fos_last_error().decode()
            assert name in msg and "weight 1" in msg, msg
        w3 = (C.c_double * 3)(0.5, 0.5, bad)                                 # a bad weight beyond nv / C is not read
        assert P.lib.fos_multinomial_kkt_scan(ptr(G), 6, 0, w3, 0.0, ptr(in_ws), P.h, ptr(ex), ptr(vi), ptr(cnt)) == 0
        ex.fill_(5.0); vi.fill_(4); cnt.fill_(4)
    torch.cuda.synchronize()
    assert bool((G == 9.0).all()) and bool((out64 == 7.0).all()) and bool((ex == 5.0).all()) and bool((vi == 4).all()) and int(cnt) == 4
    # the Python layer, before any device work: the plan of the handle is what it was
    logistic = fos.prepare(At, (b > 0).astype(np.float64), loss="logistic")
    bounded = fos.prepare_multinomial(At, y, 3, lower=0.0)
    for bad, word in ((logistic, "working_set_path"), (bounded, "bounds"), (sharded, "sharded")):
        plan = bad.plan()
        for call in (lambda: fos.multinomial_working_set_path(bad, None, alphas), lambda: fos.multinomial_certified_path(bad, None, alphas),
                     lambda: fos.multinomial_duality_gap(bad, np.zeros((n, 3)), alphas[:1]),
                     lambda: fos.multinomial_kkt_excess(bad, np.zeros((n, 3)), alphas[:1]), lambda: fos.multinomial_alpha_max(bad)):
            with pytest.raises(ValueError, match=word):
                call()
        assert bad.plan() == plan
    with pytest.raises(ValueError, match="alpha1 = 0"):
        fos.multinomial_working_set_path(fos.prepare_multinomial(At, y, 3), None, [(0.5, 0.0), (0.0, 0.1)])
    # the names they stand beside refuse a multinomial handle as before
    for call in (lambda: fos.working_set_path(P, None, alphas), lambda: fos.certified_path(P, None, alphas),
                 lambda: fos.duality_gap(P, np.zeros((n, 2)), alphas)):
        with pytest.raises(ValueError, match="multinomial"):
            call()
