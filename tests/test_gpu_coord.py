"""GPU: per-coordinate penalty factors and box bounds in the lockstep - fista_path / fista_cv / logistic_path / logistic_cv on a
prepare_penalized handle and the coordinate update kernels under them.

Every case of every cell of tests/_menu_coord.py must equal the fp64 reference of tests/_coord.py (the oracle's loop with the
gradient's ridge term, the prox and the first step replaced) within 1e-5 relative after 30 iterations, on the bf16-rounded A for
bf16 storage and on the factors and bounds as the device stores them (fp32); L comes from the oracle's power iteration and is
passed to both sides.  Every returned coefficient lies inside its box exactly, and where the reference sits at a bound the device
does too.  Neutral data (p = 1, no bounds) must reproduce the plain update bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _coord as cd, _data, _logit as lg, _menu_coord as mc

pytestmark = pytest.mark.gpu

TOL, ITERS = lg.TOL, lg.ITERS
NAMES = ("one_tile", "edges", "rb2", "panels", "whole_wgs")
KINDS = ("f32", "bf16")


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


@pytest.fixture(scope="module")
def cus(fos):
    return int(fos.prepare(torch.zeros(8, 68, device="cuda")).plan()["cus"])


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def _device(kind, A64):
    return torch.as_tensor(A64.astype(np.float32)).to(torch.bfloat16 if kind == "bf16" else torch.float32).cuda()


def _handle(fos, kind, c, loss="squared"):
    P = fos.prepare_penalized(_device(kind, c["A"]), c["b"], c["p"], c["lo"], c["hi"], loss=loss, sample_weight=c["w"])
    for t in (P.penalty_factor, P.lower, P.upper):
        assert t.dtype == torch.float32 and t.data_ptr() % 16 == 0 and t.numel() == P.n
    assert P.has_coord and P.penalty_max == float(c["p"].max()) and P.loss == loss
    return P


def _in_box(x, c, ref_x, what):
    """Inside the box exactly (fp64 against the fp32-stored bounds), and at every bound the reference is at."""
    x = _np(x)
    assert (x >= c["lo"]).all() and (x <= c["hi"]).all(), (what, float((c["lo"] - x).max()), float((x - c["hi"]).max()))
    at_lo, at_hi = ref_x == c["lo"], ref_x == c["hi"]
    assert np.array_equal(x[at_lo], c["lo"][at_lo]) and np.array_equal(x[at_hi], c["hi"][at_hi]), what


def _case(kind, cus, name, loss="squared", weighted=False):
    s = mc.shapes(kind, cus)[name]
    m, n = s["m"], s["n"]
    return cd.case(kind, loss, m, n, 3 * m + n, weighted), (kind, loss, m, n, 3 * m + n, weighted)


# ---- every cell of the coverage table --------------------------------------------------------------------------------------
@pytest.mark.parametrize("prox", mc.PROX)
@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_cells_match_the_reference(fos, cus, name, kind, form, prox):
    from fastoptsolver_amd import _core, _lib
    c, key = _case(kind, cus, name)
    P = _handle(fos, kind, c)
    enet = prox == "PROX_ENET"
    a = c["alphas"]
    ctl = None
    if form == "one-launch-plain":
        specs = [(a1, a2, None, False) for a1, a2 in a]
    elif form == "one-launch-controlled":
        ctl, keep = cd.controlled(*key)              # decisions fp32 cannot take the other way, chosen on the reference alone
        specs = [(a1, a2, None, str(cd.CONTROL_MENU.index(ctl))) for a1, a2 in keep]
    else:                                        # two families in one call: the same one launch, the prox kind per column
        specs = [(a[1][0], a[1][1], None, False), (a[2][0], a[2][1], 3.0, False), (a[1][0], a[1][1], 3.0, False)]
    hs = []
    for a1, a2, delta, ctrl in specs:
        st = _core.Fista(P)
        st.reset(1.0 / (c["L"] + (0.0 if enet else a2 * P.penalty_max)), a1, a2, mode=_lib.MODE_FISTA if delta is None else _lib.MODE_DELTA,
                 prox_kind=_lib.PROX_ENET if enet else _lib.PROX_L1, delta=delta or 0.0, **(ctl if ctrl is not False else {}))
        hs.append(st)
    assert _core.run_multi(hs, ITERS), P.lib.fos_last_error().decode()
    for (a1, a2, delta, ctrl), st in zip(specs, hs):
        ref = cd.reference(*key, a1, a2, enet=enet, delta=delta, control=ctrl)
        x, s = _np(st.x_tensor()), st.status()
        err = _data.rel(x, ref["x"])
        print(f"{name} {kind} {form} {prox} alpha=({a1:.3g}, {a2}) delta={delta}: rel err {err:.3e}, iterations {int(s.k)} / {ref['k']}, "
              f"restarts {int(s.restarts)} / {ref['restarts']}, stop {int(s.stopped)} / {ref['stopped']}, "
              f"{int(np.sum((ref['x'] == c['lo']) | (ref['x'] == c['hi'])))} at a bound")
        if ctrl is not False:
            assert (int(s.k), int(s.restarts), int(s.stopped)) == (ref["k"], ref["restarts"], ref["stopped"])
        else:
            assert (int(s.k), int(s.stopped)) == (ITERS, 0)
        assert np.linalg.norm(ref["x"]) > 0 and err <= TOL, (a1, a2, err)
        _in_box(x, c, ref["x"], (name, kind, form, prox, a1))


# ---- composition: either loss, with and without row weights, through the public solvers ------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("kind", KINDS)
def test_paths_compose_with_the_loss_and_the_weights(fos, cus, kind, loss, weighted):
    c, key = _case(kind, cus, "edges", loss, weighted)
    P = _handle(fos, kind, c, loss)
    path = fos.logistic_path if loss == "logistic" else fos.fista_path
    # the controlled half runs, as the controlled cells do, the control parameters and the penalty pairs under which the
    # reference's decisions are fp32-proof (tests/_coord.controlled; tests/test_coord_reference.py checks them): at least two
    ctl, keep = cd.controlled(*key)
    assert len(keep) >= 2
    for kw, ctrl, alphas in (({}, False, c["alphas"]), (ctl, str(cd.CONTROL_MENU.index(ctl)), keep)):
        xs, info = path(P, None, alphas, max_iter=ITERS, L=c["L"], return_info=True, **kw)
        assert len(xs) == len(alphas)
        for (a1, a2), x, (k, code) in zip(alphas, xs, info):
            ref = cd.reference(*key, a1, a2, control=ctrl)
            err = _data.rel(_np(x), ref["x"])
            print(f"{kind} {loss} weighted={weighted} controlled={ctrl is not False} alpha=({a1:.3g}, {a2}): rel err {err:.3e}, "
                  f"iterations {k} / {ref['k']}, stop {code} / {ref['stopped']}")
            assert (k, code) == (ref["k"], ref["stopped"]) and err <= TOL, (a1, a2, err, k, ref["k"])
            _in_box(x, c, ref["x"], (kind, loss, weighted, a1))
    if loss == "logistic":                         # the objective uses the factored penalties (fp32 factors as bound)
        xs = path(P, None, c["alphas"], max_iter=ITERS, L=c["L"])
        x = _np(xs[1])
        a1, a2 = c["alphas"][1]
        w = np.ones(len(c["b"])) if c["w"] is None else c["w"]
        X32 = x.astype(np.float32).astype(np.float64)
        want = float((w * lg.nll_terms(c["A"], X32, c["b"])).sum() + a1 * (c["p"] * np.abs(x)).sum() + 0.5 * a2 * (c["p"] * x * x).sum())
        from tests import _weighted as wt
        tol = float(wt.wnll_tolerance(c["A"], X32[:, None], w)[0]) + 1e-14 * abs(want)
        assert abs(fos.logistic_objective(x, P, None, a1, a2) - want) <= tol


# ---- the neutral element: p = 1, no bounds is the plain update, bit for bit ---------------------------------------------------
@pytest.mark.parametrize("prox", mc.PROX)
@pytest.mark.parametrize("ctrl", [False, True], ids=["plain", "controlled"])
@pytest.mark.parametrize("which", ["logistic", "weighted-squared"])
@pytest.mark.parametrize("kind", KINDS)
def test_neutral_data_is_bitwise_the_plain_update(fos, cus, kind, which, ctrl, prox):
    from fastoptsolver_amd import _core, _lib
    loss, weighted = ("logistic", False) if which == "logistic" else ("squared", True)
    c, _ = _case(kind, cus, "edges", loss, weighted)
    At, n = _device(kind, c["A"]), c["A"].shape[1]
    make = (lambda: fos.prepare(At, c["b"], loss="logistic")) if which == "logistic" else (lambda: fos.prepare_weighted(At, c["b"], c["w"]))
    plain, neutral = make(), make()
    neutral.set_penalty(np.ones(n), np.full(n, -np.inf), np.full(n, np.inf))
    assert neutral.has_coord and not plain.has_coord and neutral.penalty_max == 1.0
    kw = dict(prox_kind=_lib.PROX_ENET if prox == "PROX_ENET" else _lib.PROX_L1, **(cd.CONTROL if ctrl else {}))

    def run(P):
        hs = []
        for a1, a2 in c["alphas"]:
            st = _core.Fista(P)
            st.reset(1.0 / (c["L"] + a2), a1, a2, **kw)
            hs.append(st)
        assert _core.run_multi(hs, ITERS)
        return [(st.x_tensor(), tuple(getattr(st.status(), k) for k, _ in st.status()._fields_)) for st in hs]

    want = run(plain)
    assert all(torch.count_nonzero(x) > 0 for x, _ in want)
    for (x0, s0), (x1, s1) in zip(want, run(neutral)):
        assert torch.equal(x0, x1) and s0 == s1, (s0, s1)
    neutral.set_penalty()                                                   # detached: the plain kernels again
    got = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
    assert neutral.lib.fos_coord_get(C.byref(got[0]), C.byref(got[1]), C.byref(got[2]), neutral.h) == 0
    assert [g.value for g in got] == [None] * 3 and not neutral.has_coord and neutral.penalty_factor is None
    for (x0, s0), (x1, s1) in zip(want, run(neutral)):
        assert torch.equal(x0, x1) and s0 == s1, (s0, s1)
    # half-bound data is neutral too: only the factors, only one side of the box
    neutral.set_penalty(penalty_factor=1.0)
    for (x0, s0), (x1, s1) in zip(want, run(neutral)):
        assert torch.equal(x0, x1) and s0 == s1
    neutral.set_penalty(upper=np.inf)
    for (x0, s0), (x1, s1) in zip(want, run(neutral)):
        assert torch.equal(x0, x1) and s0 == s1


# ---- the two uses the feature exists for -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _intercept_data():
    rng = np.random.default_rng(77)
    m, n = 2000, 68
    A = rng.standard_normal((m, n))
    A[:, -1] = 1.0                                                          # the constant column
    xt = np.zeros(n)
    xt[:5] = (1.5, -1.0, 1.0, -0.5, 0.8)
    xt[-1] = 2.0                                                            # the true intercept: unbalanced classes
    A64 = A.astype(np.float32).astype(np.float64)
    y = (rng.random(m) < lg.sigmoid(A64 @ xt)).astype(np.float64)
    L = lg.lipschitz(A64, 77)
    a1 = 0.2 * float(np.max(np.abs(A64.T @ (y - 0.5))))
    p = np.ones(n)
    p[-1] = 0.0
    return A64, y, L, a1, p


def test_an_unpenalised_intercept(fos):
    A64, y, L, a1, p = _intercept_data()
    iters = ITERS
    free = cd.run(A64, y, a1, 0.0, L, iters, p=p, loss="logistic")["x"]
    shrunk = cd.run(A64, y, a1, 0.0, L, iters, loss="logistic")["x"]
    assert free[-1] > 1.0 and free[-1] - shrunk[-1] > 0.25, (free[-1], shrunk[-1])      # on the reference alone
    At = torch.as_tensor(A64.astype(np.float32)).cuda()
    x = _np(fos.logistic_path(fos.prepare_penalized(At, y, p, loss="logistic"), None, [(a1, 0.0)], max_iter=iters, L=L)[0])
    x_pen = _np(fos.logistic_path(fos.prepare(At, y, loss="logistic"), None, [(a1, 0.0)], max_iter=iters, L=L)[0])
    print(f"intercept: factor 0 {x[-1]:.6f} (reference {free[-1]:.6f}), penalised {x_pen[-1]:.6f} (reference {shrunk[-1]:.6f}); "
          f"rel err {_data.rel(x, free):.3e}")
    assert _data.rel(x, free) <= TOL and abs(x[-1] - free[-1]) <= TOL * abs(free[-1])
    assert _data.rel(x_pen, shrunk) <= TOL and x[-1] - x_pen[-1] > 0.25


def test_the_non_negative_lasso(fos, cus):
    c, _ = _case("f32", cus, "edges")
    n = c["A"].shape[1]
    P = fos.prepare_penalized(_device("f32", c["A"]), c["b"], lower=0.0)
    assert P.penalty_factor is None and P.upper is None and P.penalty_max == 1.0 and bool((P.lower == 0).all())
    xs = fos.fista_path(P, None, c["alphas"], max_iter=ITERS, L=c["L"])
    for (a1, a2), x in zip(c["alphas"], xs):
        ref = cd.run(c["A"], c["b"], a1, a2, c["L"], lo=np.zeros(n))["x"]
        free = cd.run(c["A"], c["b"], a1, a2, c["L"])["x"]
        assert (free < 0).any() and (ref >= 0).all() and np.count_nonzero(ref) > 0
        x = _np(x)
        assert (x >= 0).all() and np.array_equal(x[ref == 0], ref[ref == 0]) and _data.rel(x, ref) <= TOL, _data.rel(x, ref)


# ---- cross-validation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("kind", KINDS)
def test_cv_holds_its_contract(fos, cus, kind, loss):
    c, key = _case(kind, cus, "edges", loss)
    m, n = c["A"].shape
    K, alphas = 3, c["alphas"][:2]
    ids = np.arange(m) % K
    P = _handle(fos, kind, c, loss)
    cv, path = (fos.logistic_cv, fos.logistic_path) if loss == "logistic" else (fos.fista_cv, fos.fista_path)
    res = cv(P, None, alphas, ids, max_iter=ITERS, L=c["L"], return_coefs=True)
    coefs = _np(res.coefs)
    score = res.logloss if loss == "logistic" else res.mse
    assert coefs.shape == (n, K, 2) and score.shape == (K, 2)
    At = _device(kind, c["A"])
    for f in range(K):
        tr = ids != f
        sub = fos.prepare_penalized(At[torch.as_tensor(tr).cuda()], c["b"][tr], c["p"], c["lo"], c["hi"], loss=loss)
        xs = path(sub, None, alphas, max_iter=ITERS, L=c["L"])
        for a, (a1, a2) in enumerate(alphas):
            ref = cd.reference(*key, a1, a2, rows=tr.tobytes())
            e_path, e_ref = _data.rel(coefs[:, f, a], _np(xs[a])), _data.rel(coefs[:, f, a], ref["x"])
            print(f"{kind} {loss} fold {f} alpha {a}: against the path on the gathered rows {e_path:.3e}, against the reference {e_ref:.3e}")
            assert e_path <= TOL and e_ref <= TOL
            _in_box(coefs[:, f, a], c, ref["x"], (kind, loss, f, a))
        # The held-out scores: fp64 on the device's OWN coefficients (just checked against the reference), within the bound of
        # one fp32 pass - this isolates the held-out pass from solver drift - and, against the scores of the REFERENCE's
        # coefficients, within that bound plus what the coefficients' own error can move a score: the score is a sum over the
        # held-out rows of a function of z = A x with |dz_i| <= |A_i| . |dx|.
        te = ~tr
        X32 = coefs[:, f, :].astype(np.float32).astype(np.float64)           # the pass over A reads x in fp32
        if loss == "logistic":
            want, tol = lg.nll(c["A"][te], X32, c["b"][te]), lg.nll_tolerance(c["A"][te], X32)
        else:
            R = c["A"][te] @ X32 - c["b"][te][:, None]
            want = (R * R).sum(axis=0)
            _, tol = _data.fp32_pass_tolerances_cols(c["A"][te], X32, c["b"][te], np.zeros_like(X32), want)
        got = score[f] * te.sum()
        assert (np.abs(got - want) <= tol).all(), (f, got, want, tol)
        Xr = np.stack([cd.reference(*key, a1, a2, rows=tr.tobytes())["x"] for a1, a2 in alphas], axis=1)
        dz = np.abs(c["A"][te]) @ np.abs(X32 - Xr)
        if loss == "logistic":                                                # the log-loss is 1-Lipschitz in z
            want_ref, slack = lg.nll(c["A"][te], Xr, c["b"][te]), dz.sum(axis=0)
        else:                                                                 # |r'^2 - r^2| <= (2 |r| + |dz|) |dz|
            Rr = c["A"][te] @ Xr - c["b"][te][:, None]
            want_ref, slack = (Rr * Rr).sum(axis=0), ((2.0 * np.abs(Rr) + dz) * dz).sum(axis=0)
        print(f"{kind} {loss} fold {f}: held-out sums {got}, of the reference's coefficients {want_ref}, allowed {tol + slack}")
        assert (np.abs(got - want_ref) <= tol + slack).all(), (f, got, want_ref, tol, slack)
    a1, a2 = alphas[res.best]                                                # the refit runs in the lockstep too
    assert _data.rel(_np(res.x), cd.reference(*key, a1, a2)["x"]) <= TOL


# ---- a live handle ----------------------------------------------------------------------------------------------------------
def test_set_penalty_takes_effect_between_runs_and_siblings_carry_it(fos, cus):
    c, key = _case("f32", cus, "edges")
    P = fos.prepare(_device("f32", c["A"]), c["b"])
    before = fos.fista_path(P, None, c["alphas"], max_iter=ITERS, L=c["L"])
    P.set_penalty(c["p"], c["lo"], c["hi"])
    bound = fos.fista_path(P, None, c["alphas"], max_iter=ITERS, L=c["L"])
    b2 = np.roll(c["b"], 17)
    sib = P.sibling(b2)
    assert sib.has_coord and sib.penalty_max == P.penalty_max and sib.lower.data_ptr() == P.lower.data_ptr()
    other = fos.fista_path(sib, None, c["alphas"], max_iter=ITERS, L=c["L"])
    for (a1, a2), x0, x1, x2 in zip(c["alphas"], before, bound, other):
        ref = cd.reference(*key, a1, a2)
        assert _data.rel(_np(x1), ref["x"]) <= TOL and _data.rel(_np(x0), ref["x"]) > 100 * TOL
        _in_box(x1, c, ref["x"], a1)
        ref2 = cd.run(c["A"], b2, a1, a2, c["L"], p=c["p"], lo=c["lo"], hi=c["hi"])["x"]
        assert _data.rel(_np(x2), ref2) <= TOL
    with pytest.raises(ValueError):
        P.set_penalty(lower=1.0)
    assert P.has_coord                                                      # a refused call leaves the binding as it was
    P.set_penalty()
    for x0, x3 in zip(before, fos.fista_path(P, None, c["alphas"], max_iter=ITERS, L=c["L"])):
        assert torch.equal(torch.as_tensor(x0), torch.as_tensor(x3))
