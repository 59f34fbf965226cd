"""GPU: the group lasso over feature groups in the lockstep (sparse-group with l1_ratio > 0) - fista_path / fista_cv /
logistic_path / logistic_cv on a prepare_grouped handle and the three update launches under them.

Every case must equal the fp64 reference of tests/_fgroup.py (the oracle's loop with the prox replaced) within 1e-5 relative after
30 iterations, on the bf16-rounded A for bf16 storage and on the group weights as the device stores them (fp32); L comes from the
oracle's power iteration and is passed to both sides.  With l1_ratio = 0 a group is entirely 0.0 or entirely non-zero and the zero
groups are the reference's; with l1_ratio = 1 the handle is bitwise the unbound one; two runs are bitwise equal."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _coord as cd, _data, _fgroup as fg

pytestmark = pytest.mark.gpu

TOL, ITERS = fg.TOL, fg.ITERS
FIELDS = ("k", "restarts", "stopped")


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


def _labels(start):
    return np.repeat(np.arange(len(start) - 1), np.diff(start))


def _handle(fos, kind, c, loss="squared"):
    P = fos.prepare_grouped(_device(kind, c["A"]), c["b"], _labels(c["start"]), c["gw"], c["mu"], loss=loss, sample_weight=c["w"])
    got = P.feature_groups
    assert P.has_feature_groups and got.start.tolist() == c["start"].tolist() and got.l1_ratio == c["mu"] and P.loss == loss
    assert np.allclose(got.weight, fg.weights_of(c["start"], c["gw"]), rtol=1e-7)
    n, mix = C.c_int32(-1), C.c_double(-1.0)
    assert P.lib.fos_feature_groups_get(C.byref(n), C.byref(mix), P.h) == 0
    assert n.value == len(c["start"]) - 1 + (1 if P.n_dev > P.n else 0) and mix.value == c["mu"]
    return P


def _states(P, c, specs, ctl=None):
    """One state machine per (a1, a2, delta, enet); ctl: the control parameters of a controlled run."""
    from fastoptsolver_amd import _core, _lib
    hs = []
    for a1, a2, delta, enet in specs:
        kw = dict(ctl or {})
        if delta is not None:
            kw = {k: v for k, v in kw.items() if k == "tol_ratio"}
        st = _core.Fista(P)
        st.reset(1.0 / (c["L"] + (0.0 if enet else a2)), a1, a2, mode=_lib.MODE_FISTA if delta is None else _lib.MODE_DELTA,
                 prox_kind=_lib.PROX_ENET if enet else _lib.PROX_L1, delta=delta or 0.0, **kw)
        hs.append(st)
    return hs


def _check(what, c, key, specs, hs, control=False, structure=False):
    for (a1, a2, delta, enet), st in zip(specs, hs):
        ref = fg.reference(*key, a1, a2, enet=enet, delta=delta, control=control)
        x, s = _np(st.x_tensor()), st.status()
        err = _data.rel(x, ref["x"])
        print(f"{what} alpha=({a1:.3g}, {a2}) delta={delta} enet={enet}: rel err {err:.3e}, iterations {int(s.k)} / {ref['k']}, restarts "
              f"{int(s.restarts)} / {ref['restarts']}, stop {int(s.stopped)} / {ref['stopped']}, closest group {ref['closest']:.2e}")
        nr = float(np.linalg.norm(ref["x"]))
        if control is not False:
            assert (int(s.k), int(s.restarts), int(s.stopped)) == (ref["k"], ref["restarts"], ref["stopped"])
            # the status norms, within what 1e-5 on the iterate allows them: | ||x||_1 - ||r||_1 | <= sqrt(n) ||x - r||_2,
            # | ||x||^2 - ||r||^2 | <= (2 ||r|| + ||x - r||) ||x - r||, and a step moves by at most the error of its two iterates
            d = TOL * nr
            assert abs(s.xnorm1 - np.abs(ref["x"]).sum()) <= np.sqrt(len(x)) * d, (s.xnorm1, np.abs(ref["x"]).sum())
            assert abs(s.xnorm2 - nr * nr) <= (2.0 * nr + d) * d, (s.xnorm2, nr * nr)
            assert abs(s.this_step - ref["moves"][-1]) <= 2.0 * d, (s.this_step, ref["moves"][-1])
        else:
            assert (int(s.k), int(s.stopped)) == (ITERS, 0)
        assert nr > 0 and err <= TOL, (what, a1, a2, delta, enet, err)
        if structure and c["mu"] == 0.0:
            zero, full = fg.zero_groups(x, c["start"])
            assert (zero | full).all(), (what, "a group is partly zero")
            if delta is None:                      # the seeds keep every group of these runs CLOSE away from its threshold
                assert ref["closest"] >= fg.CLOSE and np.array_equal(zero, fg.zero_groups(ref["x"], c["start"])[0]), (what, a1)


# ---- every layout where it bites: plain and controlled, both prox kinds, both modes, 1 / 3 / 16 columns ----------------------
CELLS = [(name, lay, mu) for name, lay in fg.BITES for mu in (fg.MUS if name != "panels" else (0.5,))]


@pytest.mark.parametrize("kind", fg.KINDS)
@pytest.mark.parametrize("name,lay,mu", CELLS)
def test_cells_match_the_reference(fos, cus, name, lay, mu, kind):
    from fastoptsolver_amd import _core
    key = fg.key(kind, cus, name, lay, mu)
    c = fg.case(*key)
    P = _handle(fos, kind, c)
    what = f"{name} {lay} mu={mu} {kind}"
    a = c["alphas"]
    big = name == "panels"                         # a reference costs a pass over 65573 rows per iteration there: three columns
    # plain: sixteen columns of mixed families in one call (every penalty x prox kind x mode), three of one family, one alone
    sixteen = [(a1, a2, delta, enet) for enet in (False, True) for delta in (None, 3.0) for a1, a2 in a]
    runs = [[sixteen[1], sixteen[6], sixteen[11]]] if big else [sixteen, [(a1, a2, None, False) for a1, a2 in a[:3]], [(a[1][0], a[1][1], 3.0, True)]]
    for specs in runs:
        hs = _states(P, c, specs)
        assert _core.run_multi(hs, ITERS), P.lib.fos_last_error().decode()
        _check(f"{what} plain x{len(specs)}", c, key, specs, hs, structure=True)
    # controlled: decisions fp32 cannot take the other way, chosen on the reference alone; FISTA with PROX_L1 always has a case
    for enet, delta in ((False, None),) if big else ((False, None), (True, None), (False, 3.0)):
        idx, keep = fg.controlled(*key, enet=enet, delta=delta)
        assert keep or enet or delta is not None
        if not keep:
            continue
        widths = (1,) if big else (1, 3, 16) if (enet, delta) == (False, None) else (len(keep),)
        for width in widths:
            specs = [(keep[i % len(keep)][0], keep[i % len(keep)][1], delta, enet) for i in range(width)]
            hs = _states(P, c, specs, cd.CONTROL_MENU[int(idx)])
            assert _core.run_multi(hs, ITERS), P.lib.fos_last_error().decode()
            _check(f"{what} controlled x{width}", c, key, specs, hs, control=idx)


# ---- the public solvers: either loss, with and without row weights ----------------------------------------------------------
@pytest.mark.parametrize("mu", fg.MUS)
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("kind", fg.KINDS)
def test_paths_compose_with_the_loss_and_the_weights(fos, cus, kind, loss, weighted, mu):
    key = fg.key(kind, cus, "edges", "span150", mu, loss, weighted)
    c = fg.case(*key)
    P = _handle(fos, kind, c, loss)
    path = fos.logistic_path if loss == "logistic" else fos.fista_path
    idx, keep = fg.controlled(*key)
    assert keep
    for delta in (None, 3.0):
        for kw, ctrl, alphas in (({}, False, c["alphas"]), (cd.CONTROL_MENU[int(idx)], idx, keep)):
            if delta is not None and ctrl is not False:
                continue                           # the controlled FISTA-delta cells run in test_cells_match_the_reference
            xs, info = path(P, None, alphas, max_iter=ITERS, L=c["L"], delta=delta, return_info=True, **kw)
            assert len(xs) == len(alphas)
            for (a1, a2), x, (k, code) in zip(alphas, xs, info):
                ref = fg.reference(*key, a1, a2, delta=delta, control=ctrl)
                err = _data.rel(_np(x), ref["x"])
                print(f"{kind} {loss} weighted={weighted} mu={mu} delta={delta} controlled={ctrl is not False} alpha=({a1:.3g}, {a2}): "
                      f"rel err {err:.3e}, iterations {k} / {ref['k']}, stop {code} / {ref['stopped']}")
                assert (k, code) == (ref["k"], ref["stopped"]) and np.linalg.norm(ref["x"]) > 0 and err <= TOL, (a1, a2, err)
    # the host objective, on the handle and on arrays
    x = _np(xs[0])
    a1, a2 = alphas[0]
    want = fos.group_lasso_objective(x, c["A"], c["b"], a1, a2, _labels(c["start"]), c["gw"], mu, loss=loss, sample_weight=c["w"])
    got = fos.group_lasso_objective(x, P, None, a1, a2, _labels(c["start"]), c["gw"], mu)
    assert abs(got - want) <= 1e-12 * abs(want)


# ---- the neutral element: l1_ratio = 1 is the plain update, bit for bit ------------------------------------------------------
def _run_all(P, c, kw):
    from fastoptsolver_amd import _core
    hs = []
    for a1, a2 in c["alphas"]:
        st = _core.Fista(P)
        st.reset(1.0 / (c["L"] + a2), a1, a2, **kw)
        hs.append(st)
    assert _core.run_multi(hs, ITERS), P.lib.fos_last_error().decode()
    return [(st.x_tensor(), tuple(getattr(st.status(), k) for k, _ in st.status()._fields_)) for st in hs]


@pytest.mark.parametrize("prox", ["PROX_L1", "PROX_ENET"])
@pytest.mark.parametrize("ctrl", [False, True], ids=["plain", "controlled"])
@pytest.mark.parametrize("kind", fg.KINDS)
def test_l1_ratio_one_is_bitwise_the_unbound_handle(fos, cus, kind, ctrl, prox):
    from fastoptsolver_amd import _lib
    key = fg.key(kind, cus, "edges", "span150", 1.0, "logistic")
    c = fg.case(*key)
    At = _device(kind, c["A"])
    plain, neutral = fos.prepare(At, c["b"], loss="logistic"), fos.prepare(At, c["b"], loss="logistic")
    neutral.set_feature_groups(_labels(c["start"]), None, 1.0)
    assert neutral.has_feature_groups and not plain.has_feature_groups
    kw = dict(prox_kind=_lib.PROX_ENET if prox == "PROX_ENET" else _lib.PROX_L1, **(cd.CONTROL if ctrl else {}))
    want = _run_all(plain, c, kw)
    assert all(torch.count_nonzero(x) > 0 for x, _ in want)
    for (x0, s0), (x1, s1) in zip(want, _run_all(neutral, c, kw)):
        assert torch.equal(x0, x1) and s0 == s1, (s0, s1)


# ---- determinism -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", fg.KINDS)
def test_two_runs_on_fresh_handles_are_bitwise_equal(fos, cus, kind):
    from fastoptsolver_amd import _core
    key = fg.key(kind, cus, "edges", "span150", 0.5)
    c = fg.case(*key)
    specs = [(a1, a2, delta, enet) for enet in (False, True) for delta in (None, 3.0) for a1, a2 in c["alphas"]]

    def once():
        P = _handle(fos, kind, c)
        hs = _states(P, c, specs)
        assert len(hs) == 16 and _core.run_multi(hs, ITERS)
        return [(st.x_tensor().clone(), tuple(getattr(st.status(), k) for k, _ in st.status()._fields_)) for st in hs]
    first, second = once(), once()
    for (x0, s0), (x1, s1) in zip(first, second):
        assert torch.count_nonzero(x0) > 0 and torch.equal(x0, x1) and s0 == s1


# ---- a live handle -----------------------------------------------------------------------------------------------------------
def test_rebinding_takes_effect_between_runs_and_detaching_restores_the_plain_handle(fos, cus):
    key = fg.key("f32", cus, "edges", "span150", 0.0)
    c = fg.case(*key)
    other_start, other_w = fg.layout("weights", 200, 11)
    P = fos.prepare(_device("f32", c["A"]), c["b"])
    before = fos.fista_path(P, None, c["alphas"], max_iter=ITERS, L=c["L"])
    P.set_feature_groups(np.diff(c["start"]))                           # the sizes form
    first = fos.fista_path(P, None, c["alphas"], max_iter=ITERS, L=c["L"])
    P.set_feature_groups(_labels(other_start), other_w, 0.25)
    assert P.feature_groups.l1_ratio == 0.25 and len(P.feature_groups.weight) == len(other_start) - 1
    second = fos.fista_path(P, None, c["alphas"], max_iter=ITERS, L=c["L"])
    sib = P.sibling(np.roll(c["b"], 17))
    assert sib.has_feature_groups and sib.feature_groups.start.tolist() == other_start.tolist()
    with pytest.raises(ValueError):
        P.set_feature_groups([0, 1] * 100)
    assert P.feature_groups.l1_ratio == 0.25                             # a refused call leaves the binding as it was
    P.set_feature_groups(None)
    n, mix = C.c_int32(-1), C.c_double(-1.0)
    assert P.lib.fos_feature_groups_get(C.byref(n), C.byref(mix), P.h) == 0 and (n.value, mix.value) == (0, 0.0)
    assert not P.has_feature_groups and P.feature_groups is None
    after = fos.fista_path(P, None, c["alphas"], max_iter=ITERS, L=c["L"])
    for (a1, a2), x0, x1, x2, x3 in zip(c["alphas"], before, first, second, after):
        r1 = fg.reference(*key, a1, a2)["x"]
        r2 = fg.run(c["A"], c["b"], a1, a2, c["L"], start=other_start, gw=other_w, mu=0.25)["x"]
        e1, e2 = _data.rel(_np(x1), r1), _data.rel(_np(x2), r2)
        print(f"alpha=({a1:.3g}, {a2}): first binding {e1:.3e}, second {e2:.3e}, across {_data.rel(_np(x2), r1):.3e}")
        assert e1 <= TOL and e2 <= TOL and _data.rel(_np(x2), r1) > 100 * TOL and _data.rel(_np(x0), r1) > 100 * TOL
        assert torch.equal(torch.as_tensor(x0), torch.as_tensor(x3))     # detached: bitwise the plain handle


# ---- cross-validation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("kind", fg.KINDS)
def test_cv_holds_its_contract(fos, cus, kind, loss):
    from tests import _logit as lg
    key = fg.key(kind, cus, "edges", "span150", 0.5, loss)
    c = fg.case(*key)
    m, n = c["A"].shape
    K, alphas = 3, c["alphas"]
    ids = np.arange(m) % K
    P = _handle(fos, kind, c, loss)
    cv, path = (fos.logistic_cv, fos.logistic_path) if loss == "logistic" else (fos.fista_cv, fos.fista_path)
    res = cv(P, None, alphas, ids, max_iter=ITERS, L=c["L"], return_coefs=True)
    coefs = _np(res.coefs)
    assert coefs.shape == (n, K, 4) and len(alphas) == 4
    At = _device(kind, c["A"])
    ref_score = np.zeros((K, 4))
    for f in range(K):
        tr = ids != f
        sub = fos.prepare_grouped(At[torch.as_tensor(tr).cuda()], c["b"][tr], _labels(c["start"]), c["gw"], c["mu"], loss=loss)
        xs = path(sub, None, alphas, max_iter=ITERS, L=c["L"])
        for a, (a1, a2) in enumerate(alphas):
            ref = fg.reference(*key, a1, a2, rows=tr.tobytes())
            e_path, e_ref = _data.rel(coefs[:, f, a], _np(xs[a])), _data.rel(coefs[:, f, a], ref["x"])
            print(f"{kind} {loss} fold {f} alpha {a}: against the path on the gathered rows {e_path:.3e}, against the reference {e_ref:.3e}")
            assert np.linalg.norm(ref["x"]) > 0 and e_path <= TOL and e_ref <= TOL
            te = ~tr
            if loss == "logistic":
                ref_score[f, a] = lg.nll(c["A"][te], ref["x"][:, None], c["b"][te])[0] / te.sum()
            else:
                ref_score[f, a] = float(((c["A"][te] @ ref["x"] - c["b"][te]) ** 2).sum()) / te.sum()
    score = res.logloss if loss == "logistic" else res.mse
    means = ref_score.mean(axis=0)
    print(f"{kind} {loss}: mean held-out scores {score.mean(axis=0)}, of the reference's coefficients {means}")
    assert res.best == int(np.argmin(means))
    a1, a2 = alphas[res.best]                                            # the refit runs in the lockstep too
    assert _data.rel(_np(res.x), fg.reference(*key, a1, a2)["x"]) <= TOL


# ---- the bind's checks that need the handle ----------------------------------------------------------------------------------
def test_bind_checks_the_table_against_the_problem(fos):
    P = fos.prepare(torch.zeros(300, 200, device="cuda"), torch.zeros(300))

    def bind(start, weight=None, mix=0.0):
        s = (C.c_int32 * len(start))(*start)
        w = None if weight is None else (C.c_float * len(weight))(*weight)
        return P.lib.fos_feature_groups_bind(s, w, len(start) - 1, mix, P.h)
    assert bind([0, 100, 199]) == -1 and bind([0, 100, 201]) == -1 and bind(list(range(202))) == -1      # FOS_ERR_ARG
    assert "fos_feature_groups_bind" in P.lib.fos_last_error().decode()
    n, mix = C.c_int32(-1), C.c_double(-1.0)
    assert P.lib.fos_feature_groups_get(C.byref(n), C.byref(mix), P.h) == 0 and n.value == 0
    assert bind([0, 100, 200], [1.0, 0.0], 0.75) == 0 and bind(list(range(201))) == 0                    # ngroups = n is served
    assert P.lib.fos_feature_groups_get(C.byref(n), C.byref(mix), P.h) == 0 and (n.value, mix.value) == (200, 0.0)
