"""CPU: the fp64 reference of the coordinate lockstep (tests/_coord.py) is validated independently of the code under test - with
unit factors and infinite bounds it IS the unmodified oracle, and run to convergence it satisfies the optimality conditions of
the stated objective - and every recipe and case the GPU tests use shows, on the reference alone, what those tests are about."""
import numpy as np
import pytest

from oracle import fos_oracle as orc
from tests import _coord as cd, _data, _logit as lg, _menu_coord as mc, _weighted as wt

CUS = 256


def test_neutral_data_is_the_unmodified_oracle():
    A, b, _ = _data.synth(300, 40, 5)
    L = float(orc.estimate_lipschitz(A, v0=np.ones(40)))
    lam = float(np.max(np.abs(A.T @ b)))
    y = lg.labels(A, _data.synth(300, 40, 5)[2], 5)
    w = wt.weights("spread", 300, 5)
    ones, inf = np.ones(40), np.full(40, np.inf)
    for a1, a2 in ((0.1 * lam, 0.0), (0.05 * lam, 0.5)):
        for kw in ({}, dict(adaptive_restart=True, restart_threshold=0.9, tol_ratio=0.2), dict(delta=3.0)):
            got = cd.run(A, b, a1, a2, L, p=ones, lo=-inf, hi=inf, **kw)
            if "delta" in kw:
                want = orc.fista_delta(A, b, "elasticnet", a1, a2, 3.0, max_iter=lg.ITERS, L=L)
            else:
                want = orc.fista(A, b, "elasticnet", a1, a2, max_iter=lg.ITERS, L=L, **kw)
            assert np.array_equal(got["x"], want), (a1, a2, kw)
            assert np.array_equal(cd.run(A, y, a1 / lam, a2, L / 4, p=ones, lo=-inf, hi=inf, loss="logistic", **kw)["x"],
                                  lg.run(A, y, a1 / lam, a2, L / 4, **kw)[0])
            for loss, rhs in (("squared", b), ("logistic", y)):
                assert np.array_equal(cd.run(A, rhs, a1 / lam, a2, L, p=ones, lo=-inf, hi=inf, loss=loss, w=w, **kw)["x"],
                                      wt.run(A, rhs, w, a1 / lam, a2, L, loss=loss, **kw)[0])
    # the PROX_ENET form with unit factors is the oracle's ISTA-style elastic-net prox inside the same loop
    st = cd.run(A, b, 0.1 * lam, 0.5, L, 1, p=ones, lo=-inf, hi=inf, enet=True)
    g0 = A.T @ (A @ np.zeros(40) - b)
    assert np.array_equal(st["x"], orc.prox_elastic_net(-g0 / L, 1.0 / L, 0.1 * lam, 0.5))


def _converged(A, b, a1, a2, L, p, lo, hi, **kw):
    ref = cd.run(A, b, a1, a2, L, 20000, p=p, lo=lo, hi=hi, adaptive_restart=True, restart_threshold=1.0, **kw)
    return ref["prob"], ref["x"]


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("data", ["tiny", "synthetic"])
def test_the_converged_reference_satisfies_the_kkt_conditions(data, loss):
    if data == "tiny":
        A, b, _ = _data.problem("tiny")
        A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
    else:
        A, b, _ = _data.synth(300, 40, 11)
    n = A.shape[1]
    if loss == "logistic":
        b = (b > np.median(b)).astype(np.float64)
    L = float(np.linalg.eigvalsh(A.T @ A)[-1]) / (4.0 if loss == "logistic" else 1.0)
    g0 = A.T @ ((0.5 - b) if loss == "logistic" else -b)
    lam = float(np.max(np.abs(g0)))
    p = cd.factors(n, 11)
    for a1, a2, enet in ((0.05 * lam, 0.0, False), (0.02 * lam, 0.3, False), (0.02 * lam, 0.3, True)):
        x_unc = cd.run(A, b, a1, a2, L, 2000, p=p, loss=loss)["x"]
        lo, hi = cd.bounds(x_unc, 11)
        prob, x = _converged(A, b, a1, a2, L, p, lo, hi, loss=loss, enet=enet)
        viol = cd.kkt_violation(prob, x)
        active = int(np.sum((x == lo) | (x == hi)))
        print(f"{data} {loss} a1={a1:.3g} a2={a2} enet={enet}: KKT violation {viol:.3e} relative {viol / lam:.3e}, "
              f"{active} coordinates at a bound, {int(np.count_nonzero(x))} nonzero")
        assert viol <= 1e-8 * lam, (viol, lam)
        assert active >= 2 and (((x == lo) & (lo < 0)) | ((x == hi) & (hi > 0))).any()     # sign bounds and a nonzero one bind
    # the check itself: the unbounded solution violates the conditions of the bounded problem, and a clipped one too
    free_prob, x_free = _converged(A, b, a1, a2, L, p, None, None, loss=loss)
    assert cd.kkt_violation(free_prob, x_free) <= 1e-8 * lam
    assert cd.kkt_violation(prob, np.clip(x_free, lo, hi)) > 1e-4 * lam


def _cases():
    for kind in ("f32", "bf16"):
        for name, s in mc.shapes(kind, CUS).items():
            yield kind, "squared", name, s["m"], s["n"], False
    for kind in ("f32", "bf16"):                           # the composition and cross-validation cases of tests/test_gpu_coord.py
        for loss in ("squared", "logistic"):
            for weighted in (False, True):
                if (loss, weighted) != ("squared", False):
                    s = mc.shapes(kind, CUS)["edges"]
                    yield kind, loss, "edges", s["m"], s["n"], weighted


@pytest.mark.parametrize("kind,loss,name,m,n,weighted", list(_cases()))
def test_every_gpu_case_meets_its_preconditions(kind, loss, name, m, n, weighted):
    seed = 3 * m + n
    c = cd.case(kind, loss, m, n, seed, weighted)
    assert c["p"][0] == 0.0 and 0 < np.mean(c["p"] == 0.0) < 0.3 and c["p"][c["p"] > 0].max() / c["p"][c["p"] > 0].min() > 10
    assert (c["lo"] == 0).any() and (c["hi"] == 0).any() and ((c["lo"] < 0) & np.isfinite(c["lo"])).any()
    assert (c["lo"] <= 0).all() and (c["hi"] >= 0).all()
    for a1, a2 in c["alphas"]:
        ref = cd.reference(kind, loss, m, n, seed, weighted, a1, a2)
        pre = cd.preconditions(ref, c["x_unc"], c["p"], c["lo"], c["hi"])
        free = cd.run(c["A"], c["b"], a1, a2, c["L"], p=c["p"], loss=loss, w=c["w"])["x"]
        moved = _data.rel(ref["x"], free)
        print(f"{kind} {loss} {name} weighted={weighted} a1={a1:.3g} a2={a2}: {pre}, {moved:.0%} away from the unbounded fit")
        assert min(pre.values()) > 0, pre             # at EVERY weight: a nonzero lower and a nonzero upper bound active, ...
        assert moved > 100 * lg.TOL                     # the bounds change the answer by far more than the tolerance
    # the controlled runs (the controlled cells; the controlled half of the composition test): fp32-proof decisions
    ctl, keep = cd.controlled(kind, loss, m, n, seed, weighted)
    assert len(keep) >= 2, keep
    genuine = 0
    for a1, a2 in keep:
        for enet in (False, True):
            ref = cd.reference(kind, loss, m, n, seed, weighted, a1, a2, enet=enet, control=str(cd.CONTROL_MENU.index(ctl)))
            assert cd.decision_margin(ref, ctl["restart_threshold"], ctl["tol_ratio"]) >= cd.MARGIN
            assert cd.fp32_proof(ref, ctl["restart_threshold"], ctl["tol_ratio"])
            genuine += cd.genuine_restarts(ref, ctl["restart_threshold"])
    print(f"{kind} {loss} {name} weighted={weighted}: tol_ratio {ctl['tol_ratio']}, {len(keep)} controlled pairs, "
          f"{genuine} restarts on a finite ratio")
    # Restart decisions on a finite ratio (the first iteration's infinite ratio always "restarts") are exercised where a run goes
    # the full 30 iterations: the narrow and the whole-workgroup shapes and the weighted compositions.  The tall shapes (rb2,
    # panels) and the unweighted edges cases stop on the ratio rule within 2 to 8 iterations: they cover the stop, not the restart.
    if name in ("one_tile", "whole_wgs") or weighted:
        assert genuine >= 2, genuine
