"""CPU: the fp64 reference of the working-set solve (tests/_working_set.py) is validated on its own - its scan against a
coordinate-by-coordinate restatement of the header's arithmetic, its result against the optimality conditions and the minimiser
of the FULL problem, the planted growth case and the fall-back."""
import numpy as np
import pytest

from tests import _working_set as ws

CASES = [("squared", False, False), ("squared", True, True), ("logistic", False, False), ("logistic", True, True),
         ("squared", False, True), ("logistic", True, False)]
IDS = [f"{loss}{'-weighted' if w else ''}{'-factors' if p else ''}" for loss, w, p in CASES]


def _scan_by_hand(G, alpha1, slack, in_ws, p):
    n = G.shape[1]
    excess, viol = np.zeros(n, dtype=np.float32), []
    for i in range(n):
        if in_ws[i]:
            continue
        worst, bad = 0.0, False
        for j in range(G.shape[0]):
            a, d = float(abs(np.float32(G[j, i]))), float(alpha1[j]) * float(np.float32(p[i]))
            worst = max(worst, a / d if d > 0.0 else (np.inf if a > 0.0 else 0.0))
            bad = bad or a > d * (1.0 + slack)
        excess[i] = np.float32(worst)
        if bad:
            viol.append(i)
    return excess, np.asarray(viol, dtype=np.int32)


@pytest.mark.parametrize("nv", [1, 16])
def test_scan_is_the_stated_arithmetic(nv):
    rng = np.random.default_rng(5)
    n = 200
    G = rng.standard_normal((nv, n)).astype(np.float32)
    p = (10.0 ** rng.uniform(-1, 1, n)).astype(np.float32)
    p[[0, 7, 199]] = 0.0
    G[:, 7] = 0.0                                               # 0 / 0: excess 0, no violator
    a1 = rng.uniform(0.5, 2.0, nv)
    in_ws = (rng.random(n) < 0.3).astype(np.uint8)
    in_ws[[0, 7]] = 0
    for slack in (0.0, 1e-4, 0.5):
        e, v = ws.scan(G, a1, slack, in_ws, p)
        e2, v2 = _scan_by_hand(G, a1, slack, in_ws, p)
        assert e.dtype == np.float32 and v.dtype == np.int32 and np.array_equal(e, e2) and np.array_equal(v, v2)
        assert np.isinf(e[0]) and 0 in v and e[7] == 0.0 and 7 not in v and (e[in_ws != 0] == 0).all()
        assert (np.diff(v) > 0).all() and not in_ws[v].any()
    assert len(ws.scan(G, a1, 0.0, np.ones(n, dtype=np.uint8), p)[1]) == 0                      # a full set: nothing to check
    e, v = ws.scan(G, a1, 0.0, np.zeros(n, dtype=np.uint8), None)
    assert np.array_equal(v, np.nonzero((np.abs(G).astype(np.float64) > a1[:, None]).any(axis=0))[0])


@pytest.mark.parametrize("loss,weighted,penalized", CASES, ids=IDS)
def test_result_is_the_minimiser_of_the_full_problem(loss, weighted, penalized):
    c = ws.case(loss, weighted, penalized, "f32")
    kw = dict(p=c["p"], loss=loss, w=c["w"])
    Xf = ws.full(c["A"], c["b"], c["alphas"], 2 * ws.ITERS, **kw)
    # the inputs: the full-problem reference run to convergence meets the bound itself
    assert ws.kkt_violation(c["A"], c["b"], Xf, c["alphas"], **kw).max() <= 1e-8
    X, info = ws.solve(c["A"], c["b"], c["alphas"], 2 * ws.ITERS, **kw)
    assert not info["fell_back"] and info["rounds"] >= 1 and info["sizes"][0] <= 0.5 * ws.N
    assert info["full_gradients"] == info["rounds"] + 1 and info["worst_excess"] <= 1.0 + 1e-4
    assert ws.kkt_violation(c["A"], c["b"], X, c["alphas"], **kw).max() <= 1e-8
    assert (np.count_nonzero(X, axis=0) >= 1).all() and np.count_nonzero(X[:, -1]) >= ws.SUPPORT - 1
    if penalized:                                               # the unpenalised coordinates are in every set and non-zero
        assert (X[c["p"] == 0] != 0).all()
    strictly_convex = [j for j, (_, a2) in enumerate(c["alphas"]) if a2 > 0]
    assert len(strictly_convex) == ws.WEIGHTS // 2
    for j in strictly_convex:
        assert np.linalg.norm(X[:, j] - Xf[:, j]) <= 1e-8 * np.linalg.norm(Xf[:, j]), j


def test_the_planted_case_grows():
    c = ws.case("squared", False, False, "f32", **ws.GROWTH)
    X, info = ws.solve(c["A"], c["b"], c["alphas"], ws.ITERS)
    assert info["rounds"] >= 2 and not info["fell_back"], info
    assert info["sizes"][1] == 2 * info["sizes"][0] and info["sizes"][1] <= 0.5 * ws.N           # the top-k branch filled the set
    assert info["worst_excess"] <= 1.0 + 1e-4
    assert ws.kkt_violation(c["A"], c["b"], X, c["alphas"]).max() <= 1e-8
    # round 1 alone is not the answer: stopped there, the full problem's conditions are violated
    X1, one = ws.solve(c["A"], c["b"], c["alphas"], ws.ITERS, max_rounds=1)
    assert one["fell_back"] and one["rounds"] == 1


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_a_small_max_fraction_falls_back_to_the_full_solve(loss):
    c = ws.case(loss, False, False, "f32")
    X, info = ws.solve(c["A"], c["b"], c["alphas"], 2 * ws.ITERS, loss=loss, max_fraction=ws.FALLBACK_FRACTION)
    assert info["fell_back"] and info["rounds"] == 0 and info["sizes"] == []
    Xf = ws.full(c["A"], c["b"], c["alphas"], 2 * ws.ITERS, loss=loss)
    assert np.array_equal(X, Xf)                                # from X = 0 the fall-back IS the full reference
    assert info["worst_excess"] <= 1.0 + 1e-4


def test_an_initial_set_is_taken_as_given_and_corrected():
    c = ws.case("squared", False, False, "f32")
    X, info = ws.solve(c["A"], c["b"], c["alphas"], 2 * ws.ITERS, initial=c["support"][:2])
    assert info["sizes"][0] == 2 and info["rounds"] >= 2 and not info["fell_back"]
    assert ws.kkt_violation(c["A"], c["b"], X, c["alphas"]).max() <= 1e-8
    Xa, all_in = ws.solve(c["A"], c["b"], c["alphas"], ws.ITERS, initial=np.arange(ws.N), max_fraction=1.0)
    # the same iteration on a copy of A: equal up to the fp64 rounding of another memory layout in the matrix products
    Xf = ws.full(c["A"], c["b"], c["alphas"], ws.ITERS)
    assert all_in["rounds"] == 1 and np.linalg.norm(Xa - Xf) <= 1e-12 * np.linalg.norm(Xf)
