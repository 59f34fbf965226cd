"""CPU: the fp64 reference of the multinomial working set and duality gap (tests/_multinomial_ws.py) on its own - weak duality at
random points, a vanishing gap at a converged solution, the C = 2 identity with the logistic certificate, the scan against a
plain restatement, and the margins every chosen path case must keep so that an fp32 device takes the same decisions."""
import numpy as np
import pytest

from tests import _duality as du, _multinomial as mn, _multinomial_ws as mw, _working_set as wk


def _small(C, seed=3, m=120, n=30):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n)) / np.sqrt(m)
    XT = np.zeros((n, C))
    XT[rng.choice(n, 5, replace=False)] = 2.0 * rng.standard_normal((5, C))
    y = np.argmax(4.0 * (A @ XT) + rng.gumbel(size=(m, C)), axis=1).astype(np.float64)
    assert set(y.tolist()) == set(range(C))
    return A, y, rng


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("C", [2, 3, 7])
def test_the_gap_is_non_negative_at_random_points(C, grouped):
    A, y, rng = _small(C)
    n = A.shape[1]
    w = rng.uniform(0.0, 3.0, A.shape[0])
    p = rng.uniform(0.5, 2.0, n)
    amax = mw.alpha_max(A, y, C, grouped, w, p)
    fits = [rng.standard_normal((n, C)) * rng.choice([0.0, 1.0], size=(n, 1)) * scale for scale in (0.0, 0.1, 1.0, 10.0)]
    for a1, a2 in ((0.3 * amax, 0.0), (0.1 * amax, 0.05 * amax), (2.0 * amax, 0.0)):
        cert = mw.certificate(A, y, C, fits, [(a1, a2)] * len(fits), grouped, w, p)
        assert (cert["gap"] >= -1e-12 * cert["mag_gap"]).all(), cert["gap"]
        assert ((cert["scale"] >= 0.0) & (cert["scale"] <= 1.0)).all()
        assert np.isfinite(cert["dual"]).all()
    # above alpha_max X = 0 is the solution: the gap at 0 vanishes and the scale is 1
    cert = mw.certificate(A, y, C, [np.zeros((n, C))], [(1.0001 * amax, 0.0)], grouped, w, p)
    assert cert["scale"][0] == 1.0 and abs(cert["gap"][0]) <= 1e-12 * cert["mag_gap"][0]


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("a2_ratio", [0.0, 0.1])
def test_the_gap_closes_at_a_converged_solution(grouped, a2_ratio):
    C = 3
    A, y, _ = _small(C)
    n = A.shape[1]
    a1 = 0.1 * mw.alpha_max(A, y, C, grouped)
    a2 = a2_ratio * a1
    X = mw.inner(A, y, C, a1, a2, grouped, mw.lipschitz(A), 5000)
    cert = mw.certificate(A, y, C, [X], [(a1, a2)], grouped)
    p0 = mw.certificate(A, y, C, [np.zeros((n, C))], [(a1, a2)], grouped)["primal"][0]
    assert cert["dual"][0] <= cert["primal"][0] + 1e-12 * cert["mag_gap"][0]
    assert cert["gap"][0] / p0 < 1e-8, cert["gap"][0] / p0
    # and the zero rows meet their optimality condition
    excess, viol, _ = mw.scan(mw.gradient_block(A, y, C, [X]).astype(np.float32), C, grouped, [a1], 1e-6,
                              (np.abs(X).sum(axis=1) != 0).astype(np.uint8))
    assert viol.size == 0 and excess.max() <= 1.0 + 1e-6


def test_two_classes_with_a_zero_second_column_are_the_logistic_certificate():
    """C = 2, X = (x, 0): z = (a.x, 0), softmax = (sigma, 1 - sigma), the cross-entropy of label y is the log-loss of b = [y = 0]
    and G = (g, -g) gives the l1 scale of the logistic certificate.  With alpha2 = 0 the penalties agree too."""
    A, y, rng = _small(2)
    n = A.shape[1]
    b = (y == 0).astype(np.float64)
    w = rng.uniform(0.5, 2.0, A.shape[0])
    a1 = 0.2 * mw.alpha_max(A, y, 2, False, w)
    xs = [rng.standard_normal(n) * rng.choice([0.0, 1.0], size=n) * s for s in (0.0, 0.3, 3.0)]
    ref = du.certificate(du.LOGISTIC, A, b, np.stack(xs, axis=1), [(a1, 0.0)] * 3, w=w)
    got = mw.certificate(A, y, 2, [np.stack([x, np.zeros(n)], axis=1) for x in xs], [(a1, 0.0)] * 3, False, w)
    for key in ("primal", "dual", "gap", "scale"):
        np.testing.assert_allclose(got[key], ref[key], rtol=1e-12, atol=1e-12 * ref["mag_gap"].max(), err_msg=key)


@pytest.mark.parametrize("grouped", [False, True])
def test_the_scan_is_the_stated_arithmetic(grouped):
    rng = np.random.default_rng(5)
    C, n, k = 3, 41, 2
    G = rng.standard_normal((k * C, n)).astype(np.float32)
    p = rng.uniform(0.5, 2.0, n).astype(np.float32)
    p[[3, 17]] = 0.0
    G[:, 17] = 0.0                                         # an unpenalised coordinate without a gradient: excess 0
    in_ws = np.zeros(n, dtype=np.uint8)
    in_ws[[0, 5, 40]] = 1
    a1 = [0.8, 0.0]                                        # one segment with alpha1 = 0
    excess, viol, margin = mw.scan(G, C, grouped, a1, 0.25, in_ws, p)
    want_e, want_v = np.zeros(n), []
    for i in range(n):
        if in_ws[i]:
            continue
        worst, bad = 0.0, False
        for s in range(k):
            g = G[s * C:(s + 1) * C, i].astype(np.float64)
            v = float(np.sqrt(sum(float(x) * float(x) for x in g))) if grouped else float(np.abs(g).max())
            d = a1[s] * float(p[i])
            worst = max(worst, v / d if d > 0 else (np.inf if v > 0 else 0.0))
            bad = bad or v > d * 1.25
        want_e[i] = worst
        if bad:
            want_v.append(i)
    np.testing.assert_array_equal(viol, np.asarray(want_v, dtype=np.int32))
    np.testing.assert_allclose(excess.astype(np.float64), want_e.astype(np.float32).astype(np.float64), rtol=2e-7)
    assert np.isinf(excess[3]) and excess[17] == 0.0 and (excess[[0, 5, 40]] == 0).all() and margin > 0
    assert mw.alpha_max(np.eye(n), np.arange(n) % C, C, grouped) > 0


@pytest.mark.parametrize("name", list(mw.WS_CASES))
def test_the_working_set_cases_keep_their_margins(name):
    grouped, args, loop = mw.WS_CASES[name]
    cs = mw.path_case(grouped, *args)
    ref = mw.ws_reference(name)
    assert len(ref) == 2 and [len(fits) for fits, _ in ref] == [5, 2]
    for (fits, info), (first, number) in zip(ref, mw.groups(mw.PATH_WEIGHTS, cs["C"])):
        print(name, info["sizes"], info["fell_back"], info["scan_margins"], info["growth_gaps"], info["worst_excess"])
        assert info["scan_margins"].min() > mw.SCAN_MARGIN, info["scan_margins"]
        assert info["growth_gaps"].size == 0 or info["growth_gaps"].min() > mw.GROWTH_GAP, info["growth_gaps"]
        if not info["fell_back"]:                          # certified: the zero rows are right for the full problem, and on the
            #                                                well-conditioned designs the full lockstep arrives at the same point
            assert info["worst_excess"] <= 1.0 + 1e-4
            for X, (a1, a2) in zip(fits, cs["alphas"][first:first + number] if name in ("l1", "grouped") else ()):
                full = mw.inner(cs["A"], cs["y"], cs["C"], a1, a2, grouped, cs["L"], 4 * mw.WS_ITERS)
                assert mn.rel(X, full) < mw.TOL, mn.rel(X, full)     # (both are iterates on their way to the same minimiser)
    infos = [info for _, info in ref]
    if name == "fallback":
        assert infos[1]["fell_back"] and infos[1]["rounds"] == 1 and not infos[0]["fell_back"]
    elif name == "initial":
        assert all(i["rounds"] == 2 and i["sizes"][0] == 64 and i["full_gradients"] == 2 for i in infos)
    else:
        assert not any(i["fell_back"] for i in infos) and all(i["rounds"] >= 1 for i in infos)
        zero = [np.abs(X).sum(axis=1) == 0 for fits, _ in ref for X in fits]
        assert all(z.any() and (~z).any() for z in zero[1:])
        if grouped:                                        # a row is in the model for every class or for none
            assert all(((X != 0).all(axis=1) | (X == 0).all(axis=1)).all() for fits, _ in ref for X in fits)


@pytest.mark.parametrize("name", list(mw.CERT_CASES))
def test_the_certified_cases_keep_their_margins(name):
    ref = mw.cert_reference(name)
    assert [len(fits) for fits, _ in ref] == [5, 2]
    for fits, info in ref:
        print(name, info["sizes"], info["fell_back"], info["certificates"], info["stop_margins"].min(), info["scan_margins"], info["growth_gaps"])
        assert info["stop_margins"].min() > mw.STOP_MARGIN, info["stop_margins"]
        assert info["scan_margins"].min() > mw.SCAN_MARGIN, info["scan_margins"]
        assert info["growth_gaps"].size == 0 or info["growth_gaps"].min() > mw.GROWTH_GAP
        assert (info["gap"] >= -1e-12 * info["mag_gap"]).all()
    infos = [info for _, info in ref]
    if name == "beyond_max_fraction":
        assert all(i["fell_back"] and i["rounds"] == 1 and i["certificates"] == 3 for i in infos)
        assert all(i["sizes"][0] <= 0.995 * 256 for i in infos)
    else:
        assert all(i["certified"].all() and not i["fell_back"] for i in infos)
    if name == "same_set_again":
        assert any(i["sizes"][-1] == i["sizes"][-2] for i in infos)


def test_the_cases_of_the_entry_points_are_on_the_way_and_converged():
    """Some iterates have a gap worth measuring and the last one is converged; the lasso cases have an active scale, the elastic-net
    ones an active conjugate, the free case s = 0."""
    for C, grouped in ((2, False), (3, True), (7, False), (16, True)):
        for form in mw.FORMS:
            cs = mw.case(C, grouped, form, "one_tile")
            pre = cs["pre"]
            assert (pre["gap"] >= -1e-12 * pre["mag_gap"]).all()
            if form == "free":
                assert (pre["scale"][:4] == 0.0).all(), pre["scale"]
            else:
                assert pre["gap"][-1] / pre["primal"][0] < 1e-3 and pre["gap"][0] / pre["primal"][0] > 1e-3
                if form in ("lasso", "penalised"):
                    assert (pre["scale"][:3] < 1.0).any(), pre["scale"]
            if form == "weighted":
                assert (cs["w"] == 0).any()
    assert wk.PAD_COLUMNS == 64 and wk.MIN_COLUMNS == 128
