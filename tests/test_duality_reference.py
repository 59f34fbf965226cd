"""CPU: the fp64 reference of the duality-gap certificate (tests/_duality.py) on its own - weak duality at random points, the gap
along the reference's own FISTA iterates, the two ends of the scale, and the preconditions of the cases that
tests/test_gpu_duality.py runs on the device."""
import functools

import numpy as np
import pytest

from tests import _duality as du

M, N = 60, 25
FORMS = ("plain", "zero_weights", "zero_factor")


@functools.lru_cache(maxsize=None)
def _small(loss, form):
    """A 60 x 25 problem: (A, b, c, w, p, alpha_max).  zero_weights: a fifth of the row weights are 0; zero_factor: factors in
    [0.5, 2] and one unpenalised coordinate."""
    rng = np.random.default_rng(50 + 7 * du.LOSSES.index(loss) + FORMS.index(form))
    A = rng.standard_normal((M, N))
    xt = np.where(rng.random(N) < 0.2, rng.standard_normal(N), 0.0)
    c = None
    if loss == du.LOGISTIC:
        b = (rng.random(M) < 0.5 * (1.0 + np.tanh(0.5 * (A @ xt)))).astype(np.float64)
    elif loss == du.HINGE:
        b = np.where(A @ xt + 0.3 * rng.standard_normal(M) >= 0.0, 1.0, -1.0)
    else:
        b = A @ xt + 0.3 * rng.standard_normal(M)
        c = 0.4 if loss == du.HUBER else None
    w = p = None
    if form == "zero_weights":
        w = rng.uniform(0.25, 4.0, M)
        w[rng.choice(M, M // 5, replace=False)] = 0.0
    if form == "zero_factor":
        p = rng.uniform(0.5, 2.0, N).astype(np.float32).astype(np.float64)
        p[3] = 0.0
    g0 = np.abs(du.gradient(loss, A, np.zeros((N, 1)), b, c, w)[:, 0])
    pp = np.ones(N) if p is None else p
    return A, b, c, w, p, float((g0[pp > 0] / pp[pp > 0]).max())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ridge", [False, True], ids=["lasso", "enet"])
@pytest.mark.parametrize("loss", du.LOSSES)
def test_weak_duality_at_random_points(loss, ridge, form):
    A, b, c, w, p, amax = _small(loss, form)
    rng = np.random.default_rng(99)
    X = rng.standard_normal((N, 12)) * rng.choice([0.0, 0.05, 0.5, 3.0], size=(N, 12))
    X[:, 0] = 0.0
    alphas = [(amax * f, amax * f * 0.3 if ridge else 0.0) for f in np.geomspace(1.5, 0.01, 12)]
    r = du.certificate(loss, A, b, X, alphas, c, w, p)
    assert np.isfinite(r["primal"]).all() and np.isfinite(r["dual"]).all()
    assert (r["gap"] >= -1e-12 * np.abs(r["primal"])).all(), r["gap"] / np.abs(r["primal"])
    assert ((0.0 <= r["scale"]) & (r["scale"] <= 1.0)).all()
    assert (r["gap"][1:] > 1e-6 * r["primal"][1:]).all()                # random points are not optimal: the bound says so


# The iteration count at which the gap of the reference's own FISTA iterates is below 1e-9 P(0), recorded from this file's
# recipe (60 x 25, the weight a tenth of alpha_max, alpha2 = alpha1 / 10 for the elastic net): at a quarter of the count it is not.
CONVERGED_AT = {(du.SQUARED, False): 200, (du.SQUARED, True): 100, (du.LOGISTIC, False): 400, (du.LOGISTIC, True): 200,
                (du.HUBER, False): 400, (du.HUBER, True): 200, (du.HINGE, False): 400, (du.HINGE, True): 200}


@pytest.mark.parametrize("ridge", [False, True], ids=["lasso", "enet"])
@pytest.mark.parametrize("loss", du.LOSSES)
def test_the_gap_falls_below_1e_9_along_the_fista_iterates(loss, ridge):
    A, b, c, w, p, amax = _small(loss, "plain")
    a1 = 0.1 * amax
    a2 = a1 / 10.0 if ridge else 0.0
    count = CONVERGED_AT[loss, ridge]
    X = du.iterates(loss, A, b, a1, a2, du.lipschitz(loss, A), (count // 4, count), c)
    r = du.certificate(loss, A, b, X, [(a1, a2)] * 2, c)
    p0 = du.certificate(loss, A, b, np.zeros((N, 1)), [(a1, a2)], c)["primal"][0]
    print(f"{loss} ridge={ridge}: gap / P(0) = {r['gap'][0] / p0:.2e} at {count // 4}, {r['gap'][1] / p0:.2e} at {count}")
    assert -1e-12 * p0 <= r["gap"][1] <= 1e-9 * p0, r["gap"] / p0
    assert r["gap"][0] > 1e-9 * p0, r["gap"] / p0                       # the recorded count is not slack


@pytest.mark.parametrize("ridge", [False, True], ids=["lasso", "enet"])
@pytest.mark.parametrize("loss", du.LOSSES)
def test_a_free_coordinate_with_a_gradient_gives_scale_zero_and_a_finite_gap(loss, ridge):
    A, b, c, w, p, amax = _small(loss, "zero_factor")
    X = np.zeros((N, 2))
    X[5, 1] = 0.3
    alphas = [(0.3 * amax, 0.05 * amax if ridge else 0.0)] * 2
    G = du.gradient(loss, A, X, b, c, w).T
    assert (G[:, 3] != 0.0).all() and p[3] == 0.0
    r = du.certificate(loss, A, b, X, alphas, c, w, p)
    assert (r["scale"] == 0.0).all()
    assert np.isfinite(r["gap"]).all() and (r["gap"] > 0.0).all()
    # the dual point is 0: D = -F*(0) - nothing, the infimum of the data term over z
    d0 = du.dual_terms(loss, A @ X, b, 0.0, c).sum(axis=0)
    assert np.allclose(r["dual"], d0, rtol=0, atol=1e-12 * np.abs(r["primal"]).max())
    if loss == du.LOGISTIC:
        assert (r["dual"] == 0.0).all()                                  # the entropy at the labels 0 / 1, exactly
    # with the gradient gone in that coordinate it constrains nothing
    G[:, 3] = 0.0
    assert (du.scale_of(G, p, alphas) > 0.0).all()


@pytest.mark.parametrize("form", ["plain", "zero_weights"])
@pytest.mark.parametrize("loss", du.LOSSES)
def test_the_scale_is_one_with_a_ridge_on_every_coordinate(loss, form):
    A, b, c, w, _, amax = _small(loss, form)
    rng = np.random.default_rng(5)
    X = rng.standard_normal((N, 6))
    p = rng.uniform(0.5, 2.0, N)
    for pf in (None, p):
        r = du.certificate(loss, A, b, X, [(1e-3 * amax, 1e-2 * amax)] * 6, c, w, pf)
        assert (r["scale"] == 1.0).all()
    assert (du.certificate(loss, A, b, X, [(1e-3 * amax, 0.0)] * 6, c, w, p)["scale"] < 1.0).all()


def test_scale_of_in_its_stated_arithmetic():
    G = np.array([[0.5, -2.0, 0.0, 4.0], [0.25, 0.0, 0.0, 0.0]], dtype=np.float32)
    p = np.array([1.0, 2.0, 0.0, 0.0], dtype=np.float32)
    s = du.scale_of(G, p, [(1.0, 0.0), (1.0, 0.0)])
    assert s[0] == 0.0 and s[1] == 1.0                                   # p = 0 against G != 0; p = 0 against G = 0 is no constraint
    assert du.scale_of(G[:, :2], p[:2], [(1.0, 0.0), (0.125, 0.0)]).tolist() == [1.0, 0.5]     # |G| = tau keeps 1, |G| = 2 tau halves
    assert du.scale_of(G, None, [(0.0, 0.0), (0.0, 0.0)]).tolist() == [0.0, 0.0]
    assert du.scale_of(np.zeros((1, 4), np.float32), None, [(0.0, 0.0)]).tolist() == [1.0]     # the minimum of an empty set
    assert du.scale_of(G, None, [(0.1, 0.3), (0.0, 1e-300)]).tolist() == [1.0, 1.0]
    third = np.float32(3.0)
    assert du.scale_of(np.array([[third]]), np.array([0.7], np.float32), [(0.9, 0.0)])[0] == 0.9 * float(np.float32(0.7)) / 3.0


# ---- the cases of tests/test_gpu_duality.py ----------------------------------------------------------------------------------
CASES = [(loss, form, shape, "f32") for shape in du.SHAPES for loss in du.LOSSES for form in du.FORMS] + \
        [(loss, form, "edges", "bf16") for loss in du.LOSSES for form in du.FORMS]


@pytest.mark.parametrize("loss,form,shape,kind", CASES)
def test_the_points_of_the_device_cases_are_where_they_should_be(loss, form, shape, kind):
    cs = du.case(loss, form, shape, kind)
    rel = cs["pre"]["gap"] / cs["p0"]
    print(loss, form, shape, kind, " ".join(f"{g:.1e}" for g in rel))
    assert any(1e-4 <= g <= 1e-1 for g in rel[:-1]), rel                 # a point on the way
    assert -1e-12 <= rel[-1] <= 1e-9, rel                                # the converged one
    assert (cs["pre"]["gap"] >= -1e-12 * cs["pre"]["primal"]).all()
    if form == "weighted":
        assert (cs["w"] == 0).any()
    if form == "penalised":
        assert cs["p"].min() >= 0.5 and cs["p"].max() <= 2.0


def test_gap_tol_of_the_certified_path_is_met_by_the_reference_solver():
    """tests/test_gpu_duality.py runs certified_path on the planted-support recipe of tests/_working_set.py with GAP_TOL and the
    round budget below; the fp64 working-set reference, run with the same iterations per round, must end below a tenth of it."""
    from tests import _working_set as ws
    for loss in ("squared", "logistic"):
        cs = ws.case(loss, False, False, "f32")
        X, info = ws.solve(cs["A"], cs["b"], cs["alphas"], du.PATH_ITERS, loss=loss, L=None, kkt_tol=0.0, max_rounds=du.PATH_ROUNDS)
        assert not info["fell_back"] and info["rounds"] <= du.PATH_ROUNDS
        r = du.certificate(loss, cs["A"], cs["b"], X, cs["alphas"])
        p0 = du.certificate(loss, cs["A"], cs["b"], np.zeros_like(X), cs["alphas"])["primal"]
        print(loss, "rounds", info["rounds"], "gap / P(0)", (r["gap"] / p0).max())
        assert (r["gap"] <= 0.1 * du.GAP_TOL * p0).all(), r["gap"] / p0


@pytest.mark.parametrize("name", list(du.CERTIFIED_CASES))
def test_the_certified_reference_decides_by_a_margin(name):
    """A device-decided run is compared only where fp32 cannot decide otherwise: every test of the stop rule of the fp64 loop
    (tests/_duality.certified) is further than 100 * TOL of the magnitude of the gap's terms from its bound, every scan further than
    the WorkingSet cell's MARGIN from its threshold, every growth step by its GAP.  gap_tol is 1e-3 and no case runs at GAP_TOL:
    tests/_duality.py says why, next to the cases.  The branches: a set beyond max_fraction * n after a round, a round without a
    violator whose set runs again, the warm start (every round but the first of a case, and the fall-back), 20 weights."""
    groups = du.certified_reference(name)
    count = du.CERTIFIED_CASES[name][4]
    assert [len(info["gap"]) for _, info in groups] == ([16, 4] if count == 20 else [16])
    for X, info in groups:
        print(f"{name}: rounds {info['rounds']} sizes {info['sizes']} certificates {info['certificates']} fell back {info['fell_back']} "
              f"certified {int(info['certified'].sum())}; margins: stop {info['stop_margins'].min():.2e} scan {info['scan_margins'].min():.2e} "
              f"growth {info['growth_gaps'].tolist()}")
        assert info["stop_margins"].min() > du.STOP_MARGIN, info["stop_margins"].min()
        assert info["scan_margins"].min() >= du.SCAN_MARGIN and min(info["growth_gaps"].tolist() + [np.inf]) >= du.GROWTH_GAP
        assert np.isfinite(X).all() and info["certified"].all()
        assert info["certificates"] == info["rounds"] + 1 + info["fell_back"]
    info = groups[0][1]
    if name == "beyond_max_fraction":
        assert info["fell_back"] and info["rounds"] == 1 and info["certificates"] == 3 and info["sizes"][0] <= 0.95 * 256
    else:
        assert not info["fell_back"] and info["rounds"] >= 1
    if name == "same_set_again":
        assert info["rounds"] >= 2 and info["sizes"][0] == info["sizes"][1], info["sizes"]
    if name not in ("squared_weighted", "twenty_weights"):
        assert info["rounds"] + info["fell_back"] >= 2                       # a warm start from a non-zero X
