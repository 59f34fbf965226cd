"""CPU: the reference, bounds, decision and inputs of tests/_armijo.py, which tests/test_gpu_armijo.py holds the Armijo
kernels to.

  - the reference's prox is the oracle's prox_l1 / prox_elastic_net bit for bit on fp64 inputs;
  - its sums agree with exact rational arithmetic to less than 1/16 of the bound the kernels get, and its own error estimate
    stays below that as well;
  - (1-C) gd + 0.5 q' + 0.5 a2s dd is g(x_tmp) - g(y) - C grad.(x_tmp - y) of the oracle's smooth part (q' with the
    unrounded d): the cancellation-free form tests the reference's inequality;
  - decide() is iterative_solvers._armijo_accepts row by row, on rows built to make each clause the first true one and on
    a batch that accepts nothing;
  - the exact inputs have the promised counts, and the case table says what it claims about grids and loops;
  - the noise-ball case of the device decision is feasible on every shape it runs on."""
import fractions
import math

import numpy as np
import pytest

from oracle import fos_oracle as orc
from tests import _armijo as ar

LD = ar.LD


def _random_state(n, rng, beta):
    x_cur = rng.standard_normal(n) * (rng.random(n) < 0.7)
    x_prev = x_cur + 0.1 * rng.standard_normal(n) * (rng.random(n) < 0.7) if beta else x_cur.copy()
    return x_cur, x_prev


_PRMS = [dict(prox="l1", alpha1=0.3, alpha2=0.0), dict(prox="l1", alpha1=0.3, alpha2=0.25),
         dict(prox="enet", alpha1=0.3, alpha2=0.25), dict(prox="l1", alpha1=0.0, alpha2=0.25)]


@pytest.mark.parametrize("prm", _PRMS, ids=lambda p: f"{p['prox']}-{p['alpha1']}-{p['alpha2']}")
def test_prox_is_the_oracles_bit_for_bit(prm):
    rng = np.random.default_rng(ar.seed("prox"))
    v = np.concatenate([rng.standard_normal(500), [0.0, -0.0, 0.15, -0.15, 0.15 + 2.0 ** -50]])
    for t in (0.5, 0.37, 1e-3):
        got = ar.prox(v, t, prm)
        assert got.dtype == np.float64
        if prm["alpha1"] > 0:
            want = orc.prox_elastic_net(v, t, prm["alpha1"], prm["alpha2"]) if prm["prox"] == "enet" else orc.prox_l1(v, t * prm["alpha1"])
            assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
        else:
            assert got is v
    assert ar.prox(v.astype(LD), 0.5, prm).dtype == LD


@pytest.mark.parametrize("beta", [0.0, 0.6])
@pytest.mark.parametrize("prm", _PRMS, ids=lambda p: f"{p['prox']}-{p['alpha1']}-{p['alpha2']}")
def test_reference_against_rational_arithmetic(prm, beta):
    n, nv = 41, 6
    rng = np.random.default_rng(ar.seed("exact sums", prm["prox"], prm["alpha1"], prm["alpha2"], beta))
    x_cur, x_prev = _random_state(n, rng, beta)
    g = rng.standard_normal(n)
    t = float(np.linalg.norm(x_cur) / np.linalg.norm(g))
    ref = ar.reference(None, x_cur, x_prev, beta, g, prm, t, 0.7, nv)
    bnd = ar.bounds(ref, x_cur, x_prev, beta, prm)
    own = ar.reference_error(ref, x_cur, x_prev, beta, prm)
    exact = ar.exact_sums(x_cur, x_prev, beta, g, prm, t, 0.7, nv)
    assert ref["t"] == ar.steps(t, 0.7, nv) and ref["t"][3] == ((t * 0.7) * 0.7) * 0.7
    for j in range(nv):
        assert ref["rows"][j]["nnz"] == exact[j]["nnz"]
        for k in ar.SUMS:
            hi = float(ref["rows"][j][k])
            lo = float(ref["rows"][j][k] - LD(hi))
            err = abs(float(fractions.Fraction(hi) + fractions.Fraction(lo) - exact[j][k]))
            assert bnd[j][k] > 0.0
            assert err <= own[j][k] <= bnd[j][k] / 16.0, (j, k, err, own[j][k], bnd[j][k])


def test_fsum_is_exactly_rounded():
    terms = np.array([1.0, 2.0 ** -60, -1.0, 2.0 ** -62, 3.0], dtype=LD) * LD(1 + 2.0 ** -60)
    want = sum(fractions.Fraction(float(t.astype(np.float64))) + fractions.Fraction(float(t - t.astype(np.float64).astype(LD))) for t in terms)
    got = ar.fsum(terms)
    assert abs(fractions.Fraction(float(got)) + fractions.Fraction(float(got - LD(float(got)))) - want) <= want * fractions.Fraction(1, 2 ** 63)


@pytest.mark.parametrize("beta", [0.0, 0.6])
@pytest.mark.parametrize("prm", _PRMS, ids=lambda p: f"{p['prox']}-{p['alpha1']}-{p['alpha2']}")
def test_excess_is_the_references_inequality(prm, beta):
    m, n, nv, C = 23, 31, 8, ar.ARMIJO_C
    rng = np.random.default_rng(ar.seed("excess", prm["prox"], prm["alpha1"], prm["alpha2"], beta))
    A = rng.standard_normal((m, n))
    b = rng.standard_normal(m)
    x_cur, x_prev = _random_state(n, rng, beta)
    y = x_cur + beta * (x_cur - x_prev)
    a2s = ar.smooth_a2(prm)
    grad, _ = orc.gram_gradient(A, y, b, a2s)
    g = A.T @ (A @ y - b)                                   # what the pass leaves: the consumers add alpha2 y
    assert np.allclose(g + a2s * y, grad, rtol=1e-13, atol=1e-13)
    t = 4.0 / float(np.linalg.norm(A, 2)) ** 2
    ref = ar.reference(A, x_cur, x_prev, beta, g, prm, t, 0.5, nv)
    A_ld, b_ld = A.astype(LD), b.astype(LD)

    def smooth(z):                                           # orc.smooth_value in longdouble
        r = A_ld @ z - b_ld
        return LD(0.5) * ar.fsum(r * r) + LD(0.5) * LD(a2s) * ar.fsum(z * z)
    for j, tj in enumerate(ref["t"]):
        d, row = ref["d"][j], ref["rows"][j]
        x_tmp = ref["y"] + d
        # the candidate is the oracle's prox step
        want = orc.prox_elastic_net(y - tj * grad, tj, prm["alpha1"], prm["alpha2"]) if prm["prox"] == "enet" else \
            orc.prox_l1(y - tj * grad, tj * prm["alpha1"]) if prm["alpha1"] > 0 else y - tj * grad
        assert np.allclose(x_tmp.astype(np.float64), want, rtol=1e-12, atol=1e-13)
        assert float(smooth(ref["y"])) == pytest.approx(orc.smooth_value(A, b, y, a2s), rel=1e-12)
        Ad = A_ld @ d
        lhs = LD(1 - LD(C)) * row["gd"] + LD(0.5) * ar.fsum(Ad * Ad) + LD(0.5) * LD(a2s) * row["dd"]
        rhs = smooth(x_tmp) - smooth(ref["y"]) - LD(C) * ar.fsum(ref["gf"] * d)
        scale = smooth(x_tmp) + smooth(ref["y"])
        assert abs(float(lhs - rhs)) <= 64 * (n + m) * ar.EPSLD * float(scale), (j, float(lhs), float(rhs))
        assert row["q"] == pytest.approx(float(ar.fsum(Ad * Ad)), rel=1e-6)          # q on f32(d)


# ---- decide --------------------------------------------------------------------------------------------------------------
def _accepts():
    from fastoptsolver_amd import iterative_solvers as its
    assert its.C == ar.ARMIJO_C and its._BATCH == ar.NV
    return its._armijo_accepts


def _row(gd, dd, nnz, gnorm2, q, y2=2.0, rr_y=3.0):
    return dict(gd=gd, dd=dd, nnz=nnz, gnorm2=gnorm2, y2=y2, q=q, rr_y=rr_y)


_REJECT = _row(gd=-1.0, dd=1.0, nnz=5.0, gnorm2=1.0, q=4.0)                  # excess = 1.01 > noise, outside the ball
_ROWS = {
    "nnz": _row(gd=-1.0, dd=0.0, nnz=0.0, gnorm2=1.0, q=0.0),
    "nnz_alone": _row(gd=1.0, dd=1.0, nnz=0.0, gnorm2=1.0, q=4.0),            # (a row no kernel gives: the clause on its own)
    "excess": _row(gd=-1.0, dd=1.0, nnz=5.0, gnorm2=1.0, q=1.0),
    "excess_by_noise": _row(gd=-1.0, dd=1e-2, nnz=5.0, gnorm2=1e2, q=1.98 + 1e-7 - 0.25e-2),   # 0 < excess <= grad_eps sqrt(gn2 dd)
    "ball": _row(gd=-1e-10, dd=1e-20, nnz=1.0, gnorm2=1.0, q=1.0, rr_y=0.0, y2=0.0),   # excess = 0.5 > noise = 1e-16
}


@pytest.mark.parametrize("name", list(_ROWS))
@pytest.mark.parametrize("a2s", [0.0, 0.25])
def test_decide_is_armijo_accepts_row_by_row(name, a2s):
    accepts = _accepts()
    t, eta, C, grad_eps = 0.5, 0.7, ar.ARMIJO_C, ar.GRAD_EPS["f32"]
    clause = name.split("_")[0]
    for lead in (0, 1, 7, 15):
        rows = [_REJECT] * lead + [_ROWS[name]] + [_REJECT] * (15 - lead)
        j, tj, got = ar.decide(rows, t, eta, a2s, C, grad_eps)
        assert (j, got) == (lead, clause) and tj == ar.steps(t, eta, 16)[lead]
        tk = t
        for i, tr in enumerate(rows):                        # the host loop (iterative_solvers.search_on_host)
            if accepts(tr, tk, a2s, grad_eps):
                break
            tk *= eta
        assert (i, tk) == (j, tj)
    # each clause is the only true one of its row
    tr = _ROWS[name]
    excess = (1.0 - C) * tr["gd"] + 0.5 * tr["q"] + 0.5 * a2s * tr["dd"]
    noise = max(ar.EPS64 * (0.5 * tr["rr_y"] + 0.5 * a2s * tr["y2"]), grad_eps * math.sqrt(tr["gnorm2"] * tr["dd"]))
    ball = tr["dd"] <= (grad_eps * t) ** 2 * tr["gnorm2"]
    truth = dict(nnz=tr["nnz"] == 0, excess=excess <= noise, ball=ball)
    if name != "nnz":                                        # (a real nnz = 0 row has dlt = 0: every clause holds)
        assert [k for k, v in truth.items() if v] == [clause], truth


def test_decide_stalls_on_a_batch_that_accepts_nothing():
    accepts = _accepts()
    t, eta = 3.0, 0.7
    rows = [_REJECT] * 16
    j, t_end, clause = ar.decide(rows, t, eta, 0.0, ar.ARMIJO_C, ar.GRAD_EPS["f64"])
    want = t
    for tr in rows:
        assert not accepts(tr, want, 0.0, ar.GRAD_EPS["f64"])
        want *= eta
    assert (j, clause) == (None, "stall") and t_end == want


# ---- the exact inputs and the case table ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prox", list(ar.EXACT_PROX))
@pytest.mark.parametrize("n", [68, 260])
def test_exact_inputs_have_the_promised_counts(n, prox):
    y, g, prm, classes = ar.exact_inputs(n, prox)
    K, a1, a2s = ar.EXACT_K, prm["alpha1"], ar.smooth_a2(prm)
    assert sorted(classes) == sorted(ar.EXACT_CLASSES) and all(len(v) == K for v in classes.values())
    assert len(np.unique(np.concatenate(list(classes.values())))) == K * len(classes)
    gf = g + a2s * y
    ts = ar.steps(ar.EXACT_T, ar.EXACT_ETA, ar.NV)
    counts = ar.exact_counts(y, g, prm)
    exact = ar.exact_sums(y, y, 0.0, g, prm, ar.EXACT_T, ar.EXACT_ETA, ar.NV)
    ref = ar.reference(None, y, y, 0.0, g, prm, ar.EXACT_T, ar.EXACT_ETA, ar.NV)
    assert (g[classes["g_zero"]] == 0).all() and (y[classes["g_zero"]] != 0).all()
    for j, tj in enumerate(ts):
        assert counts[j] == exact[j]["nnz"] == ref["rows"][j]["nnz"], (j, counts[j], exact[j]["nnz"])
        v, thr = y - tj * gf, tj * a1
        # every comparison is exact: the fp64 values are the rational ones
        for i in range(n):
            F = fractions.Fraction
            assert F(float(v[i])) == F(float(y[i])) - F(tj) * F(float(gf[i]))
        moved = (ref["d"][j] != 0)
        for name in ("tie", "above", "below", "zero_in"):
            assert (y[classes[name]] == 0).all()
        assert (np.abs(v[classes["tie"]]) == thr).all() and not moved[classes["tie"]].any()
        assert (np.abs(v[classes["above"]]) == thr + tj * ar.EXACT_H).all() and moved[classes["above"]].all()
        assert (np.abs(v[classes["below"]]) == thr - tj * ar.EXACT_H).all() and not moved[classes["below"]].any()
        assert (np.abs(v[classes["zero_in"]]) <= thr).all() and not moved[classes["zero_in"]].any()
        assert (y[classes["live_in"]] != 0).all() and moved[classes["live_in"]].all()
        if j <= 7:
            assert (np.abs(v[classes["live_in"]]) <= thr).all()
        assert ((np.abs(v[classes["tie_at"]]) == thr).all()) == (j == ar.EXACT_TIE_AT) and moved[classes["tie_at"]].all()
        assert moved[classes["g_zero"]].all()
        assert (np.abs(v[classes["back"]]) > thr).all() and moved[classes["back"]].all() == (prox == "enet")
        if prox != "enet":
            assert not moved[classes["back"]].any()
        planted = np.concatenate(list(classes.values()))
        rest = np.setdiff1d(np.arange(n), planted)
        assert counts[j] == int(moved[rest].sum()) + K * (4 if prox != "enet" else 5)          # above, live_in, tie_at, g_zero (, back)
        # the entries at 2^-20 of the largest entry of d (the bf16 three-term split has to keep them)
        d = np.abs(ref["d"][j].astype(np.float64))
        assert d[classes["above"]].max() <= 2.0 ** -20 * d.max()
    both = [(int((np.abs(y - tj * gf) <= tj * a1).sum()), int((np.abs(y - tj * gf) > tj * a1).sum())) for tj in ts]
    assert all(lo >= 3 * K and hi >= 3 * K for lo, hi in both)


def test_case_table_reaches_the_loops_it_names():
    S = ar.SHAPES
    assert S["pad"]["n_pad"] - S["pad"]["n"] == 60 and S["pad"]["m"] < 64
    assert ar.batch_grid(S["one_wg"]["n_pad"]) == 1 and S["one_wg"]["n_pad"] == S["one_wg"]["n"]
    assert ar.batch_grid(S["two_wg"]["n_pad"]) == 2 and S["two_wg"]["n"] - 256 == 4
    assert S["bf_pad"]["n_pad"] == 128 and ar.batch_grid(S["bf_two"]["n_pad"]) == 2
    assert ar.trial_grid(S["wide"]["n"]) == 66 > 64                              # the fold's second lane trip
    assert S["wide"]["n_pad"] > 64 * 256 and ar.batch_grid(S["wide"]["n_pad"]) == 64   # the candidate kernel's second column trip
    assert S["blocks"]["n"] > 256 * 256 and ar.trial_grid(S["blocks"]["n"]) == 256       # the stride loop's second trip
    for c in S.values():
        tile = 128 if c["dtype"] == "bf16" else 64
        if c["batch"]:
            assert c["n_pad"] == -(-c["n"] // tile) * tile and c["n"] % (8 if c["dtype"] == "bf16" else 4) == 0
        assert c["batch"] == (c["route"]["path"] == 0 and not (c["route"].get("tall") and c["n"] <= 64) and not c["route"].get("resident"))
    cells = ar.cells()
    assert len(set(cells)) == len(cells) == 4 * 4 * 2 * 2 + 6 and {c[0] for c in cells} == set(S)
    for s in ar.CELL_SHAPES:
        assert {c[1:] for c in cells if c[0] == s} == {(p, st, src) for p in ar.PROX for st in ar.STATES for src in ar.SOURCES}


@pytest.mark.parametrize("shape,prox", sorted({(s, p) for s, p, _, _ in ar.cells() if ar.PROX[p][1]}))
def test_alpha1_separates_the_coordinates_in_the_rehearsal(shape, prox):
    A64, b, x0, L = ar.problem(shape)
    prm = ar.params(shape, prox)
    states = ar.fista_states(A64, b, x0, prm, ar.step_for(shape, prm), 3)
    assert states[3][2] > 0.0 and not np.array_equal(states[3][0], states[3][1])
    for x_cur, x_prev, beta in [states[0 if st == "fresh" else 3] for st in ar.states_of(shape, prox)]:
        y = x_cur + beta * (x_cur - x_prev)
        g = A64.T @ (A64 @ y - b.astype(np.float64))
        t = float(np.linalg.norm(y) / np.linalg.norm(g))
        for eta in ar.ETAS:
            ref = ar.reference(None, x_cur, x_prev, beta, g, prm, t, eta, ar.NV)
            near = ar.near_threshold(ref, prm)
            assert sum(r[0] for r in near) >= 1 and sum(r[1] for r in near) >= 1, (shape, prox, near)
            assert min(r[2] for r in near) > ar.REHEARSED * ar.NEAR, (shape, prox, near)


@pytest.mark.parametrize("source", ar.SOURCES)
@pytest.mark.parametrize("shape", ar.DECISION_SHAPES)
def test_ball_case_is_feasible(shape, source):
    """The construction of the noise-ball case on the fp64 gradient: one coordinate moves, `ball` is the only true clause at
    j = 0, with room for the device's gradient to differ from this one."""
    A64, b, _, L = ar.problem(shape)
    n = A64.shape[1]
    x = np.zeros(n)
    g = A64.T @ (A64 @ x - b.astype(np.float64))
    g = g.astype(np.float32).astype(np.float64) if source == "f32" else g
    a1, tau = ar.ball_alpha1(g, source), ar.ball_tau(L, source)
    prm = dict(prox="l1", alpha1=a1, alpha2=0.0)
    ref = ar.reference(A64, x, x, 0.0, g, prm, tau, 0.5, ar.NV)
    rows = [dict({k: float(v) for k, v in r.items()}, rr_y=float(b.astype(np.float64) @ b.astype(np.float64))) for r in ref["rows"]]
    assert rows[0]["nnz"] == 1
    j, tj, clause = ar.decide(rows, tau, 0.5, 0.0, ar.ARMIJO_C, ar.GRAD_EPS[source])
    assert (j, tj, clause) == (0, tau, "ball")
    tr = rows[0]
    excess = (1.0 - ar.ARMIJO_C) * tr["gd"] + 0.5 * tr["q"]
    noise = max(ar.EPS64 * 0.5 * tr["rr_y"], ar.GRAD_EPS[source] * math.sqrt(tr["gnorm2"] * tr["dd"]))
    assert excess > 1e3 * noise                                                   # far from the excess clause
    assert tr["dd"] <= 0.5 * (ar.GRAD_EPS[source] * tau) ** 2 * tr["gnorm2"]          # and well inside the ball
    s = np.sort(np.abs(g))
    assert s[-2] < a1 * (1.0 - 1e-4)                                              # the runner-up stays below the threshold
