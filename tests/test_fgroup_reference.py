"""CPU: the fp64 reference of the feature-group lockstep (tests/_fgroup.py) is checked on its own - the oracle has no group
penalty - by the group KKT conditions at convergence, by its degenerate layouts, and by the preconditions that make the GPU
comparisons mean something (zero and non-zero groups at every weight, no group near its threshold), decided on the reference
alone."""
import numpy as np
import pytest

from oracle import fos_oracle as orc
from tests import _coord as cd, _data, _fgroup as fg, _logit as lg, _weighted as wt

M, N = 60, 24
SIZES = (1, 3, 2, 5, 1, 4, 2, 6)                     # mixed sizes, 24 columns
START = np.concatenate(([0], np.cumsum(SIZES))).astype(np.int32)


def _small(loss, weighted, seed=5):
    A, b_sq, xt = _data.synth(M, N, seed, density=0.2)
    b = lg.labels(A, xt, seed) if loss == "logistic" else b_sq
    w = wt.as_stored(wt.weights("spread", M, seed)) if weighted else None
    ones = np.ones(M) if w is None else w
    L = wt.lipschitz(A, ones, seed, loss)
    g0 = A.T @ (ones * ((b - 0.5) if loss == "logistic" else b))
    return A, b, w, L, g0


@pytest.mark.parametrize("enet", [False, True], ids=["PROX_L1", "PROX_ENET"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("mu", [0.0, 0.3, 1.0])
def test_the_reference_satisfies_the_group_kkt_conditions(mu, loss, weighted, enet):
    A, b, w, L, g0 = _small(loss, weighted)
    gw = np.sqrt(SIZES) * np.array([1.0, 0.5, 2.0, 1.0, 0.0, 1.5, 1.0, 0.7])          # one unpenalised group
    amax = fg.alpha_max(g0, START, gw, mu)
    for frac, a2 in ((0.4, 0.0), (0.15, 0.3)):
        a1 = frac * amax
        r = fg.run(A, b, a1, a2, L, 20000, start=START, gw=gw, mu=mu, loss=loss, w=w, enet=enet)
        viol = fg.kkt_violation(r["prob"], r["x"], a1, a2)
        zero, full = fg.zero_groups(r["x"], START)
        print(f"mu={mu} {loss} weighted={weighted} enet={enet} alpha1={a1:.4g}: violation {viol:.2e} of alpha1, "
              f"{int(zero.sum())} zero groups of {len(zero)}")
        assert viol <= 1e-8, viol
        assert (~zero).any() and (mu == 1.0 or zero.any())                            # the conditions were exercised on both sides
        if mu == 0.0:
            assert (zero | full).all()                                                # whole groups or nothing


def test_the_violation_measure_sees_a_wrong_point():
    A, b, w, L, g0 = _small("squared", False)
    gw = np.sqrt(SIZES)
    a1 = 0.3 * fg.alpha_max(g0, START, gw, 0.0)
    r = fg.run(A, b, a1, 0.0, L, 20000, start=START, gw=gw, mu=0.0)
    lasso = fg.run(A, b, a1, 0.0, L, 20000, start=START, gw=gw, mu=1.0)               # the solution of another penalty
    assert fg.kkt_violation(r["prob"], r["x"], a1, 0.0) <= 1e-8 < 1e-3 < fg.kkt_violation(r["prob"], lasso["x"], a1, 0.0)


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_mu_one_is_the_oracles_lasso_exactly_and_unit_groups_are_the_lasso(loss):
    A, b, _, L, g0 = _small(loss, False)
    a1, a2 = 0.2 * float(np.max(np.abs(g0))), 0.4
    base = (orc.FistaProblem if loss == "squared" else lg.LogisticProblem)(A, b, a1, a2)
    st = base.init_state(L)
    for _ in range(50):
        base.step(st)
    r = fg.run(A, b, a1, a2, L, 50, start=START, gw=None, mu=1.0, loss=loss)
    assert np.array_equal(r["x"], st.x) and np.count_nonzero(st.x) > 0
    ones = np.arange(N + 1, dtype=np.int32)
    r1 = fg.run(A, b, a1, a2, L, 50, start=ones, gw=np.ones(N), mu=0.0, loss=loss)
    assert np.max(np.abs(r1["x"] - st.x)) <= 1e-12 and np.array_equal(r1["x"] == 0, st.x == 0)


def test_one_group_above_its_alpha_max_is_zero():
    A, b, _, L, g0 = _small("squared", False)
    one = np.array([0, N], dtype=np.int32)
    amax = fg.alpha_max(g0, one, fg.weights_of(one, None), 0.0)
    assert abs(amax - np.linalg.norm(g0) / np.sqrt(np.float32(N))) <= 1e-9 * amax
    assert not fg.run(A, b, 1.001 * amax, 0.0, L, 200, start=one)["x"].any()
    assert fg.run(A, b, 0.9 * amax, 0.0, L, 200, start=one)["x"].all()


def test_the_prox_keeps_its_three_properties():
    start = np.array([0, 2, 4, 6], dtype=np.int32)
    w = np.array([1.0, 0.0, 1.0])
    v = np.array([0.3, -0.4, 0.0, 0.0, 3.0, np.nan])
    with np.errstate(invalid="ignore"):
        x, nrm, thr = fg.group_prox(v, 1.0, 0.5, 0.0, start, w)
    assert x[0] == 0.0 and x[1] == 0.0 and nrm[0] == thr[0] == 0.5                    # at the threshold: exactly zero
    assert x[2] == 0.0 and x[3] == 0.0 and thr[1] == 0.0                              # thr = 0 and a zero norm: 0, not NaN
    assert np.isnan(x[4]) and np.isnan(x[5])                                          # a NaN norm stays a NaN


def test_layouts_partition_and_bite():
    for n in (68, 72, 200, 256):
        for name in ("ones", "small", "single", "weights") + (("cross64",) if n >= 72 else ()) + (("span150",) if n >= 200 else ()):
            start, w = fg.layout(name, n, 3)
            assert start[0] == 0 and start[-1] == n and (np.diff(start) > 0).all() and (w is None or len(w) == len(start) - 1)
    start, _ = fg.layout("cross64", 200)
    k = int(np.searchsorted(start, 60))
    assert (start[k], start[k + 1]) == (60, 70)
    start, _ = fg.layout("span150", 200)
    k = int(np.argmax(np.diff(start)))
    assert (start[k], start[k + 1]) == (44, 194)                                      # workgroups 0..3, the last one partial
    assert any(int(s) % 4 for s in fg.layout("small", 200)[0])                        # boundaries inside quads
    start, w = fg.layout("weights", 200)
    assert (w == 0).sum() >= 2 and (w > 0).sum() >= 2 and not np.allclose(w[w > 0], np.sqrt(np.diff(start))[w > 0])


@pytest.mark.parametrize("mu", fg.MUS)
@pytest.mark.parametrize("name,lay", [p for p in fg.BITES if p[0] != "panels"])
def test_the_gpu_cases_are_meaningful_on_the_reference_alone(name, lay, mu):
    """case() raises where no seed passes `meaningful`; the structure exception (groups within CLOSE of their threshold) is
    empty for the chosen seeds, which is well inside its cap of 2 % of the groups."""
    for kind in fg.KINDS:
        key = fg.key(kind, fg.CPU_CUS, name, lay, mu)
        c = fg.case(*key)
        for a1, a2 in c["alphas"]:
            r = fg.reference(*key, a1, a2)
            assert np.linalg.norm(r["x"]) > 0 and r["closest"] >= fg.CLOSE
            assert 0 < a1 < c["amax"]


@pytest.mark.parametrize("mu", fg.MUS)
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_the_path_and_cv_cases_are_meaningful_too(loss, weighted, mu):
    for kind in fg.KINDS:
        key = fg.key(kind, fg.CPU_CUS, "edges", "span150", mu, loss, weighted)
        c = fg.case(*key)
        idx, keep = fg.controlled(*key)
        assert idx is not None and len(keep) >= 1 and len(c["alphas"]) == 4
