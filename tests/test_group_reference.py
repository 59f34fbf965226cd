"""CPU: the fp64 reference of the group penalty (tests/_group.py) checks itself - the group KKT conditions at convergence, the
G = 1 prox against the oracle's soft threshold, monotone descent of the proximal gradient method - and every recipe the GPU tests
use shows an all-zero row, a non-zero row and a result that differs from the separable penalty's."""
import numpy as np
import pytest

from oracle import fos_oracle as orc
from tests import _group as gp, _multinomial as mn

M, N = 120, 20


def _small_multinomial(alpha2, p=None, enet=False):
    A64, y, L = mn.recipe(M, N, 3, 5)
    a1 = gp.multinomial_weights(A64, y, 3, 1)[0][0]
    return gp.GroupMultinomial(A64, y, 3, a1, alpha2, p=p, enet=enet), L


def _small_multitask(alpha2, p=None, enet=False):
    A64, B, L = gp.multitask_recipe(M, N, 4, 5)
    a1 = gp.multitask_weights(A64, B, 1)[0][0]
    return gp.MultiTask(A64, B, a1, alpha2, p=p, enet=enet), L


FACTORS = np.r_[0.0, np.linspace(0.5, 2.0, N - 1)]          # an unpenalised first coordinate


@pytest.mark.parametrize("enet", [False, True], ids=["l1", "enet"])
@pytest.mark.parametrize("p", [None, FACTORS], ids=["plain", "factors"])
@pytest.mark.parametrize("make", [_small_multinomial, _small_multitask], ids=["multinomial", "multitask"])
def test_the_reference_satisfies_the_group_kkt_conditions(make, p, enet):
    prob, L = make(0.5, p, enet)
    X, _ = gp.iterate(prob, L, 40000, adaptive_restart=True, move_tol=1e-15)
    zero = np.abs(X).sum(axis=1) == 0.0
    assert zero.any() and (~zero).any()
    if p is not None:
        assert not zero[0]                                  # the unpenalised row is in the model
    assert gp.kkt_violation(prob, X) <= 1e-8, gp.kkt_violation(prob, X)


def test_one_column_is_the_oracles_soft_threshold():
    rng = np.random.default_rng(0)
    v = rng.standard_normal(500)
    v[:5] = [0.0, 0.3, -0.3, 0.30000001, 1e-300]
    for step, a1 in ((0.3, 1.0), (1.0, 0.0), (0.01, 2.0)):
        got = gp.group_prox(v[:, None], step, a1, 0.0, np.ones(500))[:, 0]
        want = orc.prox_l1(v, step * a1) if a1 > 0 else v
        assert np.abs(got - want).max() <= 1e-15
    p = rng.uniform(0.0, 2.0, 500)
    got = gp.group_prox(v[:, None], 0.3, 1.0, 0.7, p)[:, 0]
    assert np.abs(got - orc.prox_l1(v, 0.3 * p) / (1.0 + 0.3 * 0.7 * p)).max() <= 1e-15


def test_rows_at_or_below_the_threshold_are_exactly_zero():
    V = np.array([[3.0, 4.0], [0.3, 0.4], [0.0, 0.0], [-6.0, 8.0]])
    X = gp.group_prox(V, 1.0, 5.0, 0.0, np.array([1.0, 1.0, 1.0, 0.0]))
    assert np.array_equal(X[:3], np.zeros((3, 2))) and not np.signbit(X[:3]).any()      # ||v|| = 5 = the threshold: zero
    assert np.array_equal(X[3], V[3])                                                    # factor 0: untouched
    assert np.allclose(gp.group_prox(V, 1.0, 2.5, 0.0, np.ones(4))[0], [1.5, 2.0], rtol=0, atol=1e-15)


@pytest.mark.parametrize("make", [_small_multinomial, _small_multitask], ids=["multinomial", "multitask"])
def test_the_objective_decreases_under_proximal_gradient_steps(make):
    prob, L = make(0.25)
    obj = []
    gp.iterate(prob, L, 200, objectives=obj, adaptive_restart=True, restart_threshold=0.0)      # a restart every iteration
    start = prob.value(np.zeros(N * prob.C))
    d = np.diff(np.r_[start, obj])
    assert (d <= 1e-12 * abs(start)).all() and obj[-1] < start


def test_the_gpu_recipes_cannot_pass_vacuously():
    """multinomial_reference / multitask_reference assert an all-zero row, a non-zero row and the distance from the separable
    reference themselves; here they run for the small shapes of the GPU tests (the large ones assert when the GPU tests ask)."""
    for multinomial, (name, G, count) in [(True, c) for c in gp.MULTINOMIAL_CASES] + [(False, c) for c in gp.MULTITASK_CASES]:
        for kind in ("f32", "bf16"):
            m, n = gp.case_shape(name, kind)
            if m > 2000:
                continue
            for enet, delta in gp.VARIANTS.values():
                if multinomial:
                    A64, y, _ = mn.recipe(m, n, G, gp.SEED, kind)
                    alphas = gp.multinomial_weights(A64, y, G, count, enet=enet)
                    refs = [gp.multinomial_reference(m, n, G, gp.SEED, kind, a1, a2, delta, enet) for a1, a2 in alphas]
                else:
                    A64, B, _ = gp.multitask_recipe(m, n, G, gp.SEED, kind)
                    alphas = gp.multitask_weights(A64, B, count, enet=enet)
                    refs = [gp.multitask_reference(m, n, G, gp.SEED, kind, a1, a2, delta, enet) for a1, a2 in alphas]
                assert any(safe.any() for _, safe in refs), (name, G, kind)      # the exact-zero check has rows to look at
