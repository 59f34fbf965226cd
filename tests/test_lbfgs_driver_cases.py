"""CPU: the inputs of the L-BFGS driver tests (tests/_lbfgs_cases.py) take the routes they are there for, and take them
whatever the order of summation.

For every case the oracle runs twice, the second time with the rows of A and b permuted (every sum over the rows in another
order): (nit, nfev, task) must be equal and every iterate must agree to 1e-8 relative.  A device run differs from the
oracle in nothing but the order of its sums, so a case that passes here can be compared with it count for count.  Runs are
kept short on purpose: 200 iterations on columns scaled over six decades already differ between SciPy and the oracle by one
evaluation."""
import numpy as np
import pytest

from tests import _lbfgs_cases as lc, _menu_lbfgs as ml

_RUNS = {}


def _run(name):
    if name not in _RUNS:
        c = lc.BY_NAME[name]
        A32, A64, b32, x0 = lc.data(c)
        _RUNS[name] = (lc.oracle(c, A64, b32, x0), A64, b32, x0)
    return _RUNS[name]


@pytest.mark.parametrize("name", [c["name"] for c in lc.CASES])
def test_oracle_route_does_not_depend_on_the_summation_order(name):
    c = lc.BY_NAME[name]
    r, A64, b32, x0 = _run(name)
    perm = np.random.default_rng(1).permutation(c["m"])
    p = lc.oracle(c, A64, b32, x0, perm)
    assert (r["nit"], r["nfev"], r["task"]) == (p["nit"], p["nfev"], p["task"]), (r["nit"], r["nfev"], p["nit"], p["nfev"])
    assert r["evals"] == p["evals"]
    for k, (a, b) in enumerate(zip(r["iterates"], p["iterates"])):
        assert np.linalg.norm(a - b) <= 1e-8 * np.linalg.norm(a), (name, k)
    if c["nonfinite"] is None:
        assert np.linalg.norm(r["x"] - p["x"]) <= 1e-8 * max(np.linalg.norm(r["x"]), 1e-300)


def test_cases_cover_every_exit_and_branch():
    runs = {c["name"]: _run(c["name"])[0] for c in lc.CASES}
    get = lambda name: (runs[name]["nit"], runs[name]["nfev"], runs[name]["task"])      # noqa: E731
    # every task code; 0 both before and after the first iteration
    assert get("div64-zero") == (0, 1, 0)
    assert runs["div64-tol"]["task"] == 0 and runs["div64-tol"]["nit"] > 0
    assert runs["div64-conv"]["task"] == 1 and runs["div64-limit"]["task"] == 2
    assert {r["task"] for r in runs.values()} == {0, 1, 2, 3}
    # task 3 from finite data: 20 evaluations of one line search, no iterate, x back at the start
    for name in ("div64-b1e20", "ragged515-b1e20", "n2048-b1e20"):
        assert get(name) == (0, 21, 3) and not runs[name]["x"].any(), name
    # max_iter 0 runs the one iteration max_iter 1 runs (SciPy: nit = 1, nfev = 3, iteration limit)
    assert get("div64-iter0") == get("div64-iter1") == (1, 3, 2)
    assert np.array_equal(runs["div64-iter0"]["x"], runs["div64-iter1"]["x"])
    # a line search of >= 4 and one of >= 10 evaluations in every length class
    for cls, member in lc.LENGTH_CLASSES.items():
        longest = [max(runs[c["name"]]["evals"], default=0) for c in lc.CASES if member(c) and c["nonfinite"] is None]
        assert any(4 <= e < 10 for e in longest) and any(e >= 10 for e in longest), (cls, longest)
    # more than three evaluations means the search left the first two trial points
    assert any(e > 2 for r in runs.values() for e in r["evals"])
    # the ring of 10 pairs wraps, in the two-loop forms and in the whole-chip form
    for name in ("div64-ring", "ragged33-ring", "n2048-ring"):
        assert runs[name]["nit"] > ml.DRIVER_M + 4, name
    # non-finite data ends within MAXLS = 20 evaluations of the first line search, x at the start point
    for c in lc.CASES:
        if c["nonfinite"]:
            assert get(c["name"]) == (0, 21, 3), c["name"]
    # the length classes sit on both sides of the switch to the whole-chip direction
    assert {ml.driver_direction(c["n"]) for c in lc.CASES} == {0, 1, "chip"}
    assert ml.driver_direction(2047) == 0 and ml.driver_direction(2048) == ml.driver_direction(2049) == "chip"
    assert runs["div64-start"]["nit"] > 3


def test_group_columns_take_different_exits():
    """The lockstep groups: per column the oracle's exit, and stable under a row permutation."""
    for name, gdef in lc.GROUPS.items():
        A32, A64, B, roles = lc.group(**gdef)
        perm = np.random.default_rng(2).permutation(gdef["m"])
        tasks = []
        for j, role in enumerate(roles):
            c = dict(a2=lc.GROUP_A2, max_iter=lc.GROUP_MAX_ITER, tol=lc.GROUP_TOL, n=gdef["n"])
            r, p = lc.oracle(c, A64, B[:, j]), lc.oracle(c, A64, B[:, j], None, perm)
            assert (r["nit"], r["nfev"], r["task"]) == (p["nit"], p["nfev"], p["task"]), (name, j, role)
            for a, b in zip(r["iterates"], p["iterates"]):
                assert np.linalg.norm(a - b) <= 1e-8 * np.linalg.norm(a), (name, j)
            tasks.append(r["task"])
            if role == "zero":
                assert (r["nit"], r["nfev"], r["task"]) == (0, 1, 0), (name, j)
            if role == "1e20":
                assert (r["nit"], r["nfev"], r["task"]) == (0, 21, 3), (name, j)
            if role == "1e8":
                assert max(r["evals"]) >= 10, (name, j, r["evals"])
        assert len(set(tasks)) >= (3 if gdef["nv"] >= 16 else 2), (name, tasks)


def test_nan_max_of_the_column_sharded_statistics():
    """max|g| over the ranks keeps a NaN wherever it sits (Python's max keeps or drops it by position), like the statistics
    kernel; the CPU stand-in of tests/test_distributed_cpu.py behaves the same way."""
    import torch
    from fastoptsolver_amd.lbfgs import _nan_max
    from tests.test_distributed_cpu import OracleLbfgsOps
    nan = float("nan")
    assert _nan_max([1.0, 3.0, 2.0]) == 3.0
    for vals in ([nan, 1.0, 2.0], [1.0, nan, 2.0], [1.0, 2.0, nan], [nan]):
        assert _nan_max(vals) != _nan_max(vals)
    ops = OracleLbfgsOps.__new__(OracleLbfgsOps)
    ops.n, ops.rr = 3, torch.zeros(1, dtype=torch.float64)
    for pos in range(3):
        g = torch.tensor([1.0, -5.0, 2.0], dtype=torch.float64)
        assert ops.stats(None, g, None)[3] == 5.0
        g[pos] = nan
        got = ops.stats(None, g, None)[3]
        assert got != got, pos
