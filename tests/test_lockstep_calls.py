"""CPU: the seven path / CV front ends make the calls into the lockstep that they made before the four model families got one
host driver.  tests/golden/lockstep_calls.json was recorded from the commit before that change with tests/_lockstep_calls.py
(stand-ins for the handles, the three launches, the fold ids and the timer: no device); every scenario is repeated here and
compared for equality - the ordered launches with the full parameter set, held list and right-hand-side block of every handle,
the returned arrays and info, the type and text of what is raised, and the number of grad_call_times entries."""
import json
import os

import pytest

from tests import _data, _lockstep_calls as calls


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(_data.GOLDEN, "lockstep_calls.json")) as fh:
        return json.load(fh)


def test_the_record_holds_every_scenario(want):
    assert sorted(want) == sorted(calls.SCENARIOS)
    for fn in ("fista_path", "fista_cv", "logistic_path", "logistic_cv", "multinomial_path", "multinomial_cv", "multitask_path"):
        mine = {k: v for k, v in want.items() if k.startswith(fn + "/")}
        assert any("result" in v and v["log"] for v in mine.values()), fn          # served, with launches logged,
        assert any(v.get("raises") == "FosError" for v in mine.values()), fn       # refused,
        assert mine[fn + "/delta_3"]["log"] and "raises" in mine[fn + "/delta_2"], fn    # and both sides of the delta check
    # 3 folds x 7 weights: two groups recounted to the 7 iterations the handles report, and the refit's 11
    assert want["logistic_cv/3x7"]["grad_num_calls"] == 2 * calls.K_DONE + calls.ITERS


@pytest.mark.parametrize("name", sorted(calls.SCENARIOS))
def test_calls_are_those_of_the_parent_commit(monkeypatch, want, name):
    got = json.loads(json.dumps(calls.run_one(monkeypatch, name)))      # as JSON holds it: tuples are lists
    assert sorted(got) == sorted(want[name]), (got.get("raises"), got.get("text"))
    for key in sorted(got):
        assert got[key] == want[name][key], (name, key)
