"""GPU: the lockstep computes and refuses what it did before its dispatch became one route decision and its separable update one
launch.  tests/golden/lockstep_parent.npz and lockstep_refusals.json were recorded from the commit before that change with
tests/_lockstep_golden.py; the calls are repeated here and compared bitwise (x and the status of every handle) and byte for byte
(return code and fos_last_error of every entry point x problem kind x handles x nv; a refused call leaves x and the status of
every handle as they were - tests/_lockstep_golden.refusals asserts that for each)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _data, _lockstep_golden as gold, _menu_multi as mm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


def test_lockstep_results_are_bitwise_those_of_the_parent_commit(fos):
    want = np.load(os.path.join(_data.GOLDEN, "lockstep_parent.npz"))
    got = gold.compute(fos, torch)
    assert sorted(got) == sorted(want.files)
    assert len({k.split("/")[1] for k in got}) == 19 and {k.split("/")[0] for k in got} == {"f32", "bf16"}
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), \
            (k, float(np.abs(got[k] - want[k]).max()))
        if k.endswith("/x"):
            assert got[k].shape[0] == gold.N and 3 <= got[k].shape[1] <= 6 and np.count_nonzero(got[k]) > 0, k
    # every case ran the matrix-core lockstep: the plain squared-loss calls (the only ones the dispatch may hand to the VALU
    # multi-vector pass or refuse for their number of handles) with a column count that takes the pair for both storages
    for kind in ("f32", "bf16"):
        for case, rhs in (("sq_l1", None), ("sq_enet", None), ("sq_mixed", None), ("rhs", "B")):
            nv = got[f"{kind}/{case}/x"].shape[1]
            assert nv >= 5 and mm.lockstep_form(kind, gold.N, nv, rhs) == "mfma", (kind, case, nv)


def test_lockstep_refusals_are_those_of_the_parent_commit(fos):
    with open(os.path.join(_data.GOLDEN, "lockstep_refusals.json")) as fh:
        want = json.load(fh)
    got = gold.refusals(fos, torch)                    # (asserts that every refused call left its handles untouched)
    assert sorted(got) == sorted(want) and len(want) == 702
    for k in sorted(want):
        assert got[k] == want[k], (k, got[k], want[k])
    assert all(msg == "" for rc, msg in want.values() if rc == 0) and all(msg for rc, msg in want.values() if rc != 0)
    served = sum(rc == 0 for rc, _ in want.values())
    assert 100 < served < len(want) - 400              # the table holds both: what is served and, mostly, what is refused
