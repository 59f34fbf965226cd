"""GPU: the seven path / CV front ends compute what they did before the four model families got one host driver.
tests/golden/front_end_parent.npz was recorded from the commit before that change with tests/_front_end_golden.py; the calls are
repeated here and compared bitwise (x and info of every path; the held-out scores, best, x and info of every CV).  The device
routes behind them are pinned by tests/test_gpu_lockstep_guard.py."""
import os

import numpy as np
import pytest
import torch

from tests import _data, _front_end_golden as gold

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


def test_front_end_results_are_bitwise_those_of_the_parent_commit(fos):
    want = np.load(os.path.join(_data.GOLDEN, "front_end_parent.npz"))
    got = gold.compute(fos)
    assert sorted(got) == sorted(want.files)
    cases = {k.rsplit("/", 1)[0] for k in got}
    assert len(cases) == 2 * (4 * 2 + 4 * 2 + 2 * 2 + 2) and {k.split("/")[0] for k in got} == {"f32", "bf16"}
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    for case in sorted(cases):
        x = got[case + "/x"]
        assert x.dtype == np.float64 and x.shape[0] == gold.N and np.count_nonzero(x) > 0, case
        assert np.array_equal(got[case + "/info"].reshape(-1, 2), [[gold.ITERS, 0]] * (got[case + "/info"].size // 2)), case
        if "_cv_" in case:
            assert got[case + "/score"].shape == (gold.FOLDS, 3) and 0 <= int(got[case + "/best"]) < 3, case
        else:
            assert x.shape[-1] == len(gold.SCALES), case
