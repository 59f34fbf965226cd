"""GPU: the six entry points of the working set and the certificate (fos_gradient_batch, fos_kkt_scan, fos_duality_gap and their
multinomial namesakes) compute and refuse what they did before they got one panel walk, one certificate tail and one scan /
column-pass kernel pair.  tests/golden/ws_parent.npz and ws_refusals.json were recorded from the commit before that change
(913a733) with tests/_ws_golden.py on a 256-CU card - the two-panel shape and the partial counts are that card's; the calls are
repeated here and compared bitwise (G, the loss sums, excess, the violators and out64 of every family x width x X x storage type
at a one-panel and a two-panel shape; the scan alone over three trips of its workgroup) and byte for byte (return code and
fos_last_error of every guard a single card can meet)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _data, _ws_golden as gold

pytestmark = pytest.mark.gpu

FIELDS = ("G", "excess", "loss", "out64", "same_G", "viol")


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


@pytest.fixture(scope="module")
def want():
    return np.load(os.path.join(_data.GOLDEN, "ws_parent.npz"))


def _same(got, want, prefix):
    keys = sorted(k for k in want.files if k.startswith(prefix))
    assert sorted(got) == keys
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("name", gold.SHAPES)
@pytest.mark.parametrize("kind", gold.KINDS)
def test_results_are_bitwise_those_of_the_parent_commit(fos, want, kind, name):
    got = gold.compute(fos, torch, kind, name)
    assert len(got) == len(gold.FAMILIES) * len(gold.WIDTHS) * len(gold.XS) * len(FIELDS)
    assert {k.rsplit("/", 1)[1] for k in got} == set(FIELDS)
    _same(got, want, f"{kind}/{name}/")
    # what the record holds: the certificate's G is the gradient entry point's, violators and coordinates at rest in every scan,
    # +inf where a factor is exactly 0, scales on both sides of 1 (both branches of the column pass), nothing non-finite elsewhere
    assert all(bool(got[k]) for k in got if k.endswith("/same_G"))
    # (in the record every coordinate outside the set violates in exactly two scans: the grouped C = 7 handle at X = 0 on the
    # 72 unpadded bf16 columns of the two-panel shape, at either width - its smallest weight is a fifth of the largest gradient)
    all_violate = {f"bf16/panels/softmax7_gwp/{which}/zero/viol" for which in gold.WIDTHS}
    for k in got:
        if k.endswith("/viol"):
            outside = got[k[:-4] + "excess"].size * 2 // 3              # a third of the coordinates is in the set
            assert (got[k].size == outside) if k in all_violate else (0 < got[k].size < outside), k
        if k.endswith("/out64"):
            assert np.isfinite(got[k]).all(), k
    assert all(np.isinf(got[k]).any() for k in got if k.endswith("/excess") and "/softmax7_gwp/" in k)
    scales = np.concatenate([got[k].reshape(4, 16)[3] for k in got if k.endswith("/out64")])
    assert ((scales > 0) & (scales < 1)).any() and (scales == 1).any()


@pytest.mark.parametrize("kind", gold.KINDS)
def test_scans_over_three_trips_are_bitwise_those_of_the_parent_commit(fos, want, kind):
    got = gold.scans(fos, torch, kind)                 # (asserts violators in every trip and on both sides of a wave boundary)
    assert len(got) == 2 * len(gold.SCANS)
    _same(got, want, f"{kind}/scan/")
    for case in gold.SCANS:
        assert got[f"{kind}/scan/{case}/excess"].shape == (gold.SCAN_NDEV,) and gold.SCAN_NDEV == 2 * 1024 + 456


def test_refusals_are_those_of_the_parent_commit(fos):
    with open(os.path.join(_data.GOLDEN, "ws_refusals.json")) as fh:
        want = json.load(fh)
    got = gold.refusals(fos, torch)
    assert sorted(got) == sorted(want) and len(want) == 40
    for k in sorted(want):
        assert got[k] == want[k], (k, got[k], want[k])
    assert all(rc in (-1, -4) and msg.startswith(k.split("/")[0] + ": ") for k, (rc, msg) in want.items())
    assert {k.split("/")[0] for k in want} == {"fos_gradient_batch", "fos_kkt_scan", "fos_duality_gap", "fos_multinomial_gradient_batch",
                                               "fos_multinomial_kkt_scan", "fos_multinomial_duality_gap"}


def test_the_guards_left_out_of_the_record_have_no_handle_to_meet(fos):
    """The record holds no multinomial refusal for missing labels, sharding, a shape without the matrix-core pair or feature groups:
    no multinomial handle can be brought into any of those states."""
    from fastoptsolver_amd.distributed import Comm
    At, y = torch.zeros(100, 4, device="cuda"), np.arange(100) % 3
    with pytest.raises(ValueError, match="labels"):
        fos.prepare_multinomial(At, None, 3)
    with pytest.raises(ValueError):
        fos.prepare_grouped(At, y, [2, 2], loss="multinomial")
    P = fos.prepare_multinomial(At, y, 3)
    comm = Comm.solo()
    for bind in (P.set_comm, P.set_comm_cols):
        with pytest.raises(fos.FosError, match="fos_problem_set_comm"):
            bind(comm)
    # 4 columns: a plain squared handle of this shape has no matrix-core pair (the "no_pair" rows of the record); the multinomial
    # one is padded into it and served
    assert P.n_dev > 4
    G = P.multinomial_gradient_block(torch.zeros(P.n_dev, 3, device="cuda"))
    out64, _ = P.multinomial_duality_gap_block(torch.zeros(P.n_dev, 3, device="cuda"), [0.5], [0.0])
    assert G.shape == (3, P.n_dev) and bool(torch.isfinite(out64).all())
