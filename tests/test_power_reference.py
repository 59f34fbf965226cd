"""CPU guard of the power-iteration menu (tests/_power.py): the restated reference is the oracle's loop, every menu entry fires
where it says with a margin that fp32 arithmetic cannot cross, the streaming representatives reach every trip class of
power_normalize_kernel, and an entry edited into the unsafe zone is reported by name."""
import numpy as np
import pytest

from oracle import fos_oracle as orc
from tests import _power as pw


@pytest.mark.parametrize("c", pw.ALL, ids=pw.case_id)
def test_reference_is_the_oracle(c):
    A, v0, Ls, Vs = pw.build(c)
    w = pw.weights_of(c)
    B = A if w is None else np.sqrt(w)[:, None] * A
    for name, n_iter, tol, step in pw.menu(c):
        L_ref, calls = orc.estimate_lipschitz(B, n_iter=n_iter, tol=tol, v0=v0, return_calls=True)
        seq, k, v = pw.sequence(B, v0, n_iter, tol)
        assert k == calls == step, (pw.case_id(c), name, k, calls)
        assert seq[-1] == pytest.approx(L_ref, rel=1e-12), (pw.case_id(c), name)
        assert np.allclose(seq, Ls[:k], rtol=1e-12, atol=0.0), (pw.case_id(c), name)
        assert np.linalg.norm(v - Vs[k - 1]) <= 1e-12, (pw.case_id(c), name)


@pytest.mark.parametrize("c", pw.ALL, ids=pw.case_id)
def test_every_entry_is_fp32_proof(c):
    Ls = pw.build(c)[2]
    names = [e[0] for e in pw.menu(c)]
    want = [f"stop{k}" for k in (pw.RANK1_STEPS if c["rank1"] else pw.STEPS)] + [f"never{k}" for k in pw.NEVER]
    assert names == want, pw.case_id(c)
    bad = [why for e in pw.menu(c) if (why := pw.unsafe(Ls, e))]
    assert not bad, (pw.case_id(c), bad)
    if not c["rank1"]:
        d = pw.diffs(Ls)
        assert np.all(np.diff(d[:30]) < 0), (pw.case_id(c), "d_k does not fall strictly over the first 30 steps")


def test_chunk_edges_are_in_the_menu():
    assert {pw.CHUNK, pw.CHUNK + 1} <= set(pw.STEPS) and min(pw.STEPS) == 1
    assert any(1 < k < pw.CHUNK for k in pw.STEPS) and any(20 <= k <= 30 for k in pw.STEPS)
    assert set(pw.NEVER) == {1, 2, 16, 17, 21} and any(k % pw.CHUNK for k in pw.NEVER if k > pw.CHUNK)


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_batch_members_break_at_their_own_steps_under_one_tol(dtype):
    members = pw.batch_members(dtype)
    assert len({step for _, step, _ in members}) >= 5
    assert members[-1][0] is members[0][0]
    for c, step, scale in members:
        assert pw.resident_fits(c["m"], c["n"]) and c["n"] < pw.BATCH_LDV
        Ls = pw.build(c, scale)[2]
        why = pw.unsafe(Ls, ("stops", pw.BATCH_N_ITER, pw.BATCH_TOL, step))
        assert why is None, (pw.case_id(c), why)


def test_resident_cases_sit_at_the_lds_limits():
    shapes = {(c["m"], c["n"]) for c in pw.RESIDENT}
    assert {(157, 64), (4096, 1), (2048, 5), (3413, 2)} <= shapes
    assert all(pw.resident_fits(m, n) for m, n in shapes)
    # one more row does not fit
    assert not any(pw.resident_fits(m + 1, n) for m, n in ((157, 64), (4096, 1), (2048, 5), (3413, 2)))
    assert {pw.RS_CHUNK, pw.RS_CHUNK + 1} <= {n for _, n in shapes} and any(m == 1 for m, _ in shapes)


def test_streaming_cases_cover_the_normalize_kernel():
    assert pw.normalize_classes() == pw.NORMALIZE_CLASSES
    # the guard guards: without the padded and the bf16 menu case the partial second trip is gone
    rest = [c for c in pw.STREAMING if c["name"] not in ("padded", "menu_bf16")]
    assert "partial_second_trip" not in pw.normalize_classes(rest)


def test_an_entry_edited_into_the_unsafe_zone_is_named():
    c = pw.RESIDENT[0]
    Ls = pw.build(c)[2]
    d = pw.diffs(Ls)
    name, n_iter, tol, step = next(e for e in pw.menu(c) if e[0] == "stop16")
    assert pw.unsafe(Ls, (name, n_iter, tol, step)) is None
    # tol moved to within 2 * TOL * L of d_16 (either side), and of an earlier d_k
    for moved in (d[15] + 1.9 * pw.TOL * Ls[15], d[15] * (1 + 1e-9), d[14] - 1.9 * pw.TOL * Ls[14]):
        why = pw.unsafe(Ls, (name, n_iter, moved, step))
        assert why is not None and why.startswith("stop16:"), why
    # a tol that fires elsewhere
    assert "fires at step 15" in pw.unsafe(Ls, (name, n_iter, 0.5 * (d[13] + d[14]), step))
