"""GPU: the power iteration on every route against the fp64 reference of tests/_power.py - L, the step at which the break
rule fires and the returned vector, for every entry of the stop menu (breaks at step 1, inside the first 16-step chunk, on
its last step, on the first step of the next chunk, later; never, with n_iter on either side of the chunk edges).

Routes: the LDS-resident kernel at its LDS limits, the batch kernel (ragged, offsets, lda > n, ldv > n, one shared tol), the
streaming host loop over one representative plan per kernel table, the weighted host loop and the column-sharded host loop.
The contract asserted on all of them: iters_out is the reference's break step exactly, L is within TOL of the reference's L
at that step, and v is the normalised iterate after exactly that step (relative 2-norm error within TOL, | ||v|| - 1 | within
4 eps32 sqrt(n)).  Everything around the operands and the outputs is NaN (a sentinel for the integers) and has to stay so.

Mutations of the library, each built aside, run once against this file on an MI355X and taken out again (as
tests/test_fista_forms.py reports its transitions):
  - the streaming loop copying out the iterate of the last enqueued step instead of slot `used - 1` of its ring (the
    behaviour before the ring): all 8 streaming cases fail, on v alone.  The report names stop1 first (the vector is 7e-8 from
    the iterate after 16 steps and 0.56 from the one after step 1) and stop20 last (7e-8 from the iterate after 32 steps, 0.099
    from the one after step 20); pytest elides the entries between them, where stop5 and stop17 break inside a chunk in the
    same way.  stop16 and the never entries end on the last enqueued step and pass; resident, batch, weighted and
    column-sharded cases pass.
  - `used = it` instead of `it + 1` in the host replay: all 8 streaming cases fail on iters_out (stop1 reports 0 steps).
  - `prev = L` dropped in power_resident_run: all 14 resident cases fail on iters_out (stop5, or stop2 on the rank-one shapes,
    runs to n_iter = 35) and both batch calls do (member 0 reports 35 steps for 16).
The largest errors seen per route are in profiles/power/README.md."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import fos_oracle as orc
from tests import _power as pw

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -777
ERR_ARG, ERR_UNSUPPORTED = -1, -4
WORST = {}                                  # route -> [L error, v error, norm error / (eps32 sqrt(n))]


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    yield f
    print("\nlargest errors per route (L relative, v relative 2-norm, | ||v|| - 1 | in eps32 sqrt(n)):")
    for route, (eL, ev, en) in sorted(WORST.items()):
        print(f"  {route:10s} L {eL:.2e}  v {ev:.2e}  norm {en:.2f}")
    pw._built.cache_clear()


@pytest.fixture(scope="module")
def comm(fos):
    from fastoptsolver_amd import distributed as fd
    return fd.Comm.solo()


def _tdt(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def _store(A64, dtype, layout):
    """(device view of A in `layout`, the buffer it sits in): everything around the operand is NaN."""
    m, n = A64.shape
    A = torch.as_tensor(A64.astype(np.float32)).to(_tdt(dtype)).cuda()
    assert np.array_equal(A.to(torch.float64).cpu().numpy(), A64)                  # the stored matrix is the truth
    if layout == "compact":
        return A, A
    if layout == "offset":
        flat = torch.full((m * n + 2,), NAN, dtype=_tdt(dtype), device="cuda")
        flat[1:1 + m * n] = A.reshape(-1)
        return flat[1:1 + m * n].view(m, n), flat
    pad = {"strided": 4, "ragged": 1}[layout]
    full = torch.full((m, n + pad), NAN, dtype=_tdt(dtype), device="cuda")
    full[:, :n] = A
    return full[:, :n], full


def _nan_around(buf, view):
    """Whether every element of `buf` outside `view` (a 2-D view with unit column stride) is still NaN."""
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    m, n = view.shape
    start = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    idx = start + (torch.arange(m, device=buf.device) * view.stride(0))[:, None] + torch.arange(n, device=buf.device)[None, :]
    mask[idx.reshape(-1)] = False
    return bool(torch.isnan(buf.reshape(-1)[mask]).all())


def _note(route, eL, ev=0.0, en=0.0):
    w = WORST.setdefault(route, [0.0, 0.0, 0.0])
    w[:] = [max(a, b) for a, b in zip(w, (eL, ev, en))]


def _check(route, where, L, it, v, Ls, Vs, step):
    v = np.asarray(v, dtype=np.float64)
    n = v.size
    assert it == step, (where, "iters_out", it, step)
    eL = abs(L - Ls[step - 1]) / Ls[step - 1]
    ev = float(np.linalg.norm(v - Vs[step - 1]))                       # ||v_ref|| = 1
    en = abs(float(np.linalg.norm(v)) - 1.0) / (pw.EPS32 * np.sqrt(n))
    _note(route, eL, ev, en)
    assert eL <= pw.TOL, (where, "L", L, Ls[step - 1], eL)
    assert ev <= pw.TOL, (where, "v", ev, "after 16 / 32 steps:", [float(np.linalg.norm(v - Vs[k - 1])) for k in (16, 32)])
    assert en <= 4.0, (where, "norm", en)


def _c_power_iter(prob, v0, n_iter, tol):
    """fos_power_iter called directly on a start vector inside a NaN-filled buffer: (rc, L, it, v, the buffer stayed NaN)."""
    from fastoptsolver_amd import _core
    buf = torch.full((prob.n_dev + 8,), NAN, dtype=torch.float32, device="cuda")
    buf[4:4 + prob.n_dev] = 0.0
    buf[4:4 + prob.n] = torch.as_tensor(np.array(v0))
    L, it = C.c_double(-1.0), C.c_int(SENTINEL)
    with prob.ctx():
        rc = prob.lib.fos_power_iter(prob.h, _core.ptr(buf[4:]), int(n_iter), float(tol), C.byref(L), C.byref(it))
    out = buf.cpu().numpy()
    clean = bool(np.isnan(out[:4]).all() and np.isnan(out[4 + prob.n_dev:]).all())
    return rc, L.value, it.value, out[4:4 + prob.n_dev], clean


def _problem(fos, c):
    """The handle of a resident or streaming case on its route, the route asserted through plan()."""
    A64 = pw.build(c)[0]
    if c["layout"] == "host":
        view = buf = None
        prob = fos.prepare(A64.astype(np.float32), None, pad=True)
        assert (prob.n, prob.n_dev) == (c["n"], c["n_dev"])
    else:
        view, buf = _store(A64, c["dtype"], c["layout"])
        prob = fos.prepare(view, None, pad=False)
        assert prob.n_dev == c["n"] and prob.A.data_ptr() == view.data_ptr()          # borrowed as it is
    if c.get("no_resident"):
        prob.replan(no_resident=True)
    plan = prob.plan()
    if c["route"] == "resident":
        assert plan["resident"] == 1 and pw.resident_fits(c["m"], c["n"]), (pw.case_id(c), plan)
    else:
        want = dict(c["plan"])
        geo = want.pop("geo", None)
        assert {k: plan[k] for k in want} == want, (pw.case_id(c), plan)
        if geo is not None:
            assert (plan["threads"], plan["chunks"], plan["rows"]) == tuple(geo), (pw.case_id(c), plan)
    return prob, view, buf


# ---- resident and streaming: every entry through the C entry point and through Problem.power_iter -------------------------
@pytest.mark.parametrize("c", pw.RESIDENT + pw.STREAMING, ids=pw.case_id)
def test_every_stop_on_the_single_problem_routes(fos, c):
    _, v0, Ls, Vs = pw.build(c)
    v0 = np.array(v0)                                                                 # (the shared one is read-only)
    prob, view, buf = _problem(fos, c)
    n = c["n"]
    failed = []                                   # every entry runs: the report names all that fail, not the first
    for name, n_iter, tol, step in pw.menu(c):
        where = (pw.case_id(c), name)
        rc, L, it, v, clean = _c_power_iter(prob, v0, n_iter, tol)
        assert rc == 0 and clean, (where, rc)
        assert not v[n:].any(), where                                                 # padding columns stay zero
        try:
            _check(c["route"], where, L, it, v[:n], Ls, Vs, step)
        except AssertionError as e:
            failed.append(str(e).splitlines()[0])
        L2, it2, v2 = prob.power_iter(v0, n_iter=n_iter, tol=tol)
        assert v2.numel() == n and (L2, it2) == (L, it) and np.array_equal(v2.cpu().numpy(), v[:n]), where
    if failed:
        print("\n".join(failed))                  # in full: the assertion message is elided in the middle
    assert not failed, failed
    if buf is not None:
        assert _nan_around(buf, view), pw.case_id(c)
        if c["route"] == "resident" and c["layout"] != "compact":
            # the NaN around A changed nothing: the compact copy of the same elements gives the same bits
            name, n_iter, tol, step = pw.menu(c)[1]
            twin = fos.prepare(view.contiguous(), None, pad=False)
            assert twin.plan()["resident"] == 1
            assert twin.power_iter(v0, n_iter=n_iter, tol=tol)[:2] == prob.power_iter(v0, n_iter=n_iter, tol=tol)[:2]


# ---- batch ----------------------------------------------------------------------------------------------------------------
def _batch_call(lib, A, dtype, items, V, ldv, n_iter, tol, Lbuf, used, count=None):
    from fastoptsolver_amd import _core, _lib
    count = len(items) if count is None else count
    work = torch.empty(max(count, 1) * C.sizeof(_lib.BatchItem) // 8 + 1, dtype=torch.float64, device="cuda")
    return lib.fos_power_iter_batch(_core.ptr(A), 1 if dtype == "bf16" else 0, _core.batch_items(items), count,
                                    C.c_void_p(V.data_ptr() + 4 * ldv), ldv, n_iter, tol, C.c_void_p(Lbuf.data_ptr() + 8),
                                    C.c_void_p(used.data_ptr() + 4), _core.ptr(work), _core.stream_ptr())


def _batch_setup(dtype):
    """One flat NaN-filled buffer holding the members at non-zero offsets (every second one with lda = n + 3), the start
    vectors in rows 1..P of a NaN-filled (P + 2) x ldv block, L_out and iters_used one element into guarded arrays."""
    members = pw.batch_members(dtype)
    P, ldv = len(members), pw.BATCH_LDV
    items, blocks, off = [], [], 5
    for i, (c, step, scale) in enumerate(members[:-1]):
        m, n = c["m"], c["n"]
        lda = n + 3 * (i % 2)
        items.append((off, lda, 0, m, n))
        blocks.append((off, lda, pw.build(c, scale)[0]))
        off += m * lda + 3
    items.append(items[0])                                                            # the duplicate: same a_offset
    A = torch.full((off,), NAN, dtype=_tdt(dtype), device="cuda")
    live = torch.zeros(off, dtype=torch.bool, device="cuda")
    for o, lda, A64 in blocks:
        m, n = A64.shape
        torch.as_strided(A, (m, n), (lda, 1), o)[:] = torch.as_tensor(A64.astype(np.float32)).to(_tdt(dtype)).cuda()
        torch.as_strided(live, (m, n), (lda, 1), o)[:] = True
    V0 = torch.full((P + 2, ldv), NAN, dtype=torch.float32, device="cuda")
    for i, (c, step, scale) in enumerate(members):
        V0[1 + i, : c["n"]] = torch.as_tensor(np.array(pw.build(c, scale)[1]))
    return members, items, A, live, V0


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_batch_one_call_one_tol_every_member_at_its_own_step(fos, dtype):
    from fastoptsolver_amd import _lib
    lib = _lib.load()
    members, items, A, live, V0 = _batch_setup(dtype)
    P, ldv = len(members), pw.BATCH_LDV
    for name, n_iter, tol in pw.BATCH_ENTRIES:
        V = V0.clone()
        Lbuf = torch.full((P + 2,), NAN, dtype=torch.float64, device="cuda")
        used = torch.full((P + 2,), SENTINEL, dtype=torch.int32, device="cuda")
        rc = _batch_call(lib, A, dtype, items, V, ldv, n_iter, tol, Lbuf, used)
        assert rc == 0, lib.fos_last_error()
        Vh, Lh, uh = V.cpu().numpy(), Lbuf.cpu().numpy(), used.cpu().numpy()
        assert np.isnan(Lh[[0, -1]]).all() and (uh[[0, -1]] == SENTINEL).all(), name
        assert np.isnan(Vh[0]).all() and np.isnan(Vh[-1]).all(), name
        for i, (c, step, scale) in enumerate(members):
            where = ("batch", dtype, name, i, pw.case_id(c))
            assert pw.resident_fits(c["m"], c["n"]), where
            _, _, Ls, Vs = pw.build(c, scale)
            assert np.isnan(Vh[1 + i, c["n"]:]).all(), where                          # the gap between n and ldv
            _check("batch", where, Lh[1 + i], int(uh[1 + i]), Vh[1 + i, : c["n"]], Ls, Vs, step if tol > 0 else n_iter)
        assert Lh[P] == Lh[1] and uh[P] == uh[1] and np.array_equal(Vh[P, : members[0][0]["n"]], Vh[1, : members[0][0]["n"]])
        assert bool(torch.isnan(A[~live]).all())                                     # the NaN around the members is still there


def test_batch_argument_checks_leave_the_outputs_alone(fos):
    from fastoptsolver_amd import _lib
    lib = _lib.load()
    members, items, A, live, V0 = _batch_setup("f32")
    P, ldv = len(members), pw.BATCH_LDV
    V = V0.clone()
    Lbuf = torch.full((P + 2,), NAN, dtype=torch.float64, device="cuda")
    used = torch.full((P + 2,), SENTINEL, dtype=torch.int32, device="cuda")
    ao, lda, _, m, n = items[0]

    def call(its, ldv_=ldv, n_iter=5):
        return _batch_call(lib, A, "f32", its, V, ldv_, n_iter, 0.5, Lbuf, used)

    assert call(items, ldv_=n - 1) == ERR_ARG                                          # ldv < n
    assert call(items, n_iter=0) == ERR_ARG and call(items, n_iter=-3) == ERR_ARG
    assert call([(-1, lda, 0, m, n)] + items[1:]) == ERR_ARG                           # a negative offset
    assert call([(ao, n - 1, 0, m, n)] + items[1:]) == ERR_ARG                         # lda < n
    for m_out, n_out in ((158, 64), (4097, 1), (2049, 5), (10, 65)):                  # one past each resident limit
        assert not pw.resident_fits(m_out, n_out)
        assert call(items[:1] + [(ao, n_out, 0, m_out, n_out)]) == ERR_UNSUPPORTED, (m_out, n_out)
    torch.cuda.synchronize()
    assert torch.equal(V.nan_to_num(nan=-1.0), V0.nan_to_num(nan=-1.0))
    assert bool(torch.isnan(Lbuf).all()) and bool((used == SENTINEL).all())


# ---- weighted and column-sharded: the loops report only L; their steps are counted ----------------------------------------------
def _counted(monkeypatch, obj, attr):
    calls, inner = [], getattr(obj, attr)

    def counting(*a, **kw):
        calls.append(1)
        return inner(*a, **kw)
    monkeypatch.setattr(obj, attr, counting)
    return calls


@pytest.mark.parametrize("c", pw.WEIGHTED, ids=pw.case_id)
def test_every_stop_on_the_weighted_loop(fos, monkeypatch, c):
    from fastoptsolver_amd import iterative_solvers as ist
    A64, v0, Ls, Vs = pw.build(c)
    w = pw.weights_of(c)
    P = fos.prepare_weighted(torch.as_tensor(A64.astype(np.float32)).to(_tdt(c["dtype"])).cuda(), np.zeros(c["m"]), w,
                             dtype=c["dtype"])
    assert P.n_dev == c["n"] and P.dtype == c["dtype"] and P.sample_weight is not None
    calls = _counted(monkeypatch, P, "gram_apply")
    for name, n_iter, tol, step in pw.menu(c):
        del calls[:]
        L = ist._weighted_lipschitz(P, v0.astype(np.float64), n_iter, tol)
        where = (pw.case_id(c), name)
        assert len(calls) == step, (where, len(calls), step)
        eL = abs(L - Ls[step - 1]) / Ls[step - 1]
        _note("weighted", eL)
        assert eL <= pw.TOL, (where, L, Ls[step - 1])


@pytest.mark.parametrize("c", pw.COLS, ids=pw.case_id)
def test_every_stop_on_the_column_sharded_loop(fos, comm, monkeypatch, c):
    from fastoptsolver_amd import iterative_solvers as ist
    A64, v0, Ls, Vs = pw.build(c)
    n = c["n"]
    view, _ = _store(A64, c["dtype"], "compact")
    prob = fos.prepare(view, None, pad=False)
    prob.set_comm_cols(comm)
    plan = prob.plan()
    assert (plan["path"], plan["colblock"], plan["tall"]) == (0, 1, 0), plan
    # the single-problem entry refuses the handle, outputs untouched
    rc, L, it, v, clean = _c_power_iter(prob, v0, 5, 0.0)
    assert rc == ERR_UNSUPPORTED and (L, it) == (-1.0, SENTINEL) and clean and np.array_equal(v, v0)
    calls = _counted(monkeypatch, prob, "gemv_pair")
    monkeypatch.setattr(np.random, "randn", lambda k: v0.astype(np.float64)[:k].copy())    # the loop draws its own v0
    for name, n_iter, tol, step in pw.menu(c):
        del calls[:]
        L = ist._lipschitz_cols(prob, comm, (0, n, n), n_iter, tol)
        where = (pw.case_id(c), name)
        assert len(calls) == step, (where, len(calls), step)
        eL = abs(L - Ls[step - 1]) / Ls[step - 1]
        _note("cols", eL)
        assert eL <= pw.TOL, (where, L, Ls[step - 1])


# ---- estimate_lipschitz through the public API, one case per route -------------------------------------------------------------
def _drawn(n_total, seed_):
    """The draw estimate_lipschitz makes after np.random.seed(seed_), and the next normal of the stream after it."""
    np.random.seed(seed_)
    v0 = np.random.randn(n_total)
    return v0, np.random.randn()


@pytest.mark.parametrize("route", ("resident", "streaming", "batch", "weighted", "cols"))
def test_estimate_lipschitz_public_api(fos, comm, route):
    from fastoptsolver_amd import iterative_solvers as ist
    by = {pw.case_id(c): c for c in pw.ALL}
    if route == "batch":
        cs = [by["resident-lds_full-f32"], by["resident-m3413-f32"], by["resident-chunk_plus-f32"]]
    else:
        cs = [by[{"resident": "resident-lds_full-f32", "streaming": "streaming-menu_f32-f32", "weighted": "weighted-edges-f32",
                  "cols": "cols-cols-f32"}[route]]]
    mats = [pw.build(c)[0] for c in cs]
    v0, nxt = _drawn(sum(c["n"] for c in cs), 5)
    np.random.seed(5)
    if route == "batch":
        got = list(fos.estimate_lipschitz([A.astype(np.float32) for A in mats]))
    elif route == "weighted":
        P = fos.prepare_weighted(mats[0].astype(np.float32), np.zeros(cs[0]["m"]), pw.weights_of(cs[0]))
        got = [fos.estimate_lipschitz(P)]
        mats = [np.sqrt(pw.weights_of(cs[0]))[:, None] * mats[0]]
    elif route == "cols":
        prob = fos.prepare(_store(mats[0], "f32", "compact")[0], None, pad=False)
        prob.set_comm_cols(comm)
        got = [ist._lipschitz_cols(prob, comm, (0, cs[0]["n"], cs[0]["n"]))]
    else:
        prob, _, _ = _problem(fos, cs[0])
        got = [fos.estimate_lipschitz(prob)]
    assert np.random.randn() == nxt                                                   # exactly n normals per problem, as ref:50
    o = 0
    for c, A, L in zip(cs, mats, got):
        v = v0[o:o + c["n"]].astype(np.float32).astype(np.float64) if route != "weighted" else v0[o:o + c["n"]]
        o += c["n"]
        assert L == pytest.approx(orc.estimate_lipschitz(A, v0=v), rel=pw.TOL), (route, pw.case_id(c))


# ---- a zero matrix: L = 0, one iteration, a NaN vector - as the reference, and it returns ------------------------------------------
@pytest.mark.parametrize("m,n,no_resident", [(50, 8, False), (300, 1024, True)], ids=["resident", "streaming"])
def test_zero_matrix(fos, m, n, no_resident):
    A = np.zeros((m, n))
    v0 = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    seq, k, v_ref = pw.sequence(A, v0, 40, 1e-3)
    assert (list(seq), k) == ([0.0], 1) and np.isnan(v_ref).all()                     # abs(0 - 0) < tol on the first step
    prob = fos.prepare(torch.zeros(m, n, device="cuda"), None, pad=False)
    if no_resident:
        prob.replan(no_resident=True)
    assert prob.plan()["resident"] == (0 if no_resident else 1)
    rc, L, it, v, clean = _c_power_iter(prob, v0, 40, 1e-3)
    assert rc == 0 and clean and L == 0.0 and it == 1 and np.isnan(v).all(), (rc, L, it)


# ---- argument checks of the single-problem entry -----------------------------------------------------------------------------------
def test_power_iter_argument_checks_leave_the_outputs_alone(fos):
    c = pw.RESIDENT[0]
    _, v0, _, _ = pw.build(c)
    prob, _, _ = _problem(fos, c)
    rc, L, it, v, clean = _c_power_iter(prob, v0, 0, 0.0)                             # n_iter = 0
    assert rc == ERR_ARG and (L, it) == (-1.0, SENTINEL) and clean and np.array_equal(v, v0)
    L, it = C.c_double(-1.0), C.c_int(SENTINEL)
    assert prob.lib.fos_power_iter(prob.h, None, 5, 0.0, C.byref(L), C.byref(it)) == ERR_ARG      # a null v_inout
    assert (L.value, it.value) == (-1.0, SENTINEL)
