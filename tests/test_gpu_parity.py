"""GPU parity tests: the HIP path (through the C ABI) vs the oracle and vs the golden vectors captured from
the reference.  Tolerance: 1e-5 relative on iterates (BASELINE.json north_star: "iterates match the NumPy
reference to 1e-5 relative fp32"); counts (gradient calls, line-search shrinks, iterations) must be equal."""
import numpy as np
import pytest
import torch

from oracle import fos_oracle as orc
from tests import _data

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def fos():
    import fastoptsolver_amd as f
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return f


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype, device="cuda")


# --------------------------------------------------------------------------------------------------
# K2 / K5 / prox / power iteration against the oracle
# --------------------------------------------------------------------------------------------------
SHAPES = [(64, 16), (777, 129), (1000, 5), (4096, 512), (300, 1024), (1, 8), (3, 4), (513, 2052), (2050, 8192),
          (1031, 16384), (700, 4100)]


@pytest.mark.parametrize("m,n", SHAPES)
@pytest.mark.parametrize("with_b", [True, False])
def test_gemv_pair(fos, m, n, with_b):
    rng = np.random.default_rng(m * 31 + n)
    A = rng.standard_normal((m, n)).astype(np.float32)
    b = rng.standard_normal(m).astype(np.float32) if with_b else None
    y = rng.standard_normal(n).astype(np.float32)
    prob = fos.prepare(A, b)
    rr = torch.zeros(1, dtype=torch.float64, device="cuda")
    g = prob.gemv_pair(_dev(y), alpha2=0.3, rr_out=rr).cpu().numpy().astype(np.float64)
    g_ref, rr_ref = orc.gram_gradient(A.astype(np.float64), y.astype(np.float64),
                                      None if b is None else b.astype(np.float64), 0.3)
    assert _data.rel(g, g_ref) < TOL, prob.plan()
    assert float(rr.cpu()) == pytest.approx(rr_ref, rel=TOL)
    r2, x2, x1 = prob.residual_objective(_dev(y))
    assert r2 == pytest.approx(rr_ref, rel=TOL)
    assert x2 == pytest.approx(float(y.astype(np.float64) @ y), rel=1e-6)
    assert x1 == pytest.approx(float(np.abs(y.astype(np.float64)).sum()), rel=1e-6)


def test_gemv_pair_paths_and_layouts(fos):
    """Strided A (lda > n), misaligned views (two-pass kernels when borrowed as they are, pad=False; a compact aligned
    copy on the single pass by default from 2^20 elements on) and a misaligned y must agree with the fused path."""
    rng = np.random.default_rng(5)
    m, n = 1500, 1024
    big = torch.as_tensor(rng.standard_normal((m, n + 8)).astype(np.float32), device="cuda")
    b = rng.standard_normal(m).astype(np.float32)
    ybuf = torch.as_tensor(rng.standard_normal(n + 1).astype(np.float32), device="cuda")
    y = ybuf[1:]                                     # 4-byte aligned only
    ref = None
    for name, view, pad in (("aligned-strided", big[:, :n], None), ("misaligned", big[:, 1:n + 1], False),
                            ("misaligned-copied", big[:, 1:n + 1], None), ("shifted4", big[:, 4:n + 4], None)):
        prob = fos.prepare(view, b, pad=pad)
        plan = prob.plan()
        assert plan["path"] == (1 if name == "misaligned" else 0), (name, plan)
        g = prob.gemv_pair(y, alpha2=0.0).cpu().numpy()
        A64 = view.cpu().numpy().astype(np.float64)
        g_ref, _ = orc.gram_gradient(A64, y.cpu().numpy().astype(np.float64), b.astype(np.float64), 0.0)
        assert _data.rel(g, g_ref) < TOL, name


@pytest.mark.parametrize("threads,chunks,rows", [(256, 4, 2), (512, 4, 1), (512, 8, 1), (1024, 4, 1), (1024, 2, 2)])
def test_every_fused_geometry(fos, threads, chunks, rows):
    rng = np.random.default_rng(threads + chunks)
    m = 1237
    n = min(threads * chunks * 4, 4096)
    A = rng.standard_normal((m, n)).astype(np.float32)
    b = rng.standard_normal(m).astype(np.float32)
    y = rng.standard_normal(n).astype(np.float32)
    prob = fos.prepare(A, b)
    prob.tune(threads, chunks, rows, 37)
    plan = prob.plan()
    assert (plan["threads"], plan["chunks"], plan["rows"]) == (threads, chunks, rows)
    g = prob.gemv_pair(_dev(y)).cpu().numpy()
    g_ref, _ = orc.gram_gradient(A.astype(np.float64), y.astype(np.float64), b.astype(np.float64), 0.0)
    assert _data.rel(g, g_ref) < TOL, plan


@pytest.mark.parametrize("m,n,kind", [(1237, 8192, "f32"), (300, 5000, "f32"), (2050, 16384, "f32"), (100, 12288, "f32"),
                                      (900, 8192, "bf16"), (333, 16384, "bf16"), (5, 8192, "f32"), (257, 16384, "f32")])
def test_interleaved_rows_equal_block_rows(fos, m, n, kind):
    """FOS_PLAN_INTERLEAVE: rows dealt round-robin to the workgroups instead of one contiguous block each (fp32 pass,
    residual-only pass, DUAL/history pass, fp64 `fg` pass) - same sums in another order: against the oracle at 1e-5 /
    1e-12, against the block form at 1e-6, a whole FISTA run with history against the oracle, fewer rows than workgroups."""
    from fastoptsolver_amd import _core, _lib
    lib = _lib.load()
    rng = np.random.default_rng(m + n)
    A = rng.standard_normal((m, n)).astype(np.float32)
    At = torch.as_tensor(A).to(torch.bfloat16 if kind == "bf16" else torch.float32)
    A64 = At.to(torch.float64).numpy()
    b = rng.standard_normal(m).astype(np.float32)
    y = rng.standard_normal(n).astype(np.float32)
    prob = fos.prepare(At.cuda(), b)
    g_blk = prob.gemv_pair(_dev(y), alpha2=0.2).cpu().numpy()
    prob.replan(interleave=True)
    plan = prob.plan()
    assert plan["interleave"] == 1 and plan["path"] == 0, plan
    rr = torch.zeros(1, dtype=torch.float64, device="cuda")
    g_il = prob.gemv_pair(_dev(y), alpha2=0.2, rr_out=rr).cpu().numpy()
    g_ref, rr_ref = orc.gram_gradient(A64, y.astype(np.float64), b.astype(np.float64), 0.2)
    assert _data.rel(g_il, g_ref) < TOL, plan
    assert _data.rel(g_il, g_blk) < 1e-6
    assert float(rr.cpu()) == pytest.approx(rr_ref, rel=TOL)
    assert prob.residual_objective(_dev(y))[0] == pytest.approx(rr_ref, rel=TOL)        # residual-only instantiation
    x = rng.standard_normal(n) * (1.0 + 1e-9 * rng.standard_normal(n))
    out = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
    _lib.check(lib.fos_gemv_pair_dd(prob.h, _core.ptr(_dev(x, torch.float64)), 0.37, _core.ptr(out)))   # fp64 fg pass
    gd_ref, rrd_ref = orc.gram_gradient(A64, x, b.astype(np.float64), 0.37)
    assert _data.rel(out.cpu().numpy()[:n], gd_ref) < 1e-12
    assert float(out[n].cpu()) == pytest.approx(rrd_ref, rel=1e-12)
    # a whole run with history (DUAL pass) on the interleaved plan
    a1 = 0.1 * float(np.max(np.abs(A64.T @ b)))
    np.random.seed(3)
    v0 = np.random.randn(n)
    np.random.seed(3)
    xg, hg = fos.fista(prob, None, "lasso", a1, 0.0, max_iter=12, return_history=True)
    xr, hr = orc.fista(A64, b.astype(np.float64), "lasso", a1, 0.0, max_iter=12, return_history=True, v0=v0)
    assert _data.rel(_np(xg), xr) < TOL
    assert np.allclose([float(o) for o in hg["obj"]], hr["obj"], rtol=2e-5)


def test_gemv_pair_bf16(fos):
    """bf16 A / fp32 accumulate: judged against the oracle run on the bf16-rounded A."""
    rng = np.random.default_rng(11)
    for m, n in ((900, 2048), (333, 16384), (100, 24)):
        A16 = torch.as_tensor(rng.standard_normal((m, n)).astype(np.float32)).to(torch.bfloat16)
        b = rng.standard_normal(m).astype(np.float32)
        y = rng.standard_normal(n).astype(np.float32)
        prob = fos.prepare(A16.cuda(), b)
        assert prob.dtype == "bf16"
        g = prob.gemv_pair(_dev(y), alpha2=0.1).cpu().numpy()
        g_ref, _ = orc.gram_gradient(A16.to(torch.float64).numpy(), y.astype(np.float64), b.astype(np.float64), 0.1)
        assert _data.rel(g, g_ref) < TOL, (m, n, prob.plan())


def test_prox_kernels(fos):
    fx = _data.load("leaf")
    v = fx["leaf/v"].astype(np.float32)
    for thr in (0.7, 0.0):
        got = fos.prox_l1(v, thr)
        want = orc.prox_l1(v.astype(np.float64), np.float64(np.float32(thr)))
        assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-6, atol=1e-7)
        assert np.array_equal(got == 0, want == 0)
        assert np.array_equal(np.signbit(got), np.signbit(want))          # -0.0 for shrunk negatives
    got = fos.prox_elastic_net(v, 0.3, 2.0, 0.5)
    assert np.allclose(got, orc.prox_elastic_net(v.astype(np.float64), 0.3, 2.0, 0.5), rtol=1e-6, atol=1e-7)
    # identities from SURVEY §4
    assert np.array_equal(fos.prox_l1(v, 0.0), v.astype(np.float64))
    assert np.allclose(fos.prox_elastic_net(v, 0.4, 1.5, 0.0), fos.prox_l1(v, 0.4 * 1.5), rtol=1e-6)
    t = fos.prox_l1(_dev(v), 0.7)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.numel() == v.size
    assert fos.prox_l1(np.zeros(0, dtype=np.float32), 0.1).size == 0
    # array-valued tau, as the reference's broadcasting expression allows
    thr = np.abs(np.random.default_rng(1).standard_normal(v.size)).astype(np.float32)
    assert np.allclose(fos.prox_l1(v, thr), orc.prox_l1(v.astype(np.float64), thr.astype(np.float64)), rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError):
        fos.prox_l1(v, thr[:5])
    got = fos.prox_elastic_net(v, thr, 2.0, 0.5)                            # prox_operators.py:15-16 broadcasts too
    assert np.allclose(got, orc.prox_elastic_net(v.astype(np.float64), thr.astype(np.float64), 2.0, 0.5), rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError):
        fos.prox_elastic_net(v, thr[:5], 2.0, 0.5)


def test_compute_objective(fos):
    fx = _data.load("leaf")
    v, A, b = fx["leaf/v"], fx["leaf/A"], fx["leaf/b"]
    got = [fos.compute_objective(v, A, b, r, 0.3, 0.7) for r in ("lasso", "ridge", "elasticnet")]
    assert np.allclose(got, fx["leaf/obj"], rtol=TOL)
    with pytest.raises(ValueError):
        fos.compute_objective(v, A, b, "l0", 0.3, 0.7)


@pytest.mark.parametrize("tag", ["tiny", "ragged", "aligned", "boston"])
def test_estimate_lipschitz(fos, tag):
    A, b, fx = _data.problem(tag)
    np.random.seed(0)
    L = fos.estimate_lipschitz(A)
    assert L == pytest.approx(float(fx[f"{tag}/L"]), rel=TOL)
    # consumed exactly n normals from the global stream, like iterative_solvers.py:50
    after = np.random.randn()
    np.random.seed(0)
    np.random.randn(A.shape[1])
    assert after == np.random.randn()


# --------------------------------------------------------------------------------------------------
# solver families against the goldens
# --------------------------------------------------------------------------------------------------
def _check_linesearch_counts(ours, ref, key, progress):
    """Per-iteration Armijo shrink counts must equal the reference's for every search that ends by a genuine
    acceptance.  Two regimes of the REFERENCE are decided by float64 rounding noise and are excluded:
    (1) STEP UNDERFLOW: when grad.(x_tmp - y) > 0 the reference halves t ~50 times until x_tmp == y bit for bit
        (iterative_solvers.py:187-194) and the solver is frozen from then on because tau persists (:197).  The
        device evaluates the same test on the difference vector in float64 and underflows after about as many
        halvings; counts are compared up to the first such event, which must be an underflow here as well.
    (2) STAGNATION: once an iteration changes the objective / iterate by less than 1e-10 relative
        (`progress[k]`), the reference's g(x_tmp) - g(y) is below the resolution of its own subtraction: such an
        iteration may disagree, and only a disagreement ends the comparison (round 3; it used to end at the first one)."""
    assert len(ours) == len(ref), key
    for k, (a, r) in enumerate(zip(ours, ref)):
        if progress[k] < 1e-10:
            if a != r:          # a different count here leaves a different step behind (tau persists): nothing to compare after
                return
            continue            # stagnating but in agreement: keep comparing
        if r >= 40:
            assert a >= r - 10, (key, k, a, int(r))
            return
        assert a == r, (key, k, a, int(r))


def _rel_progress(obj):
    obj = np.asarray(obj, dtype=np.float64)
    return np.concatenate([[1.0], np.abs(np.diff(obj)) / np.abs(obj[1:])])


def _call(fos, c, A, b, **extra):
    kw = dict(c["kw"])
    kw.update(extra)
    if c["algo"] == "fista":
        return fos.fista(A, b, c["reg"], c["alpha1"], c["alpha2"], max_iter=c["max_iter"], **kw)
    return fos.fista_delta(A, b, c["reg"], c["alpha1"], c["alpha2"], c["delta"], max_iter=c["max_iter"], **kw)


@pytest.mark.parametrize("tag", ["tiny", "ragged", "aligned"])
def test_fista_family_vs_reference_goldens(fos, tag):
    A, b, fx = _data.problem(tag)
    prob = fos.prepare(A, b)
    n_cases = 0
    for c in _data.cases(tag)["cases"]:
        if c["algo"] not in ("fista", "fista_delta"):
            continue
        key = c["key"]
        np.random.seed(0)
        x, h = _call(fos, c, prob, None, return_history=True)
        met = fos.get_metrics()
        if key + "/niter" in fx:
            assert len(h["obj"]) == int(fx[key + "/niter"]), key
            assert _data.rel(x, fx[key + "/x"]) < TOL, key
            continue
        off = 1 if c["algo"] == "fista" else 0
        for k, xr in zip(fx[key + "/ks"], fx[key + "/xs"]):
            assert _data.rel(h["x"][k - 1 + off], xr) < TOL, (key, int(k))
        assert np.allclose(h["obj"], fx[key + "/obj"], rtol=TOL), key
        assert [met["grad_num_calls"], met["ls_num_calls"]] == list(fx[key + "/counts"][:2]), key
        from fastoptsolver_amd import iterative_solvers as its
        _check_linesearch_counts(list(its.ls_call_iters), fx[key + "/ls_iters"], key, _rel_progress(fx[key + "/obj"]))
        assert set(met) == {"grad_num_calls", "grad_time_total", "grad_time_mean", "ls_num_calls", "ls_time_total",
                            "ls_time_mean", "ls_iters_total"}
        # the device-driven fast path (no history) must land on the same final iterate
        np.random.seed(0)
        x_fast = _call(fos, c, prob, None)
        assert isinstance(x_fast, np.ndarray) and x_fast.dtype == np.float64
        assert _data.rel(x_fast, fx[key + "/x"]) < TOL, key
        n_cases += 1
    assert n_cases >= 20


def test_boston_config1(fos):
    """BASELINE config 1: Boston-like Lasso through the device path (n = 5: LDS-resident loop; the split entry points
    and larger m take the row-per-thread single pass)."""
    fx = _data.load("boston")
    A, b = fx["boston/A"], fx["boston/b"]
    np.random.seed(0)
    x, h = fos.fista(A, b, "lasso", 1.0, 0.0, max_iter=500, return_history=True)
    plan = fos.prepare(A, b).plan()
    assert plan["resident"] == 1 and plan["tall"] == 1 and plan["path"] == 0
    for k, xr in zip(fx["boston/fista_lasso/ks"], fx["boston/fista_lasso/xs"]):
        assert _data.rel(h["x"][k], xr) < TOL, int(k)
    assert np.allclose(h["obj"], fx["boston/fista_lasso/obj"], rtol=TOL)
    assert fos.get_metrics()["grad_num_calls"] == 500
    np.random.seed(0)
    x = fos.fista_delta(A, b, "elasticnet", 1.0, 0.5, 3.0, max_iter=500)
    assert _data.rel(x, fx["boston/fdelta_enet/x"]) < TOL
    with pytest.raises(AssertionError):
        fos.fista_delta(A, b, "lasso", 1.0, 0.0, 2.0)


@pytest.mark.parametrize("tag", ["tiny", "ragged"])
def test_ista_vs_reference_goldens(fos, tag):
    A, b, fx = _data.problem(tag)
    n = 0
    for c in _data.cases(tag)["cases"]:
        if c["algo"] != "ista":
            continue
        key, a1, a2 = c["key"], c["alpha1"], c["alpha2"]
        s2 = a2 if c["in_smooth"] else 0.0
        ls = fos.LeastSquares(A, b, alpha2=s2)
        prox = fos.ElasticNetProx(a1, a2) if c["prox"] == "enet_prox" else fos.L1Prox(a1)
        L = float(fx[f"{tag}/ista/L"]) + s2
        x, log = fos.ista(np.zeros(A.shape[1]), ls, ls.grad, prox, L, max_iter=c["max_iter"], return_history=True,
                          **c["kw"])
        met = fos.get_metrics()
        assert _data.rel(x, fx[key + "/x"]) < TOL, key
        for k, xr in zip(fx[key + "/ks"], fx[key + "/xs"]):
            assert _data.rel(log["x"][k], xr) < TOL, (key, int(k))
        # step norms: an fp32 pass over A resolves ||x_new - x|| down to ~1e-7 ||x||
        assert np.allclose(log["delta"], fx[key + "/delta"], rtol=1e-4, atol=2e-6 * np.linalg.norm(x)), key
        assert [met["grad_num_calls"], met["ls_num_calls"]] == list(fx[key + "/counts"][:2]), key
        from fastoptsolver_amd import iterative_solvers as its
        progress = fx[key + "/delta"] / np.linalg.norm(fx[key + "/x"])
        _check_linesearch_counts(list(its.ls_call_iters), fx[key + "/ls_iters"], key, progress)
        live = int(np.argmax(progress < 1e-10)) if (progress < 1e-10).any() else len(progress)
        assert np.allclose(log["t"][:live + 1], fx[key + "/t"][:live + 1], rtol=1e-12), key
        # generic-callable path (arbitrary closures on device tensors) must agree with the fused one
        g = lambda x, ls=ls: ls(x)                                        # noqa: E731
        grad = lambda x, ls=ls: ls.grad(x)                                # noqa: E731
        prox_fn = lambda v, t, prox=prox: prox(v, t)                      # noqa: E731
        x2 = fos.ista(np.zeros(A.shape[1]), g, grad, prox_fn, L, max_iter=c["max_iter"], **c["kw"])
        assert _data.rel(x2, fx[key + "/x"]) < TOL, key
        n += 1
    assert n == 6


@pytest.mark.parametrize("tag", ["tiny", "ragged", "aligned"])
def test_lbfgs_vs_reference_goldens(fos, tag):
    """SciPy's float64 iterates captured through lbfgs.py:64 vs the fp64 device optimiser on the fp32-stored A (every
    sum of fg in fp64: fos_gemv_pair_dd): every iterate, the end point and the loss at the north-star tolerance, and
    the same number of iterations and fg evaluations as SciPy, ending on SciPy's own exit."""
    A, b, fx = _data.problem(tag)
    prob = fos.prepare(A, b)
    n = 0
    for c in _data.cases(tag)["cases"]:
        if c["algo"] != "lbfgs":
            continue
        key = c["key"]
        s = fos.LBFGSSolver(c["reg"], c["alpha1"], c["alpha2"]).fit(prob, None)
        assert (s.reg_type, s.alpha1, s.alpha2) == (c["norm_reg"], c["norm_a1"], c["norm_a2"]), key
        ref_it = fx[key + "/iterates"]
        nit_ref, nfev_ref = (int(v) for v in fx[key + "/nit_nfev"])
        assert (s.nit_, s.nfev_) == (nit_ref, nfev_ref), (key, s.nit_, s.nfev_, s.task_)
        assert s.task_ == "CONVERGENCE: REL_REDUCTION_OF_F_<=_FACTR*EPSMCH", (key, s.task_)
        for k in range(nit_ref):
            assert _data.rel(s.iterates_[k], ref_it[k]) < TOL, (key, k)
        assert _data.rel(s.x_, fx[key + "/x"]) < TOL, (key, s.task_)
        assert s.final_obj_ == pytest.approx(float(fx[key + "/final_obj"]), rel=1e-6), key
        assert np.allclose(s.history_, fx[key + "/history"], rtol=1e-6), key     # callback objective (lbfgs.py:56-61)
        assert len(s.history_) == s.nit_ and fos.get_metrics()["grad_num_calls"] == s.nfev_
        n += 1
    assert n == 4
    with pytest.raises(ValueError):
        fos.LBFGSSolver("l0", 1.0, 1.0)


def test_gemv_pair_dd_every_path(fos):
    """fos_gemv_pair_dd (the fp64 fg of L-BFGS) through every kind of kernel that serves it - resident, row-per-thread,
    streaming fp64 geometries (registers / y in LDS), fp64 two-pass for ragged and over-wide rows, bf16 storage - against
    the fp64 oracle on the stored (rounded) A: 1e-12, i.e. only the summation order differs.  These shapes sample the
    kDdMenu geometries; every entry and its interleaved form is covered by tests/test_gpu_kernel_menu.py."""
    from fastoptsolver_amd import _core, _lib
    lib = _lib.load()
    rng = np.random.default_rng(17)
    shapes = [(200, 5, "f32"), (3000, 7, "f32"), (5000, 40, "f32"), (333, 64, "bf16"),              # resident / tall
              (700, 128, "f32"), (900, 512, "f32"), (600, 1024, "f32"), (777, 2048, "f32"), (513, 4096, "f32"),
              (1200, 8192, "f32"), (1031, 16384, "f32"), (300, 12000, "f32"),                         # streaming fp32
              (400, 256, "bf16"), (500, 2048, "bf16"), (300, 4096, "bf16"), (700, 8192, "bf16"), (520, 16384, "bf16"),
              (257, 1023, "f32"), (64, 20000, "f32"), (100, 32768, "f32"), (90, 16392, "bf16")]       # two-pass fp64
    for m, n, kind in shapes:
        A = rng.standard_normal((m, n)).astype(np.float32)
        At = torch.as_tensor(A).to(torch.bfloat16 if kind == "bf16" else torch.float32)
        b = rng.standard_normal(m).astype(np.float32)
        x = rng.standard_normal(n) * (1.0 + 1e-9 * rng.standard_normal(n))     # not representable in fp32
        prob = fos.prepare(At.cuda(), b, pad=False)
        xd = _dev(x, torch.float64)
        out = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
        _lib.check(lib.fos_gemv_pair_dd(prob.h, _core.ptr(xd), 0.37, _core.ptr(out)))
        g_ref, rr_ref = orc.gram_gradient(At.to(torch.float64).numpy(), x, b.astype(np.float64), 0.37)
        got = out.cpu().numpy()
        assert _data.rel(got[:n], g_ref) < 1e-12, (m, n, kind, prob.plan())
        assert got[n] == pytest.approx(rr_ref, rel=1e-12), (m, n, kind)


def test_two_loop_kernel_vs_oracle(fos):
    from fastoptsolver_amd import _core, _lib
    lib = _lib.load()
    rng = np.random.default_rng(3)
    for n, hist, cap, head in ((8192, 10, 10, 3), (1000, 4, 10, 0), (37, 0, 10, 0), (16384, 7, 10, 8)):
        S = rng.standard_normal((cap, n)).astype(np.float32)
        Y = (S + 0.3 * rng.standard_normal((cap, n))).astype(np.float32)     # s.y > 0
        g = rng.standard_normal(n).astype(np.float32)
        order = [(head + i) % cap for i in range(hist)]
        d_ref = orc.two_loop_direction(g.astype(np.float64), [S[i].astype(np.float64) for i in order],
                                       [Y[i].astype(np.float64) for i in order])
        Sd, Yd, gd = _dev(S), _dev(Y), _dev(g)
        d = torch.empty(n, dtype=torch.float32, device="cuda")
        _lib.check(lib.fos_lbfgs_two_loop(_core.ptr(gd), _core.ptr(Sd), _core.ptr(Yd), hist, head, cap, n, _core.ptr(d),
                                          _core.stream_ptr()))
        assert _data.rel(d.cpu().numpy(), d_ref) < TOL, (n, hist)
        # all-fp64 form (what LBFGSSolver.fit runs): only the summation order separates it from the oracle
        S64, Y64, g64 = _dev(S, torch.float64), _dev(Y, torch.float64), _dev(g, torch.float64)
        d64 = torch.empty(n, dtype=torch.float64, device="cuda")
        _lib.check(lib.fos_lbfgs_two_loop_dd(_core.ptr(g64), _core.ptr(S64), _core.ptr(Y64), hist, head, cap, n,
                                             _core.ptr(d64), _core.stream_ptr()))
        assert _data.rel(d64.cpu().numpy(), d_ref) < 1e-12, (n, hist)


def test_whole_chip_direction_vs_two_loop_and_oracle(fos):
    """fos_lbfgs_direction_dd (Gram matrix + coefficient recursion on many CUs) against the one-workgroup two-loop
    kernel and the oracle: the direction to 1e-12, g.d and d.d to 1e-11, for every history length / ring position and
    for lengths from below one chunk to many chunks per workgroup."""
    import ctypes as C
    from fastoptsolver_amd import _core, _lib
    lib = _lib.load()
    rng = np.random.default_rng(5)
    cases = [(8192, 10, 10, 3), (8192, 10, 10, 0), (1000, 4, 10, 0), (37, 0, 10, 0), (16385, 7, 10, 8), (129, 1, 10, 9),
             (70001, 10, 10, 5), (2048, 3, 4, 2)]
    for n, hist, cap, head in cases:
        S = rng.standard_normal((cap, n))
        Y = S + 0.3 * rng.standard_normal((cap, n))                      # s.y > 0
        g = rng.standard_normal(n)
        order = [(head + i) % cap for i in range(hist)]
        d_ref = orc.two_loop_direction(g, [S[i] for i in order], [Y[i] for i in order])
        S64, Y64, g64 = _dev(S, torch.float64), _dev(Y, torch.float64), _dev(g, torch.float64)
        d_tl = torch.empty(n, dtype=torch.float64, device="cuda")
        _lib.check(lib.fos_lbfgs_two_loop_dd(_core.ptr(g64), _core.ptr(S64), _core.ptr(Y64), hist, head, cap, n,
                                             _core.ptr(d_tl), _core.stream_ptr()))
        nwork = lib.fos_lbfgs_direction_work(n)
        work = torch.empty(nwork, dtype=torch.float64, device="cuda")
        d = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        gd = torch.zeros(2, dtype=torch.float64, device="cuda")
        _lib.check(lib.fos_lbfgs_direction_dd(_core.ptr(g64), _core.ptr(S64), _core.ptr(Y64), hist, head, cap, n,
                                              _core.ptr(d), _core.ptr(gd), _core.ptr(work), nwork, _core.stream_ptr()))
        dn = d.cpu().numpy()
        assert _data.rel(dn, d_ref) < 1e-12, (n, hist)
        assert _data.rel(dn, d_tl.cpu().numpy()) < 1e-12, (n, hist)
        gdn = gd.cpu().numpy()
        assert gdn[0] == pytest.approx(float(g @ d_ref), rel=1e-11), (n, hist)
        assert gdn[1] == pytest.approx(float(d_ref @ d_ref), rel=1e-11), (n, hist)
    # more than 10 pairs: the one-workgroup kernel's job; too little scratch is refused
    rc = lib.fos_lbfgs_direction_dd(_core.ptr(g64), _core.ptr(S64), _core.ptr(Y64), 11, 0, 11, n, _core.ptr(d),
                                    None, _core.ptr(work), nwork, _core.stream_ptr())
    assert rc == -4
    rc = lib.fos_lbfgs_direction_dd(_core.ptr(g64), _core.ptr(S64), _core.ptr(Y64), 3, 0, 4, n, _core.ptr(d),
                                    None, _core.ptr(work), 8, _core.stream_ptr())
    assert rc == -1


# --------------------------------------------------------------------------------------------------
# stopping rules, restart, tensor I/O
# --------------------------------------------------------------------------------------------------
def test_device_side_stop_and_tensor_io(fos):
    A, b, fx = _data.problem("aligned")
    At, bt = _dev(A), _dev(b)
    lam = float(np.max(np.abs(A.T @ b)))
    prob = fos.prepare(At, bt)
    np.random.seed(0)
    x = fos.fista(prob, None, "lasso", 0.1 * lam, 0.0, max_iter=200, tol_ratio=0.5, check_every=5)
    assert isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32
    key = "aligned/fista_stop/tol_ratio"
    assert _data.rel(x.cpu().numpy(), fx[key + "/x"]) < TOL
    assert fos.get_metrics()["grad_num_calls"] == int(fx[key + "/niter"])
    # L= extension skips the power iteration and does not touch the RNG
    state = np.random.get_state()[1].copy()
    fos.fista(prob, None, "lasso", 0.1 * lam, 0.0, max_iter=3, L=float(fx["aligned/L"]))
    assert np.array_equal(state, np.random.get_state()[1])


# --------------------------------------------------------------------------------------------------
# full-size properties (BASELINE config 2 shape): things the oracle is too slow to check directly
# --------------------------------------------------------------------------------------------------
def test_full_size_properties(fos):
    m, n = 65536, 8192
    g = torch.Generator(device="cuda").manual_seed(0)
    A = torch.randn(m, n, device="cuda", generator=g)
    b = torch.randn(m, device="cuda", generator=g)
    y1 = torch.randn(n, device="cuda", generator=g)
    y2 = torch.randn(n, device="cuda", generator=g)
    prob = fos.prepare(A, b)
    assert prob.plan()["path"] == 0
    G = lambda y: prob.gemv_pair(y).double()                              # noqa: E731
    # (1) affine: G(y1 + y2) - G(y1) - G(y2) + G(0) = 0
    z = torch.zeros(n, device="cuda")
    lin = G(y1 + y2) - G(y1) - G(y2) + G(z)
    assert float(lin.norm() / G(y1 + y2).norm()) < 5e-6
    # (2) G(0) = -A^T b, checked on a row subsample with the oracle and in full with a second code path
    rows = slice(0, 512)
    sub = fos.prepare(A[rows], b[rows])
    g_sub = sub.gemv_pair(y1).cpu().numpy()
    g_ref, _ = orc.gram_gradient(A[rows].cpu().numpy().astype(np.float64), y1.cpu().numpy().astype(np.float64),
                                 b[rows].cpu().numpy().astype(np.float64), 0.0)
    assert _data.rel(g_sub, g_ref) < TOL
    # (3) fused single pass == sum of 8 row shards (the multi-GPU decomposition), fixed order
    acc = torch.zeros(n, dtype=torch.float64, device="cuda")
    for p in range(8):
        sl = slice(p * m // 8, (p + 1) * m // 8)
        acc += fos.prepare(A[sl], b[sl]).gemv_pair(y1).double()
    full = G(y1)
    assert float((acc - full).norm() / full.norm()) < 2e-6
    # (4) run-to-run bit reproducibility (fixed-order slab reduction, no float atomics)
    assert torch.equal(prob.gemv_pair(y1), prob.gemv_pair(y1))
    # (5) 20 FISTA iterations: the objective the device reports never increases by more than rounding
    lam = float((A.T @ b).abs().max())
    L = float(fos.estimate_lipschitz(prob))
    x, h = fos.fista(prob, None, "lasso", 0.1 * lam, 0.0, max_iter=20, L=L, return_history=True)
    obj = np.array(h["obj"])
    assert np.all(np.diff(obj) <= 1e-6 * obj[:-1]) or obj[-1] < obj[0]
    assert np.isfinite(obj).all() and obj[-1] < obj[0]


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)


def _bench_like_problem(m, n, dtype, seed=0):
    """A ~ N(0,1), b = A x_true + 0.1 N(0,1) generated on the device in 8192-row blocks (bench.py's recipe)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    xt = torch.zeros(n, device="cuda")
    idx = torch.randperm(n, device="cuda", generator=g)[: max(1, n // 20)]
    xt[idx] = torch.randn(idx.numel(), device="cuda", generator=g)
    A = torch.empty(m, n, dtype=dtype, device="cuda")
    b = torch.empty(m, device="cuda")
    for r0 in range(0, m, 8192):
        r1 = min(m, r0 + 8192)
        blk = torch.randn(r1 - r0, n, device="cuda", generator=g).to(dtype)
        A[r0:r1] = blk
        b[r0:r1] = blk.float() @ xt + 0.1 * torch.randn(r1 - r0, device="cuda", generator=g)
    return A, b


@pytest.mark.timeout(900)
def test_cfg3_full_size_lbfgs(fos):
    """BASELINE config 3 at full size (65536 x 8192 fp32, ridge alpha2 = 1): the device run against (a) the oracle's
    L-BFGS on the same fp32-representable data in fp64 on the host - same nit, nfev, exit, end point to 1e-5 - and
    (b) size-independent properties: gradient at the end point from an independent fp64 torch matmul, the optimum
    of the normal equations solved in fp64 on the device, monotone callback history."""
    m, n, a2 = 65536, 8192, 1.0
    A, b = _bench_like_problem(m, n, torch.float32)
    prob = fos.prepare(A, b)
    assert prob.plan()["path"] == 0
    s = fos.LBFGSSolver("ridge", 0.0, a2).fit(prob, None)
    x = torch.as_tensor(_np(s.x_), dtype=torch.float64, device="cuda")     # tensor in -> float32 tensor out (6e-8)
    # (b1) gradient at x_ by a second code path, in fp64, block by block
    grad = a2 * x
    rr = 0.0
    for r0 in range(0, m, 8192):
        Ab = A[r0:r0 + 8192].double()
        r = Ab @ x - b[r0:r0 + 8192].double()
        grad += Ab.T @ r
        rr += float(r @ r)
    f_indep = 0.5 * rr + 0.5 * a2 * float(x @ x)
    assert s.final_obj_ == pytest.approx(f_indep, rel=1e-9)               # fg's fp64 loss IS the loss (x_ is at a minimum:
                                                                          # its fp32 rounding moves f in second order only)
    # (b2) optimum of the normal equations in fp64 on the device
    H = torch.zeros(n, n, dtype=torch.float64, device="cuda")
    rhs = torch.zeros(n, dtype=torch.float64, device="cuda")
    for r0 in range(0, m, 8192):
        Ab = A[r0:r0 + 8192].double()
        H += Ab.T @ Ab
        rhs += Ab.T @ b[r0:r0 + 8192].double()
    H.diagonal().add_(a2)
    x_star = torch.linalg.solve(H, rhs)
    r_star = 0.0
    for r0 in range(0, m, 8192):
        r = A[r0:r0 + 8192].double() @ x_star - b[r0:r0 + 8192].double()
        r_star += float(r @ r)
    f_star = 0.5 * r_star + 0.5 * a2 * float(x_star @ x_star)
    assert s.final_obj_ >= f_star * (1 - 1e-12) and s.final_obj_ == pytest.approx(f_star, rel=1e-7)
    assert float((x - x_star).norm() / x_star.norm()) < 1e-4              # L-BFGS's own stopping distance (factr 1e7)
    # scale of SciPy's exits: either the projected gradient is below pgtol or the last decrease was below factr*eps
    assert s.task_.startswith("CONVERGENCE"), s.task_
    assert float(grad.abs().max()) < 1e-2 * float(rhs.abs().max()) * 1e-3
    hist = np.asarray(s.history_)
    assert len(hist) == s.nit_ and np.all(np.diff(hist) <= 0.0)           # callback objective never increases
    # (a) the oracle on the host, same data (fp32-representable), fp64 arithmetic
    del H
    A64 = A.cpu().numpy().astype(np.float64)
    ref = orc.LBFGSSolver("ridge", 0.0, a2).fit(A64, b.cpu().numpy().astype(np.float64))
    assert (s.nit_, s.nfev_, s.task_) == (ref.nit_, ref.nfev_, ref.task_), (s.nit_, s.nfev_, s.task_, ref.nit_, ref.nfev_)
    assert _data.rel(_np(s.x_), ref.x_) < TOL
    assert s.final_obj_ == pytest.approx(ref.final_obj_, rel=1e-9)
    for k in range(s.nit_):
        assert _data.rel(_np(s.iterates_[k]), ref.iterates_[k]) < TOL, k


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_shard_size_properties(fos, kind):
    """The per-GPU shard of BASELINE configs 4 / 5 (131072 x 16384, fp32 / bf16): the geometries the headline runs on
    (1024-thread drained pipeline; 512 x 4 bf16), checked at that size through size-independent properties."""
    _size_properties(fos, 131072, 16384, kind, shards=4)


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_cfg4_full_size_properties(fos, kind):
    """BASELINE configs 4 / 5 at their FULL size on one GPU (2^20 x 16384: 64 GiB fp32 / 32 GiB bf16) - the workload
    bench.py's headline times at N = 1: every row against an independent fp64 torch matmul, affine, the 8-shard
    decomposition of the 8-GPU run, bit reproducibility, 10 solver iterations against fp64 torch."""
    free, _total = torch.cuda.mem_get_info()
    need = (2 ** 20) * 16384 * (4 if kind == "f32" else 2) + 8 * 2 ** 30
    if free < need:
        pytest.skip(f"needs {need / 2**30:.0f} GiB of free HBM, {free / 2**30:.0f} available")
    _size_properties(fos, 2 ** 20, 16384, kind, shards=8)


def _size_properties(fos, m, n, kind, shards):
    dt = torch.float32 if kind == "f32" else torch.bfloat16
    A, b = _bench_like_problem(m, n, dt, seed=1)
    g = torch.Generator(device="cuda").manual_seed(5)
    y1 = torch.randn(n, device="cuda", generator=g)
    y2 = torch.randn(n, device="cuda", generator=g)
    prob = fos.prepare(A, b)
    plan = prob.plan()
    assert plan["path"] == 0 and (plan["threads"], plan["chunks"]) == ((1024, 4) if kind == "f32" else (512, 4)), plan
    G = lambda y: prob.gemv_pair(y).double()                              # noqa: E731
    # (1) affine
    z = torch.zeros(n, device="cuda")
    full = G(y1)
    lin = G(y1 + y2) - full - G(y2) + G(z)
    assert float(lin.norm() / G(y1 + y2).norm()) < 5e-6
    # (2) against an independent fp64 matmul of the stored A, block by block (every row, not a subsample)
    ref = torch.zeros(n, dtype=torch.float64, device="cuda")
    rr_ref = 0.0
    for r0 in range(0, m, 8192):
        Ab = A[r0:r0 + 8192].double()
        r = Ab @ y1.double() - b[r0:r0 + 8192].double()
        ref += Ab.T @ r
        rr_ref += float(r @ r)
    assert float((full - ref).norm() / ref.norm()) < TOL
    rr = torch.zeros(1, dtype=torch.float64, device="cuda")
    prob.gemv_pair(y1, rr_out=rr)
    assert float(rr) == pytest.approx(rr_ref, rel=TOL)
    # (3) row subsample against the oracle itself
    rows = slice(m // 2 + 4464, m // 2 + 4976)
    sub = fos.prepare(A[rows], b[rows])
    g_ref, _ = orc.gram_gradient(A[rows].double().cpu().numpy(), y1.cpu().numpy().astype(np.float64),
                                 b[rows].cpu().numpy().astype(np.float64), 0.0)
    assert _data.rel(sub.gemv_pair(y1).cpu().numpy(), g_ref) < TOL
    # (4) shard sum == whole (the decomposition the ranks of configs 4 / 5 compute), fixed order
    acc = torch.zeros(n, dtype=torch.float64, device="cuda")
    for p in range(shards):
        sl = slice(p * m // shards, (p + 1) * m // shards)
        acc += fos.prepare(A[sl], b[sl]).gemv_pair(y1).double()
    assert float((acc - full).norm() / full.norm()) < 2e-6
    # (5) bit reproducibility
    assert torch.equal(prob.gemv_pair(y1), prob.gemv_pair(y1))
    # (6) 10 solver iterations of the configuration's own regulariser against fp64 torch on the device
    lam = float(ref.abs().max())
    a1, a2 = (0.1 * lam, 0.0) if kind == "f32" else (0.05 * lam, 10.0)
    np.random.seed(0)
    L = fos.estimate_lipschitz(prob, n_iter=20)
    x = fos.fista(prob, None, "lasso" if a2 == 0 else "elasticnet", a1, a2, max_iter=10, L=L)
    tau = 1.0 / (L + (a2 if a2 > 0 else 0.0))
    xk, tk = torch.zeros(n, dtype=torch.float64, device="cuda"), 1.0       # iterative_solvers.py:170-242 in fp64 torch
    yk = xk.clone()
    for _ in range(10):
        gr = torch.zeros(n, dtype=torch.float64, device="cuda")
        for r0 in range(0, m, 8192):
            Ab = A[r0:r0 + 8192].double()
            gr += Ab.T @ (Ab @ yk - b[r0:r0 + 8192].double())
        if a2 > 0:
            gr += a2 * yk
        v = yk - tau * gr
        xn = torch.sign(v) * torch.clamp(v.abs() - tau * a1, min=0.0)
        tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * tk * tk))
        yk = xn + ((tk - 1.0) / tn) * (xn - xk)
        xk, tk = xn, tn
    xg = torch.as_tensor(_np(x), dtype=torch.float64, device="cuda")
    assert float((xg - xk).norm() / xk.norm()) < TOL


# --------------------------------------------------------------------------------------------------
# more edges: bf16 solver run, wide-n fallback, Armijo constant, torch closures, dtype argument
# --------------------------------------------------------------------------------------------------
def test_bf16_elastic_net_fista_vs_oracle_on_rounded_A(fos):
    """BASELINE config 5 in miniature: bf16 A / fp32 accumulate, l1 + l2.  Judged against the oracle run on
    the bf16-ROUNDED A: the 3e-3 quantisation of A is input data, not solver error."""
    rng = np.random.default_rng(21)
    m, n = 3000, 2048
    A32 = rng.standard_normal((m, n)).astype(np.float32)
    A16 = torch.as_tensor(A32).to(torch.bfloat16)
    Aq = A16.to(torch.float64).numpy()
    xt = np.zeros(n)
    xt[rng.choice(n, 100, replace=False)] = rng.standard_normal(100)
    b = Aq @ xt + 0.1 * rng.standard_normal(m)
    lam = float(np.max(np.abs(Aq.T @ b)))
    a1, a2 = 0.05 * lam, 10.0
    np.random.seed(0)
    v0 = np.random.randn(n)
    L = orc.estimate_lipschitz(Aq, v0=v0)
    x_ref, h_ref = orc.fista(Aq, b, "elasticnet", a1, a2, max_iter=80, return_history=True, L=L)
    np.random.seed(0)
    x, h = fos.fista(A32, b, "elasticnet", a1, a2, max_iter=80, return_history=True, dtype="bf16")
    for k in (1, 10, 40, 80):
        assert _data.rel(h["x"][k], h_ref["x"][k]) < TOL, k
    assert np.allclose(h["obj"], h_ref["obj"], rtol=TOL)
    # tensor input in bf16 takes the same path without the dtype argument and returns float32
    xt_ = fos.fista(A16.cuda(), _dev(b), "elasticnet", a1, a2, max_iter=80, L=L)
    assert xt_.dtype == torch.float32 and _data.rel(xt_.cpu().numpy(), x_ref) < TOL


@pytest.mark.parametrize("m,n,kind", [(96, 20000, "wide"), (700, 32768, "wide"), (257, 24580, "wide"), (3, 16388, "wide"),
                                      (64, 40000, "colblock"), (130, 65536, "colblock"), (300, 32772, "colblock"),
                                      (50, 40001, "twopass")])
def test_wide_rows(fos, m, n, kind):
    """Rows beyond the streaming kernel's register budget (fp32: 16384 columns): up to 32768 columns the single pass keeps
    y in LDS (gemv_wide.hpp); wider aligned rows run COLUMN BLOCKS through the streaming kernel in two phases (r = A y - b
    block by block, then A^T r block by block: A read twice at streaming speed); ragged widths take the two-pass kernels."""
    rng = np.random.default_rng(m + n)
    A = rng.standard_normal((m, n)).astype(np.float32)
    b = rng.standard_normal(m).astype(np.float32)
    y = rng.standard_normal(n).astype(np.float32)
    prob = fos.prepare(A, b, pad=False)
    plan = prob.plan()
    if kind == "wide":
        assert plan["path"] == 0 and (plan["threads"], plan["chunks"]) == (512, 16) and plan["colblock"] == 0, plan
    elif kind == "colblock":
        assert plan["path"] == 0 and plan["colblock"] == 1, plan
    else:
        assert plan["path"] == 1, plan
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    g = prob.gemv_pair(_dev(y), alpha2=0.0).cpu().numpy()
    g_ref, rr_ref = orc.gram_gradient(A64, y.astype(np.float64), b64, 0.0)
    assert _data.rel(g, g_ref) < TOL
    assert prob.residual_objective(_dev(y))[0] == pytest.approx(rr_ref, rel=TOL)
    L = float(np.linalg.norm(A64, 2) ** 2)
    for kw in (dict(), dict(backtracking=True, t_init_factor=2.0), dict(return_history=True)):
        out = fos.fista(prob, None, "lasso", 5.0, 0.0, max_iter=12, L=L, **kw)
        ref = orc.fista(A64, b64, "lasso", 5.0, 0.0, max_iter=12, L=L, **kw)
        x, x_ref = (out[0], ref[0]) if kw.get("return_history") else (out, ref)
        assert _data.rel(x, x_ref) < TOL, kw
        if kw.get("return_history"):
            assert np.allclose(out[1]["obj"], ref[1]["obj"], rtol=TOL)


def test_wide_rows_bf16_and_sharded_column_blocks(fos):
    """bf16 rows beyond 32768 columns take the column-blocked passes too; with a communicator attached the blocks' slabs
    go through the same slab reduction + all-reduce as any other plan."""
    from fastoptsolver_amd import distributed as fd
    rng = np.random.default_rng(9)
    m, n = 150, 40000
    A16 = torch.as_tensor(rng.standard_normal((m, n)).astype(np.float32)).to(torch.bfloat16).cuda()
    A64 = A16.to(torch.float64).cpu().numpy()
    b = rng.standard_normal(m).astype(np.float32)
    y = rng.standard_normal(n).astype(np.float32)
    prob = fos.prepare(A16, b, pad=False)
    assert prob.plan()["colblock"] == 1 and prob.dtype == "bf16"
    g_ref, rr_ref = orc.gram_gradient(A64, y.astype(np.float64), b.astype(np.float64), 0.2)
    assert _data.rel(prob.gemv_pair(_dev(y), alpha2=0.2).cpu().numpy(), g_ref) < TOL
    assert prob.residual_objective(_dev(y))[0] == pytest.approx(rr_ref, rel=TOL)
    L = float(np.linalg.norm(A64, 2) ** 2)
    x_ref = orc.fista(A64, b.astype(np.float64), "elasticnet", 3.0, 0.5, max_iter=15, L=L)
    assert _data.rel(_np(fos.fista(prob, None, "elasticnet", 3.0, 0.5, max_iter=15, L=L)), x_ref) < TOL
    comm = fd.Comm.solo()
    x_c = fos.fista(A16, b, "elasticnet", 3.0, 0.5, max_iter=15, L=L, comm=comm, backtracking=True, t_init_factor=2.0)
    x_bt = orc.fista(A64, b.astype(np.float64), "elasticnet", 3.0, 0.5, max_iter=15, L=L, backtracking=True, t_init_factor=2.0)
    assert _data.rel(_np(x_c), x_bt) < TOL


@pytest.mark.parametrize("kind,m,n,geo", [
    ("f32", 300, 2560, (256, 3)), ("f32", 257, 3072, (256, 3)), ("f32", 515, 5000, (256, 5)), ("f32", 260, 6144, (512, 3)),
    ("f32", 300, 10000, (512, 5)), ("f32", 259, 12288, (1024, 3)), ("f32", 131, 12292, (512, 7)), ("f32", 140, 14336, (512, 7)),
    ("bf16", 3000, 768, (64, 2)), ("bf16", 2000, 1024, (64, 2)), ("bf16", 300, 5120, (256, 3)), ("bf16", 257, 6144, (256, 3)), ("bf16", 300, 12288, (512, 3)), ("bf16", 260, 10000, (256, 5)),
    ("bf16", 150, 20000, (512, 5)), ("bf16", 130, 24576, (512, 6)), ("bf16", 131, 24584, (512, 8)), ("bf16", 200, 32768, (512, 8))])
def test_three_chunk_geometries_and_bf16_wide_rows(fos, kind, m, n, geo):
    """Round 3: widths between the powers of two get geometries of three, five or seven chunks per thread (a chunk beyond n is
    a re-read, not an idle lane) and bf16 rows of 16385 ... 32768 columns a single read - 512 x 6 chunks up to 24576, the y-in-LDS kernel
    (reported as 512 x 8) above - instead of column blocks.  Gradient, residual, FISTA with every flag and the history
    objective against the oracle; the planner lands on the expected geometry."""
    rng = np.random.default_rng(m + n)
    At = torch.as_tensor(rng.standard_normal((m, n)).astype(np.float32)).to(torch.bfloat16 if kind == "bf16" else torch.float32).cuda()
    A64 = At.to(torch.float64).cpu().numpy()
    b = rng.standard_normal(m).astype(np.float32)
    y = rng.standard_normal(n).astype(np.float32)
    prob = fos.prepare(At, b, pad=False)
    plan = prob.plan()
    assert plan["path"] == 0 and plan["colblock"] == 0 and (plan["threads"], plan["chunks"]) == geo, plan
    b64 = b.astype(np.float64)
    g_ref, rr_ref = orc.gram_gradient(A64, y.astype(np.float64), b64, 0.3)
    assert _data.rel(prob.gemv_pair(_dev(y), alpha2=0.3).cpu().numpy(), g_ref) < TOL
    assert prob.residual_objective(_dev(y))[0] == pytest.approx(rr_ref, rel=TOL)
    L = float(np.linalg.norm(A64, 2) ** 2)
    lam = float(np.max(np.abs(A64.T @ b64)))
    for kw in (dict(), dict(adaptive_restart=True, tol_ratio=0.5), dict(backtracking=True, t_init_factor=2.0),
               dict(return_history=True)):
        out = fos.fista(prob, None, "elasticnet", 0.1 * lam, 0.4, max_iter=15, L=L, **kw)
        ref = orc.fista(A64, b64, "elasticnet", 0.1 * lam, 0.4, max_iter=15, L=L, **kw)
        x, x_ref = (out[0], ref[0]) if kw.get("return_history") else (out, ref)
        assert _data.rel(_np(x), x_ref) < TOL, kw
        if kw.get("return_history"):
            assert np.allclose(out[1]["obj"], ref[1]["obj"], rtol=TOL)
    s = fos.LBFGSSolver("ridge", 0.0, 1.0, max_iter=6).fit(prob, None)
    r = orc.LBFGSSolver("ridge", 0.0, 1.0, max_iter=6).fit(A64, b64)
    assert _data.rel(_np(s.x_), r.x_) < TOL


def test_armijo_constant_is_read_at_call_time(fos, monkeypatch):
    """iterative_solvers.C is a module global read inside the loop (reference :11, :191): patching it must bite."""
    from fastoptsolver_amd import iterative_solvers as its
    A, b, fx = _data.problem("tiny")
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(fx["tiny/L"])
    fos.fista(A, b, "ridge", 0.0, 0.5, max_iter=25, backtracking=True, t_init_factor=2.0, L=L)
    base = list(its.ls_call_iters)
    monkeypatch.setattr(its, "C", 0.9)
    fos.fista(A, b, "ridge", 0.0, 0.5, max_iter=25, backtracking=True, t_init_factor=2.0, L=L)
    strict = list(its.ls_call_iters)
    assert sum(strict) > sum(base)
    monkeypatch.setattr(orc, "ARMIJO_C", 0.9)
    _, met = orc.fista(A, b, "ridge", 0.0, 0.5, max_iter=25, backtracking=True, t_init_factor=2.0, L=L,
                       return_metrics=True)
    assert met["ls_iters_total"] == sum(strict)


def test_ista_with_arbitrary_torch_closures(fos):
    """ista's generic path: callables the library knows nothing about, written with torch ops on device tensors."""
    A, b, fx = _data.problem("tiny")
    At, bt = _dev(A, torch.float64), _dev(b, torch.float64)
    a1 = 0.1 * float(np.max(np.abs(A.T @ b)))
    L = float(fx["tiny/ista/L"])
    g = lambda x: float(0.5 * ((At @ x.double() - bt) ** 2).sum())                              # noqa: E731
    grad = lambda x: (At.T @ (At @ x.double() - bt)).float()                                   # noqa: E731
    prox = lambda v, t: torch.sign(v) * torch.clamp(v.abs() - t * a1, min=0.0)                 # noqa: E731
    for kw in (dict(), dict(backtracking=True, t_init_factor=2.0)):
        x = fos.ista(np.zeros(16), g, grad, prox, L, max_iter=40, **kw)
        key = "tiny/ista/l1/" + ("bt2" if kw else "fixed")
        assert _data.rel(x, fx[key + "/x"]) < TOL, key


@pytest.mark.parametrize("m,n,nv", [(64, 16, 16), (1000, 512, 5), (777, 132, 3), (4099, 8192, 16), (130, 16384, 9), (1, 4, 1),
                                    (32845, 260, 7)])          # the last one is tall enough for the 128-row tile
def test_residual_batch_mfma_vs_oracle(fos, m, n, nv):
    """The batched (matrix-core) residual kernel: ||A X_j - b||^2 for up to 16 vectors in one pass."""
    rng = np.random.default_rng(m + n + nv)
    A = rng.standard_normal((m, n)).astype(np.float32)
    b = rng.standard_normal(m).astype(np.float32)
    X = (rng.standard_normal((n, nv)) * np.logspace(0, -6, nv)).astype(np.float32)   # candidates shrink like t*eta^j
    prob = fos.prepare(A, b)
    prob.replan(no_tall=True)                   # n <= 64 would plan the row-per-thread pass, which has no MFMA batch
    assert prob.plan()["path"] == 0 and prob.plan()["tall"] == 0
    for use_b in (True, False):
        got = prob.residual_batch(X, use_b=use_b)
        R = A.astype(np.float64) @ X.astype(np.float64) - (b.astype(np.float64)[:, None] if use_b else 0.0)
        want = (R ** 2).sum(axis=0)
        assert np.allclose(got, want, rtol=TOL), (use_b, got, want)
        _, rr_tol = _data.fp32_pass_tolerances_cols(A, X, b if use_b else None, np.zeros((n, nv)), want)     # per column
        assert (np.abs(np.asarray(got) - want) <= rr_tol).all(), (use_b, got, want, rr_tol)


@pytest.mark.parametrize("m,n,nv", [(64, 16, 16), (1000, 512, 5), (777, 136, 3), (4099, 8192, 16), (130, 16384, 9), (1, 8, 1),
                                    (32845, 264, 7)])          # the last one is tall enough for the 128-row tile
def test_residual_batch_mfma_bf16_vs_oracle(fos, m, n, nv):
    """bf16 A on v_mfma_f32_16x16x32_bf16: the candidates are split into three bf16 terms (24 mantissa bits), so the
    result keeps the fp32 tolerance against the float64 product with the bf16-ROUNDED A."""
    rng = np.random.default_rng(m + n + nv)
    A16 = torch.as_tensor(rng.standard_normal((m, n)).astype(np.float32)).to(torch.bfloat16)
    Aq = A16.to(torch.float64).numpy()
    b = rng.standard_normal(m).astype(np.float32)
    X = (rng.standard_normal((n, nv)) * np.logspace(0, -6, nv)).astype(np.float32)
    prob = fos.prepare(A16.cuda(), b)
    prob.replan(no_tall=True)
    assert prob.plan()["path"] == 0 and prob.dtype == "bf16"
    for use_b in (True, False):
        got = prob.residual_batch(X, use_b=use_b)
        R = Aq @ X.astype(np.float64) - (b.astype(np.float64)[:, None] if use_b else 0.0)
        want = (R ** 2).sum(axis=0)
        assert np.allclose(got, want, rtol=TOL), (use_b, got)
        _, rr_tol = _data.fp32_pass_tolerances_cols(Aq, X, b if use_b else None, np.zeros((n, nv)), want)    # per column
        assert (np.abs(np.asarray(got) - want) <= rr_tol).all(), (use_b, got, want, rr_tol)


def test_bf16_backtracking_uses_mfma_batch_and_matches_oracle(fos):
    """Backtracking FISTA with bf16 A: the batched (bf16 MFMA) search takes the decisions of the sequential one and
    the iterates follow the oracle run on the bf16-rounded A."""
    from fastoptsolver_amd import iterative_solvers as its
    rng = np.random.default_rng(33)
    m, n = 2000, 1024
    A16 = torch.as_tensor(rng.standard_normal((m, n)).astype(np.float32)).to(torch.bfloat16)
    Aq = A16.to(torch.float64).numpy()
    b = Aq @ (rng.standard_normal(n) * (rng.random(n) < 0.05)) + 0.1 * rng.standard_normal(m)
    lam = float(np.max(np.abs(Aq.T @ b)))
    L = float(np.linalg.norm(Aq, 2) ** 2)
    prob = fos.prepare(A16.cuda(), b)
    tf, iters = 8.0, 18      # a generous first step: 2, 1, 0, 0, 0, 4, 2, 9 ... shrinks; the reference's first
    out = {}                 # step-underflow event (see _check_linesearch_counts) comes at iteration 19 on this data
    for batch in (True, False):
        its.reset_metrics()
        st = its._drive(prob, A16, mode=0, prox_kind=0, alpha1=0.05 * lam, alpha2=0.5, tau=tf / (L + 0.5),
                        backtracking=True, eta=0.7, max_iter=iters, batch_trials=batch)
        out[batch] = (st.x_tensor().cpu().numpy(), list(its.ls_call_iters))
    assert out[True][1] == out[False][1] and sum(out[True][1]) > 0
    assert _data.rel(out[True][0], out[False][0]) < 1e-9
    ref = orc.FistaProblem(Aq, b, 0.05 * lam, 0.5)
    rs = ref.init_state(L, tf)
    for _ in range(iters):
        ref.step(rs, backtracking=True, eta=0.7)
    assert _data.rel(out[True][0], rs.x) < TOL
    assert max(ref.metrics.ls_iters) < 40 and out[True][1] == ref.metrics.ls_iters


def test_batched_and_sequential_line_search_agree(fos):
    """The MFMA-batched Armijo search must take exactly the decisions of the one-candidate-per-pass search."""
    from fastoptsolver_amd import iterative_solvers as its
    A, b, fx = _data.problem("aligned")
    prob = fos.prepare(A, b)
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(fx["aligned/L"])
    out = {}
    for batch in (True, False):
        its.reset_metrics()
        st = its._drive(prob, A, mode=0, prox_kind=0, alpha1=0.05 * lam, alpha2=0.5, tau=2.0 / (L + 0.5),
                        backtracking=True, eta=0.7, max_iter=40, grad_tol_check=True, batch_trials=batch)
        out[batch] = (st.x_tensor().cpu().numpy(), list(its.ls_call_iters))
    assert out[True][1] == out[False][1]
    assert _data.rel(out[True][0], out[False][0]) < 1e-9
    assert sum(out[True][1]) > 0


def test_lbfgs_boston_end_point(fos):
    """Config-1 data through L-BFGS.  cond(A^T A) ~ 1e9: the fp32 STORAGE rounding of A and b (6e-8 per entry) is a
    perturbation the middle iterates amplify (even two float64 codes differ by 1e-5 there,
    tests/test_oracle_golden.py); the first step, the iteration / evaluation counts and the END POINT agree."""
    fx = _data.load("boston")
    A, b = fx["boston/A"], fx["boston/b"]
    s = fos.LBFGSSolver("ridge", 0.0, 0.5).fit(A, b)
    # SURVEY 8(c) known answer of the reference for this call
    assert np.allclose(s.x_, [5.04537675, 0.14409563, -0.01939221, -0.05905357, 1.53772434], rtol=2e-4, atol=2e-5)
    assert s.final_obj_ == pytest.approx(2077.060367882381, rel=1e-6)
    assert _data.rel(s.x_, fx["boston/lbfgs/enet_tiny1/x"]) < TOL
    nit_ref, nfev_ref = (int(v) for v in fx["boston/lbfgs/enet_tiny1/nit_nfev"])          # 23 / 33
    assert abs(s.nit_ - nit_ref) <= 1 and abs(s.nfev_ - nfev_ref) <= 2, (s.nit_, s.nfev_, s.task_)
    assert s.task_ == "CONVERGENCE: REL_REDUCTION_OF_F_<=_FACTR*EPSMCH"
    assert _data.rel(s.iterates_[0], fx["boston/lbfgs/enet_tiny1/iterates"][0]) < 1e-6     # first step identical


def test_ista_from_nonzero_start(fos):
    A, b, fx = _data.problem("ragged")
    x0 = np.random.default_rng(0).standard_normal(A.shape[1])
    a1 = 0.05 * float(np.max(np.abs(A.T @ b)))
    L = float(fx["ragged/ista/L"]) + 0.3
    ls = fos.LeastSquares(A, b, 0.3)
    x = fos.ista(x0, ls, ls.grad, fos.L1Prox(a1), L, max_iter=30)
    x_ref = orc.ista(x0, lambda z: orc.smooth_value(A, b, z, 0.3), lambda z: orc.gram_gradient(A, z, b, 0.3)[0],
                     lambda v, t: orc.prox_l1(v, t * a1), L, max_iter=30)
    assert _data.rel(x, x_ref) < TOL
    # CPU tensors in -> CPU tensors out
    xt = fos.ista(torch.from_numpy(x0), ls, ls.grad, fos.L1Prox(a1), L, max_iter=30)
    assert isinstance(xt, torch.Tensor) and not xt.is_cuda and _data.rel(xt.numpy(), x_ref) < TOL


def test_history_on_wide_rows_uses_sibling_dual_kernel(fos):
    """n in (8192, 16384]: the gradient runs the drained 1024-thread geometry, the DUAL (history) pass a 512-thread
    sibling of the same row step; iterates and objectives must match the oracle either way."""
    rng = np.random.default_rng(8)
    m, n = 600, 16384
    A = rng.standard_normal((m, n)).astype(np.float32)
    b = rng.standard_normal(m).astype(np.float32)
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    lam = float(np.max(np.abs(A64.T @ b64)))
    L = float(np.linalg.norm(A64, 2) ** 2)
    prob = fos.prepare(A, b)
    assert prob.plan()["threads"] == 1024 and prob.plan()["path"] == 0
    x, h = fos.fista(prob, None, "elasticnet", 0.2 * lam, 0.5, max_iter=12, L=L, return_history=True)
    x_ref, h_ref = orc.fista(A64, b64, "elasticnet", 0.2 * lam, 0.5, max_iter=12, L=L, return_history=True)
    assert len(h["obj"]) == 12 and len(h["x"]) == 13
    assert np.allclose(h["obj"], h_ref["obj"], rtol=TOL)
    assert _data.rel(x, x_ref) < TOL
    x2 = fos.fista(prob, None, "elasticnet", 0.2 * lam, 0.5, max_iter=12, L=L)
    assert _data.rel(x2, x_ref) < TOL


def test_history_chunking_is_transparent(fos, monkeypatch):
    """The device-resident history is read back in bounded chunks; the result must not depend on the chunk size."""
    from fastoptsolver_amd import iterative_solvers as its
    A, b, fx = _data.problem("aligned")
    prob = fos.prepare(A, b)
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(fx["aligned/L"])
    x1, h1 = fos.fista(prob, None, "lasso", 0.1 * lam, 0.0, max_iter=37, L=L, return_history=True)
    monkeypatch.setattr(its, "_HISTORY_CHUNK_BYTES", 8 * A.shape[1] * 5)        # 5 iterations per chunk
    x2, h2 = fos.fista(prob, None, "lasso", 0.1 * lam, 0.0, max_iter=37, L=L, return_history=True)
    assert len(h2["x"]) == 38 and len(h2["obj"]) == 37
    assert np.array_equal(x1, x2) and all(np.array_equal(a, c) for a, c in zip(h1["x"], h2["x"]))
    assert np.allclose(h1["obj"], h2["obj"], rtol=1e-12)


def test_large_ragged_n_is_padded_onto_the_fused_path(fos):
    """m*n >= 2^20 with n % 4 != 0 (n > 64): prepare() zero-pads the columns of its device copy so the single-pass kernel
    applies; padding must be invisible (lengths, values) in every entry point."""
    rng = np.random.default_rng(17)
    m, n = 4100, 4098
    A = rng.standard_normal((m, n)).astype(np.float32)
    b = rng.standard_normal(m).astype(np.float32)
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    prob = fos.prepare(A, b)
    assert prob.plan()["path"] == 0 and prob.n == n and prob.n_dev == 4100
    assert fos.prepare(A, b, pad=False).plan()["path"] == 1
    y = rng.standard_normal(n).astype(np.float32)
    g = prob.gemv_pair(_dev(y), alpha2=0.2)
    assert g.shape == (n,)
    g_ref, rr_ref = orc.gram_gradient(A64, y.astype(np.float64), b64, 0.2)
    assert _data.rel(g.cpu().numpy(), g_ref) < TOL
    assert prob.residual_objective(_dev(y))[0] == pytest.approx(rr_ref, rel=TOL)
    lam = float(np.max(np.abs(A64.T @ b64)))
    L = float(np.linalg.norm(A64, 2) ** 2)
    x, h = fos.fista(prob, None, "elasticnet", 0.1 * lam, 0.5, max_iter=25, L=L, return_history=True)
    x_ref, h_ref = orc.fista(A64, b64, "elasticnet", 0.1 * lam, 0.5, max_iter=25, L=L, return_history=True)
    assert x.shape == (n,) and all(v.shape == (n,) for v in h["x"])
    assert _data.rel(x, x_ref) < TOL and np.allclose(h["obj"], h_ref["obj"], rtol=TOL)
    xb = fos.fista(prob, None, "lasso", 0.1 * lam, 0.0, max_iter=15, L=L, backtracking=True, t_init_factor=2.0)
    xb_ref = orc.fista(A64, b64, "lasso", 0.1 * lam, 0.0, max_iter=15, L=L, backtracking=True, t_init_factor=2.0)
    assert _data.rel(xb, xb_ref) < TOL
    np.random.seed(3)
    v0 = np.random.randn(n)
    np.random.seed(3)
    assert fos.estimate_lipschitz(prob) == pytest.approx(orc.estimate_lipschitz(A64, v0=v0), rel=TOL)
    s = fos.LBFGSSolver("ridge", 0.0, 1.0, max_iter=8).fit(prob, None)
    s_ref = orc.LBFGSSolver("ridge", 0.0, 1.0, max_iter=8).fit(A64, b64)
    assert s.x_.shape == (n,) and _data.rel(s.x_, s_ref.x_) < TOL and (s.nit_, s.nfev_) == (s_ref.nit_, s_ref.nfev_)


@pytest.mark.parametrize("nlam", [2, 3, 4, 6])
def test_fista_path_equals_one_by_one(fos, nlam):
    """Multi-lambda lockstep run (one pass over A per iteration for up to 4 weights) == independent solves."""
    A, b, fx = _data.problem("aligned")
    prob = fos.prepare(A, b)
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(fx["aligned/L"])
    alphas = [(lam * 0.3 * 0.5 ** i, 0.5 if i % 2 else 0.0) for i in range(nlam)]
    xs = fos.fista_path(prob, None, alphas, max_iter=40, L=L)
    assert len(xs) == nlam
    for (a1, a2), x in zip(alphas, xs):
        x_one = fos.fista(prob, None, "elasticnet", a1, a2, max_iter=40, L=L)
        x_ref = orc.fista(A, b, "elasticnet", a1, a2, max_iter=40, L=L)
        assert _data.rel(x, x_one) < 1e-6, (a1, a2)          # same arithmetic, other geometry (summation order) of the pass
        assert _data.rel(x, x_ref) < TOL, (a1, a2)
    xd = fos.fista_path(prob, None, alphas[:2], max_iter=30, L=L, delta=3.0)
    assert _data.rel(xd[1], orc.fista_delta(A, b, "elasticnet", alphas[1][0], alphas[1][1], 3.0, max_iter=30, L=L)) < TOL


@pytest.mark.parametrize("kind,m,n,nlam", [("f32", 4096, 512, 16), ("f32", 1000, 200, 7), ("f32", 333, 16384, 16),
                                           ("bf16", 2000, 1024, 16), ("bf16", 700, 264, 5), ("f32", 70000, 128, 9)])
def test_fista_path_sixteen_weights_on_the_matrix_cores(fos, kind, m, n, nlam):
    """5..16 weights in lockstep: two GEMM-shaped products per iteration on MFMA (R = A Y - b, G = A^T R) for all of
    them.  Equal to one-by-one runs (1e-6: same arithmetic, other summation order) and to the oracle (1e-5) - on the
    bf16-ROUNDED A for bf16 storage; FISTA and FISTA-delta; ragged row counts, partial tiles, several panels."""
    A, b, _ = _data.synth(m, n, 77 + n)
    if kind == "bf16":
        At = torch.as_tensor(A.astype(np.float32)).to(torch.bfloat16).cuda()
        A = At.to(torch.float64).cpu().numpy()
    else:
        At = torch.as_tensor(A.astype(np.float32)).cuda()
        A = At.to(torch.float64).cpu().numpy()
    b = b.astype(np.float32).astype(np.float64)
    prob = fos.prepare(At, b.astype(np.float32))
    assert prob.plan()["path"] == 0
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(np.linalg.norm(A, 2) ** 2) if n <= 1024 else float(np.linalg.norm(A, "fro") ** 2)
    alphas = [(lam * 0.4 * 0.7 ** i, 0.5 if i % 3 == 1 else 0.0) for i in range(nlam)]
    xs = fos.fista_path(prob, None, alphas, max_iter=30, L=L)
    assert len(xs) == nlam
    for i, ((a1, a2), x) in enumerate(zip(alphas, xs)):
        x_ref = orc.fista(A, b, "elasticnet", a1, a2, max_iter=30, L=L)
        assert _data.rel(_np(x), x_ref) < TOL, (i, a1, a2)
        if i in (0, nlam - 1):
            x_one = fos.fista(prob, None, "elasticnet", a1, a2, max_iter=30, L=L)
            assert _data.rel(_np(x), _np(x_one)) < 1e-6, (i, a1, a2)
    xd = fos.fista_path(prob, None, alphas, max_iter=20, L=L, delta=3.0)
    assert _data.rel(_np(xd[2]), orc.fista_delta(A, b, "elasticnet", alphas[2][0], alphas[2][1], 3.0, max_iter=20, L=L)) < TOL
    # the handles stay usable by the single-vector path afterwards (state machines are shared, y is rebuilt)
    x_again = fos.fista_path(prob, None, alphas[:2], max_iter=30, L=L)
    assert _data.rel(_np(x_again[0]), _np(xs[0])) < 1e-6


@pytest.mark.parametrize("kind,m,n,nlam", [("f32", 3000, 512, 8), ("bf16", 1500, 1024, 5), ("f32", 900, 2048, 16)])
def test_fista_path_lockstep_with_restart_and_ratio_stop(fos, kind, m, n, nlam):
    """Data-dependent control per weight INSIDE the lockstep pass (round 3): adaptive restart and the ratio stop are decided
    on the device for every state machine every iteration; a stopped weight is a masked column.  Every weight must stop
    at the oracle's iteration with the oracle's iterate, whatever the others do; the tolerance-with-gradient-rule case
    (`tol`) falls back to one-by-one runs and must agree as well."""
    A, b, _ = _data.synth(m, n, 31 + n)
    At = torch.as_tensor(A.astype(np.float32)).to(torch.bfloat16 if kind == "bf16" else torch.float32).cuda()
    A = At.to(torch.float64).cpu().numpy()
    b = b.astype(np.float32).astype(np.float64)
    prob = fos.prepare(At, b.astype(np.float32))
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(np.linalg.norm(A, 2) ** 2)
    alphas = [(lam * 0.5 * 0.6 ** i, 0.3 if i % 3 == 2 else 0.0) for i in range(nlam)]
    for kw in (dict(adaptive_restart=True), dict(adaptive_restart=True, restart_threshold=0.9, tol_ratio=0.5),
               dict(tol_ratio=0.8), dict(tol=1e-3 * lam)):
        xs, info = fos.fista_path(prob, None, alphas, max_iter=60, L=L, return_info=True, **kw)
        stops = set()
        for (a1, a2), x, (k, code) in zip(alphas, xs, info):
            x_ref, h_ref = orc.fista(A, b, "elasticnet", a1, a2, max_iter=60, L=L, return_history=True, **kw)
            assert k == len(h_ref["obj"]), (kw, a1, k, len(h_ref["obj"]))
            assert _data.rel(_np(x), x_ref) < TOL, (kw, a1)
            stops.add(k)
        if "tol_ratio" in kw:
            assert len(stops) > 1 or min(stops) < 60, "the case must exercise a stop"


@pytest.mark.parametrize("m,n", [(3000, 2048), (2100, 4096), (2561, 6144), (4099, 8192)])
def test_fused_persistent_mfma_step(fos, m, n):
    """BASELINE north_star's literal step, opt-in (fos_fista_run_fused / FOS_PLAN_FUSED_MFMA): ONE persistent launch per run,
    A staged through LDS in 4-row panels, the row dots on v_mfma_f32_4x4x1_16B_f32, prox + momentum by the workgroup that
    owns the columns, the iterate resident in LDS.  Against the oracle (1e-5) and the default two-launch step (1e-6) for
    FISTA (lasso, l2 in the smooth part), FISTA-delta and the fused ISTA with the elastic-net prox; the state carries over
    between fused calls and between the two forms; ragged row counts (partial last panel); unsupported shapes refuse."""
    from fastoptsolver_amd import _core
    A, b, _ = _data.synth(m, n, 5 + n)
    At = torch.as_tensor(A.astype(np.float32)).cuda()
    A = At.to(torch.float64).cpu().numpy()
    b = b.astype(np.float32).astype(np.float64)
    prob = fos.prepare(At, b.astype(np.float32))
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(np.linalg.norm(A, "fro") ** 2)
    cases = [dict(mode=_core._lib.MODE_FISTA, a1=0.1 * lam, a2=0.0, kind=_core._lib.PROX_L1),
             dict(mode=_core._lib.MODE_FISTA, a1=0.05 * lam, a2=0.7, kind=_core._lib.PROX_L1),
             dict(mode=_core._lib.MODE_DELTA, a1=0.1 * lam, a2=0.0, kind=_core._lib.PROX_L1, delta=3.0),
             dict(mode=_core._lib.MODE_ISTA, a1=0.1 * lam, a2=0.4, kind=_core._lib.PROX_ENET)]
    for c in cases:
        a1, a2 = c["a1"], c["a2"]
        tau = 1.0 / (L + (a2 if c["kind"] == _core._lib.PROX_L1 and a2 > 0 else 0.0))
        kw = dict(mode=c["mode"], prox_kind=c["kind"], delta=c.get("delta", 0.0))
        ref = _core.Fista(prob); ref.reset(tau, a1, a2, **kw); ref.run(22)
        fz = _core.Fista(prob); fz.reset(tau, a1, a2, **kw)
        assert fz.run_fused(7) and fz.run_fused(9)                    # the state carries over between fused calls ...
        fz.run(3)                                                     # ... to the two-launch form ...
        assert fz.run_fused(3)                                        # ... and back
        xf, xr = _np(fz.x_tensor()), _np(ref.x_tensor())
        assert _data.rel(xf, xr) < 1e-6, (c, _data.rel(xf, xr))
        sf, sr = fz.status(), ref.status()
        assert int(sf.k) == int(sr.k) == 22 and sf.this_step == pytest.approx(sr.this_step, rel=1e-4)
        if c["mode"] == _core._lib.MODE_FISTA:
            x_o = orc.fista(A, b, "elasticnet", a1, a2, max_iter=22, L=L)
        elif c["mode"] == _core._lib.MODE_DELTA:
            x_o = orc.fista_delta(A, b, "lasso", a1, 0.0, 3.0, max_iter=22, L=L)
        else:
            from oracle.fos_oracle import prox_elastic_net
            A_, b_ = A, b
            x_o = orc.ista(np.zeros(n), lambda x: 0.5 * float(np.sum((A_ @ x - b_) ** 2)), lambda x: A_.T @ (A_ @ x - b_),
                           lambda v, t: prox_elastic_net(v, t, a1, a2), L, max_iter=22)
        assert _data.rel(xf, x_o) < TOL, c
    # the plan flag routes the public front-end through it
    prob.replan(fused_mfma=True)
    assert prob.plan()["fused_mfma"] == 1
    x_pub = fos.fista(prob, None, "lasso", 0.1 * lam, 0.0, max_iter=30, L=L)
    assert _data.rel(_np(x_pub), orc.fista(A, b, "lasso", 0.1 * lam, 0.0, max_iter=30, L=L)) < TOL
    # shapes / configurations it does not serve refuse (the caller keeps the default step)
    small = fos.prepare(At[:512], b[:512].astype(np.float32))
    st = _core.Fista(small); st.reset(1.0 / L, 0.1 * lam, 0.0)
    assert st.run_fused(3) is False
    st = _core.Fista(prob); st.reset(1.0 / L, 0.1 * lam, 0.0, adaptive_restart=True)
    assert st.run_fused(3) is False


@pytest.mark.parametrize("m,n,nlam", [(4133, 8188, 16), (2100, 16384, 11), (8200, 4096, 16), (4200, 5000, 6)])
def test_fista_path_one_read_cluster_pass(fos, m, n, nlam):
    """The opt-in one-read form of the matrix-core pass (cluster_pass.hpp: clusters of 4 / 8 / 16 workgroups share row panels,
    both products from one LDS tile, partial residuals handed over through L2): equal to the two-product form (1e-6: same
    arithmetic, other summation order) for every weight and to the oracle (1e-5); ragged row counts (masked tail panel),
    strips that end inside a 1024-column block, members without any column (n = 5000 on 8 members), repeated launches
    (flag epochs) and bit-reproducibility."""
    A, b, _ = _data.synth(m, n, 5 + n)
    At = torch.as_tensor(A.astype(np.float32)).cuda()
    A = At.to(torch.float64).cpu().numpy()
    b = b.astype(np.float32).astype(np.float64)
    prob = fos.prepare(At, b.astype(np.float32))
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(np.linalg.norm(A, "fro") ** 2)
    alphas = [(lam * 0.4 * 0.7 ** i, 0.5 if i % 3 == 1 else 0.0) for i in range(nlam)]
    xt = fos.fista_path(prob, None, alphas, max_iter=12, L=L)            # default: the two-product form
    assert prob.plan()["cluster"] == 0
    prob.replan(cluster=True)
    xs = fos.fista_path(prob, None, alphas, max_iter=12, L=L)
    assert prob.plan()["cluster"] == 1
    xs2 = fos.fista_path(prob, None, alphas, max_iter=12, L=L)
    for x, x2 in zip(xs, xs2):
        assert torch.equal(x, x2)
    for i, (x, x_two) in enumerate(zip(xs, xt)):
        assert _data.rel(_np(x), _np(x_two)) < 1e-6, i
    for i in (0, nlam // 2, nlam - 1):
        a1, a2 = alphas[i]
        assert _data.rel(_np(xs[i]), orc.fista(A, b, "elasticnet", a1, a2, max_iter=12, L=L)) < TOL, i


def test_fista_path_falls_back_on_shapes_without_multi_kernel(fos):
    A, b, fx = _data.problem("ragged")          # two-pass path: no multi-vector kernel -> one by one, same answers
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(fx["ragged/L"])
    alphas = [(0.2 * lam, 0.0), (0.05 * lam, 0.5)]
    xs = fos.fista_path(A, b, alphas, max_iter=25, L=L)
    for (a1, a2), x in zip(alphas, xs):
        assert _data.rel(x, orc.fista(A, b, "elasticnet", a1, a2, max_iter=25, L=L)) < TOL


def test_ista_with_the_reference_users_numpy_closures(fos):
    """What a user of the reference actually passes to ista(): closures over a NumPy A (ref:65-77 call sites).  They
    must keep working unchanged (fed ndarrays), with the same answers as the fused path."""
    A, b, fx = _data.problem("tiny")
    a1 = 0.1 * float(np.max(np.abs(A.T @ b)))
    L = float(fx["tiny/ista/L"])
    g = lambda x: 0.5 * float((A @ x - b) @ (A @ x - b))                       # noqa: E731
    grad_g = lambda x: A.T @ (A @ x - b)                                      # noqa: E731
    prox_h = lambda v, t: np.sign(v) * np.maximum(np.abs(v) - t * a1, 0.0)    # noqa: E731
    for kw, name in ((dict(), "fixed"), (dict(backtracking=True, t_init_factor=2.0), "bt2")):
        x, log = fos.ista(np.zeros(16), g, grad_g, prox_h, L, max_iter=40, return_history=True, **kw)
        key = f"tiny/ista/l1/{name}"
        assert isinstance(x, np.ndarray) and x.dtype == np.float64
        assert _data.rel(x, fx[key + "/x"]) < TOL, key
        assert len(log["x"]) == 41 and len(log["delta"]) == 40


# --------------------------------------------------------------------------------------------------
# LDS-resident loop (small problems): continuity with the multi-launch state machine, API semantics
# --------------------------------------------------------------------------------------------------
def test_resident_loop_and_split_entry_points_share_one_state(fos):
    """10 iterations inside the resident launch, 10 through grad()/update(), 10 resident again == 30 oracle
    iterations: the kernel continues from and leaves behind the same device state as the multi-launch path."""
    from fastoptsolver_amd import _core, _lib
    A, b, fx = _data.problem("tiny")
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(fx["tiny/L"])
    a1, a2 = 0.05 * lam, 0.5
    prob = fos.prepare(A, b)
    assert prob.plan()["resident"] == 1
    for mode, delta in ((_lib.MODE_FISTA, 0.0), (_lib.MODE_DELTA, 3.0)):
        st = _core.Fista(prob)
        st.reset(1.0 / (L + a2), a1, a2, mode=mode, prox_kind=_lib.PROX_L1, delta=delta)
        st.run(10)                                   # resident
        for _ in range(10):                          # split entry points (two launches + bookkeeping per iteration)
            st.grad()
            st.update()
        st.run(10)                                   # resident again
        assert int(st.status().k) == 30
        if mode == _lib.MODE_FISTA:
            x_ref = orc.fista(A, b, "elasticnet", a1, a2, max_iter=30, L=L)
        else:
            x_ref = orc.fista_delta(A, b, "elasticnet", a1, a2, delta, max_iter=30, L=L)
        assert _data.rel(st.x_tensor().cpu().numpy(), x_ref) < TOL, mode


@pytest.mark.parametrize("mode", ["fista", "delta"])
def test_plain_run_forms_share_one_momentum_state(fos, mode):
    """A streaming plan driven through a mix of entry points - plain run, grad()/update() leaving their bookkeeping
    pending, status(), the recorded DUAL run, plain run again - is the uninterrupted 18-iteration run and the oracle."""
    from fastoptsolver_amd import _core, _lib
    A, b, fx = _data.problem("aligned")
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(fx["aligned/L"])
    a1, a2 = 0.1 * lam, 0.5
    prob = fos.prepare(A, b)
    plan = prob.plan()
    assert plan["resident"] == 0 and plan["path"] == 0, plan
    md, delta = (_lib.MODE_FISTA, 0.0) if mode == "fista" else (_lib.MODE_DELTA, 3.0)

    def handle():
        st = _core.Fista(prob)
        st.reset(1.0 / (L + a2), a1, a2, mode=md, prox_kind=_lib.PROX_L1, delta=delta)
        return st

    mixed, whole = handle(), handle()
    mixed.run(5)
    for _ in range(3):
        mixed.grad()
        mixed.update()
    assert int(mixed.status().k) == 8
    assert mixed.run_history(4) is not None
    mixed.run(6)
    whole.run(18)
    assert int(mixed.status().k) == 18 and int(whole.status().k) == 18
    x_mixed, x_whole = mixed.x_tensor().cpu().numpy(), whole.x_tensor().cpu().numpy()
    if mode == "fista":
        x_ref = orc.fista(A, b, "elasticnet", a1, a2, max_iter=18, L=L)
    else:
        x_ref = orc.fista_delta(A, b, "elasticnet", a1, a2, delta, max_iter=18, L=L)
    assert _data.rel(x_mixed, x_whole) < 1e-6
    assert _data.rel(x_mixed, x_ref) < TOL


@pytest.mark.parametrize("m,n", [(4096, 512), (2000, 128)])
def test_lockstep_continues_single_runs(fos, m, n):
    """Four handles run 3 iterations on their own, then 5 in lockstep: each equals its own uninterrupted 8-iteration run.
    4096 x 512 takes the VALU multi-vector kernel, 2000 x 128 (chunk-per-lane rows) the matrix-core form."""
    from fastoptsolver_amd import _core, _lib
    A, b, _ = _data.synth(m, n, 91 + n)
    At = torch.as_tensor(A.astype(np.float32)).cuda()
    A = At.to(torch.float64).cpu().numpy()
    b = b.astype(np.float32).astype(np.float64)
    prob = fos.prepare(At, b.astype(np.float32))
    plan = prob.plan()
    assert plan["path"] == 0 and plan["resident"] == 0 and plan["tall"] == (n <= 128), plan   # tall: no VALU multi kernel
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(np.linalg.norm(A, 2) ** 2)
    alphas = [(lam * 0.3 * 0.6 ** i, 0.5 if i % 2 else 0.0) for i in range(4)]

    def handle(a1, a2):
        st = _core.Fista(prob)
        st.reset(1.0 / (L + a2), a1, a2, mode=_lib.MODE_FISTA, prox_kind=_lib.PROX_L1)
        return st

    hs = [handle(a1, a2) for a1, a2 in alphas]
    for st in hs:
        st.run(3)
    assert _core.run_multi(hs, 5)
    for (a1, a2), st in zip(alphas, hs):
        one = handle(a1, a2)
        one.run(8)
        assert int(st.status().k) == 8
        x = st.x_tensor().cpu().numpy()
        assert _data.rel(x, one.x_tensor().cpu().numpy()) < 1e-6, (a1, a2)
        assert _data.rel(x, orc.fista(A, b, "elasticnet", a1, a2, max_iter=8, L=L)) < TOL, (a1, a2)


def test_resident_run_reports_stops_steps_and_counts(fos):
    from fastoptsolver_amd import _core, _lib
    A, b, fx = _data.problem("tiny")
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(fx["tiny/L"])
    prob = fos.prepare(A, b)
    st = _core.Fista(prob)
    # ISTA with a generous first step: 2 genuine shrinks, then the step-size stop after 11 iterations (no momentum, so
    # none of the reference's step-underflow events)
    a1, a2, tol = 0.05 * lam, 0.5, 1e-5
    st.reset(8.0 / (L + a2), a1, a2, mode=_lib.MODE_ISTA, prox_kind=_lib.PROX_L1, tol_step=tol)
    res = st.run_resident(400, backtracking=True, eta=0.5, armijo_c=1e-2, record=True)
    (x_ref, log), met = orc.ista(np.zeros(A.shape[1]), lambda z: orc.smooth_value(A, b, z, a2),
                                 lambda z: orc.gram_gradient(A, z, b, a2)[0], lambda v, t: orc.prox_l1(v, t * a1),
                                 L + a2, backtracking=True, eta=0.5, t_init_factor=8.0, max_iter=400, tol=tol,
                                 return_history=True, return_metrics=True)
    k = len(log["delta"])
    assert res["done"] == k < 400 and st.status().stopped == _lib.STOP_STEP                 # delta < tol (:122)
    assert sum(res["ls"]) == met["ls_iters_total"] > 0
    assert np.allclose(res["taus"], log["t"][1:], rtol=1e-12) and res["tau"] == res["taus"][-1]
    assert res["x"].shape == (k, A.shape[1]) and _data.rel(res["x"][-1].cpu().numpy(), x_ref) < TOL
    assert np.allclose(np.sqrt(res["hist"][:, 3].cpu().numpy()), log["delta"], rtol=1e-4, atol=1e-12)
    assert st.run_resident(5)["done"] == 0               # a stopped solver stays stopped
    # a problem beyond the LDS budget reports "not resident" and the caller falls back to the multi-launch loop
    big = fos.prepare(np.zeros((4097, 8), dtype=np.float32), np.zeros(4097, dtype=np.float32))
    assert big.plan()["resident"] == 0 and _core.Fista(big).run_resident(1) is None


def test_resident_and_multi_launch_paths_agree(fos):
    """replan(no_resident=True) keeps small problems on the multi-launch kernels: same iterates either way."""
    A, b, fx = _data.problem("tiny")
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(fx["tiny/L"])
    kw = dict(max_iter=60, L=L, backtracking=True, t_init_factor=2.0, return_history=True)
    x1, h1 = fos.fista(A, b, "lasso", 0.05 * lam, 0.0, **kw)
    prob = fos.prepare(A, b)
    assert prob.plan()["resident"] == 1
    prob.replan(no_resident=True)
    assert prob.plan()["resident"] == 0
    x2, h2 = fos.fista(prob, None, "lasso", 0.05 * lam, 0.0, **kw)
    assert _data.rel(x1, x2) < 1e-6 and np.allclose(h1["obj"], h2["obj"], rtol=1e-6)


def test_resident_loop_with_bf16_storage(fos):
    """A stored in bf16 also runs in the LDS-resident loop (converted to fp32 once, when it is copied into LDS)."""
    A, b, fx = _data.problem("tiny")
    A16 = torch.as_tensor(A.astype(np.float32)).to(torch.bfloat16)
    Aq = A16.to(torch.float64).numpy()
    lam = float(np.max(np.abs(Aq.T @ b)))
    L = float(np.linalg.norm(Aq, 2) ** 2)
    prob = fos.prepare(A16.cuda(), b)
    assert prob.dtype == "bf16" and prob.plan()["resident"] == 1
    np.random.seed(3)
    assert fos.estimate_lipschitz(prob) == pytest.approx(orc.estimate_lipschitz(Aq, v0=np.random.RandomState(3).randn(16)),
                                                         rel=1e-6)
    for kw in (dict(), dict(backtracking=True, t_init_factor=2.0, eta=0.7)):
        x, h = fos.fista(prob, None, "elasticnet", 0.05 * lam, 0.5, max_iter=40, L=L, return_history=True, **kw)
        x_ref, h_ref = orc.fista(Aq, b, "elasticnet", 0.05 * lam, 0.5, max_iter=40, L=L, return_history=True, **kw)
        assert _data.rel(x.cpu().numpy() if torch.is_tensor(x) else x, x_ref) < TOL, kw
        assert np.allclose(h["obj"], h_ref["obj"], rtol=TOL), kw


# --------------------------------------------------------------------------------------------------
# tall-skinny single pass (n <= 64 row per thread; aligned rows up to 128 columns chunk per lane): many samples, few features
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,kind", [(20000, 5, "f32"), (20001, 7, "f32"), (70000, 8, "f32"), (33333, 16, "f32"),
                                      (9000, 33, "f32"), (12345, 64, "f32"), (5000, 32, "strided"), (6000, 12, "bf16"),
                                      (200, 64, "f32"), (1, 40, "f32"),
                                      # aligned rows: a row per 4 / 8 / 16 lanes, one 16-byte chunk per lane
                                      (40001, 12, "f32"), (30000, 24, "f32"), (25000, 40, "f32"), (1027, 60, "f32"),
                                      (7000, 48, "strided"), (9000, 16, "bf16"), (8000, 40, "bf16"), (5003, 64, "bf16"),
                                      # round 3: 65..128 columns, a row per 32 lanes (fp32) / 16 lanes (bf16)
                                      (30001, 68, "f32"), (20000, 100, "f32"), (9000, 128, "f32"), (3, 72, "f32"),
                                      (7001, 120, "strided"), (8000, 72, "bf16"), (5003, 128, "bf16"),
                                      (6000, 192, "bf16"), (4001, 256, "bf16")])           # bf16: 32 lanes per row up to 256 columns
def test_tall_skinny_gemv_pair(fos, m, n, kind):
    rng = np.random.default_rng(m + n)
    A = rng.standard_normal((m, n)).astype(np.float32)
    b = rng.standard_normal(m).astype(np.float32)
    y = rng.standard_normal(n).astype(np.float32)
    if kind == "strided":                                   # rows 40 floats apart: lda > n, borrowed as it is
        big = torch.as_tensor(np.hstack([A, np.zeros((m, 8), np.float32)])).cuda()
        At = big[:, :n]
    elif kind == "bf16":
        At = torch.as_tensor(A).to(torch.bfloat16).cuda()
        A = At.float().cpu().numpy()
    else:
        At = torch.as_tensor(A).cuda()
    prob = fos.prepare(At, b)
    plan = prob.plan()
    assert plan["tall"] == 1 and plan["path"] == 0 and prob.n_dev == n
    g = prob.gemv_pair(_dev(y), alpha2=0.3).cpu().numpy()
    g_ref, rr_ref = orc.gram_gradient(A.astype(np.float64), y.astype(np.float64), b.astype(np.float64), 0.3)
    assert _data.rel(g, g_ref) < 1e-6, (m, n, kind)
    rr, x2, x1 = prob.residual_objective(_dev(y))
    assert rr == pytest.approx(rr_ref, rel=1e-6) and x1 == pytest.approx(np.abs(y.astype(np.float64)).sum(), rel=1e-6)
    # deterministic: bit-identical across launches
    assert torch.equal(prob.gemv_pair(_dev(y), alpha2=0.3), prob.gemv_pair(_dev(y), alpha2=0.3))
    # the fp64 form of the same kernel (L-BFGS fg) and the DUAL form (history objective from the gradient pass)
    from fastoptsolver_amd import _core, _lib
    out = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
    yd = _dev(y, torch.float64)
    _lib.check(_lib.load().fos_gemv_pair_dd(prob.h, _core.ptr(yd), 0.3, _core.ptr(out)))
    assert _data.rel(out[:n].cpu().numpy(), g_ref) < 1e-12 and float(out[n]) == pytest.approx(rr_ref, rel=1e-12)
    if m >= 1000:
        lam = float(np.max(np.abs(A.T.astype(np.float64) @ b)))
        L = float(np.linalg.norm(A.astype(np.float64), 2) ** 2)
        x, h = fos.fista(prob, None, "lasso", 0.05 * lam, 0.0, max_iter=12, L=L, return_history=True, adaptive_restart=True)
        x_ref, h_ref = orc.fista(A.astype(np.float64), b.astype(np.float64), "lasso", 0.05 * lam, 0.0, max_iter=12, L=L,
                                 return_history=True, adaptive_restart=True)
        assert _data.rel(_np(x), x_ref) < TOL and np.allclose(h["obj"], h_ref["obj"], rtol=TOL)
        if n > 64:           # aligned rows of 65..128 columns keep the matrix-core passes: 16 candidates, 16 weights
            A64, b64 = A.astype(np.float64), b.astype(np.float64)
            xb = fos.fista(prob, None, "elasticnet", 0.05 * lam, 0.3, max_iter=12, L=L, backtracking=True, t_init_factor=2.0)
            xb_ref, met = orc.fista(A64, b64, "elasticnet", 0.05 * lam, 0.3, max_iter=12, L=L, backtracking=True,
                                    t_init_factor=2.0, return_metrics=True)
            # (shrink counts: equal except for the length of the reference's ~50-halving step-underflow event, which is
            #  decided by fp64 rounding noise - see _check_linesearch_counts; the streaming plan gives the same count)
            from fastoptsolver_amd import iterative_solvers as its
            per_search = list(its.ls_call_iters)
            slack = 25 if max(per_search) >= 25 else 0
            assert _data.rel(_np(xb), xb_ref) < TOL and abs(sum(per_search) - met["ls_iters_total"]) <= slack, per_search
            alphas = [(lam * 0.3 * 0.7 ** i, 0.2 if i % 2 else 0.0) for i in range(6)]
            for x_j, (p1, p2) in zip(fos.fista_path(prob, None, alphas, max_iter=15, L=L), alphas):
                assert _data.rel(_np(x_j), orc.fista(A64, b64, "elasticnet", p1, p2, max_iter=15, L=L)) < TOL


def test_tall_skinny_solvers_on_unstandardised_features(fos):
    """50000 x 5 Boston-like data (cond(A^T A) ~ 1e9): every solver family through the row-per-thread pass."""
    from fastoptsolver_amd.easy_boston_data import generate_correlated_boston_like_data
    A, b, _ = generate_correlated_boston_like_data(m=50000, seed=7)
    prob = fos.prepare(A, b)
    assert prob.plan()["tall"] == 1 and prob.plan()["resident"] == 0
    np.random.seed(0)
    L = fos.estimate_lipschitz(prob)
    np.random.seed(0)
    assert L == pytest.approx(orc.estimate_lipschitz(A, v0=np.random.randn(5)), rel=1e-6)
    for kw in (dict(), dict(adaptive_restart=True), dict(backtracking=True, t_init_factor=2.0)):
        x, h = fos.fista(prob, None, "lasso", 1.0, 0.0, max_iter=120, L=L, return_history=True, **kw)
        x_ref, h_ref = orc.fista(A, b, "lasso", 1.0, 0.0, max_iter=120, L=L, return_history=True, **kw)
        assert _data.rel(x, x_ref) < TOL, kw
        assert np.allclose(h["obj"], h_ref["obj"], rtol=TOL), kw
    x = fos.fista_delta(prob, None, "elasticnet", 1.0, 0.5, 3.0, max_iter=120, L=L)
    assert _data.rel(x, orc.fista_delta(A, b, "elasticnet", 1.0, 0.5, 3.0, max_iter=120, L=L)) < TOL
    s = fos.LBFGSSolver("ridge", 0.0, 0.5).fit(prob, None)
    # cond(A^T A) ~ 1e9: the point at which the factr test stops the run is itself only determined to ~1e-5 (two
    # float64 codes with different summation orders end 1e-5 apart, tests/test_oracle_golden.py), and the fp32 STORAGE
    # rounding of A and b moves it by another ~2e-5.  Judged: the leading iterates at 1e-5 and the loss at 2e-8 against
    # the oracle on exactly the stored data, the end point at 1e-4 against both oracles.
    A32, b32 = A.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    s_ref = orc.LBFGSSolver("ridge", 0.0, 0.5).fit(A32, b32)
    for k in range(4):
        assert _data.rel(s.iterates_[k], s_ref.iterates_[k]) < TOL, k
    # (the factr test stops a run once a step lowers f by less than 2.2e-9 relative: the two end values may differ by that)
    assert _data.rel(s.x_, s_ref.x_) < 1e-4 and s.final_obj_ == pytest.approx(s_ref.final_obj_, rel=2e-8)
    # (iteration counts are not compared here: at cond 1e9 the run length itself is chaotic - 34 vs 40 iterations for two
    # float64-accurate runs whose data differ in the 8th digit; the well-conditioned cases above compare nit / nfev exactly)
    assert s.task_.startswith("CONVERGENCE") and 0.5 * s_ref.nit_ <= s.nit_ <= 2 * s_ref.nit_
    s_raw = orc.LBFGSSolver("ridge", 0.0, 0.5).fit(A, b)
    assert _data.rel(s.x_, s_raw.x_) < 1e-4 and s.final_obj_ == pytest.approx(s_raw.final_obj_, rel=1e-6)


def test_prepared_problem_follows_torchs_current_stream(fos):
    """A problem prepared on the default stream and then used inside `with torch.cuda.stream(s)`: the handle moves to the
    caller's stream (fos_problem_set_stream), so kernels and the caching allocator's temporaries share it; results equal
    the default-stream run, also when the two are interleaved."""
    A, b, fx = _data.problem("aligned")
    prob = fos.prepare(A, b)
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(fx["aligned/L"])
    x_ref = orc.fista(A, b, "lasso", 0.1 * lam, 0.0, max_iter=50, L=L)
    x0 = fos.fista(prob, None, "lasso", 0.1 * lam, 0.0, max_iter=50, L=L)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x1, h1 = fos.fista(prob, None, "lasso", 0.1 * lam, 0.0, max_iter=50, L=L, return_history=True,
                           backtracking=True, t_init_factor=2.0)
        x2 = fos.fista(prob, None, "lasso", 0.1 * lam, 0.0, max_iter=50, L=L)
        s = fos.LBFGSSolver("ridge", 0.0, 1.0, max_iter=6).fit(prob, None)
    x3 = fos.fista(prob, None, "lasso", 0.1 * lam, 0.0, max_iter=50, L=L)
    assert np.array_equal(x0, x2) and np.array_equal(x0, x3) and _data.rel(x0, x_ref) < TOL
    x_bt = orc.fista(A, b, "lasso", 0.1 * lam, 0.0, max_iter=50, L=L, backtracking=True, t_init_factor=2.0)
    assert _data.rel(x1, x_bt) < TOL
    s_ref = orc.LBFGSSolver("ridge", 0.0, 1.0, max_iter=6).fit(A, b)
    assert _data.rel(s.x_, s_ref.x_) < TOL


def test_gradient_norm_stop_runs_on_the_device_and_long_power_iterations(fos):
    """fista(tol > 0) without backtracking / history is enqueue-only: the ||grad|| < tol test of iterative_solvers.py:179
    is a kernel between the reduced gradient and the update.  Same stopping iteration, iterate and gradient-call count as
    the oracle.  And estimate_lipschitz accepts any n_iter (the reference has no cap)."""
    A, b, fx = _data.problem("ragged")
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(fx["ragged/L"])
    prob = fos.prepare(A, b)
    prob.replan(no_resident=True)
    for tol in (2.0, 1e-2):
        x = fos.fista(prob, None, "ridge", 0.0, 2.0, max_iter=400, tol=tol, L=L, check_every=4)
        x_ref, met = orc.fista(A, b, "ridge", 0.0, 2.0, max_iter=400, tol=tol, L=L, return_metrics=True)
        assert fos.get_metrics()["grad_num_calls"] == met["grad_num_calls"] < 400, tol
        assert _data.rel(x, x_ref) < TOL, tol
    np.random.seed(3)
    v0 = np.random.randn(A.shape[1])
    np.random.seed(3)
    assert fos.estimate_lipschitz(prob, n_iter=450, tol=0.0) == pytest.approx(
        orc.estimate_lipschitz(A, n_iter=450, tol=0.0, v0=v0), rel=1e-6)


@pytest.mark.parametrize("tag", ["aligned", "ragged_padded"])
def test_device_driven_backtracking_equals_host_driven(fos, tag):
    """fista(backtracking=True) without history decides every search on the device (fos_fista_run_backtracking: no host
    round trip per iteration); with history the host decides.  Same kernels, same clauses: identical shrink counts and
    iterates, also across poll chunks (the step persists on the device), through a parked search (t_init_factor so large
    that the first search needs more than one batch of 16 candidates: the host finishes it and hands the loop back),
    with the stopping rules, and for FISTA-delta; all against the oracle."""
    from fastoptsolver_amd import iterative_solvers as its
    if tag == "aligned":
        A, b, fx = _data.problem("aligned")
        L = float(fx["aligned/L"])
    else:
        A, b, _ = _data.synth(3000, 700, 21)                     # ragged n, padded onto the streaming pass (m*n >= 2^20)
        L = float(np.linalg.norm(A, 2) ** 2)
    prob = fos.prepare(A, b)
    assert prob.plan()["path"] == 0 and prob.plan()["resident"] == 0
    lam = float(np.max(np.abs(A.T @ b)))
    cases = [dict(t_init_factor=2.0), dict(t_init_factor=4.0, eta=0.7), dict(t_init_factor=3.0e6, eta=0.5),
             dict(t_init_factor=2.0, tol=2e-2), dict(t_init_factor=2.0, tol_ratio=0.95)]
    from fastoptsolver_amd import _core
    for kw in cases:
        x_dev = fos.fista(prob, None, "elasticnet", 0.05 * lam, 0.5, max_iter=30, L=L, backtracking=True, check_every=4, **kw)
        ls_dev, met_dev = list(its.ls_call_iters), fos.get_metrics()
        # history recorded on the device (fos_fista_run_recorded), polled in chunks of 5
        x_rec, h_rec = fos.fista(prob, None, "elasticnet", 0.05 * lam, 0.5, max_iter=30, L=L, backtracking=True,
                                 return_history=True, check_every=5, **kw)
        ls_rec, met_rec = list(its.ls_call_iters), fos.get_metrics()
        # the host-driven loop (one synchronising batch per iteration): what runs when the device forms do not apply
        saved = _core.Fista.run_recorded
        _core.Fista.run_recorded = lambda self, *a, **k: None
        try:
            x_host, h = fos.fista(prob, None, "elasticnet", 0.05 * lam, 0.5, max_iter=30, L=L, backtracking=True,
                                  return_history=True, **kw)
        finally:
            _core.Fista.run_recorded = saved
        ls_host, met_host = list(its.ls_call_iters), fos.get_metrics()
        assert ls_dev == ls_host == ls_rec, (kw, ls_dev, ls_host, ls_rec)
        for met in (met_dev, met_rec):
            assert met["grad_num_calls"] == met_host["grad_num_calls"] and met["ls_num_calls"] == met_host["ls_num_calls"], kw
        assert _data.rel(x_dev, x_host) < 1e-12 and _data.rel(x_rec, x_host) < 1e-12, kw
        assert len(h_rec["x"]) == len(h["x"]) and len(h_rec["obj"]) == len(h["obj"]), kw
        assert np.allclose(h_rec["obj"], h["obj"], rtol=1e-6) and _data.rel(h_rec["x"][-1], h["x"][-1]) < 1e-12, kw
        x_ref, h_ref = orc.fista(A, b, "elasticnet", 0.05 * lam, 0.5, max_iter=30, L=L, backtracking=True,
                                 return_history=True, **kw)
        _, met_ref = orc.fista(A, b, "elasticnet", 0.05 * lam, 0.5, max_iter=30, L=L, backtracking=True,
                               return_metrics=True, **kw)
        assert _data.rel(x_dev, x_ref) < TOL, kw
        assert len(h_rec["obj"]) == len(h_ref["obj"]) and np.allclose(h_rec["obj"], h_ref["obj"], rtol=TOL), kw
        assert met_dev["grad_num_calls"] == met_ref["grad_num_calls"], kw
        if kw["t_init_factor"] < 1e3:
            # exact unless a search hit the reference's step-underflow regime (~45 halvings until x_tmp == y bit for bit:
            # decided by float64 rounding on both sides, see _check_linesearch_counts)
            slack = 10 if max(ls_dev) >= 40 else 0
            assert abs(sum(ls_dev) - met_ref["ls_iters_total"]) <= slack, (kw, ls_dev)
    # adaptive restart / stopping rules with history, no backtracking: recorded on the device too
    for kw in (dict(adaptive_restart=True), dict(tol=2e-2), dict(tol_ratio=0.95, adaptive_restart=True)):
        x, h = fos.fista(prob, None, "elasticnet", 0.05 * lam, 0.5, max_iter=40, L=L, return_history=True, check_every=7, **kw)
        x_ref, h_ref = orc.fista(A, b, "elasticnet", 0.05 * lam, 0.5, max_iter=40, L=L, return_history=True, **kw)
        assert len(h["obj"]) == len(h_ref["obj"]) and len(h["x"]) == len(h_ref["x"]), kw
        assert _data.rel(x, x_ref) < TOL and np.allclose(h["obj"], h_ref["obj"], rtol=TOL), kw
        assert _data.rel(h["x"][len(h["x"]) // 2], h_ref["x"][len(h_ref["x"]) // 2]) < TOL, kw
    assert max(ls_dev) >= 0
    xd = fos.fista_delta(prob, None, "lasso", 0.1 * lam, 0.0, 3.0, max_iter=25, L=L, backtracking=True, t_init_factor=2.0)
    assert _data.rel(xd, orc.fista_delta(A, b, "lasso", 0.1 * lam, 0.0, 3.0, max_iter=25, L=L, backtracking=True,
                                         t_init_factor=2.0)) < TOL


def test_fused_ista_log_is_recorded_on_the_device(fos):
    """ista(return_history=True) on a streaming-size problem: x, t and ||dx|| of every iteration are recorded by the
    device-driven loop (fixed step and backtracking, with the delta < tol stop), equal to the oracle's log."""
    A, b, fx = _data.problem("aligned")
    x0 = np.random.default_rng(4).standard_normal(A.shape[1]) * 0.01
    a1 = 0.05 * float(np.max(np.abs(A.T @ b)))
    L = float(fx["aligned/L"]) + 0.3
    ls = fos.LeastSquares(A, b, 0.3)
    assert ls.prob.plan()["resident"] == 0 and ls.prob.plan()["path"] == 0
    g = lambda z: orc.smooth_value(A, b, z, 0.3)                        # noqa: E731
    grad = lambda z: orc.gram_gradient(A, z, b, 0.3)[0]                 # noqa: E731
    prox = lambda v, t: orc.prox_l1(v, t * a1)                          # noqa: E731
    for kw in (dict(), dict(backtracking=True, t_init_factor=2.0), dict(tol=5e-3), dict(backtracking=True, t_init_factor=4.0, eta=0.7, tol=5e-3)):
        x, log = fos.ista(x0, ls, ls.grad, fos.L1Prox(a1), L, max_iter=40, return_history=True, **kw)
        x_ref, log_ref = orc.ista(x0, g, grad, prox, L, max_iter=40, return_history=True, **kw)
        assert len(log["x"]) == len(log_ref["x"]) and len(log["delta"]) == len(log_ref["delta"]), kw
        assert _data.rel(x, x_ref) < TOL and np.allclose(log["t"], log_ref["t"], rtol=1e-12), kw
        # delta = ||x_new - x||: each iterate carries the fp32 pass's ~1e-7 of ||x||, so small deltas agree absolutely
        assert np.allclose(log["delta"], log_ref["delta"], rtol=1e-5, atol=2e-6 * float(np.linalg.norm(x_ref))), kw
        assert _data.rel(log["x"][len(log["x"]) // 2], log_ref["x"][len(log_ref["x"]) // 2]) < TOL, kw


def test_stream_read_probe(fos):
    """The measurement aid bench.py reports beside the nominal peak: a loads-only pass; bad arguments are refused."""
    from fastoptsolver_amd import _core, _lib
    t = torch.ones(1 << 24, device="cuda")
    gbps, us = _core.stream_read_probe(t, launches=5)
    assert gbps > 100.0 and us > 0.0 and abs(gbps - t.numel() * 4 / us / 1e3) < 1e-6 * gbps
    import ctypes as C
    g = C.c_double()
    rc = _lib.load().fos_stream_read_probe(C.c_void_p(t.data_ptr() + 4), 1024, 1, None, C.byref(g), None)
    assert rc == -1


def test_prepare_from_host_arrays(fos):
    """The boundary handed HOST matrices (the reference's callers pass float64 ndarrays): float64 / float32 / Fortran-ordered
    / strided sources, fp32 and bf16 storage, with and without column padding - the bound matrix equals the host cast bit
    for bit, whatever the upload block size, and the solve from ndarrays equals the solve on the prepared problem."""
    from fastoptsolver_amd import _core
    A, b, _ = _data.synth(517, 260, 3)
    F = np.asfortranarray(A)
    old = _core.UPLOAD_CHUNK_BYTES
    try:
        for chunk in (old, 100_000):
            _core.UPLOAD_CHUNK_BYTES = chunk
            for src in (A, F, A.astype(np.float32), A[::2, ::2], F[:, 4:204], A[:, :257]):
                for kind, tdt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
                    for pad in (False, True):
                        prob = fos.prepare(src, b[: src.shape[0]], dtype=kind, pad=pad)
                        want = torch.from_numpy(np.ascontiguousarray(src)).to(tdt)
                        got = prob.A[:, : src.shape[1]].cpu()
                        assert torch.equal(got, want), (src.shape, src.strides, kind, pad, chunk)
                        assert prob.n_dev == src.shape[1] or float(prob.A[:, src.shape[1]:].abs().sum()) == 0.0
    finally:
        _core.UPLOAD_CHUNK_BYTES = old
    Ar = A.astype(np.float32).astype(np.float64)            # what the device holds
    br = b.astype(np.float32).astype(np.float64)
    L = float(np.linalg.norm(Ar, 2) ** 2)
    lam = float(np.max(np.abs(Ar.T @ br)))
    x_nd = fos.fista(F, b, "lasso", 0.1 * lam, 0.0, max_iter=40, L=L)
    assert isinstance(x_nd, np.ndarray) and x_nd.dtype == np.float64
    assert _data.rel(x_nd, orc.fista(Ar, br, "lasso", 0.1 * lam, 0.0, max_iter=40, L=L)) < TOL


def test_handles_release_their_device_memory(fos):
    """Every workspace the library allocates under a problem / solver handle (slabs, fp64 slabs, candidate blocks, the
    multi-lambda panels, L-BFGS workspace, persistent-step barriers) goes back with the handle: device memory in use after
    40 rounds of create -> every solver family -> destroy equals the level after the first round."""
    import gc
    from fastoptsolver_amd import _core, _lib
    A, b, _ = _data.synth(3000, 2048, 77)
    At = torch.as_tensor(A.astype(np.float32)).cuda()
    bt = b.astype(np.float32)
    B3 = np.stack([bt, 0.5 * bt, -bt], axis=1)
    L = float(np.linalg.norm(A, 2) ** 2)
    lam = float(np.max(np.abs(A.T @ b)))

    def one_round():
        prob = fos.prepare(At, bt)
        fos.fista(prob, None, "lasso", 0.1 * lam, 0.0, max_iter=5, L=L)
        fos.fista(prob, None, "elasticnet", 0.1 * lam, 0.5, max_iter=5, L=L, backtracking=True, return_history=True)
        fos.fista_delta(prob, None, "lasso", 0.1 * lam, 0.0, 3.0, max_iter=5, L=L, tol_ratio=1e-9)
        fos.fista_path(prob, None, [(0.1 * lam * 0.8 ** i, 0.0) for i in range(6)], max_iter=4, L=L)
        fos.fista_path(prob, None, [(0.1 * lam * 0.8 ** i, 0.0) for i in range(3)], max_iter=4, L=L, adaptive_restart=True)
        fos.LBFGSSolver("ridge", 0.0, 1.0, max_iter=3).fit(prob, None)
        fos.LBFGSSolver("ridge", 0.0, 1.0, max_iter=3).fit(prob, B3)
        st = _core.Fista(prob); st.reset(1.0 / L, 0.1 * lam, 0.0)
        assert st.run_fused(3)
        del st
        # every group is reset and built again before the handle goes: re-plan, tune both passes, run the families again
        prob.replan(cluster=False)
        prob.tune(256, 2, 4, 300)
        _lib.check(prob.lib.fos_problem_tune_dd(prob.h, 200), "fos_problem_tune_dd")
        fos.fista(prob, None, "elasticnet", 0.1 * lam, 0.5, max_iter=5, L=L, backtracking=True)
        fos.fista_path(prob, None, [(0.1 * lam * 0.8 ** i, 0.0) for i in range(6)], max_iter=4, L=L)
        fos.LBFGSSolver("ridge", 0.0, 1.0, max_iter=3).fit(prob, None)
        fos.LBFGSSolver("ridge", 0.0, 1.0, max_iter=3).fit(prob, B3)
        del prob
        gc.collect()
        torch.cuda.synchronize()

    one_round()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(40):
        one_round()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (8 << 20), f"device memory in use grew by {(free0 - free1) / 2 ** 20:.1f} MiB over 40 rounds"


# --------------------------------------------------------------------------------------------------
# Re-planning, tuning and attaching a communicator AFTER the first pass: the groups of the plan that were derived from
# the changed input are rebuilt (fos_internal.hpp: invalidate).  Each order is checked against the fp64 oracle at the
# tolerance of the neighbouring tests of the same pass, and bit for bit against a fresh handle brought into the same
# state before its first pass.
# --------------------------------------------------------------------------------------------------
def _pair_dd(prob, xd):
    from fastoptsolver_amd import _core, _lib
    out = torch.zeros(prob.n_dev + 1, dtype=torch.float64, device="cuda")
    _lib.check(prob.lib.fos_gemv_pair_dd(prob.h, _core.ptr(xd), 0.37, _core.ptr(out)), "fos_gemv_pair_dd")
    return out


@pytest.mark.parametrize("m,n", [(40000, 100), (20001, 7)])
def test_tune_after_an_fp64_pass_on_tall_plans(fos, m, n):
    """Tall plans share the fp32 pass's grid with the fp64 pass: fos_problem_tune(0, 0, 0, workgroups) after the first
    fos_gemv_pair_dd, with more and with fewer workgroups than planned, re-sizes the fp64 slabs with the grid.
    40000 x 100 takes the chunk-per-lane pass, 20001 x 7 the row-per-thread pass (more rows than the resident loop)."""
    rng = np.random.default_rng(m + n)
    A = rng.standard_normal((m, n)).astype(np.float32)
    b = rng.standard_normal(m).astype(np.float32)
    x = rng.standard_normal(n) * (1.0 + 1e-9 * rng.standard_normal(n))
    At, xd, yd = torch.as_tensor(A).cuda(), _dev(x, torch.float64), _dev(x.astype(np.float32))
    g_ref, rr_ref = orc.gram_gradient(A.astype(np.float64), x, b.astype(np.float64), 0.37)
    g32_ref, _ = orc.gram_gradient(A.astype(np.float64), x.astype(np.float32).astype(np.float64), b.astype(np.float64), 0.37)
    prob = fos.prepare(At, b, pad=False)
    plan = prob.plan()
    assert plan["tall"] == 1 and plan["resident"] == 0, plan
    planned = plan["workgroups"]

    def check(out, g32, where):
        got = out.cpu().numpy()
        assert _data.rel(got[:n], g_ref) < 1e-12, where
        assert got[n] == pytest.approx(rr_ref, rel=1e-12), where
        assert _data.rel(g32.cpu().numpy(), g32_ref) < 1e-6, where          # test_tall_skinny_gemv_pair's bounds

    check(_pair_dd(prob, xd), prob.gemv_pair(yd, alpha2=0.37), ("planned", plan))
    for wg in (2 * planned + 3, max(1, 2 * planned // 3)):
        prob.tune(0, 0, 0, wg)
        assert prob.plan()["workgroups"] != planned
        out, g32 = _pair_dd(prob, xd), prob.gemv_pair(yd, alpha2=0.37)
        check(out, g32, (wg, prob.plan()))
        fresh = fos.prepare(At, b, pad=False)
        fresh.tune(0, 0, 0, wg)
        assert fresh.plan() == prob.plan()
        assert torch.equal(_pair_dd(fresh, xd), out), wg
        assert torch.equal(fresh.gemv_pair(yd, alpha2=0.37), g32), wg


def _six_weights(fos, m, n, seed):
    A, b, _ = _data.synth(m, n, seed)
    At = torch.as_tensor(A.astype(np.float32)).cuda()
    A = At.to(torch.float64).cpu().numpy()
    b = b.astype(np.float32).astype(np.float64)
    lam = float(np.max(np.abs(A.T @ b)))
    L = float(np.linalg.norm(A, "fro") ** 2)
    alphas = [(lam * 0.4 * 0.7 ** i, 0.5 if i % 3 == 1 else 0.0) for i in range(6)]
    refs = [orc.fista(A, b, "elasticnet", a1, a2, max_iter=15, L=L) for a1, a2 in alphas]
    return At, b.astype(np.float32), alphas, L, refs


def _check_path(xs, refs, same_as=None):
    for i, (x, x_ref) in enumerate(zip(xs, refs)):
        assert _data.rel(_np(x), x_ref) < TOL, i
        if same_as is not None:
            assert np.array_equal(_np(x), _np(same_as[i])), i


def test_replan_after_a_lockstep_run(fos):
    """A 6-weight path on the matrix cores in the one-read cluster form, then replan(cluster=False): the panel, the slab
    sets and the hand-off ring of the cluster layout go, the two-product layout is planned on the next run."""
    At, b, alphas, L, refs = _six_weights(fos, 8200, 4096, 5)
    prob = fos.prepare(At, b)
    prob.replan(cluster=True)
    _check_path(fos.fista_path(prob, None, alphas, max_iter=15, L=L), refs)
    assert prob.plan()["cluster"] == 1
    prob.replan(cluster=False)
    xs = fos.fista_path(prob, None, alphas, max_iter=15, L=L)
    assert prob.plan()["cluster"] == 0
    fresh = fos.prepare(At, b)
    fresh.replan(cluster=False)
    _check_path(xs, refs, same_as=fos.fista_path(fresh, None, alphas, max_iter=15, L=L))


def test_set_comm_after_a_lockstep_run(fos):
    """A 6-weight path, then a one-rank communicator attached with set_comm: the lockstep layout is planned again with
    the communicator in view (no one-read form, whose launch has no exchange step)."""
    from fastoptsolver_amd import distributed as fd
    At, b, alphas, L, refs = _six_weights(fos, 3000, 2048, 6)
    comm = fd.Comm.solo()
    prob = fos.prepare(At, b)
    _check_path(fos.fista_path(prob, None, alphas, max_iter=15, L=L), refs)
    xs = fos.fista_path(prob, None, alphas, max_iter=15, L=L, comm=comm)
    assert prob.comm is comm
    fresh = fos.prepare(At, b)
    _check_path(xs, refs, same_as=fos.fista_path(fresh, None, alphas, max_iter=15, L=L, comm=comm))


def test_set_comm_cols_after_an_fp64_pass(fos):
    """A streaming plan runs fos_gemv_pair_dd on its fp64 geometry, then becomes the one block of a column-sharded problem
    (one-rank communicator): the fp64 pass is planned again and takes the two-pass form with the residual exchange."""
    from fastoptsolver_amd import distributed as fd
    m, n = 600, 1024
    rng = np.random.default_rng(23)
    A = rng.standard_normal((m, n)).astype(np.float32)
    b = rng.standard_normal(m).astype(np.float32)
    x = rng.standard_normal(n) * (1.0 + 1e-9 * rng.standard_normal(n))
    At, xd = torch.as_tensor(A).cuda(), _dev(x, torch.float64)
    g_ref, rr_ref = orc.gram_gradient(A.astype(np.float64), x, b.astype(np.float64), 0.37)
    comm = fd.Comm.solo()

    def check(out, where):
        got = out.cpu().numpy()
        assert _data.rel(got[:n], g_ref) < 1e-12, where
        assert got[n] == pytest.approx(rr_ref, rel=1e-12), where

    prob = fos.prepare(At, b, pad=False)
    assert (prob.plan()["path"], prob.plan()["tall"], prob.plan()["colblock"]) == (0, 0, 0)
    check(_pair_dd(prob, xd), prob.plan())
    prob.set_comm_cols(comm)
    assert prob.plan()["colblock"] == 1
    out = _pair_dd(prob, xd)
    check(out, prob.plan())
    fresh = fos.prepare(At, b, pad=False)
    fresh.set_comm_cols(comm)
    assert torch.equal(_pair_dd(fresh, xd), out)


def test_distinct_handles_from_distinct_threads(fos):
    """include/fos.h: "a handle is single-threaded; distinct handles may be used from distinct threads".  Four threads, each
    with its own stream, problem (a different kernel family each: streaming fp32, bf16, chunk-per-lane, y-in-LDS) and solver
    handle, run concurrently - plain and device-controlled loops and the fp64 pass; every result equals, bit for bit, what
    the same calls give one after the other."""
    import threading
    from fastoptsolver_amd import _core, _lib
    shapes = [(3000, 2048, torch.float32), (2500, 4096, torch.bfloat16), (40000, 100, torch.float32), (300, 20000, torch.float32)]
    data = []
    for i, (m, n, dt) in enumerate(shapes):
        g = torch.Generator(device="cuda").manual_seed(100 + i)
        A = torch.randn(m, n, device="cuda", generator=g).to(dt)
        b = torch.randn(m, device="cuda", generator=g)
        data.append((A, b, 1.0 / float((A.float() ** 2).sum())))

    def work(i, out):
        A, b, tau = data[i]
        with torch.cuda.stream(torch.cuda.Stream()):
            prob = fos.prepare(A, b)
            res = []
            for kw in (dict(), dict(adaptive_restart=True, restart_threshold=1.0)):
                st = _core.Fista(prob); st.reset(tau, 0.5, 0.1, **kw)
                for _ in range(4):
                    st.run(25)
                res.append(st.x_tensor().clone())
            x64 = res[0].double()
            o = torch.zeros(prob.n_dev + 1, dtype=torch.float64, device="cuda")
            _lib.check(prob.lib.fos_gemv_pair_dd(prob.h, _core.ptr(x64), 0.1, _core.ptr(o)))
            res.append(o.clone())
            torch.cuda.current_stream().synchronize()
            out[i] = res

    seq, par = {}, {}
    for i in range(len(shapes)):
        work(i, seq)
    errors = []

    def guarded(i):
        try:
            work(i, par)
        except Exception as exc:        # surfaces in the main thread
            errors.append((i, repr(exc)))

    for _ in range(3):
        par.clear()
        threads = [threading.Thread(target=guarded, args=(i,)) for i in range(len(shapes))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for i in range(len(shapes)):
            for a, c in zip(seq[i], par[i]):
                assert torch.equal(a, c), (i, shapes[i])


@pytest.mark.parametrize("m,n", [(9000, 5), (20000, 5), (100000, 5), (300001, 8), (50000, 13), (40000, 16), (700, 3), (300, 3)])
def test_chip_resident_plain_loop(fos, m, n):
    """Opt-in (fos_fista_run_chip): tall-skinny plain runs with A resident in the LDS of up to all CUs and ONE grid barrier
    per iteration - every workgroup reads all partial gradients and updates its own copy of the iterate.  Against the oracle
    (1e-5) and the default two-launch loop (1e-6) for FISTA (lasso; l2 in the smooth
    part), FISTA-delta and fused ISTA with the elastic-net prox; adaptive restart and the ratio stop decided on the device; the
    state carries over between chip calls and between the two forms, step norms included; ill-conditioned columns (the
    reference's unstandardised features); unsupported runs refuse or fall through."""
    from fastoptsolver_amd import _core
    rng = np.random.default_rng(m + n)
    A = rng.standard_normal((m, n)).astype(np.float32)
    A[:, 0] *= 300.0                                          # unstandardised scale, as in easy_boston_data.py
    b = (A.astype(np.float64) @ rng.standard_normal(n) + rng.standard_normal(m)).astype(np.float32)
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    prob = fos.prepare(torch.as_tensor(A).cuda(), b)
    prob.replan(no_resident=True, chip_resident=False)       # run() = the two-launch loop; run_chip() is explicit below
    L = float(np.linalg.norm(A64, 2) ** 2)
    lam = float(np.max(np.abs(A64.T @ b64)))
    cases = [dict(mode=_core._lib.MODE_FISTA, a1=0.05 * lam, a2=0.0, kind=_core._lib.PROX_L1),
             dict(mode=_core._lib.MODE_FISTA, a1=0.02 * lam, a2=0.7, kind=_core._lib.PROX_L1),
             dict(mode=_core._lib.MODE_DELTA, a1=0.05 * lam, a2=0.0, kind=_core._lib.PROX_L1, delta=3.0),
             dict(mode=_core._lib.MODE_ISTA, a1=0.05 * lam, a2=0.5, kind=_core._lib.PROX_ENET)]
    for c in cases:
        tau = 1.0 / (L + (c["a2"] if c["kind"] == _core._lib.PROX_L1 and c["a2"] > 0 else 0.0))
        kw = dict(mode=c["mode"], delta=c.get("delta", 0.0), prox_kind=c["kind"])
        ref = _core.Fista(prob); ref.reset(tau, c["a1"], c["a2"], **kw); ref.run(40)
        ch = _core.Fista(prob); ch.reset(tau, c["a1"], c["a2"], **kw)
        served = ch.run_chip(7)
        if m < 512:
            assert not served
            return
        assert served and ch.run_chip(1) and ch.run_chip(12)           # state carries over between chip calls ...
        ch.run(10)                                                     # ... into the two-launch form ...
        assert ch.run_chip(10)                                         # ... and back
        xr, xc = ref.x_tensor().cpu().numpy(), ch.x_tensor().cpu().numpy()
        assert _data.rel(xc, xr) < 1e-6, c                              # (the two-launch plain loop hands y over as fp32)
        sr, sc = ref.status(), ch.status()
        # (near a fixed point the two-launch loop's step norms are the rounding noise of its fp32 y: absolute slack)
        slack = 1e-6 * float(np.linalg.norm(xr))
        assert int(sc.k) == int(sr.k) == 40 and sc.this_step == pytest.approx(sr.this_step, rel=1e-3, abs=slack)
        assert sc.prev_step == pytest.approx(sr.prev_step, rel=1e-3, abs=slack) and sc.rr == pytest.approx(sr.rr, rel=1e-5)
        if c["mode"] == _core._lib.MODE_FISTA:
            x_o = orc.fista(A64, b64, "elasticnet" if c["a2"] else "lasso", c["a1"], c["a2"], max_iter=40, L=L)
            assert _data.rel(xc, x_o) < TOL, c
    st = _core.Fista(prob); st.reset(1.0 / L, 0.05 * lam, 0.0, tol_grad=1e-3)
    assert not st.run_chip(3)                                          # the gradient-norm rule is not served
    # data-dependent control - adaptive restart, ratio stop - decided on the device by every workgroup alike: same iterate,
    # same restarts / stopping iteration as the two-launch loop with its one-wave bookkeeping kernel
    # (on STANDARDISED columns, where 40 iterations are still moving: with the x300 column above the loop is at its fixed point
    #  after two steps, the two-launch loop's step norms are then the rounding noise of its fp32 y against exact zeros here,
    #  and restart decisions on noise are not comparable)
    As = rng.standard_normal((m, n)).astype(np.float32)
    As[:, 1] += 0.9 * As[:, 0]
    probs = fos.prepare(torch.as_tensor(As).cuda(), b)
    probs.replan(no_resident=True, chip_resident=False)
    Ls = float(np.linalg.norm(As.astype(np.float64), 2) ** 2)
    lams = float(np.max(np.abs(As.astype(np.float64).T @ b64)))
    for ckw in (dict(adaptive_restart=True), dict(adaptive_restart=True, restart_threshold=0.9, tol_ratio=0.5), dict(tol_ratio=0.9)):
        ref = _core.Fista(probs); ref.reset(1.0 / Ls, 1e-3 * lams, 0.0, **ckw); ref.run(40)
        ch = _core.Fista(probs); ch.reset(1.0 / Ls, 1e-3 * lams, 0.0, **ckw)
        assert ch.run_chip(15) and ch.run_chip(10)
        ch.run(5)
        assert ch.run_chip(10)
        sr, sc = ref.status(), ch.status()
        assert (int(sc.k), int(sc.stopped), int(sc.restarts)) == (int(sr.k), int(sr.stopped), int(sr.restarts)), ckw
        assert _data.rel(ch.x_tensor().cpu().numpy(), ref.x_tensor().cpu().numpy()) < 1e-6, ckw
    # The Python boundary's plain calls take it by the planner's choice (n <= 8, up to 131072 rows) or by the plan flag
    # (FOS_PLAN_CHIP_RESIDENT: wherever served); flagged runs fall through to the two-launch loop.  Kernel timing tells
    # which loop ran: the chip loop is ONE profiled launch per call, the two-launch loop one per iteration.
    x_o = orc.fista(A64, b64, "lasso", 0.05 * lam, 0.0, max_iter=60, L=L)
    in_region = m >= 512 and (m <= 131072 if n <= 8 else m <= 32768)
    for force, expect_chip in ((None, in_region), (True, m >= 512), (False, False)):
        prob2 = fos.prepare(torch.as_tensor(A).cuda(), b)
        prob2.replan(no_resident=True, chip_resident=force)
        assert prob2.plan()["chip_resident"] == (1 if force else 0)
        prob2.profile(1); prob2.profile_read()
        x1 = fos.fista(prob2, None, "lasso", 0.05 * lam, 0.0, max_iter=60, L=L)
        launches = prob2.profile_read()[1]
        prob2.profile(0)
        assert _data.rel(_np(x1), x_o) < TOL, force
        assert (launches <= 2) == expect_chip, (force, launches)
    prob2 = fos.prepare(torch.as_tensor(A).cuda(), b)
    prob2.replan(no_resident=True, chip_resident=True)
    for fkw in (dict(adaptive_restart=True), dict(adaptive_restart=True, tol_ratio=0.7), dict(tol=1e-9 * lam), dict(backtracking=True)):
        x2 = fos.fista(prob2, None, "lasso", 0.05 * lam, 0.0, max_iter=60, L=L, **fkw)
        x_o2, met = orc.fista(A64, b64, "lasso", 0.05 * lam, 0.0, max_iter=60, L=L, return_metrics=True, **fkw)
        assert _data.rel(_np(x2), x_o2) < TOL, fkw
        assert fos.get_metrics()["grad_num_calls"] == met["grad_num_calls"], fkw
