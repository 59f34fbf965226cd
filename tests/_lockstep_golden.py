"""The lockstep calls whose results tests/golden/lockstep_parent.npz and lockstep_refusals.json record from the commit before the
lockstep got one route decision and one separable update launch (a helper: no tests in here).  tests/test_gpu_lockstep_guard.py
repeats them and compares bitwise / byte for byte: neither a result nor a refusal changed.

compute(): every update form of the matrix-core lockstep on the 1001 x 200 recipe of tests/_logit_golden.py (rows padded, the
last 64-column update workgroup partial), fp32 and bf16 storage, 30 iterations, at most 6 columns per case; x of every handle
and (k, restarts, stopped).  The plain squared-loss cases run 5 or 6 handles: up to 4 fp32 handles take the VALU multi-vector
pass (tests/_menu_multi.lockstep_form), which is not the lockstep recorded here; every other case is served by the matrix-core
pair alone.  refusals(): (return code, fos_last_error) of the three entry points over problem kind x handles x
nv at one small shape, at most 2 iterations; a refused call must also leave x and the status of every handle as they were."""
import ctypes as C

import numpy as np

from tests import _logit_golden as base

M, N, ITERS = base.M, base.N, base.ITERS
CONTROL = dict(adaptive_restart=True, tol_ratio=1e-3)
FGROUP_SIZES = (5, 3, 8, 4) * 10                       # 200 columns in 40 contiguous groups
RM, RN, RITERS = 300, 200, 2                           # the shape and the iterations of the refusal calls


def inputs():
    """A (fp32), b, the labels and classes derived from b, row weights, factors, bounds, fold ids, a block B, L, max |A^T b|."""
    A32, b, _, L = base.inputs()
    rng = np.random.default_rng(base.SEED + 1)
    d = dict(A=A32, b=b, L=L)
    d["amax"] = float(np.max(np.abs(A32.astype(np.float64).T @ b)))
    d["y"] = (b > np.median(b)).astype(np.float64)
    d["cls"] = np.digitize(b, np.quantile(b, [1 / 3, 2 / 3])).astype(np.float64)          # 0, 1, 2
    d["w"] = rng.uniform(0.25, 1.0, M).astype(np.float32).astype(np.float64)
    d["p"] = rng.uniform(0.5, 2.0, N).astype(np.float32).astype(np.float64)
    d["p"][::17] = 0.0
    d["lo"] = np.where(rng.random(N) < 0.5, -0.05, -np.inf)
    d["hi"] = np.where(rng.random(N) < 0.5, 0.08, np.inf)
    d["folds"] = (np.arange(M) % base.K).astype(np.uint8)
    A64 = A32.astype(np.float64)
    d["amax_logit"] = float(np.max(np.abs(A64.T @ (d["w"] * (d["y"] - 0.5)))))
    d["amax_soft"] = float(np.max(np.abs(A64.T @ ((d["cls"][:, None] == np.arange(3)) - 1.0 / 3.0))))
    d["B"] = np.stack([b, np.roll(b, 1), -b, 0.5 * b + np.roll(b, 7), np.roll(b, 3) - 0.25 * b], axis=1).astype(np.float32)
    return d


def _specs(d, form, amax="amax"):
    """reset() keyword sets of one case: (alpha1, alpha2, keywords); amax: the key of the problem's max |gradient at 0|."""
    from fastoptsolver_amd import _lib
    a = d[amax]
    l1, enet, delta = dict(prox_kind=_lib.PROX_L1), dict(prox_kind=_lib.PROX_ENET), dict(mode=_lib.MODE_DELTA, delta=3.0)
    if form == "l1":
        return [(0.3 * a, 0.0, l1), (0.1 * a, 0.5, l1), (0.05 * a, 1.0, l1), (0.2 * a, 0.0, l1), (0.15 * a, 0.25, l1)]
    if form == "enet":
        return [(0.3 * a, 0.5, enet), (0.1 * a, 0.5, enet), (0.05 * a, 1.0, enet), (0.2 * a, 0.0, enet), (0.15 * a, 0.25, enet)]
    if form == "ctrl":
        return [(0.3 * a, 0.0, dict(l1, **CONTROL)), (0.1 * a, 0.5, dict(l1, **CONTROL)), (0.05 * a, 1.0, dict(l1, **CONTROL))]
    if form == "mixed":                                # two families and both prox kinds in one plain call
        return [(0.1 * a, 0.5, l1), (0.05 * a, 1.0, dict(delta, **enet)), (0.1 * a, 0.5, dict(delta, **l1)), (0.2 * a, 0.5, enet),
                (0.3 * a, 0.0, dict(delta, **l1)), (0.15 * a, 0.25, l1)]
    raise KeyError(form)


def _handles(P, L, specs, group=0, x0=None):
    from fastoptsolver_amd import _core
    hs = []
    for a1, a2, kw in specs:
        st = _core.Fista(P)
        st.reset(1.0 / (L + 2.0 * a2), a1, a2, group=group, x0=x0, **kw)       # (factors are at most 2)
        hs.append(st)
    return hs


def _record(out, name, hs):
    out[name + "/x"] = np.stack([st.x_tensor().detach().cpu().numpy().astype(np.float64) for st in hs], axis=1)
    out[name + "/status"] = np.array([[int(s.k), int(s.restarts), int(s.stopped)] for s in (st.status() for st in hs)], dtype=np.int64)


def compute(fos, torch):
    """{name: ndarray}: x (n x nv, float64) and status (nv x 3, int64) of every case."""
    from fastoptsolver_amd import _core
    d = inputs()
    L = d["L"]
    out = {}
    for kind, tdtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        At = torch.as_tensor(d["A"]).to(tdtype).cuda()
        plain = fos.prepare(At, d["b"])
        coord = fos.prepare_penalized(At, d["b"], d["p"], d["lo"], d["hi"])
        for tag, P in (("sq", plain), ("coord", coord)):
            for form in ("l1", "enet", "ctrl", "mixed"):
                hs = _handles(P, L, _specs(d, form))
                assert _core.run_multi(hs, ITERS), (tag, form)
                _record(out, f"{kind}/{tag}_{form}", hs)
        hs = _handles(plain, L, _specs(d, "l1"))
        assert _core.run_multi_rhs(hs, torch.as_tensor(d["B"]).cuda(), ITERS)
        _record(out, f"{kind}/rhs", hs)
        hs = _handles(plain, L, _specs(d, "l1"))
        assert _core.run_multi_folds(hs, _core.fold_ids_tensor(d["folds"], At.device), [0, 1, -1, 4, 2], ITERS)
        _record(out, f"{kind}/folds", hs)
        wlogit = fos.prepare_weighted(At, d["y"], d["w"], loss="logistic")
        hs = _handles(wlogit, L, _specs(d, "l1", "amax_logit"))
        assert _core.run_multi(hs, ITERS)
        _record(out, f"{kind}/wlogit", hs)
        soft = fos.prepare_multinomial(At, d["cls"], 3)
        hs = _handles(soft, L, [s for s in _specs(d, "l1", "amax_soft")[:2] for _ in range(3)])
        assert _core.run_multi(hs, ITERS)
        _record(out, f"{kind}/softmax", hs)
        factors = fos.prepare_penalized(At, d["b"], d["p"])
        hs = _handles(factors, L, [s for s in _specs(d, "enet")[:2] for _ in range(2)], group=2)
        assert _core.run_multi(hs, ITERS)
        _record(out, f"{kind}/group", hs)
        for ratio in (0.0, 0.5):
            fg = fos.prepare_grouped(At, d["b"], list(FGROUP_SIZES), l1_ratio=ratio)
            for form in ("l1", "mixed", "ctrl"):
                hs = _handles(fg, L, _specs(d, form)[:3])
                assert _core.run_multi(hs, ITERS), (ratio, form)
                _record(out, f"{kind}/fgroup{ratio}_{form}", hs)
    return out


# ---- refusals ----------------------------------------------------------------------------------------------------------------
ENTRIES = ("fos_fista_run_multi", "fos_fista_run_multi_rhs", "fos_fista_run_multi_folds")
KINDS = ("squared", "logistic", "weighted", "factors", "bounds", "softmax3", "softmax2", "fgroups", "no_b")
HANDLES = ("plain", "ctrl_one_family", "ctrl_mixed", "tol_grad", "group2", "group3", "group2_mismatch", "group2_ungrouped",
           "plain_heldsplit", "group2_heldsplit")
NVS = (1, 2, 3)


def refusal_problems(fos, torch):
    d = inputs()
    A = torch.as_tensor(d["A"][:RM, :RN]).cuda()
    b, y, cls, w, p = d["b"][:RM], d["y"][:RM], d["cls"][:RM], d["w"][:RM], d["p"][:RN]
    return {
        "squared": fos.prepare(A, b),
        "logistic": fos.prepare(A, y, loss="logistic"),
        "weighted": fos.prepare_weighted(A, b, w),
        "factors": fos.prepare_penalized(A, b, p),
        "bounds": fos.prepare_penalized(A, b, p, d["lo"][:RN], d["hi"][:RN]),
        "softmax3": fos.prepare_multinomial(A, cls, 3),
        "softmax2": fos.prepare_multinomial(A, y, 2),
        "fgroups": fos.prepare_grouped(A, b, list(FGROUP_SIZES), l1_ratio=0.5),
        "no_b": fos.prepare(A),
    }


def _refusal_handles(P, which, nv, x0):
    from fastoptsolver_amd import _core, _lib
    hs = []
    for v in range(nv):
        kw, a1 = {}, 0.1 + 0.01 * v
        if which == "ctrl_one_family":
            kw = dict(CONTROL)
        elif which == "ctrl_mixed":
            kw = dict(CONTROL, mode=_lib.MODE_FISTA if v == 0 else _lib.MODE_DELTA, delta=0.0 if v == 0 else 3.0)
        elif which == "tol_grad":
            kw = dict(tol_grad=1e-3) if v == 0 else {}
        elif which in ("group2", "group2_heldsplit"):
            kw, a1 = dict(group=2), 0.1 + 0.01 * (v // 2)
        elif which == "group3":
            kw, a1 = dict(group=3), 0.1 + 0.01 * (v // 3)
        elif which == "group2_mismatch":
            kw = dict(group=2)                           # a1 differs inside the fit
        elif which == "group2_ungrouped":
            kw = dict(group=2 if v == 0 else 0)
        st = _core.Fista(P)
        st.reset(1e-4, a1, 0.5, x0=x0, **kw)
        hs.append(st)
    return hs


def _snapshot(hs):
    out = []
    for st in hs:
        s = st.status()
        out.append((st.x_tensor().clone(), tuple(getattr(s, k) for k, _ in s._fields_)))
    return out


def refusals(fos, torch, problems=None):
    """{"entry/kind/handles/nv": [code, message]} (message "" for a served call).  A refused call that changed x or the status
    of a handle raises AssertionError."""
    from fastoptsolver_amd import _core
    problems = problems or refusal_problems(fos, torch)
    out = {}
    for kind in KINDS:
        P = problems[kind]
        lib = P.lib
        x0 = torch.linspace(-1.0, 1.0, P.n, dtype=torch.float64, device=P.device)
        B = torch.zeros(RM, 3, dtype=torch.float32, device=P.device)
        folds = _core.fold_ids_tensor(np.arange(RM) % 3, P.device)
        for which in HANDLES:
            for nv in NVS:
                for entry in ENTRIES:
                    if which.endswith("heldsplit") and entry != "fos_fista_run_multi_folds":
                        continue
                    hs = _refusal_handles(P, which, nv, x0)
                    arr = (C.c_void_p * nv)(*[h.h for h in hs])
                    before = _snapshot(hs)
                    with P.ctx():
                        if entry == "fos_fista_run_multi":
                            rc = lib.fos_fista_run_multi(arr, nv, RITERS)
                        elif entry == "fos_fista_run_multi_rhs":
                            rc = lib.fos_fista_run_multi_rhs(arr, nv, _core.ptr(B), 3, RITERS)
                        else:
                            held = [v % 2 for v in range(nv)] if which.endswith("heldsplit") else [0] * nv
                            rc = lib.fos_fista_run_multi_folds(arr, nv, RITERS, _core.ptr(folds), (C.c_int32 * nv)(*held))
                    key = f"{entry}/{kind}/{which}/{nv}"
                    out[key] = [int(rc), lib.fos_last_error().decode("utf-8") if rc != 0 else ""]
                    if rc != 0:
                        for (xa, sa), (xb, sb) in zip(before, _snapshot(hs)):
                            assert torch.equal(xa, xb) and sa == sb, (key, sa, sb)
    return out
