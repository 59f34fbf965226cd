"""The working-set and certificate calls whose results tests/golden/ws_parent.npz and ws_refusals.json record from the commit
before the six entry points (fos_gradient_batch, fos_kkt_scan, fos_duality_gap and their multinomial namesakes) got one panel
walk, one certificate tail and one scan / column-pass kernel pair (a helper: no tests in here).  tests/test_gpu_ws_guard.py
repeats them and compares bitwise / byte for byte: neither a result nor a refusal changed.

compute(kind, shape): every family x width x X of one storage type at one shape through the `Problem` methods - G and the
loss sums of the gradient entry point, excess and the violators of the scan on that G, out64 of the certificate and whether
its G is the gradient entry point's.  Shapes: "one" (301 x 131: one row panel, rows and columns padded) and "panels" (the
two-panel shape of tests/_menu_cv.shapes on a 256-CU card: the copy of the loss partials and the panel offsets of b, the labels
and the row weights).  scans(kind): the scan alone on a synthetic G over n_dev = 2504 coordinates (three trips of 1024, the last
partial).  refusals(): (return code, fos_last_error) of every guard of the six entry points that a single card can meet, each
on a configuration that meets it and none before it.  (A multinomial handle is never sharded, never without labels and always
padded into the matrix-core pair, and feature groups refuse the multinomial loss when they are bound: those guards of the
multinomial entry points have no handle to meet.)"""
import ctypes as C

import numpy as np

from tests import _menu_cv as cv, _menu_multi as mm

KINDS = ("f32", "bf16")
SHAPES = ("one", "panels")
FAMILIES = ("squared", "squared_wp", "logistic_w", "huber", "hinge", "softmax3", "softmax7_gwp")
CLASSES = {"softmax3": 3, "softmax7_gwp": 7}
WIDTHS = ("wide", "narrow")                            # 16 and 3 columns; multinomial: 15 / 14 and one fit (3 / 7)
XS = ("sparse", "zero")
SLACK = 1e-4
SCAN_N, SCAN_NDEV = 2501, 2504
SCANS = ("plain16_factors", "plain3", "softmax3_l1", "softmax3_grouped", "softmax7_l1", "softmax7_grouped")


def shape(name, kind):
    if name == "one":
        return 301, 131
    case = cv.shapes(kind, mm.GPU_CUS)["panels"]
    return case["m"], case["n"]


def width(family, which):
    Cn = CLASSES.get(family)
    if Cn is None:
        return 16 if which == "wide" else 3
    return 16 // Cn * Cn if which == "wide" else Cn


def inputs(name, kind):
    m, n = shape(name, kind)
    rng = np.random.default_rng(20 + SHAPES.index(name))
    d = dict(m=m, n=n)
    d["A"] = rng.standard_normal((m, n)).astype(np.float32)
    d["b"] = rng.standard_normal(m).astype(np.float32).astype(np.float64)
    d["y"] = (d["b"] > 0).astype(np.float64)
    d["pm"] = np.where(d["b"] > 0, 1.0, -1.0)
    d["cls3"] = (np.arange(m) * 7 % 3).astype(np.float64)
    d["cls7"] = (np.arange(m) * 5 % 7).astype(np.float64)
    d["w"] = rng.uniform(0.25, 1.0, m).astype(np.float32).astype(np.float64)
    d["p"] = rng.uniform(0.5, 2.0, n).astype(np.float32).astype(np.float64)          # strictly positive
    d["p0"] = d["p"].copy()
    d["p0"][1] = 0.0                                   # outside the set of compute() (1 % 3 != 0): +inf in the scan
    X = 0.1 * rng.standard_normal((n, 16)) * (rng.random((n, 16)) < 0.2)
    d["X"] = X.astype(np.float32)
    return d


def handles(fos, torch, d, kind):
    At = torch.as_tensor(d["A"]).to(torch.bfloat16 if kind == "bf16" else torch.float32).cuda()
    return {
        "squared": fos.prepare(At, d["b"], pad=True),
        "squared_wp": fos.prepare_penalized(At, d["b"], d["p"], sample_weight=d["w"]),
        "logistic_w": fos.prepare_weighted(At, d["y"], d["w"], loss="logistic"),
        "huber": fos.prepare_huber(At, d["b"], 0.75),
        "hinge": fos.prepare_hinge(At, d["pm"]),
        "softmax3": fos.prepare_multinomial(At, d["cls3"], 3),
        "softmax7_gwp": fos.prepare_multinomial(At, d["cls7"], 7, sample_weight=d["w"], penalty_factor=d["p0"], grouped=True),
    }


def _np(t):
    return t.detach().cpu().numpy()


def compute(fos, torch, kind, name):
    """{case/field: ndarray} of one storage type at one shape."""
    d = inputs(name, kind)
    hs = handles(fos, torch, d, kind)
    out = {}
    for family in FAMILIES:
        P, Cn = hs[family], CLASSES.get(family)
        in_ws = torch.as_tensor((np.arange(P.n_dev) % 3 == 0).astype(np.uint8)).cuda()
        for which in WIDTHS:
            nv = width(family, which)
            fits = nv // (Cn or 1)
            for xk in XS:
                X = torch.as_tensor(d["X"][:, :nv] if xk == "sparse" else np.zeros((d["n"], nv), np.float32)).cuda()
                key = f"{kind}/{name}/{family}/{which}/{xk}"
                G, loss = (P.multinomial_gradient_block if Cn else P.gradient_block)(X, want_loss=True)
                top = float(G.abs().max())
                a1 = [top * (0.2 + 0.7 * j / max(fits - 1, 1)) for j in range(fits)]     # violators and coordinates at rest
                a2 = [0.0 if j % 2 == 0 else 0.1 * (j + 1) for j in range(fits)]         # both branches of the scale
                excess, viol = (P.multinomial_kkt_scan if Cn else P.kkt_scan)(G, a1, SLACK, in_ws)
                out64, Gc = (P.multinomial_duality_gap_block if Cn else P.duality_gap_block)(X, a1, a2)
                out[key + "/G"] = _np(G)
                out[key + "/loss"] = np.asarray(loss, dtype=np.float64)
                out[key + "/excess"] = _np(excess)
                out[key + "/viol"] = _np(viol)
                out[key + "/out64"] = _np(out64)
                out[key + "/same_G"] = np.array(bool(torch.equal(G, Gc)))
    return out


def scans(fos, torch, kind):
    """{case/field: ndarray}: the scan alone, on a synthetic G over three trips of the workgroup."""
    tdtype = torch.bfloat16 if kind == "bf16" else torch.float32
    rng = np.random.default_rng(77)
    p = (10.0 ** rng.uniform(-1.0, 1.0, size=SCAN_N)).astype(np.float32).astype(np.float64)
    p[[1, 1030, 2500]] = 0.0                           # outside the set below: +inf where G is not 0
    y = np.arange(8)
    At = torch.zeros(8, SCAN_N, dtype=tdtype, device="cuda")
    in_ws = np.zeros(SCAN_NDEV, dtype=np.uint8)
    in_ws[rng.random(SCAN_NDEV) < 0.3] = 3
    in_ws[[1, 1030, 2500]] = 0
    out = {}
    for case in SCANS:
        if case.startswith("plain"):
            nv, Cn, grouped = (16, None, False) if case == "plain16_factors" else (3, None, False)
            P = fos.prepare_penalized(At, np.zeros(8), p) if case == "plain16_factors" else fos.prepare(At, np.zeros(8), pad=True)
        else:
            Cn, grouped = int(case[7]), case.endswith("grouped")
            nv = 16 // Cn * Cn
            P = fos.prepare_multinomial(At, (y % Cn).astype(np.float64), Cn, penalty_factor=p)
        assert P.n_dev == SCAN_NDEV, P.n_dev
        fits = nv // (Cn or 1)
        G = np.zeros((nv, SCAN_NDEV), dtype=np.float32)
        G[:, :SCAN_N] = rng.standard_normal((nv, SCAN_N)).astype(np.float32)
        G[:, 5] = 0.0
        a1 = rng.uniform(1.5, 3.0, size=fits)
        Gd, md = torch.as_tensor(G).cuda(), torch.as_tensor(in_ws).cuda()
        if Cn:
            excess, viol = P.multinomial_kkt_scan(Gd, list(a1), SLACK, md, grouped=grouped)
        else:
            excess, viol = P.kkt_scan(Gd, list(a1), SLACK, md)
        ex, vi = _np(excess), _np(viol)
        # the scenario, not the arithmetic: violators in every trip and on both sides of a wave boundary, coordinates at rest too
        assert all(((vi >= lo) & (vi < hi)).any() for lo, hi in ((0, 1024), (1024, 2048), (2048, SCAN_NDEV))), case
        assert ((vi % 64 == 63).any() and (vi % 64 == 0).any()) and 0 < vi.size < int((in_ws == 0).sum()), case
        assert case == "plain3" or np.isinf(ex).any(), case
        out[f"{kind}/scan/{case}/excess"] = ex
        out[f"{kind}/scan/{case}/viol"] = vi
    return out


# ---- refusals ----------------------------------------------------------------------------------------------------------------
RM, RN = 67, 200


def refusals(fos, torch):
    """{"entry/guard": [code, message]}."""
    from fastoptsolver_amd.distributed import Comm
    rng = np.random.default_rng(3)
    At = torch.as_tensor(rng.standard_normal((RM, RN)).astype(np.float32)).cuda()
    b = rng.standard_normal(RM).astype(np.float32).astype(np.float64)
    y = (np.arange(RM) % 3).astype(np.float64)
    sq = fos.prepare(At, b, pad=True)
    sharded = fos.prepare(At, b)
    sharded.set_comm(Comm.solo())
    H = dict(sq=sq, no_b=fos.prepare(At, pad=True), sharded=sharded,
             narrow=fos.prepare(torch.zeros(100, 4, device="cuda"), torch.zeros(100)),
             box=fos.prepare_penalized(At, b, None, 0.0, None), fgroups=fos.prepare_grouped(At, b, [5] * (RN // 5)),
             mn=fos.prepare_multinomial(At, y, 3), mn_box=fos.prepare_multinomial(At, y, 3, lower=0.0))
    lib = sq.lib
    X = torch.zeros(RN, 16, device="cuda")
    G = torch.zeros(16, RN, device="cuda")
    out64 = torch.zeros(64, dtype=torch.float64, device="cuda")
    ex = torch.zeros(RN, device="cuda")
    vi, cnt = torch.zeros(RN, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    in_ws = torch.zeros(RN, dtype=torch.uint8, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    good = (C.c_double * 16)(*([0.5] * 16))
    bad = (C.c_double * 16)(*([0.5, -1.0] + [0.5] * 14))
    nan = float("nan")

    def grad(P, nv=6, x=X):
        return lib.fos_gradient_batch(ptr(x) if x is not None else None, nv, P.h, ptr(G), None)

    def scan(P, nv=6, a=good, slack=0.0):
        return lib.fos_kkt_scan(ptr(G), nv, a, slack, ptr(in_ws), P.h, ptr(ex), ptr(vi), ptr(cnt))

    def gap(P, nv=6, a1=good, a2=good):
        return lib.fos_duality_gap(ptr(X), nv, a1, a2, P.h, ptr(G), ptr(out64))

    def mgrad(P, nv=6, x=X):
        return lib.fos_multinomial_gradient_batch(ptr(x) if x is not None else None, nv, P.h, ptr(G), None)

    def mscan(P, nv=6, a=good, slack=0.0, grouped=0):
        return lib.fos_multinomial_kkt_scan(ptr(G), nv, grouped, a, slack, ptr(in_ws), P.h, ptr(ex), ptr(vi), ptr(cnt))

    def mgap(P, nv=6, a1=good, a2=good, grouped=0):
        return lib.fos_multinomial_duality_gap(ptr(X), nv, grouped, a1, a2, P.h, ptr(G), ptr(out64))

    table = {
        "fos_gradient_batch": [("arg_nv", lambda: grad(sq, nv=0)), ("arg_null", lambda: grad(sq, x=None)),
                               ("multinomial", lambda: grad(H["mn"])), ("no_b", lambda: grad(H["no_b"])),
                               ("sharded", lambda: grad(H["sharded"])), ("no_pair", lambda: grad(H["narrow"], nv=2))],
        "fos_kkt_scan": [("arg_nv", lambda: scan(sq, nv=17)), ("slack_negative", lambda: scan(sq, slack=-1.0)),
                         ("slack_nan", lambda: scan(sq, slack=nan)), ("weight", lambda: scan(sq, a=bad)),
                         ("box", lambda: scan(H["box"])), ("fgroups", lambda: scan(H["fgroups"])),
                         ("multinomial", lambda: scan(H["mn"]))],
        "fos_duality_gap": [("arg_nv", lambda: gap(sq, nv=0)), ("weight_alpha1", lambda: gap(sq, a1=bad)),
                            ("weight_alpha2", lambda: gap(sq, a2=bad)), ("multinomial", lambda: gap(H["mn"])),
                            ("no_b", lambda: gap(H["no_b"])), ("sharded", lambda: gap(H["sharded"])),
                            ("no_pair", lambda: gap(H["narrow"], nv=2)), ("box", lambda: gap(H["box"])),
                            ("fgroups", lambda: gap(H["fgroups"]))],
        "fos_multinomial_gradient_batch": [("arg_nv", lambda: mgrad(H["mn"], nv=17)), ("arg_null", lambda: mgrad(H["mn"], x=None)),
                                           ("not_multinomial", lambda: mgrad(sq)), ("not_a_multiple", lambda: mgrad(H["mn"], nv=4))],
        "fos_multinomial_kkt_scan": [("arg_nv", lambda: mscan(H["mn"], nv=0)), ("arg_grouped", lambda: mscan(H["mn"], grouped=2)),
                                     ("slack_negative", lambda: mscan(H["mn"], slack=-1.0)), ("not_multinomial", lambda: mscan(sq)),
                                     ("not_a_multiple", lambda: mscan(H["mn"], nv=4)), ("weight", lambda: mscan(H["mn"], a=bad)),
                                     ("box", lambda: mscan(H["mn_box"]))],
        "fos_multinomial_duality_gap": [("arg_nv", lambda: mgap(H["mn"], nv=0)), ("arg_grouped", lambda: mgap(H["mn"], grouped=-1)),
                                        ("not_multinomial", lambda: mgap(sq)), ("not_a_multiple", lambda: mgap(H["mn"], nv=4)),
                                        ("weight_alpha1", lambda: mgap(H["mn"], a1=bad)), ("weight_alpha2", lambda: mgap(H["mn"], a2=bad)),
                                        ("box", lambda: mgap(H["mn_box"]))],
    }
    out = {}
    for entry, rows in table.items():
        for guard, call in rows:
            rc = int(call())
            out[f"{entry}/{guard}"] = [rc, lib.fos_last_error().decode("utf-8") if rc != 0 else ""]
    return out
