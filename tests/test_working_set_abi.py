"""CPU: the three entry points of include/fos_working_set.h (fos_gradient_batch, fos_gather_columns, fos_kkt_scan) are exported,
bound and declared with the signatures the header documents, stand outside the closed list of fos.h, and refuse bad arguments
before any HIP call; working_set_path, kkt_excess and alpha_max refuse what they do not serve before any device work.

fos_gather_columns reads n from the handle for its first range check (n_ws outside 1..n), so the stand-in handle of this file -
never dereferenced - reaches its pointer checks only; its scalar checks run against a real handle in tests/test_gpu_working_set.py."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

NEW = ("fos_gradient_batch", "fos_gather_columns", "fos_kkt_scan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
P, D = ctypes.c_void_p(0x1000), lambda k=0: ctypes.c_void_p(0x2000 + 0x100 * k)     # stand-ins: never dereferenced


@pytest.fixture(scope="module")
def lib():
    from fastoptsolver_amd import build, _lib
    build.build()
    return _lib.load()


def _header(name="fos_working_set.h"):
    with open(os.path.join(ROOT, "include", name)) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def test_symbols_exported_bound_and_declared(lib):
    from fastoptsolver_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = _header()
    assert sorted(re.findall(r"\b(fos_[a-z0-9_]+)\s*\(", header)) == sorted(NEW) == sorted(_lib.WORKING_SET_SIGNATURES)
    for name in NEW:
        assert f" T {name}" in out, name
        assert name not in _lib.SIGNATURES                      # that table is fos.h itself
        assert getattr(lib, name).argtypes == _lib.WORKING_SET_SIGNATURES[name][1]
    assert lib.fos_abi_version() == 3                           # the ABI only grew
    sig = r"\s*,\s*".join
    assert re.search(r"int\s+fos_gradient_batch\s*\(\s*" + sig([r"const\s+float\s*\*\s*X", r"int\s+nv", r"fos_problem\s*\*\s*p",
                                                                  r"float\s*\*\s*G", r"double\s*\*\s*loss16"]) + r"\s*\)", header)
    assert re.search(r"int\s+fos_gather_columns\s*\(\s*" + sig([r"const\s+int32_t\s*\*\s*idx", r"int32_t\s+n_ws", r"void\s*\*\s*A_ws",
                                                                  r"int64_t\s+lda_ws", r"int32_t\s+n_ws_pad",
                                                                  r"const\s+fos_problem\s*\*\s*p"]) + r"\s*\)", header)
    assert re.search(r"int\s+fos_kkt_scan\s*\(\s*" + sig([r"const\s+float\s*\*\s*G", r"int\s+nv", r"const\s+double\s*\*\s*alpha1",
                                                            r"double\s+slack", r"const\s+uint8_t\s*\*\s*in_ws", r"fos_problem\s*\*\s*p",
                                                            r"float\s*\*\s*excess", r"int32_t\s*\*\s*viol_idx",
                                                            r"int32_t\s*\*\s*viol_count"]) + r"\s*\)", header)


def test_the_closed_list_of_fos_h_did_not_grow():
    from tests import _logit_guard as gd
    fos_h = _header("fos.h")
    assert not [n for n in NEW if re.search(r"\b" + n + r"\b", fos_h)]
    assert not (set(NEW) & gd.header_handle_functions())
    assert gd.header_handle_functions() == gd.SERVES | gd.LOSS_FREE | gd.REFUSES


def test_kernels_live_in_their_own_header_and_use_no_atomics():
    with open(os.path.join(ROOT, "fastoptsolver_amd", "csrc", "working_set.hpp")) as fh:
        code = re.sub(r"//[^\n]*", "", fh.read())
    assert re.search(r"template\s*<int ESZ>\s*static\s+__global__\s+__launch_bounds__\(WS_THREADS\)\s+void\s+gather_columns_kernel", code)
    assert re.search(r"__global__\s+__launch_bounds__\(KS_THREADS\)\s+void\s+kkt_scan_kernel", code)
    assert "__builtin_nontemporal_load" in code and not re.search(r"atomic", code, flags=re.I)
    # the scan's body is written once for every loss family (C columns of a fit seen together) and kkt_scan_kernel is its
    # instantiation with C = 1, l1 known at compile time; that part of the header - comments too - has no atomics, flags or
    # waits, and the grouped decision compares squares: the one square root of the body feeds the excess alone
    assert re.search(r"template\s*<bool ONE_COLUMN>\s*__device__\s+__forceinline__\s+void\s+kkt_scan_body\(", code)
    assert re.search(r"kkt_scan_kernel\([^)]*\)\s*\{\s*kkt_scan_body<true>\(G, n, nv, 1, 0, w,", code)
    assert code.count("__global__") == 2
    with open(os.path.join(ROOT, "fastoptsolver_amd", "csrc", "working_set.hpp")) as fh:
        text = fh.read()
    for word in ("atomic", "volatile", "while", "__threadfence", "asm"):
        assert not re.search(word, text[text.index("---- KKT scan"):], flags=re.I), word
    scan = code[code.index("kkt_scan_body"):]
    assert scan.count("sqrt(") == 1 and re.search(r"viol\s*=\s*viol\s*\|\|\s*q\s*>\s*thr\s*\*\s*thr", scan)
    from fastoptsolver_amd import build
    assert os.path.join(ROOT, "include", "fos_working_set.h") in build.HEADERS
    assert os.path.join(ROOT, "fastoptsolver_amd", "csrc", "working_set.hpp") in build.HEADERS


@pytest.mark.parametrize("case", ["null_X", "null_p", "null_G", "nv_0", "nv_17", "nv_minus_1"])
def test_gradient_batch_argument_checks(lib, case):
    X, nv, p, G = D(0), 3, P, D(1)
    if case == "null_X":
        X = None
    elif case == "null_p":
        p = None
    elif case == "null_G":
        G = None
    else:
        nv = {"nv_0": 0, "nv_17": 17, "nv_minus_1": -1}[case]
    for loss16 in (None, D(2)):                                  # loss16 may be NULL: it is never the reason
        assert lib.fos_gradient_batch(X, nv, p, G, loss16) == ARG
        assert "fos_gradient_batch" in lib.fos_last_error().decode()


@pytest.mark.parametrize("case", ["null_idx", "null_A_ws", "null_p", "all_null"])
def test_gather_columns_pointer_checks(lib, case):
    idx, A_ws, p = D(0), D(1), P
    if case in ("null_idx", "all_null"):
        idx = None
    if case in ("null_A_ws", "all_null"):
        A_ws = None
    if case in ("null_p", "all_null"):
        p = None
    assert lib.fos_gather_columns(idx, 8, A_ws, 8, 8, p) == ARG
    assert "fos_gather_columns" in lib.fos_last_error().decode()


@pytest.mark.parametrize("case", ["null_G", "null_alpha1", "null_in_ws", "null_p", "null_excess", "null_viol_idx", "null_viol_count",
                                  "nv_0", "nv_17", "alpha_negative", "alpha_nan", "alpha_inf", "slack_negative", "slack_nan"])
def test_kkt_scan_argument_checks(lib, case):
    a = (ctypes.c_double * 16)(*([0.5] * 16))
    args = dict(G=D(0), nv=3, alpha1=a, slack=1e-4, in_ws=D(1), p=P, excess=D(2), viol_idx=D(3), viol_count=D(4))
    if case.startswith("null_"):
        args[case[5:]] = None
    elif case.startswith("nv_"):
        args["nv"] = int(case[3:])
    elif case.startswith("alpha_"):
        a[2] = {"negative": -1e-300, "nan": float("nan"), "inf": float("inf")}[case[6:]]
    else:
        args["slack"] = {"negative": -1e-12, "nan": float("nan")}[case[6:]]
    assert lib.fos_kkt_scan(*args.values()) == ARG
    assert "fos_kkt_scan" in lib.fos_last_error().decode()


A, B = np.ones((10, 4)), np.arange(10.0) / 10.0


def test_python_refusals_come_before_any_device_work():
    """No GPU here: a call that got past the host checks would raise FosError, not ValueError."""
    import fastoptsolver_amd as fos
    from fastoptsolver_amd import _core, working_set
    for kw in (dict(grow=1.0), dict(max_fraction=0.0), dict(max_fraction=1.5), dict(max_rounds=0), dict(kkt_tol=-1.0)):
        with pytest.raises(ValueError):
            fos.working_set_path(A, B, [(0.1, 0.0)], **kw)
    with pytest.raises(ValueError):
        fos.working_set_path(A, B, [])
    with pytest.raises(ValueError):
        fos.working_set_path(A, None, [(0.1, 0.0)])

    def handle(**kw):                    # what _handle reads of a Problem, without a device
        h = _core.Problem.__new__(_core.Problem)
        h.loss, h.grouped, h._coord, h._fgroups, h.n, h.b = "squared", False, (None, None, None), None, 4, object()
        for k, v in kw.items():
            setattr(h, k, v)
        h.h = None
        return h
    lo = types.SimpleNamespace(__getitem__=None)
    for bad, word in ((handle(loss="multinomial"), "multinomial"), (handle(grouped=True), "group penalty"),
                      (handle(_coord=(None, np.zeros(4), None)), "bounds"), (handle(_coord=(None, None, np.zeros(4))), "bounds"),
                      (handle(_fgroups=(lo, lo, 0.0)), "feature groups"), (handle(comm=object()), "sharded"),
                      (handle(col_sharded=True), "sharded"), (handle(b=None), "without b")):
        for call in (lambda: fos.working_set_path(bad, None, [(0.1, 0.0)]), lambda: fos.kkt_excess(bad, np.zeros(4), [(0.1, 0.0)]),
                     lambda: fos.alpha_max(bad)):
            with pytest.raises(ValueError, match=word):
                call()
    # alpha1 = 0 on a penalised coordinate: the working set would be everything
    with pytest.raises(ValueError, match="alpha1 = 0"):
        working_set._check_weights(handle(n_dev=4), [(0.1, 0.0), (0.0, 0.5)])


def test_signatures():
    import fastoptsolver_amd as fos
    ws = inspect.signature(fos.working_set_path).parameters
    assert list(ws) == ["A", "b", "alphas", "max_iter", "kkt_tol", "max_rounds", "grow", "max_fraction", "L", "t_init_factor", "dtype",
                        "initial", "return_info"]
    assert [ws[k].default for k in ("max_iter", "kkt_tol", "max_rounds", "grow", "max_fraction", "t_init_factor")] == [500, 1e-4, 20, 2.0, 0.5, 1.0]
    assert all(ws[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(ws)[4:])
    assert list(inspect.signature(fos.kkt_excess).parameters) == ["prob", "X", "alphas"]
    assert list(inspect.signature(fos.alpha_max).parameters) == ["prob"]
    assert fos.WorkingSetInfo._fields == ("rounds", "sizes", "full_gradients", "worst_excess", "fell_back")
