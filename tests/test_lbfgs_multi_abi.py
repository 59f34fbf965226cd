"""CPU: the lockstep L-BFGS entry points (fos_gemv_pair_dd_multi, fos_lbfgs_minimize_multi) are exported, declared and
bound, and refuse bad arguments before any HIP call; LBFGSSolver.fit refuses what a 2-D b cannot be combined with."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fos_gemv_pair_dd_multi", "fos_lbfgs_minimize_multi")


@pytest.fixture(scope="module")
def lib():
    from fastoptsolver_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_exported_declared_and_bound(lib):
    from fastoptsolver_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fos.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert f" T {name}" in out, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in doc, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def _err(lib):
    return lib.fos_last_error().decode()


def _dbuf(n=64):
    return ctypes.cast((ctypes.c_double * n)(), ctypes.c_void_p)


@pytest.mark.parametrize("case", ["null_p", "null_X", "null_B", "null_G", "null_rr", "nv_0", "nv_17", "ldb_lt_nv", "ldx_lt_n"])
def test_gemv_pair_dd_multi_argument_checks(lib, case):
    fbuf = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    a = dict(p=ctypes.c_void_p(0x1000), X=_dbuf(), nv=3, ldx=8, B=fbuf, ldb=3, G=_dbuf(), rr=_dbuf())
    if case.startswith("null_"):
        a[case[5:]] = None
    elif case == "nv_0":
        a["nv"] = 0
    elif case == "nv_17":
        a["nv"], a["ldb"] = 17, 17
    elif case == "ldb_lt_nv":
        a["ldb"] = 2
    elif case == "ldx_lt_n":
        a["ldx"] = 0                 # below every n (a real handle is checked against its own n)
    rc = lib.fos_gemv_pair_dd_multi(a["p"], a["X"], a["nv"], a["ldx"], a["B"], a["ldb"], 0.5, a["G"], a["rr"])
    assert rc == -1
    assert "fos_gemv_pair_dd_multi" in _err(lib) and "bad argument" in _err(lib)


@pytest.mark.parametrize("case", ["null_p", "null_B", "null_X", "null_res", "nv_1", "nv_17", "ldb_lt_nv", "ldx_lt_n",
                                  "negative_max_iter"])
def test_lbfgs_minimize_multi_argument_checks(lib, case):
    from fastoptsolver_amd import _lib
    fbuf = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    res = (_lib.LbfgsResult * 17)()
    a = dict(p=ctypes.c_void_p(0x1000), nv=3, B=fbuf, ldb=3, max_iter=10, X=_dbuf(), ldx=8, res=res)
    if case.startswith("null_"):
        a[case[5:]] = None
    elif case == "nv_1":
        a["nv"] = 1
    elif case == "nv_17":
        a["nv"], a["ldb"] = 17, 17
    elif case == "ldb_lt_nv":
        a["ldb"] = 2
    elif case == "ldx_lt_n":
        a["ldx"] = 0
    elif case == "negative_max_iter":
        a["max_iter"] = -1
    rounds = ctypes.c_int(0)
    rc = lib.fos_lbfgs_minimize_multi(a["p"], a["nv"], a["B"], a["ldb"], 0.5, a["max_iter"], 1e-6, a["X"], a["ldx"], None,
                                      None, 0, ctypes.byref(rounds), a["res"])
    assert rc == -1
    assert "fos_lbfgs_minimize_multi" in _err(lib) and "bad argument" in _err(lib)


@pytest.mark.parametrize("kw", [dict(group=object()), dict(comm=object()), dict(cols=(0, 4, 4)), dict(ops=object())])
def test_fit_two_d_b_refuses_sharding_and_ops(kw):
    """Refused before any device work, so the message is the same with or without a GPU."""
    from fastoptsolver_amd.lbfgs import LBFGSSolver
    A, B = np.ones((8, 4)), np.ones((8, 3))
    with pytest.raises(ValueError, match="several targets"):
        LBFGSSolver("ridge", 0.0, 1.0, max_iter=5).fit(A, B, **kw)
