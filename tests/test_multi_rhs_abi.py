"""CPU: the multi-target entry points (fos_fista_run_multi_rhs, fos_residual_batch_rhs) are exported, bound, and refuse bad
arguments before any HIP call; the Python front-ends refuse what a 2-D b cannot be combined with."""
import ctypes
import subprocess

import numpy as np
import pytest

NEW = ("fos_fista_run_multi_rhs", "fos_residual_batch_rhs")


@pytest.fixture(scope="module")
def lib():
    from fastoptsolver_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    from fastoptsolver_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert f" T {name}" in out, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def _handles(nv):
    # never dereferenced: every case below fails the argument check first
    return (ctypes.c_void_p * nv)(*[0x1000] * nv)


def _err(lib):
    return lib.fos_last_error().decode()


@pytest.mark.parametrize("case", ["null_fs", "nv_17", "nv_0", "ldb_lt_nv", "null_B", "negative_iters"])
def test_run_multi_rhs_argument_checks(lib, case):
    B = (ctypes.c_float * 64)()
    fs, nv, b, ldb, iters = _handles(2), 2, ctypes.cast(B, ctypes.c_void_p), 2, 5
    if case == "null_fs":
        fs = None
    elif case == "nv_17":
        fs, nv, ldb = _handles(17), 17, 17
    elif case == "nv_0":
        nv = 0
    elif case == "ldb_lt_nv":
        ldb = 1
    elif case == "null_B":
        b = None
    elif case == "negative_iters":
        iters = -1
    rc = lib.fos_fista_run_multi_rhs(fs, nv, b, ldb, iters)
    assert rc == -1
    assert "fos_fista_run_multi_rhs" in _err(lib) and "bad argument" in _err(lib)


@pytest.mark.parametrize("case", ["null_p", "null_X", "nv_17", "nv_0", "ldb_lt_nv", "null_B", "null_out"])
def test_residual_batch_rhs_argument_checks(lib, case):
    buf = (ctypes.c_float * 64)()
    out = (ctypes.c_double * 16)()
    p, X, nv, B, ldb, o = ctypes.c_void_p(0x1000), ctypes.cast(buf, ctypes.c_void_p), 3, ctypes.cast(buf, ctypes.c_void_p), 3, \
        ctypes.cast(out, ctypes.c_void_p)
    if case == "null_p":
        p = None
    elif case == "null_X":
        X = None
    elif case == "nv_17":
        nv, ldb = 17, 17
    elif case == "nv_0":
        nv = 0
    elif case == "ldb_lt_nv":
        ldb = 2
    elif case == "null_B":
        B = None
    elif case == "null_out":
        o = None
    rc = lib.fos_residual_batch_rhs(p, X, nv, B, ldb, o)
    assert rc == -1
    assert "fos_residual_batch_rhs" in _err(lib) and "bad argument" in _err(lib)


def test_multi_target_shape_rule():
    """Which b makes a call multi-target: a 2-D b with k >= 2 columns; never a vector in any orientation."""
    from fastoptsolver_amd.iterative_solvers import _targets
    A = np.ones((6, 4))
    assert _targets(A, np.ones((6, 3))) is not None
    assert _targets(A, np.ones(6)) is None
    assert _targets(A, np.ones((6, 1))) is None
    assert _targets(A, np.ones((1, 6))) is None
    assert _targets(A, None) is None


def test_two_d_b_refuses_sharding_and_history():
    """Refused before any device work, so the message is the same with or without a GPU."""
    import fastoptsolver_amd as fos
    A, B = np.ones((8, 4)), np.ones((8, 3))
    for kw in (dict(comm=object()), dict(group=object()), dict(cols=(0, 4, 4)), dict(return_history=True)):
        with pytest.raises(ValueError):
            fos.fista(A, B, "lasso", 0.1, 0.0, max_iter=2, **kw)
        with pytest.raises(ValueError):
            fos.fista_delta(A, B, "lasso", 0.1, 0.0, 3.0, max_iter=2, **kw)
