"""CPU: the cross-validation entry points (fos_fista_run_multi_folds, fos_residual_batch_folds) are exported, bound, named in
the header and refuse bad arguments before any HIP call; fista_cv refuses bad folds before any device work."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

NEW = ("fos_fista_run_multi_folds", "fos_residual_batch_folds")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from fastoptsolver_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_exported_bound_and_declared(lib):
    from fastoptsolver_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    with open(os.path.join(ROOT, "include", "fos.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in NEW:
        assert f" T {name}" in out, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert lib.fos_abi_version() == 3                       # the ABI only grew


def _handles(nv):
    # never dereferenced: every case that uses them fails an earlier check
    return (ctypes.c_void_p * nv)(*[0x1000] * nv)


def _err(lib):
    return lib.fos_last_error().decode()


def _aligned_ids():
    """A host buffer standing in for the device ids (never read): its address, 4-byte aligned, and the buffer (kept alive)."""
    buf = (ctypes.c_uint8 * 64)()
    return (ctypes.addressof(buf) + 3) // 4 * 4, buf


RUN_CASES = ["null_fs", "null_fold", "null_held", "nv_0", "nv_17", "negative_iters", "misaligned_fold", "held_below",
             "held_above", "different_problems"]


@pytest.mark.parametrize("case", RUN_CASES)
def test_run_multi_folds_argument_checks(lib, case):
    addr, keep = _aligned_ids()
    fs, nv, iters, fold, held = _handles(2), 2, 5, ctypes.c_void_p(addr), (ctypes.c_int32 * 17)(*([0, 1] + [-1] * 15))
    if case == "null_fs":
        fs = None
    elif case == "null_fold":
        fold = None
    elif case == "null_held":
        held = None
    elif case == "nv_0":
        nv = 0
    elif case == "nv_17":
        fs, nv = _handles(17), 17
    elif case == "negative_iters":
        iters = -1
    elif case == "misaligned_fold":
        fold = ctypes.c_void_p(addr + 1)
    elif case == "held_below":
        held[1] = -2
    elif case == "held_above":
        held[0] = 255
    elif case == "different_problems":
        # two stand-in handles whose first member (the problem pointer, all the check reads) differs
        a, b = (ctypes.c_void_p * 64)(), (ctypes.c_void_p * 64)()
        a[0], b[0] = 0x1000, 0x2000
        fs = (ctypes.c_void_p * 2)(ctypes.addressof(a), ctypes.addressof(b))
        keep = (keep, a, b)
    rc = lib.fos_fista_run_multi_folds(fs, nv, iters, fold, held)
    assert rc == -1
    assert "fos_fista_run_multi_folds" in _err(lib)
    assert ("share one problem" if case == "different_problems" else "bad argument") in _err(lib)


@pytest.mark.parametrize("case", ["null_p", "null_X", "null_fold", "null_held", "null_out", "nv_0", "nv_17",
                                  "misaligned_fold", "held_below", "held_above"])
def test_residual_batch_folds_argument_checks(lib, case):
    addr, keep = _aligned_ids()
    buf = (ctypes.c_float * 64)()
    out = (ctypes.c_double * 16)()
    p, X, nv, fold, o = ctypes.c_void_p(0x1000), ctypes.cast(buf, ctypes.c_void_p), 3, ctypes.c_void_p(addr), \
        ctypes.cast(out, ctypes.c_void_p)
    held = (ctypes.c_int32 * 17)(*([0, 1, 254] + [-1] * 14))
    if case == "null_p":
        p = None
    elif case == "null_X":
        X = None
    elif case == "null_fold":
        fold = None
    elif case == "null_held":
        held = None
    elif case == "null_out":
        o = None
    elif case == "nv_0":
        nv = 0
    elif case == "nv_17":
        nv = 17
    elif case == "misaligned_fold":
        fold = ctypes.c_void_p(addr + 2)
    elif case == "held_below":
        held[0] = -2
    elif case == "held_above":
        held[2] = 255
    rc = lib.fos_residual_batch_folds(p, X, nv, fold, held, o)
    assert rc == -1
    assert "fos_residual_batch_folds" in _err(lib) and "bad argument" in _err(lib)


# ---- fista_cv: fold validation, before any device work (so the same with or without a GPU) ---------------------------------
def test_int_folds_give_the_contiguous_split():
    from fastoptsolver_amd.iterative_solvers import _cv_folds
    ids, sizes = _cv_folds(3, 10)
    assert sizes.tolist() == [4, 3, 3]
    assert ids.tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2, 2] and ids.dtype == np.uint8
    ids, sizes = _cv_folds(5, 1001)
    assert sizes.tolist() == [201, 200, 200, 200, 200] and np.all(np.diff(ids.astype(int)) >= 0)


def test_id_arrays_are_taken_as_given():
    import torch
    from fastoptsolver_amd.iterative_solvers import _cv_folds
    want = np.array([2, 0, 1, 1, 0, 2, 2])
    for given in (want, want.tolist(), want.astype(np.uint8), torch.as_tensor(want)):
        ids, sizes = _cv_folds(given, 7)
        assert ids.tolist() == want.tolist() and sizes.tolist() == [2, 2, 3]
    ids, sizes = _cv_folds(np.arange(255), 255)              # the most folds the byte ids hold
    assert len(sizes) == 255 and ids[-1] == 254


@pytest.mark.parametrize("folds", [1, 0, -3, 256, 11, True, 2.0, "5", None,
                                   np.array([0, 1, 3, 3, 0, 1, 0, 1, 0, 1]),          # fold 2 is empty
                                   np.zeros(10, dtype=np.int64),                     # one fold only
                                   np.arange(9) % 3, np.arange(11) % 3,              # wrong length
                                   np.arange(10).reshape(2, 5) % 2,                   # not 1-D
                                   np.array([0, 1] * 4 + [255, 0]),                   # an id above 254
                                   np.array([0, 1] * 4 + [-1, 0]),                    # a negative id
                                   np.array([0.0, 1.0] * 5)],                         # not integers
                         ids=["K=1", "K=0", "K<0", "K=256", "K>m", "bool", "float", "str", "None", "empty_fold", "one_fold",
                              "short", "long", "2-D", "id_255", "id_negative", "float_ids"])
def test_fista_cv_refuses_bad_folds(folds):
    import fastoptsolver_amd as fos
    A, b = np.ones((10, 4)), np.ones(10)
    with pytest.raises(ValueError):
        fos.fista_cv(A, b, [(0.1, 0.0), (0.2, 0.0)], folds=folds, max_iter=2, L=1.0)


def test_fista_cv_refuses_an_empty_path_and_small_delta():
    import fastoptsolver_amd as fos
    A, b = np.ones((10, 4)), np.ones(10)
    with pytest.raises(ValueError):
        fos.fista_cv(A, b, [], folds=2, max_iter=2, L=1.0)
    with pytest.raises(AssertionError):
        fos.fista_cv(A, b, [(0.1, 0.0)], folds=2, delta=2.0, max_iter=2, L=1.0)


def test_fista_cv_has_no_tol_backtracking_or_sharding_arguments():
    import inspect
    import fastoptsolver_amd as fos
    names = list(inspect.signature(fos.fista_cv).parameters)
    assert names == ["A", "b", "alphas", "folds", "t_init_factor", "max_iter", "delta", "L", "dtype", "tol_ratio",
                     "adaptive_restart", "restart_threshold", "refit", "return_coefs"]
    assert fos.CVResult._fields == ("alphas", "mse", "mean_mse", "best", "x", "coefs", "info")
