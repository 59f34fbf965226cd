"""CPU: the loss of a problem handle (fos_problem_set_loss / fos_problem_get_loss) is exported, bound, declared and refuses bad
arguments before any HIP call; logistic_path / logistic_cv keep their signatures and refuse bad arguments before any device
work."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

NEW = ("fos_problem_set_loss", "fos_problem_get_loss")
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
    assert re.search(r"FOS_LOSS_SQUARED\s*=\s*0\s*,\s*FOS_LOSS_LOGISTIC\s*=\s*1", header)
    assert (_lib.LOSS_SQUARED, _lib.LOSS_LOGISTIC) == (0, 1)
    assert lib.fos_abi_version() == 3                       # the ABI only grew
    assert ctypes.sizeof(_lib.FistaParams) == 8 * 8 + 4 * 4  # fos_fista_params keeps its size: the loss is the problem's


def test_no_new_fista_entry_point():
    """The logistic loss is served by the existing lockstep entry points: the header gained no fos_fista_* function."""
    with open(os.path.join(ROOT, "include", "fos.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    assert not [n for n in re.findall(r"\b(fos_fista_[a-z0-9_]+)\s*\(", header) if "logi" in n or "loss" in n]


@pytest.mark.parametrize("case", ["null", "loss_2", "loss_minus_1"])
def test_set_loss_argument_checks(lib, case):
    # the stand-in handle is never dereferenced: every case fails the argument check first
    p, loss = ctypes.c_void_p(0x1000), 1
    if case == "null":
        p = None
    elif case == "loss_2":
        loss = 2
    else:
        loss = -1
    assert lib.fos_problem_set_loss(p, loss) == -1
    assert "fos_problem_set_loss" in lib.fos_last_error().decode()


def test_get_loss_argument_checks(lib):
    out = ctypes.c_int(7)
    assert lib.fos_problem_get_loss(None, ctypes.byref(out)) == -1
    assert lib.fos_problem_get_loss(ctypes.c_void_p(0x1000), None) == -1
    assert "fos_problem_get_loss" in lib.fos_last_error().decode() and out.value == 7


def test_signatures():
    import fastoptsolver_amd as fos
    path = list(inspect.signature(fos.logistic_path).parameters)
    assert path == ["A", "y", "alphas", "t_init_factor", "max_iter", "delta", "L", "dtype", "tol_ratio", "adaptive_restart",
                    "restart_threshold", "return_info"]
    cv = list(inspect.signature(fos.logistic_cv).parameters)
    assert cv == ["A", "y", "alphas", "folds", "t_init_factor", "max_iter", "delta", "L", "dtype", "tol_ratio",
                  "adaptive_restart", "restart_threshold", "refit", "return_coefs"]
    kinds = inspect.signature(fos.logistic_path).parameters
    assert all(kinds[k].kind is inspect.Parameter.KEYWORD_ONLY for k in path[5:])
    assert fos.LogisticCVResult._fields == ("alphas", "logloss", "mean_logloss", "best", "x", "coefs", "info")
    assert list(inspect.signature(fos.logistic_objective).parameters) == ["x", "A", "y", "alpha1", "alpha2"]
    prep = inspect.signature(fos.prepare).parameters
    assert list(prep) == ["A", "b", "dtype", "pad", "loss"] and prep["loss"].default == "squared"
    assert prep["loss"].kind is inspect.Parameter.KEYWORD_ONLY
    # the squared-loss signatures are what they were
    assert list(inspect.signature(fos.fista_cv).parameters)[:4] == ["A", "b", "alphas", "folds"]
    assert fos.CVResult._fields == ("alphas", "mse", "mean_mse", "best", "x", "coefs", "info")


A, Y = np.ones((10, 4)), np.array([0.0, 1.0] * 5)


@pytest.mark.parametrize("folds", [1, 0, 256, 11, True, 2.0, None, np.zeros(10, dtype=np.int64), np.arange(9) % 3,
                                   np.array([0, 1] * 4 + [255, 0])],
                         ids=["K=1", "K=0", "K=256", "K>m", "bool", "float", "None", "one_fold", "short", "id_255"])
def test_logistic_cv_refuses_bad_folds(folds):
    import fastoptsolver_amd as fos
    with pytest.raises(ValueError):
        fos.logistic_cv(A, Y, [(0.1, 0.0), (0.2, 0.0)], folds=folds, max_iter=2, L=1.0)


@pytest.mark.parametrize("delta", [2.0, 1.0, -3.0])
def test_empty_path_and_small_delta_are_value_errors(delta):
    import fastoptsolver_amd as fos
    with pytest.raises(ValueError):
        fos.logistic_path(A, Y, [], max_iter=2, L=1.0)
    with pytest.raises(ValueError):
        fos.logistic_cv(A, Y, [], folds=2, max_iter=2, L=1.0)
    with pytest.raises(ValueError):
        fos.logistic_path(A, Y, [(0.1, 0.0)], delta=delta, max_iter=2, L=1.0)
    with pytest.raises(ValueError):
        fos.logistic_cv(A, Y, [(0.1, 0.0)], folds=2, delta=delta, max_iter=2, L=1.0)


def test_unknown_loss_is_a_value_error():
    import fastoptsolver_amd as fos
    with pytest.raises(ValueError):
        fos.prepare(A, Y, loss="hinge")
