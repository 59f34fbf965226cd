"""CPU: the row weights of a problem handle (fos_row_weights_bind / fos_row_weights_get) and fos_gram_apply are exported, bound,
declared and refuse bad arguments before any HIP call; prepare_weighted refuses bad weights before any device work; the pinned
signatures are what they were."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

NEW = ("fos_row_weights_bind", "fos_row_weights_get", "fos_gram_apply")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1


@pytest.fixture(scope="module")
def lib():
    from fastoptsolver_amd import build, _lib
    build.build()
    return _lib.load()


def _header():
    with open(os.path.join(ROOT, "include", "fos.h")) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def test_symbols_exported_bound_declared_and_documented(lib):
    from fastoptsolver_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = _header()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        integration = fh.read()
    for name in NEW:
        assert f" T {name}" in out, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in integration, name
    assert lib.fos_abi_version() == 3                       # the ABI only grew
    assert ctypes.sizeof(_lib.FistaParams) == 8 * 8 + 4 * 4  # fos_fista_params keeps its size: the weights are the problem's


def test_new_entry_points_take_their_data_pointer_first():
    """The guard tables file every function whose first parameter is a handle and every fos_fista_* function: the header gained
    neither."""
    from tests import _logit_guard as gd
    header = _header()
    assert not [n for n in re.findall(r"\b(fos_fista_[a-z0-9_]+)\s*\(", header) if "weight" in n or "gram" in n]
    assert not (set(NEW) & gd.header_handle_functions())
    assert gd.header_handle_functions() == gd.SERVES | gd.LOSS_FREE | gd.REFUSES
    assert re.search(r"fos_row_weights_bind\s*\(\s*const\s+float\s*\*\s*w\s*,\s*fos_problem\s*\*\s*p\s*\)", header)
    assert re.search(r"fos_row_weights_get\s*\(\s*const\s+float\s*\*\*\s*w_out\s*,\s*const\s+fos_problem\s*\*\s*p\s*\)", header)
    assert re.search(r"fos_gram_apply\s*\(\s*const\s+float\s*\*\s*X\s*,\s*int\s+nv\s*,\s*fos_problem\s*\*\s*p\s*,\s*float\s*\*\s*G\s*\)", header)


@pytest.mark.parametrize("case", ["null_problem", "misaligned_4", "misaligned_8", "null_problem_null_w"])
def test_bind_argument_checks(lib, case):
    # the stand-in handle is never dereferenced: every case fails the argument check first
    w, p = ctypes.c_void_p(0x2000), ctypes.c_void_p(0x1000)
    if case == "null_problem":
        p = None
    elif case == "null_problem_null_w":
        w, p = None, None
    else:
        w = ctypes.c_void_p(0x2000 + int(case.rsplit("_", 1)[1]))
    assert lib.fos_row_weights_bind(w, p) == ARG
    assert "fos_row_weights_bind" in lib.fos_last_error().decode()


def test_get_argument_checks(lib):
    out = ctypes.c_void_p(7)
    assert lib.fos_row_weights_get(None, ctypes.c_void_p(0x1000)) == ARG
    assert lib.fos_row_weights_get(ctypes.byref(out), None) == ARG
    assert "fos_row_weights_get" in lib.fos_last_error().decode() and out.value == 7


@pytest.mark.parametrize("case", ["null_X", "null_p", "null_G", "nv_0", "nv_17", "nv_minus_1"])
def test_gram_apply_argument_checks(lib, case):
    X, nv, p, G = ctypes.c_void_p(0x2000), 3, ctypes.c_void_p(0x1000), ctypes.c_void_p(0x3000)
    if case == "null_X":
        X = None
    elif case == "null_p":
        p = None
    elif case == "null_G":
        G = None
    else:
        nv = {"nv_0": 0, "nv_17": 17, "nv_minus_1": -1}[case]
    assert lib.fos_gram_apply(X, nv, p, G) == ARG
    assert "fos_gram_apply" in lib.fos_last_error().decode()


A, B = np.ones((10, 4)), np.arange(10.0)


@pytest.mark.parametrize("w", [np.ones(9), np.ones(11), np.ones((10, 1)), -np.ones(10), np.r_[np.ones(9), -1e-30],
                               np.r_[np.nan, np.ones(9)], np.r_[np.inf, np.ones(9)], np.zeros(10), None],
                         ids=["short", "long", "2-D", "negative", "one_negative", "nan", "inf", "all_zero", "none"])
@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_prepare_weighted_refuses_bad_weights_before_any_device_work(w, loss):
    import fastoptsolver_amd as fos
    with pytest.raises(ValueError):
        fos.prepare_weighted(A, B / 10.0, w, loss=loss)
    if w is not None:
        with pytest.raises(ValueError):
            fos.prepare_weighted(A, B / 10.0, torch.as_tensor(w), loss=loss)


def test_a_zero_weight_fold_is_a_value_error():
    from fastoptsolver_amd import iterative_solvers as its
    ids = np.arange(10) % 3
    prob = types.SimpleNamespace(sample_weight=torch.tensor([1.0, 0, 2] * 3 + [1.0]))
    with pytest.raises(ValueError, match="fold 1"):
        its._cv_weight_sums(prob, ids, 3)
    prob = types.SimpleNamespace(sample_weight=torch.tensor([1.0, 0.5, 2] * 3 + [1.0]))
    assert its._cv_weight_sums(prob, ids, 3).tolist() == [4.0, 1.5, 6.0]


def test_signatures():
    import fastoptsolver_amd as fos
    from fastoptsolver_amd import _core
    pw = inspect.signature(fos.prepare_weighted).parameters
    assert list(pw) == ["A", "b", "sample_weight", "dtype", "loss"] and pw["loss"].default == "squared"
    assert pw["loss"].kind is inspect.Parameter.KEYWORD_ONLY and pw["dtype"].default is None
    assert "prepare_weighted" in fos.__all__
    init = inspect.signature(_core.Problem.__init__).parameters
    assert list(init) == ["self", "A", "b", "dtype", "pad", "loss", "sample_weight"] and init["sample_weight"].default is None
    # the pinned signatures are what they were
    prep = inspect.signature(fos.prepare).parameters
    assert list(prep) == ["A", "b", "dtype", "pad", "loss"] and prep["loss"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(fos.logistic_path).parameters) == [
        "A", "y", "alphas", "t_init_factor", "max_iter", "delta", "L", "dtype", "tol_ratio", "adaptive_restart",
        "restart_threshold", "return_info"]
    assert list(inspect.signature(fos.logistic_cv).parameters) == [
        "A", "y", "alphas", "folds", "t_init_factor", "max_iter", "delta", "L", "dtype", "tol_ratio", "adaptive_restart",
        "restart_threshold", "refit", "return_coefs"]
    assert list(inspect.signature(fos.logistic_objective).parameters) == ["x", "A", "y", "alpha1", "alpha2"]
    assert list(inspect.signature(fos.fista_cv).parameters) == [
        "A", "b", "alphas", "folds", "t_init_factor", "max_iter", "delta", "L", "dtype", "tol_ratio", "adaptive_restart",
        "restart_threshold", "refit", "return_coefs"]
    assert list(inspect.signature(fos.fista_path).parameters) == [
        "A", "b", "alphas", "t_init_factor", "max_iter", "delta", "L", "dtype", "comm", "cols", "tol", "tol_ratio",
        "adaptive_restart", "restart_threshold", "return_info"]
    assert list(inspect.signature(fos.estimate_lipschitz).parameters) == ["A", "n_iter", "tol", "group"]
    assert fos.CVResult._fields == ("alphas", "mse", "mean_mse", "best", "x", "coefs", "info")
    assert fos.LogisticCVResult._fields == ("alphas", "logloss", "mean_logloss", "best", "x", "coefs", "info")
