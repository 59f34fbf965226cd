"""CPU: the multinomial loss of a problem handle (fos_problem_set_multinomial / fos_problem_get_classes) is exported, bound,
declared and refuses bad arguments before any HIP call; labels, classes and column counts are refused on the host before any
device work; the packing of fits into lockstep groups is what the documentation says."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

NEW = ("fos_problem_set_multinomial", "fos_problem_get_classes")
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
    assert re.search(r"FOS_LOSS_SQUARED\s*=\s*0\s*,\s*FOS_LOSS_LOGISTIC\s*=\s*1\s*,\s*FOS_LOSS_MULTINOMIAL\s*=\s*2\s*\}", header)
    assert (_lib.LOSS_SQUARED, _lib.LOSS_LOGISTIC, _lib.LOSS_MULTINOMIAL) == (0, 1, 2)
    assert lib.fos_abi_version() == 3                       # the ABI only grew
    assert ctypes.sizeof(_lib.FistaParams) == 8 * 8 + 4 * 4  # fos_fista_params keeps its size: loss and classes are the problem's
    # the data first, the handle second - and no new fos_fista_* entry point
    assert re.search(r"fos_problem_set_multinomial\s*\(\s*int\s+classes\s*,\s*fos_problem\s*\*\s*p\s*\)", header)
    assert re.search(r"fos_problem_get_classes\s*\(\s*int\s*\*\s*classes\s*,\s*const\s+fos_problem\s*\*\s*p\s*\)", header)
    assert not [n for n in re.findall(r"\b(fos_fista_[a-z0-9_]+)\s*\(", header) if "multinom" in n or "softmax" in n or "class" in n]


@pytest.mark.parametrize("classes", [1, 0, -3, 17, 1 << 20])
def test_set_multinomial_refuses_bad_class_counts_before_touching_the_handle(lib, classes):
    # the stand-in handle is never dereferenced: every case fails the argument check first
    assert lib.fos_problem_set_multinomial(classes, ctypes.c_void_p(0x1000)) == ARG
    assert "fos_problem_set_multinomial" in lib.fos_last_error().decode() and "2..16" in lib.fos_last_error().decode()


def test_null_arguments(lib):
    assert lib.fos_problem_set_multinomial(3, None) == ARG
    out = ctypes.c_int(7)
    assert lib.fos_problem_get_classes(None, ctypes.c_void_p(0x1000)) == ARG
    assert lib.fos_problem_get_classes(ctypes.byref(out), None) == ARG
    assert "fos_problem_get_classes" in lib.fos_last_error().decode() and out.value == 7


def test_set_loss_still_refuses_loss_two_and_points_to_the_new_call(lib):
    assert lib.fos_problem_set_loss(ctypes.c_void_p(0x1000), 2) == ARG
    msg = lib.fos_last_error().decode()
    assert "fos_problem_set_loss" in msg and "fos_problem_set_multinomial" in msg


A = np.ones((10, 4))
BAD_LABELS = {
    "fraction": [0, 1, 2, 1.5, 0, 1, 2, 0, 1, 2], "negative": [0, 1, 2, -1, 0, 1, 2, 0, 1, 2], "nan": [0, 1, np.nan] + [0] * 7,
    "inf": [0, 1, np.inf] + [0] * 7, "one_class": [0] * 10, "seventeen": list(range(10)) + [16], "2-D": np.zeros((10, 1)),
    "strings": ["a"] * 10, "empty": [], "none": None,
}


@pytest.mark.parametrize("bad", sorted(BAD_LABELS))
def test_bad_labels_are_value_errors_before_any_device_work(bad):
    """No GPU here: a call that got past the host checks would raise FosError, not ValueError."""
    import fastoptsolver_amd as fos
    y = BAD_LABELS[bad]
    with pytest.raises(ValueError):
        fos.prepare(A, y, loss="multinomial")
    with pytest.raises(ValueError):
        fos.prepare_multinomial(A, y)
    with pytest.raises(ValueError):
        fos.multinomial_path(A, y, [(0.1, 0.0)], max_iter=2, L=1.0)
    if y is not None:
        with pytest.raises(ValueError):
            fos.prepare_weighted(A, y, np.ones(10), loss="multinomial")
        with pytest.raises(ValueError):
            fos.prepare_penalized(A, y, lower=0.0, loss="multinomial")


@pytest.mark.parametrize("classes", [1, 0, 17, -2, 2.0, True, "3", 2])
def test_bad_class_counts_are_value_errors_before_any_device_work(classes):
    import fastoptsolver_amd as fos
    y = np.arange(10) % 3                                    # three classes: classes = 2 is too few for the labels
    with pytest.raises(ValueError):
        fos.prepare_multinomial(A, y, classes=classes)
    with pytest.raises(ValueError):
        fos.multinomial_path(A, y, [(0.1, 0.0)], classes=classes, max_iter=2, L=1.0)
    with pytest.raises(ValueError):
        fos.multinomial_cv(A, y, [(0.1, 0.0)], folds=2, classes=classes, max_iter=2, L=1.0)


def test_classes_belongs_to_the_multinomial_loss_and_good_labels_reach_the_device():
    import fastoptsolver_amd as fos
    from fastoptsolver_amd import _core
    lab, C = _core.checked_labels(torch.tensor([0, 2, 1, 1]))
    assert C == 3 and lab.dtype == np.float64 and lab.tolist() == [0.0, 2.0, 1.0, 1.0]
    assert _core.checked_labels(np.array([0.0, 1.0]), 16)[1] == 16           # a class no row carries
    assert _core.checked_labels([True, False])[1] == 2
    if not torch.cuda.is_available():
        with pytest.raises(fos.FosError):                                    # past the host checks: the device is needed
            fos.prepare(A, np.arange(10) % 3, loss="multinomial")


@pytest.mark.parametrize("C,nv", [(3, 4), (3, 16), (5, 16), (2, 1), (7, 15), (16, 8), (4, 0), (2, 18)])
def test_columns_that_are_no_whole_class_groups_are_value_errors(C, nv):
    from fastoptsolver_amd import _core
    with pytest.raises(ValueError):
        _core.checked_class_groups(nv, C)
    # the lockstep wrappers check before they touch the library: stand-in handles without one
    hs = [types.SimpleNamespace(prob=types.SimpleNamespace(classes=C), lib=None, h=None) for _ in range(nv)]
    if nv:
        with pytest.raises(ValueError):
            _core.run_multi(hs, 3)
        with pytest.raises(ValueError):
            _core.run_multi_folds(hs, None, [0] * nv, 3)


def test_whole_class_groups_pass():
    from fastoptsolver_amd import _core
    assert [_core.checked_class_groups(nv, C) for C, nv in ((2, 16), (3, 15), (5, 5), (7, 14), (16, 16))] == [8, 5, 1, 2, 1]


@pytest.mark.parametrize("C,per", [(2, 8), (3, 5), (5, 3), (7, 2), (16, 1)])
def test_packing(C, per):
    from fastoptsolver_amd.multinomial import pack_groups
    assert pack_groups(0, C) == []
    for count in (1, per - 1, per, per + 1, 2 * per, 2 * per + 1, 23):       # both sides of a group boundary
        if count < 1:
            continue
        groups = pack_groups(count, C)
        assert [f for f, _ in groups] == list(range(0, count, per))
        assert sum(k for _, k in groups) == count and all(1 <= k <= per for _, k in groups)
        assert all(k == per for _, k in groups[:-1]) and all(k * C <= 16 for _, k in groups)
        assert groups[-1][1] == (count - 1) % per + 1
    for bad in (1, 17, 0):
        with pytest.raises(ValueError):
            pack_groups(3, bad)


def test_signatures():
    import fastoptsolver_amd as fos
    path = inspect.signature(fos.multinomial_path).parameters
    assert list(path) == ["A", "y", "alphas", "classes", "t_init_factor", "max_iter", "delta", "L", "dtype", "return_info"]
    assert all(path[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(path)[6:])
    assert (path["classes"].default, path["t_init_factor"].default, path["max_iter"].default) == (None, 1.0, 500)
    cv = inspect.signature(fos.multinomial_cv).parameters
    assert list(cv) == ["A", "y", "alphas", "folds", "classes", "t_init_factor", "max_iter", "delta", "L", "dtype", "refit",
                        "return_coefs"]
    assert cv["folds"].default == 5 and cv["refit"].default is True and cv["return_coefs"].default is False
    for name in ("tol_ratio", "adaptive_restart", "restart_threshold", "tol"):
        assert name not in path and name not in cv
    assert list(inspect.signature(fos.multinomial_objective).parameters) == ["X", "A", "y", "alpha1", "alpha2"]
    assert fos.MultinomialCVResult._fields == fos.LogisticCVResult._fields
    for name in ("multinomial_path", "multinomial_cv", "multinomial_objective", "MultinomialCVResult", "prepare_multinomial"):
        assert name in fos.__all__


def test_empty_path_small_delta_and_bad_folds_are_value_errors():
    import fastoptsolver_amd as fos
    y = np.arange(10) % 3
    with pytest.raises(ValueError):
        fos.multinomial_path(A, y, [], max_iter=2, L=1.0)
    with pytest.raises(ValueError):
        fos.multinomial_path(A, y, [(0.1, 0.0)], delta=2.0, max_iter=2, L=1.0)
    for folds in (1, 11, None, np.zeros(10, dtype=np.int64)):
        with pytest.raises(ValueError):
            fos.multinomial_cv(A, y, [(0.1, 0.0)], folds=folds, max_iter=2, L=1.0)
