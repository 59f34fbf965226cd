"""CPU: the Huber and squared-hinge losses of a problem handle (fos_problem_set_link_loss / fos_problem_get_link_loss) are
exported, bound and declared in a header of their own; the setter refuses bad arguments before any HIP call; the public functions
of fastoptsolver_amd.robust have the signatures and result tuples the package documents."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

NEW = ("fos_problem_set_link_loss", "fos_problem_get_link_loss")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
HUBER, HINGE = 3, 4


@pytest.fixture(scope="module")
def lib():
    from fastoptsolver_amd import build, _lib
    build.build()
    return _lib.load()


def _header(name="fos_link_loss.h"):
    with open(os.path.join(ROOT, "include", name)) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def test_symbols_exported_bound_and_declared(lib):
    from fastoptsolver_amd import _lib, build
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = _header()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        integration = fh.read()
    for name in NEW:
        assert f" T {name}" in out, name
        assert name in _lib.LINK_LOSS_SIGNATURES and name not in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.LINK_LOSS_SIGNATURES[name][1]
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in integration, name
    assert re.search(r"fos_problem_set_link_loss\s*\(\s*int\s+loss\s*,\s*double\s+param\s*,\s*fos_problem\s*\*\s*p\s*\)", header)
    assert re.search(r"fos_problem_get_link_loss\s*\(\s*int\s*\*\s*loss\s*,\s*double\s*\*\s*param\s*,\s*const\s+fos_problem\s*\*\s*p\s*\)", header)
    assert re.search(r"enum\s*\{\s*FOS_LOSS_HUBER\s*=\s*3\s*,\s*FOS_LOSS_SQUARED_HINGE\s*=\s*4\s*\}\s*;", header)
    assert (_lib.LOSS_HUBER, _lib.LOSS_SQUARED_HINGE) == (HUBER, HINGE)
    # a header of its own beside fos.h: it declares these two and nothing else, and fos.h knows neither them nor the two losses
    assert sorted(set(re.findall(r"\b(fos_[a-z0-9_]+)\s*\(", header))) == sorted(NEW) == sorted(_lib.LINK_LOSS_SIGNATURES)
    fos_h = _header("fos.h")
    assert '#include "fos.h"' in header and not [n for n in NEW + ("FOS_LOSS_HUBER", "FOS_LOSS_SQUARED_HINGE") if n in fos_h]
    assert os.path.join(ROOT, "include", "fos_link_loss.h") in build.HEADERS
    assert lib.fos_abi_version() == 3                       # the ABI only grew
    assert ctypes.sizeof(_lib.FistaParams) == 8 * 8 + 4 * 4  # fos_fista_params keeps its size: the loss is the problem's


BAD = {
    "null_problem_huber": (HUBER, 1.0, None), "null_problem_hinge": (HINGE, 0.0, None),
    "loss_squared": (0, 1.0, 0x1000), "loss_logistic": (1, 1.0, 0x1000), "loss_multinomial": (2, 1.0, 0x1000),
    "loss_beyond": (5, 1.0, 0x1000), "loss_negative": (-1, 0.0, 0x1000),
    "huber_zero": (HUBER, 0.0, 0x1000), "huber_negative": (HUBER, -1.0, 0x1000), "huber_nan": (HUBER, float("nan"), 0x1000),
    "huber_inf": (HUBER, float("inf"), 0x1000), "huber_minus_inf": (HUBER, float("-inf"), 0x1000),
    "hinge_param": (HINGE, 1.0, 0x1000), "hinge_param_tiny": (HINGE, -1e-300, 0x1000), "hinge_param_nan": (HINGE, float("nan"), 0x1000),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_set_refuses_bad_arguments_before_any_device_call(lib, case):
    # no device here, and the stand-in handle is never dereferenced: every case fails a check that does not need it
    loss, param, p = BAD[case]
    assert lib.fos_problem_set_link_loss(loss, param, None if p is None else ctypes.c_void_p(p)) == ARG
    assert "fos_problem_set_link_loss" in lib.fos_last_error().decode()


def test_get_argument_checks(lib):
    loss, param = ctypes.c_int(7), ctypes.c_double(0.25)
    assert lib.fos_problem_get_link_loss(ctypes.byref(loss), ctypes.byref(param), None) == ARG
    assert lib.fos_problem_get_link_loss(None, ctypes.byref(param), ctypes.c_void_p(0x1000)) == ARG
    assert lib.fos_problem_get_link_loss(ctypes.byref(loss), None, ctypes.c_void_p(0x1000)) == ARG
    assert "fos_problem_get_link_loss" in lib.fos_last_error().decode() and (loss.value, param.value) == (7, 0.25)
    # fos_problem_set_loss keeps refusing the two: they need their parameter (null first: the handle is never read)
    assert lib.fos_problem_set_loss(None, HUBER) == ARG


def test_the_checks_that_need_the_handle_come_after_the_ones_that_do_not():
    from tests import _link_guard as gd
    body = gd.body_of("fos_problem_set_link_loss")
    order = [body.index("null problem"), body.index("FOS_LOSS_SQUARED_HINGE"), body.index("std::isfinite(param)"), body.index("param != 0.0"),
             body.index("p->b"), body.index("FOS_ERR_UNSUPPORTED"), body.index("p->loss = loss")]
    assert order == sorted(order)
    for cond in (r"!p->b", r"p->comm\s*\|\|\s*p->col_sharded", r"!pair_dd_multi_supported\(p\)"):
        assert re.search(cond, body), cond
    assert "has_fgroups" not in body                                                  # feature groups compose
    assert "invalidate(" not in body and "plan" not in body and "hip" not in body    # nothing is replanned, no HIP call
    # the other setters leave the link loss again
    assert "link_param = 0.0" in gd.body_of("fos_problem_set_loss") and "link_param = 0.0" in gd.body_of("fos_problem_set_multinomial")
    unknown = gd.body_of("fos_problem_set_loss")
    assert re.search(r"loss\s*!=\s*FOS_LOSS_SQUARED\s*&&\s*loss\s*!=\s*FOS_LOSS_LOGISTIC", unknown)


def test_public_signatures_and_result_tuples():
    import fastoptsolver_amd as fos
    from fastoptsolver_amd import robust

    def params(fn):
        return [(p.name, p.kind is p.KEYWORD_ONLY, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    tail = [("delta", True, None), ("L", True, None), ("dtype", True, None), ("tol_ratio", True, 0.0), ("adaptive_restart", True, False),
            ("restart_threshold", True, 1.0)]
    assert params(fos.huber_path) == [("A", False, E), ("b", False, E), ("alphas", False, E), ("threshold", False, None),
                                      ("t_init_factor", False, 1.0), ("max_iter", False, 500)] + tail + [("return_info", True, False)]
    assert params(fos.hinge_path) == [("A", False, E), ("y", False, E), ("alphas", False, E), ("t_init_factor", False, 1.0),
                                      ("max_iter", False, 500)] + tail + [("return_info", True, False)]
    cv_tail = tail + [("refit", True, True), ("return_coefs", True, False)]
    assert params(fos.huber_cv) == [("A", False, E), ("b", False, E), ("alphas", False, E), ("folds", False, 5), ("threshold", False, None),
                                    ("t_init_factor", False, 1.0), ("max_iter", False, 500)] + cv_tail
    assert params(fos.hinge_cv) == [("A", False, E), ("y", False, E), ("alphas", False, E), ("folds", False, 5),
                                    ("t_init_factor", False, 1.0), ("max_iter", False, 500)] + cv_tail
    assert params(fos.huber_objective) == [("x", False, E), ("A", False, E), ("b", False, E), ("alpha1", False, E), ("alpha2", False, E),
                                           ("threshold", False, None)]
    assert params(fos.hinge_objective) == [("x", False, E), ("A", False, E), ("y", False, E), ("alpha1", False, E), ("alpha2", False, E)]
    assert params(fos.prepare_huber) == [("A", False, E), ("b", False, E), ("threshold", False, E), ("dtype", False, None),
                                         ("sample_weight", True, None)]
    assert params(fos.prepare_hinge) == [("A", False, E), ("y", False, E), ("dtype", False, None), ("sample_weight", True, None)]
    fields = ("alphas", "loss", "mean_loss", "best", "x", "coefs", "info")
    assert fos.HuberCVResult._fields == fields == fos.HingeCVResult._fields and fos.HuberCVResult is not fos.HingeCVResult
    # importable from the package, absent from __all__ (the guard tables of the handle kinds file __all__ name by name)
    names = ("huber_path", "huber_cv", "huber_objective", "hinge_path", "hinge_cv", "hinge_objective", "HuberCVResult", "HingeCVResult",
             "prepare_huber", "prepare_hinge")
    for name in names:
        assert hasattr(fos, name) and name not in fos.__all__, name
    assert all(getattr(fos, n) is getattr(robust, n) for n in names[:8])
    # prepare keeps its signature
    assert [p for p in inspect.signature(fos.prepare).parameters] == ["A", "b", "dtype", "pad", "loss"]


def test_python_argument_checks_come_before_any_device_work():
    """No GPU here: a check that raised ValueError did so before require_gpu()."""
    import numpy as np
    import fastoptsolver_amd as fos
    A, b = np.zeros((6, 4)), np.zeros(6)
    for bad in (0.0, -1.0, float("nan"), float("inf"), None, "1", True):
        with pytest.raises(ValueError):
            fos.prepare_huber(A, b, bad)
    for y in ([1, -1, 0, 1, 1, -1], [1, -1, 0.5, 1, 1, -1], [1, -1, float("nan"), 1, 1, -1], np.ones((6, 1)), None):
        with pytest.raises(ValueError):
            fos.prepare_hinge(A, y)
    with pytest.raises(ValueError, match="threshold"):
        fos.huber_path(A, b, [(0.1, 0.0)])                    # no handle, no threshold
    with pytest.raises(ValueError, match="threshold"):
        fos.prepare(A, b, loss="huber")                       # the loss takes its parameter: prepare_huber
    with pytest.raises(ValueError):
        fos.huber_path(A, b, [], 1.0)
    with pytest.raises(ValueError):
        fos.hinge_path(A, [1, -1, 1, 1, 2, -1], [(0.1, 0.0)])
