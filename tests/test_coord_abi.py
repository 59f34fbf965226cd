"""CPU: the coordinate data of a problem handle (fos_coord_bind / fos_coord_get) is exported, bound, declared and documented and
refuses bad arguments before any HIP call; prepare_penalized refuses bad factors and bounds before any device work."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

NEW = ("fos_coord_bind", "fos_coord_get")
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
    assert ctypes.sizeof(_lib.FistaParams) == 8 * 8 + 4 * 4  # fos_fista_params keeps its size: the data is the problem's


def test_new_entry_points_take_their_data_pointers_first():
    """The guard tables file every function whose first parameter is a handle and every fos_fista_* function: the header gained
    neither."""
    from tests import _logit_guard as gd
    header = _header()
    assert not [n for n in re.findall(r"\b(fos_fista_[a-z0-9_]+)\s*\(", header) if "coord" in n or "penalty" in n]
    assert not (set(NEW) & gd.header_handle_functions())
    assert gd.header_handle_functions() == gd.SERVES | gd.LOSS_FREE | gd.REFUSES
    assert re.search(r"fos_coord_bind\s*\(\s*const\s+float\s*\*\s*penalty_factor\s*,\s*const\s+float\s*\*\s*lower\s*,\s*const\s+float\s*\*\s*"
                     r"upper\s*,\s*fos_problem\s*\*\s*p\s*\)", header)
    assert re.search(r"fos_coord_get\s*\(\s*const\s+float\s*\*\*\s*penalty_factor\s*,\s*const\s+float\s*\*\*\s*lower\s*,\s*const\s+float\s*"
                     r"\*\*\s*upper\s*,\s*const\s+fos_problem\s*\*\s*p\s*\)", header)


@pytest.mark.parametrize("case", ["null_problem", "all_null_null_problem", "factor_4", "lower_8", "upper_12", "upper_4_alone"])
def test_bind_argument_checks(lib, case):
    # the stand-in handle is never dereferenced: every case fails the argument check first
    pf, lo, hi, p = ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000), ctypes.c_void_p(0x4000), ctypes.c_void_p(0x1000)
    if case == "null_problem":
        p = None
    elif case == "all_null_null_problem":
        pf = lo = hi = p = None
    elif case == "factor_4":
        pf = ctypes.c_void_p(0x2004)
    elif case == "lower_8":
        lo = ctypes.c_void_p(0x3008)
    elif case == "upper_12":
        hi = ctypes.c_void_p(0x400c)
    else:
        pf, lo, hi = None, None, ctypes.c_void_p(0x4004)
    assert lib.fos_coord_bind(pf, lo, hi, p) == ARG
    assert "fos_coord_bind" in lib.fos_last_error().decode()


def test_get_argument_checks(lib):
    a, b, c = ctypes.c_void_p(7), ctypes.c_void_p(8), ctypes.c_void_p(9)
    assert lib.fos_coord_get(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), None) == ARG
    for args in ((None, ctypes.byref(b), ctypes.byref(c)), (ctypes.byref(a), None, ctypes.byref(c)), (ctypes.byref(a), ctypes.byref(b), None)):
        assert lib.fos_coord_get(*args, ctypes.c_void_p(0x1000)) == ARG
    assert "fos_coord_get" in lib.fos_last_error().decode() and (a.value, b.value, c.value) == (7, 8, 9)


A, B = np.ones((10, 4)), np.arange(10.0) / 10.0
BAD = {
    "factor_short": dict(penalty_factor=np.ones(3)), "factor_long": dict(penalty_factor=np.ones(5)),
    "factor_2d": dict(penalty_factor=np.ones((4, 1))), "factor_negative": dict(penalty_factor=[1, 1, -1e-30, 1]),
    "factor_nan": dict(penalty_factor=[1, np.nan, 1, 1]), "factor_inf": dict(penalty_factor=[1, np.inf, 1, 1]),
    "factor_negative_scalar": dict(penalty_factor=-1.0),
    "lower_positive": dict(lower=[0, 0, 1e-30, 0]), "lower_positive_scalar": dict(lower=0.5), "lower_nan": dict(lower=[0, np.nan, 0, 0]),
    "lower_short": dict(lower=np.zeros(3)),
    "upper_negative": dict(upper=[0, -1e-30, 0, 0]), "upper_nan": dict(upper=np.nan), "upper_long": dict(upper=np.zeros(5)),
    "zero_factors_nan_bounds": dict(penalty_factor=np.zeros(4), lower=[np.nan] * 4, upper=[np.nan] * 4),
    "nothing": {},
}


@pytest.mark.parametrize("bad", sorted(BAD))
@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_prepare_penalized_refuses_bad_data_before_any_device_work(bad, loss):
    """No GPU here: a call that got past the host checks would raise FosError, not ValueError."""
    import fastoptsolver_amd as fos
    with pytest.raises(ValueError):
        fos.prepare_penalized(A, B, loss=loss, **BAD[bad])
    with pytest.raises(ValueError):
        fos.prepare_penalized(A, B, loss=loss, **{k: torch.as_tensor(np.asarray(v, dtype=np.float64)) for k, v in BAD[bad].items()})


def test_checked_data_broadcasts_scalars_and_keeps_infinite_bounds():
    from fastoptsolver_amd import _core
    pf, lo, hi = _core.checked_coord(None, 0.0, [np.inf, 0.0, 1.0, np.inf], 4)
    assert pf is None and lo.tolist() == [0.0] * 4 and hi.tolist() == [np.inf, 0.0, 1.0, np.inf]
    pf, lo, hi = _core.checked_coord(np.zeros(4), -np.inf, None, 4)              # all-zero factors are a bounded least squares
    assert pf.tolist() == [0.0] * 4 and np.isneginf(lo).all() and hi is None


def test_signatures():
    import fastoptsolver_amd as fos
    from fastoptsolver_amd import _core, iterative_solvers as its
    pp = inspect.signature(fos.prepare_penalized).parameters
    assert list(pp) == ["A", "b", "penalty_factor", "lower", "upper", "dtype", "loss", "sample_weight"]
    assert pp["loss"].kind is inspect.Parameter.KEYWORD_ONLY and pp["sample_weight"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "prepare_penalized" in fos.__all__
    assert list(inspect.signature(_core.Problem.set_penalty).parameters) == ["self", "penalty_factor", "lower", "upper"]
    assert all(v.default is None for k, v in inspect.signature(_core.Problem.set_penalty).parameters.items() if k != "self")
    # the step rule: alpha2 max_j p_j joins L; a unit maximum is the step of a handle without factors, bit for bit
    assert its._tau(3.0, 0.5, 2.0, 4.0) == 2.0 / (3.0 + 0.5 * 4.0) and its._tau(3.0, 0.0, 1.0, 4.0) == 1.0 / 3.0
    assert its._tau(3.7, 0.3, 1.0) == its._tau(3.7, 0.3, 1.0, 1.0) == 1.0 / (3.7 + 0.3)
