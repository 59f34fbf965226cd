"""CPU: the batch entry points (fos_fista_run_batch, fos_fista_batch_workspace, fos_power_iter_batch) are exported, declared,
bound and documented, and refuse bad arguments before any HIP call; the Python front-ends tell a batch from a multi-target
call and refuse what a batch cannot be combined with, before any device work."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fos_fista_run_batch", "fos_fista_batch_workspace", "fos_power_iter_batch")


@pytest.fixture(scope="module")
def lib():
    from fastoptsolver_amd import build, _lib
    build.build()
    return _lib.load()


def _err(lib):
    return lib.fos_last_error().decode()


def test_symbols_exported_declared_bound_documented(lib):
    from fastoptsolver_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fos.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert f" T {name}" in out, name
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert name in doc, name
    assert "fos_batch_item" in header and ctypes.sizeof(_lib.BatchItem) == 32


def test_workspace_size(lib):
    one = lib.fos_fista_batch_workspace(1, 8)
    assert one > 8 * 8 and one % 8 == 0
    assert lib.fos_fista_batch_workspace(10, 8) == 10 * one
    assert lib.fos_fista_batch_workspace(0, 8) == 0
    assert lib.fos_fista_batch_workspace(-1, 8) == -1
    assert lib.fos_fista_batch_workspace(3, 0) == -1


def _items(lib, shapes):
    from fastoptsolver_amd import _core
    return _core.batch_items(shapes)


def _prm(count, **kw):
    from fastoptsolver_amd import _lib
    arr = (_lib.FistaParams * count)()
    for p in arr:
        p.tau, p.restart_threshold = 0.01, 1.0
        for k, v in kw.items():
            setattr(p, k, v)
    return arr


# never dereferenced: every case below fails the argument check first
FAKE = ctypes.c_void_p(0x1000)


@pytest.mark.parametrize("case", ["null_A", "null_b", "null_items", "null_prm", "null_x", "null_done", "null_stopped",
                                  "null_tau", "null_work", "count_neg", "iters_neg", "eta_0", "eta_1", "ldx_lt_n",
                                  "lda_lt_n", "neg_offset", "bad_dtype", "bad_mode", "bad_tau", "neg_tol", "too_big",
                                  "too_many_cols", "too_many_rows"])
def test_run_batch_argument_checks(lib, case):
    shapes = [(0, 5, 0, 100, 5), (500, 5, 100, 100, 5)]
    args = dict(A=FAKE, dt=0, b=FAKE, items=None, prm=_prm(2), count=2, iters=10, bt=1, eta=0.5, c=1e-2, ldx=8, x=FAKE,
                done=FAKE, stopped=FAKE, tau=FAKE, work=FAKE)
    expect = -1
    if case.startswith("null_"):
        key = {"null_A": "A", "null_b": "b", "null_items": "items", "null_prm": "prm", "null_x": "x", "null_done": "done",
               "null_stopped": "stopped", "null_tau": "tau", "null_work": "work"}[case]
        args[key] = None
        if key == "items":
            args["items"] = "none"
    elif case == "count_neg":
        args["count"] = -1
    elif case == "iters_neg":
        args["iters"] = -1
    elif case == "eta_0":
        args["eta"] = 0.0
    elif case == "eta_1":
        args["eta"] = 1.0
    elif case == "ldx_lt_n":
        args["ldx"] = 4
    elif case == "lda_lt_n":
        shapes[1] = (500, 4, 100, 100, 5)
    elif case == "neg_offset":
        shapes[1] = (-5, 5, 100, 100, 5)
    elif case == "bad_dtype":
        args["dt"] = 7
    elif case == "bad_mode":
        args["prm"] = _prm(2, mode=5)
    elif case == "bad_tau":
        args["prm"] = _prm(2, tau=0.0)
    elif case == "neg_tol":
        args["prm"] = _prm(2, tol_grad=-1.0)
    elif case == "too_big":                       # m * (n | 1) > 10240
        shapes[1], expect = (500, 40, 100, 1000, 40), -4
        args["ldx"] = 64
    elif case == "too_many_cols":
        shapes[1], expect = (500, 65, 100, 10, 65), -4
        args["ldx"] = 65
    elif case == "too_many_rows":
        shapes[1], expect = (500, 1, 100, 5000, 1), -4
    items = None if args["items"] == "none" else _items(lib, shapes)
    rc = lib.fos_fista_run_batch(args["A"], args["dt"], args["b"], items, args["prm"], args["count"], args["iters"],
                                 args["bt"], args["eta"], args["c"], args["ldx"], args["x"], args["done"], args["stopped"],
                                 args["tau"], None, None, None, None, args["work"], None)
    assert rc == expect, (case, rc, _err(lib))
    assert "fos_fista_run_batch" in _err(lib)


@pytest.mark.parametrize("case", ["null_A", "null_items", "null_v", "null_L", "null_used", "null_work", "count_neg",
                                  "n_iter_0", "ldv_lt_n", "bad_dtype", "too_big"])
def test_power_iter_batch_argument_checks(lib, case):
    shapes = [(0, 5, 0, 100, 5), (500, 5, 0, 100, 5)]
    a = dict(A=FAKE, dt=0, count=2, v=FAKE, ldv=8, n_iter=100, L=FAKE, used=FAKE, work=FAKE)
    expect = -1
    items_null = False
    if case == "null_items":
        items_null = True
    elif case.startswith("null_"):
        a[case[5:]] = None
    elif case == "count_neg":
        a["count"] = -1
    elif case == "n_iter_0":
        a["n_iter"] = 0
    elif case == "ldv_lt_n":
        a["ldv"] = 3
    elif case == "bad_dtype":
        a["dt"] = 3
    elif case == "too_big":
        shapes[1], expect = (500, 30, 0, 4000, 30), -4
        a["ldv"] = 30
    items = None if items_null else _items(lib, shapes)
    rc = lib.fos_power_iter_batch(a["A"], a["dt"], items, a["count"], a["v"], a["ldv"], a["n_iter"], 1e-6, a["L"],
                                  a["used"], a["work"], None)
    assert rc == expect, (case, rc, _err(lib))
    assert "fos_power_iter_batch" in _err(lib)


def test_empty_batch_is_a_no_op(lib):
    assert lib.fos_fista_run_batch(None, 0, None, None, None, 0, 10, 0, 0.5, 1e-2, 8, None, None, None, None, None, None,
                                   None, None, None, None) == 0
    assert lib.fos_power_iter_batch(None, 0, None, 0, None, 8, 100, 1e-6, None, None, None, None) == 0


def test_resident_fits_mirrors_the_kernel_limits():
    from fastoptsolver_amd._core import resident_fits
    assert resident_fits(1000, 5) and resident_fits(4096, 1) and resident_fits(160, 63) and resident_fits(10240 // 65, 64)
    assert not resident_fits(4097, 1) and not resident_fits(10, 65) and not resident_fits(1000, 40)
    assert not resident_fits(0, 5) and not resident_fits(5, 0)


def test_batch_detection_rules():
    """A 3-D A and a list / tuple of matrices are batches; a 2-D A with a 2-D b stays multi-target."""
    import torch
    from fastoptsolver_amd.iterative_solvers import _is_batch, _targets
    assert _is_batch(np.ones((3, 6, 4)))
    assert _is_batch(torch.ones(3, 6, 4))
    assert _is_batch([np.ones((6, 4)), np.ones((5, 3))])
    assert _is_batch((np.ones((6, 4)),))
    assert _is_batch([])
    assert not _is_batch(np.ones((6, 4)))
    assert not _is_batch(torch.ones(6, 4))
    assert _targets(np.ones((6, 4)), np.ones((6, 3))) is not None


def test_batch_refusals_without_device_work():
    """ValueError before any device work - the same with or without a GPU."""
    import fastoptsolver_amd as fos
    A3, b2 = np.ones((3, 8, 4)), np.ones((3, 8))
    for fn, extra in ((fos.fista, ()), (fos.fista_delta, (3.0,))):
        for kw in (dict(comm=object()), dict(group=object()), dict(cols=(0, 4, 4))):
            with pytest.raises(ValueError):
                fn(A3, b2, "lasso", 0.1, 0.0, *extra, max_iter=2, **kw)
        with pytest.raises(ValueError):                      # 3-D b
            fn(A3, np.ones((3, 8, 1)), "lasso", 0.1, 0.0, *extra, max_iter=2)
        with pytest.raises(ValueError):                      # P mismatch
            fn(A3, np.ones((2, 8)), "lasso", 0.1, 0.0, *extra, max_iter=2)
        with pytest.raises(ValueError):                      # row-count mismatch
            fn(A3, np.ones((3, 7)), "lasso", 0.1, 0.0, *extra, max_iter=2)
        with pytest.raises(ValueError):                      # sequence length mismatch
            fn([np.ones((8, 4)), np.ones((6, 3))], [np.ones(8)], "lasso", 0.1, 0.0, *extra, max_iter=2)
        with pytest.raises(ValueError):                      # member row-count mismatch
            fn([np.ones((8, 4)), np.ones((6, 3))], [np.ones(8), np.ones(5)], "lasso", 0.1, 0.0, *extra, max_iter=2)
        with pytest.raises(ValueError):                      # a member that is not 2-D
            fn([np.ones((8, 4)), np.ones(6)], [np.ones(8), np.ones(6)], "lasso", 0.1, 0.0, *extra, max_iter=2)
        with pytest.raises(ValueError):                      # L of the wrong length
            fn(A3, b2, "lasso", 0.1, 0.0, *extra, max_iter=2, L=[1.0, 2.0])
