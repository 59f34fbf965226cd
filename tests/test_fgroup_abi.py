"""CPU: the feature groups of a problem handle (fos_feature_groups_bind / fos_feature_groups_get) are exported, bound, declared
and documented; the bind refuses a malformed table before any HIP call; the Python layer refuses bad groups before any device
work; the guard tables of tests/_fgroup_guard.py are complete."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _fgroup_guard as gd

NEW = ("fos_feature_groups_bind", "fos_feature_groups_get")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1


@pytest.fixture(scope="module")
def lib():
    from fastoptsolver_amd import build, _lib
    build.build()
    return _lib.load()


def _header(name="fos_feature_groups.h"):
    with open(os.path.join(ROOT, "include", name)) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def test_symbols_exported_bound_declared_and_documented(lib):
    from fastoptsolver_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = _header()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        integration = fh.read()
    for name in NEW:
        assert f" T {name}" in out, name
        assert name in _lib.FEATURE_GROUP_SIGNATURES and name not in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.FEATURE_GROUP_SIGNATURES[name][1]
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in integration, name
    assert re.search(r"fos_feature_groups_bind\s*\(\s*const\s+int32_t\s*\*\s*group_start\s*,\s*const\s+float\s*\*\s*group_weight\s*,\s*"
                     r"int32_t\s+ngroups\s*,\s*double\s+l1_mix\s*,\s*fos_problem\s*\*\s*p\s*\)", header)
    assert re.search(r"fos_feature_groups_get\s*\(\s*int32_t\s*\*\s*ngroups\s*,\s*double\s*\*\s*l1_mix\s*,\s*const\s+fos_problem\s*\*\s*p\s*\)",
                     header)
    # a header of its own beside fos.h, whose handle-taking entry points are a closed list: it declares these two and nothing else
    assert sorted(set(re.findall(r"\b(fos_[a-z0-9_]+)\s*\(", header))) == sorted(NEW) == sorted(_lib.FEATURE_GROUP_SIGNATURES)
    assert '#include "fos.h"' in header and not [n for n in NEW if n in _header("fos.h")]
    assert lib.fos_abi_version() == 3                       # the ABI only grew
    assert ctypes.sizeof(_lib.FistaParams) == 8 * 8 + 4 * 4  # fos_fista_params keeps its size: the groups are the problem's


def _bind(lib, start, weight, ngroups, mix, p=0x1000):
    s = None if start is None else (ctypes.c_int32 * len(start))(*start)
    w = None if weight is None else (ctypes.c_float * len(weight))(*weight)
    return lib.fos_feature_groups_bind(s, w, ngroups, mix, None if p is None else ctypes.c_void_p(p))


BAD_TABLES = {
    "null_problem": dict(start=[0, 2, 4], weight=None, ngroups=2, mix=0.0, p=None),
    "detach_null_problem": dict(start=None, weight=None, ngroups=0, mix=0.0, p=None),
    "null_table": dict(start=None, weight=None, ngroups=2, mix=0.0),
    "no_groups": dict(start=[0], weight=None, ngroups=0, mix=0.0),
    "negative_count": dict(start=[0, 2], weight=None, ngroups=-1, mix=0.0),
    "first_not_zero": dict(start=[1, 2, 4], weight=None, ngroups=2, mix=0.0),
    "empty_group": dict(start=[0, 2, 2, 4], weight=None, ngroups=3, mix=0.0),
    "decreasing": dict(start=[0, 3, 2, 4], weight=None, ngroups=3, mix=0.0),
    "negative_weight": dict(start=[0, 2, 4], weight=[1.0, -1e-30], ngroups=2, mix=0.0),
    "nan_weight": dict(start=[0, 2, 4], weight=[float("nan"), 1.0], ngroups=2, mix=0.0),
    "inf_weight": dict(start=[0, 2, 4], weight=[1.0, float("inf")], ngroups=2, mix=0.0),
    "mix_below": dict(start=[0, 2, 4], weight=None, ngroups=2, mix=-1e-9),
    "mix_above": dict(start=[0, 2, 4], weight=None, ngroups=2, mix=1.0000001),
    "mix_nan": dict(start=[0, 2, 4], weight=None, ngroups=2, mix=float("nan")),
}


@pytest.mark.parametrize("case", sorted(BAD_TABLES))
def test_bind_refuses_a_bad_table_before_any_device_call(lib, case):
    # no device here, and the stand-in handle is never dereferenced: every case fails a check that does not need it
    assert _bind(lib, **BAD_TABLES[case]) == ARG
    assert "fos_feature_groups_bind" in lib.fos_last_error().decode()


def test_the_checks_that_need_the_handle_come_after_the_ones_that_do_not():
    body = gd.body_of("fos_feature_groups_bind")
    order = [body.index("null problem"), body.index("group_start[0] != 0"), body.index("group_start[g + 1] <= group_start[g]"),
             body.index("std::isfinite(group_weight[g])"), body.index("p->n"), body.index("FOS_ERR_UNSUPPORTED"), body.index("hip")]
    assert order == sorted(order)
    assert re.search(r"\(int64_t\)ngroups\s*>\s*p->n\s*\|\|\s*\(int64_t\)group_start\[ngroups\]\s*!=\s*p->n", body)
    for cond in (r"!p->b", r"p->comm\s*\|\|\s*p->col_sharded", r"!pair_dd_multi_supported\(p\)", r"has_coord\(p\)", r"FOS_LOSS_MULTINOMIAL"):
        assert re.search(cond, body), cond
    assert "invalidate(" not in body and "plan" not in body                          # nothing is replanned
    assert re.search(r"has_fgroups\(p\)", gd.body_of("fos_coord_bind")) and re.search(r"has_fgroups\(p\)", gd.body_of("fos_problem_set_multinomial"))


def test_get_argument_checks(lib):
    n, mix = ctypes.c_int32(7), ctypes.c_double(0.25)
    assert lib.fos_feature_groups_get(ctypes.byref(n), ctypes.byref(mix), None) == ARG
    assert lib.fos_feature_groups_get(None, ctypes.byref(mix), ctypes.c_void_p(0x1000)) == ARG
    assert lib.fos_feature_groups_get(ctypes.byref(n), None, ctypes.c_void_p(0x1000)) == ARG
    assert "fos_feature_groups_get" in lib.fos_last_error().decode() and (n.value, mix.value) == (7, 0.25)


def test_the_guard_reaches_the_feature_group_refusal_and_the_dispatchers_serve_it():
    from tests._menu_product1 import FISTA, PLAN, _body, _text
    guard = _body(_text(PLAN), r"int\s+" + gd.GUARD + r"\s*\([^)]*\)\s*(?=\{)")
    assert guard.index("p->loss") < guard.index("fgroup_refusal(p, fn)") < guard.index("coord_refusal(p, fn)")
    refusal = _body(_text(PLAN), r"int\s+fgroup_refusal\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"p\s*&&\s*has_fgroups\s*\(\s*p\s*\)", refusal) and len(re.findall(r"FOS_ERR_UNSUPPORTED", refusal)) == 1
    assert "fos_feature_groups_bind" in refusal and "std::string(fn)" in refusal     # a message of its own, naming the caller
    assert "hipLaunchKernelGGL" not in refusal and not re.search(r"->\w+\s*=[^=]", refusal)
    text = _text(FISTA)
    # both entry points reach the matrix-core pair through the pair-only branch of the one route decision
    route = _body(text, r"static\s+int\s+lockstep_route\s*\([^)]*\)\s*(?=\{)")
    m = re.search(r"if\s*\([^{]*\|\|\s*has_fgroups\(p\)\s*\)\s*\{", route)
    assert m and re.search(r"\*r\s*=\s*LockstepRoute\{ENGINE_MFMA,", route[:m.start()])
    assert "engine" not in _body(route[m.start():], r"has_fgroups\(p\)\s*\)\s*(?=\{)")
    for name in ("fos_fista_run_multi", "fos_fista_run_multi_folds"):
        assert re.search(r"return\s+run_lockstep\(LockstepCall\{", gd.body_of(name)), name
    mfma = _body(text, r"static\s+int\s+run_multi_mfma\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"const\s+bool\s+two_products\s*=[^;]*\|\|\s*fgroup\s*;", mfma) and "launch_fgroup_update" in mfma
    assert "has_fgroups(p)" in _body(text, r"static\s+int\s+group_refusal\s*\([^)]*\)\s*(?=\{)")


def test_the_update_kernels_have_no_waits_flags_or_atomics():
    with open(os.path.join(gd.mgd.CSRC, "reduce_update.hpp")) as fh:
        code = re.sub(r"//[^\n]*", "", fh.read())
    first, last = code.index("struct FeatureGroupData"), code.index("inline void fista_finalize_body")
    new = code[first:last]
    assert all(k in new for k in ("fgroup_form_u_kernel", "fgroup_norm_kernel", "fgroup_scale_kernel"))
    for word in ("atomic", "__threadfence", "while", "volatile", "cooperative", "s_sleep"):
        assert word not in new, word
    assert not re.search(r"\w+\[\s*e\s*\]", new.replace("acc[", ""))                 # no register array indexed by the loop counter


def test_the_c_table_is_complete_against_the_header():
    header = gd.header_handle_functions()
    filed = gd.SERVES | gd.LOSS_FREE | gd.REFUSES
    assert header - filed == set() and filed - header == set(), header ^ filed
    assert not (gd.SERVES & gd.LOSS_FREE or gd.SERVES & gd.REFUSES or gd.LOSS_FREE & gd.REFUSES)
    assert set(NEW) == gd.NEW <= gd.LOSS_FREE and gd.OWN_CHECK <= gd.REFUSES
    for name in sorted(gd.REFUSES - gd.OWN_CHECK):                                   # the one helper, in front of everything else
        body = gd.body_of(name)
        m = re.search(gd.GUARD + r"\s*\(", body)
        assert m, name
        assert not re.search(r"hipLaunchKernelGGL|hipMalloc|hipMemcpy|hipMemset|reserve\(|->\w+\s*=[^=]|invalidate\(", body[:m.start()]), name
        assert "has_fgroups" not in body and "fg." not in body, name                  # the refusing bodies know nothing of the groups


def test_the_python_table_is_in_step_with_the_public_names():
    import fastoptsolver_amd as fos
    assert set(gd.PYTHON) == set(fos.__all__), set(gd.PYTHON) ^ set(fos.__all__)
    assert len(fos.__all__) == len(set(fos.__all__))                                 # every name exactly once
    assert set(gd.PYTHON.values()) == {"serves", "loss_free", "refuses", "no_handle"}
    assert {"prepare_grouped", "group_lasso_objective"} <= set(fos.__all__)


A, B = np.ones((10, 6)), np.arange(10.0) / 10.0
BAD = {
    "labels_reappear": dict(groups=[0, 0, 1, 1, 0, 0]), "labels_reappear_strings": dict(groups=["a", "b", "b", "a", "c", "c"]),
    "sizes_short": dict(groups=[2, 3]), "sizes_long": dict(groups=[2, 3, 2]), "size_zero": dict(groups=[3, 0, 3]),
    "size_negative": dict(groups=[7, -1]), "sizes_fractional": dict(groups=[2.5, 3.5]), "groups_2d": dict(groups=[[3, 3]]),
    "groups_empty": dict(groups=[]),
    "weights_short": dict(groups=[2, 4], group_weight=[1.0]), "weights_long": dict(groups=[2, 4], group_weight=[1.0, 1.0, 1.0]),
    "weights_per_column": dict(groups=[0, 0, 1, 1, 1, 1], group_weight=np.ones(6)),
    "weight_negative": dict(groups=[2, 4], group_weight=[1.0, -1e-30]), "weight_nan": dict(groups=[2, 4], group_weight=[np.nan, 1.0]),
    "weight_inf": dict(groups=[2, 4], group_weight=[1.0, np.inf]), "weight_negative_scalar": dict(groups=[2, 4], group_weight=-1.0),
    "ratio_below": dict(groups=[2, 4], l1_ratio=-0.1), "ratio_above": dict(groups=[2, 4], l1_ratio=1.5),
    "ratio_nan": dict(groups=[2, 4], l1_ratio=np.nan),
}


@pytest.mark.parametrize("bad", sorted(BAD))
@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_prepare_grouped_refuses_bad_groups_before_any_device_work(bad, loss):
    """No GPU here: a call that got past the host checks would raise FosError, not ValueError."""
    import fastoptsolver_amd as fos
    with pytest.raises(ValueError):
        fos.prepare_grouped(A, B, loss=loss, **BAD[bad])


def test_a_reappearing_label_says_to_permute_the_columns():
    import fastoptsolver_amd as fos
    with pytest.raises(ValueError, match="permute the columns"):
        fos.prepare_grouped(A, B, [0, 1, 0, 1, 2, 2])
    with pytest.raises(ValueError):
        fos.prepare_grouped(A, None, [3, 3])
    with pytest.raises(ValueError):
        fos.prepare_grouped(A, B, None)


def test_checked_groups_take_both_forms_and_default_the_weights():
    from fastoptsolver_amd import _core
    s, w, r = _core.checked_feature_groups([5, 5, 7, 7, 7, 2], None, 0.25, 6)        # labels need not be sorted or dense
    assert s.tolist() == [0, 2, 5, 6] and s.dtype == np.int32 and np.allclose(w, np.sqrt([2, 3, 1])) and r == 0.25
    s2, w2, _ = _core.checked_feature_groups([2, 3, 1], [1.0, 0.0, 2.5], 1.0, 6)
    assert s2.tolist() == s.tolist() and w2.tolist() == [1.0, 0.0, 2.5]
    s3, w3, _ = _core.checked_feature_groups(np.arange(6), 2.0, 0, 6)                # all of size 1; a scalar weight broadcasts
    assert s3.tolist() == list(range(7)) and w3.tolist() == [2.0] * 6
    assert _core.checked_feature_groups([1] * 6, None, 0.0, 6)[0].tolist() == [0, 6]  # n entries are labels: one group


def test_signatures():
    import fastoptsolver_amd as fos
    from fastoptsolver_amd import _core
    pp = inspect.signature(fos.prepare_grouped).parameters
    assert list(pp) == ["A", "b", "groups", "group_weight", "l1_ratio", "dtype", "loss", "sample_weight"]
    assert pp["loss"].kind is inspect.Parameter.KEYWORD_ONLY and pp["sample_weight"].kind is inspect.Parameter.KEYWORD_ONLY
    assert pp["group_weight"].default is None and pp["l1_ratio"].default == 0.0
    assert list(inspect.signature(_core.Problem.set_feature_groups).parameters) == ["self", "groups", "group_weight", "l1_ratio"]
    assert isinstance(_core.Problem.feature_groups, property)
    oo = inspect.signature(fos.group_lasso_objective).parameters
    assert list(oo) == ["x", "A", "b", "alpha1", "alpha2", "groups", "group_weight", "l1_ratio", "loss", "sample_weight"]
    assert oo["loss"].kind is inspect.Parameter.KEYWORD_ONLY


def test_the_objective_is_the_stated_one():
    import fastoptsolver_amd as fos
    rng = np.random.default_rng(3)
    A_, b_, x = rng.standard_normal((20, 6)), rng.standard_normal(20), rng.standard_normal(6)
    x[2:5] = 0.0
    w = rng.uniform(0.5, 2.0, 20)
    gw = [1.0, 0.5, 2.0]
    pen = 0.7 * (0.75 * (1.0 * np.linalg.norm(x[:2]) + 0.5 * np.linalg.norm(x[2:5]) + 2.0 * abs(x[5])) + 0.25 * np.abs(x).sum()) + 0.5 * 0.3 * (x @ x)
    assert abs(fos.group_lasso_objective(x, A_, b_, 0.7, 0.3, [2, 3, 1], gw, 0.25, sample_weight=w) - (0.5 * (w * (A_ @ x - b_) ** 2).sum() + pen)) <= 1e-12
    y = (b_ > 0).astype(float)
    z = A_ @ x
    got = fos.group_lasso_objective(np.stack([x, 0 * x], axis=1), A_, y, 0.7, 0.3, [0, 0, 1, 1, 1, 2], gw, 0.25, loss="logistic")
    assert abs(got[0] - ((np.logaddexp(0, z) - y * z).sum() + pen)) <= 1e-12 and abs(got[1] - 20 * np.log(2.0)) <= 1e-12
    assert abs(fos.group_lasso_objective(x, A_, b_, 0.7, 0.0, [2, 3, 1]) - (0.5 * ((A_ @ x - b_) ** 2).sum() + 0.7 * (
        np.sqrt(2) * np.linalg.norm(x[:2]) + np.sqrt(3) * np.linalg.norm(x[2:5]) + abs(x[5])))) <= 1e-12
