"""CPU: the group penalty is a solver parameter - fos_fista_params.group stands where `reserved` stood, the struct keeps its size
and the ABI its version, no handle-taking entry point was added; fos_fista_reset refuses a bad group before any HIP call; the
packing and right-hand-side tiling of multitask_path are what the documentation says; bad arguments are ValueErrors before any
device work; every single-handle entry point calls the one group guard before anything launch-like and the grouped update takes the
place of the one separable update launch of run_multi_mfma."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import _logit_guard as lgd, _multinomial_guard as gd
from tests._menu_product1 import FISTA, _body, _text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -4
GUARD = "need_separable"
SINGLE = ("fos_fista_run", "fos_fista_run_history", "fos_fista_run_resident", "fos_fista_run_fused", "fos_fista_run_chip",
          "fos_fista_grad", "fos_fista_grad_dual", "fos_fista_update", "fos_fista_trial", "fos_fista_trial_batch",
          "fos_fista_run_backtracking", "fos_fista_run_recorded", "fos_fista_resume_after_stall")
LAUNCHY = r"hipLaunchKernelGGL|hipMalloc|hipMemcpy|hipMemset|reserve\(|->\w+\s*=[^=]|invalidate\(|flush_pending|begin_plain|hand_to_device"


@pytest.fixture(scope="module")
def lib():
    from fastoptsolver_amd import build, _lib
    build.build()
    return _lib.load()


def _header():
    with open(os.path.join(ROOT, "include", "fos.h")) as fh:
        return fh.read()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_group_stands_where_reserved_stood(lib):
    from fastoptsolver_amd import _lib
    struct = re.search(r"typedef struct fos_fista_params \{(.*?)\} fos_fista_params;", _header(), flags=re.S).group(1)
    fields = re.findall(r"^\s*(double|int32_t)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", struct, flags=re.S), flags=re.M)
    assert fields == [("double", k) for k in ("tau", "alpha1", "alpha2", "delta", "restart_threshold", "tol_step", "tol_ratio",
                                              "tol_grad")] + [("int32_t", k) for k in ("mode", "prox_kind", "adaptive_restart", "group")]
    assert [(("double" if t is ctypes.c_double else "int32_t"), k) for k, t in _lib.FistaParams._fields_] == fields
    assert ctypes.sizeof(_lib.FistaParams) == 8 * 8 + 4 * 4 and _lib.FistaParams.group.offset == 8 * 8 + 3 * 4
    assert lib.fos_abi_version() == 3
    assert "group penalty" in struct or "Euclidean norm" in struct                       # documented where it is declared
    status = re.search(r"typedef struct fos_fista_status \{(.*?)\} fos_fista_status;", _header(), flags=re.S).group(1)
    assert "not the group norm" in status


def test_no_entry_point_was_added_for_the_penalty():
    assert gd.header_handle_functions() == gd.SERVES | gd.LOSS_FREE | gd.REFUSES
    assert not [n for n in re.findall(r"\b(fos_[a-z0-9_]+)\s*\(", _header()) if "group" in n or "multitask" in n]


@pytest.mark.parametrize("group", [-1, 17, 1 << 20])
def test_reset_refuses_a_bad_group_before_touching_the_handle(lib, group):
    from fastoptsolver_amd import _lib
    prm = _lib.FistaParams(tau=1.0, alpha1=0.1, group=group)
    # the stand-in handle is never dereferenced: the argument check comes first
    assert lib.fos_fista_reset(ctypes.c_void_p(0x1000), ctypes.byref(prm), None) == ARG
    assert "fos_fista_reset" in lib.fos_last_error().decode() and "0..16" in lib.fos_last_error().decode()


def test_run_batch_refuses_grouped_parameters_before_any_device_work(lib):
    from fastoptsolver_amd import _lib
    items = (_lib.BatchItem * 1)()
    items[0].a_offset, items[0].lda, items[0].b_offset, items[0].m, items[0].n = 0, 4, 0, 8, 4
    stand_in = ctypes.c_void_p(0x1000)
    for group, want in ((3, UNSUPPORTED), (17, ARG)):
        prm = (_lib.FistaParams * 1)(_lib.FistaParams(tau=1.0, alpha1=0.1, group=group))
        rc = lib.fos_fista_run_batch(stand_in, _lib.FOS_F32, stand_in, items, prm, 1, 3, 0, 0.5, 1e-2, 4, stand_in, stand_in, stand_in,
                                     stand_in, None, None, None, None, stand_in, None)
        assert rc == want and "group" in lib.fos_last_error().decode()


def test_the_python_layers_pass_the_field_through():
    from fastoptsolver_amd import _core, _lib, iterative_solvers as its
    assert "group" not in its._params(0.1, 1.0, 0.0, mode=_lib.MODE_FISTA)            # absent: the separable penalty
    assert its._params(0.1, 1.0, 0.0, mode=_lib.MODE_FISTA, group=5)["group"] == 5
    assert inspect.signature(_core.Fista.reset).parameters["group"].default == 0
    assert inspect.signature(its._params).parameters["group"].default == 0


# ---- pure functions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,per", [(2, 8), (3, 5), (5, 3), (8, 2), (9, 1), (16, 1)])
def test_packing_and_tiling(T, per):
    from fastoptsolver_amd import multitask
    for count in (1, per, per + 1, 3 * per + 2):
        groups = multitask.pack_groups(count, T)
        assert [f for f, _ in groups] == list(range(0, count, per)) and sum(k for _, k in groups) == count
        assert all(k == per for _, k in groups[:-1]) and 1 <= groups[-1][1] <= per
    B = np.arange(7 * T, dtype=np.float32).reshape(7, T)
    for number in (1, per):
        for src in (B, torch.from_numpy(B)):
            tiled = multitask.tile_targets(src, number)
            assert type(tiled) is type(src) and tuple(tiled.shape) == (7, number * T)
            tn = np.asarray(tiled)
            assert all(np.array_equal(tn[:, i * T:(i + 1) * T], B) for i in range(number))
    with pytest.raises(ValueError):
        multitask.tile_targets(B, 0)


def test_signatures_and_exports():
    import fastoptsolver_amd as fos
    path = inspect.signature(fos.multitask_path).parameters
    assert list(path) == ["A", "B", "alphas", "t_init_factor", "max_iter", "delta", "L", "dtype", "return_info"]
    assert all(path[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(path)[5:])
    assert (path["t_init_factor"].default, path["max_iter"].default, path["return_info"].default) == (1.0, 500, False)
    assert list(inspect.signature(fos.multitask_objective).parameters) == ["X", "A", "B", "alpha1", "alpha2"]
    assert "multitask_path" in fos.__all__ and "multitask_objective" in fos.__all__
    # the grouped multinomial penalty belongs to the handle: the three solvers keep their parameter lists
    for fn in (fos.multinomial_path, fos.multinomial_cv, fos.multinomial_objective):
        assert "grouped" not in inspect.signature(fn).parameters
    prep = inspect.signature(fos.prepare_multinomial).parameters
    assert prep["grouped"].default is False and prep["grouped"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(fos.Problem.set_grouped).parameters) == ["self", "on"]
    for doc in (fos.multitask_path.__doc__, inspect.getmodule(fos.multitask_path).__doc__):
        for words in ("ross-validation", "parse-group", "within one column", "harded"):
            assert words in doc, words


# ---- ValueErrors before any device work --------------------------------------------------------------------------------------
A = np.ones((10, 70))


@pytest.mark.parametrize("B", [np.ones((10, 1)), np.ones((10, 17)), np.ones(10), np.ones((9, 3)), np.ones((11, 2))],
                         ids=["T=1", "T=17", "1-D", "9-rows", "11-rows"])
def test_bad_targets_are_value_errors(B):
    import fastoptsolver_amd as fos
    with pytest.raises(ValueError):
        fos.multitask_path(A, B, [(0.1, 0.0)], max_iter=2, L=1.0)
    with pytest.raises(ValueError):
        fos.multitask_objective(np.zeros((70, 3)), A, B, 0.1, 0.0)


def test_empty_path_and_small_delta_are_value_errors():
    import fastoptsolver_amd as fos
    B = np.ones((10, 3))
    with pytest.raises(ValueError):
        fos.multitask_path(A, B, [], max_iter=2, L=1.0)
    with pytest.raises(ValueError):
        fos.multitask_path(A, B, [(0.1, 0.0)], delta=2.0, max_iter=2, L=1.0)


def _stand_in(loss, lower=None, upper=None, weights=None, classes=None):
    """A Problem that was never bound: what the host checks read, nothing a device call could use."""
    from fastoptsolver_amd import _core
    P = _core.Problem.__new__(_core.Problem)
    P.loss, P.classes, P.m, P.n, P.n_dev, P.sample_weight = loss, classes, 10, 70, 72, weights
    P._coord = (None, lower, upper)
    P.grouped = False
    return P


@pytest.mark.parametrize("bound", ["lower", "upper"])
def test_grouped_with_bounds_is_a_value_error(bound):
    import fastoptsolver_amd as fos
    P = _stand_in("multinomial", classes=3, **{bound: np.zeros(72, dtype=np.float32)})
    with pytest.raises(ValueError, match="box bounds"):
        P.set_grouped()
    assert P.grouped is False
    P.grouped = True                                        # bounds bound after the handle became a grouped one
    for call in (lambda: fos.multinomial_path(P, None, [(0.1, 0.0)], max_iter=2, L=1.0),
                 lambda: fos.multinomial_cv(P, None, [(0.1, 0.0)], folds=2, max_iter=2, L=1.0),
                 lambda: fos.multinomial_objective(np.zeros((70, 3)), P, None, 0.1, 0.0)):
        with pytest.raises(ValueError, match="box bounds"):
            call()
    with pytest.raises(ValueError, match="box bounds"):     # before any device work: nothing is uploaded
        fos.prepare_multinomial(np.ones((10, 70)), np.arange(10) % 3, grouped=True, **{bound: 0.0})
    with pytest.raises(ValueError, match="multinomial handle"):
        _stand_in("squared").set_grouped()
    free = _stand_in("multinomial", classes=3)
    free.set_grouped()
    assert free.grouped is True
    free.set_grouped(False)
    assert free.grouped is False
    Q = _stand_in("squared", **{bound: np.zeros(72, dtype=np.float32)})
    with pytest.raises(ValueError, match="box bounds"):
        fos.multitask_path(Q, np.ones((10, 3)), [(0.1, 0.0)], max_iter=2, L=1.0)


def test_multitask_refuses_other_losses_and_row_weights():
    import fastoptsolver_amd as fos
    B = np.ones((10, 3))
    for P in (_stand_in("logistic"), _stand_in("multinomial", classes=3), _stand_in("squared", weights=np.ones(10))):
        with pytest.raises(ValueError):
            fos.multitask_path(P, B, [(0.1, 0.0)], max_iter=2, L=1.0)


# ---- source checks -----------------------------------------------------------------------------------------------------------
def test_there_is_one_group_guard_and_it_names_the_penalty():
    text = _text(FISTA)
    assert len(re.findall(r"^static\s+int\s+" + GUARD + r"\s*\([^;{]*\)\s*\{", text, flags=re.M)) == 1
    body = _body(text, r"static\s+int\s+" + GUARD + r"\s*\([^)]*\)\s*(?=\{)")
    assert len(re.findall(r"FOS_ERR_UNSUPPORTED", body)) == 1 and "group penalty" in body and "std::string(fn)" in body
    assert "hipLaunchKernelGGL" not in body and not re.search(r"->\w+\s*=[^=]", body)


@pytest.mark.parametrize("name", SINGLE)
def test_every_single_handle_entry_point_calls_the_group_guard_first(name):
    body = lgd.body_of(name)
    m = re.search(GUARD + r"\s*\(\s*f\s*,\s*\"" + name + r"\"\s*\)", body)
    assert m, name
    assert not re.search(LAUNCHY, body[:m.start()]), name
    assert body.index(lgd.GUARD) < m.start()                 # behind the loss guard, whose message keeps precedence


def test_the_batch_entry_point_refuses_grouped_parameters_before_its_first_copy():
    body = lgd.body_of("fos_fista_run_batch")
    m = re.search(r"q\.group\s*>=\s*2", body)
    assert m and "FOS_ERR_UNSUPPORTED" in body[m.start():m.start() + 200]
    assert not re.search(r"hipLaunchKernelGGL|hipMemcpy|hipMemset", body[:m.start()])


def test_the_grouped_update_takes_the_place_of_the_separable_launch():
    from tests import _menu_coord as mc
    text = _text(FISTA)
    mfma = _body(text, r"static\s+int\s+run_multi_mfma\s*\([^)]*\)\s*(?=\{)")
    # the update stage: feature groups, else the group penalty, else the one separable launch - each launcher named once
    m = re.search(mc.UPDATE_STAGE, mfma)
    assert m, "the update stage of run_multi_mfma"
    assert mfma.index("launch_group_update") < mfma.index("launch_separable_update")
    assert mfma.count("launch_group_update") == 1 and "fista_update_group_kernel" not in mfma
    assert mfma.count("launch_separable_update") == 1 and "fista_update_multi_kernel" not in mfma
    # never the cluster form: the one expression of two_products names the group penalty
    assert re.search(r"const\s+bool\s+two_products\s*=[^;]*\|\|\s*group_penalty\b[^;]*;", mfma) and len(re.findall(r"\btwo_products\s*=[^=]", mfma)) == 1
    helper = _body(text, r"static\s+int\s+launch_group_update\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"fos::fista_update_group_kernel,\s*dim3\(fs\[0\]->nupd,\s*nv\s*/\s*G\),\s*dim3\(256\)", helper)
    # one launch site each in the whole unit
    for kernel in ("fista_update_multi_kernel", "fista_update_group_kernel", "fgroup_form_u_kernel", "fgroup_norm_kernel", "fgroup_scale_kernel"):
        assert len(re.findall(r"fos::" + kernel + r"\b", text)) == (2 if kernel == "fista_update_multi_kernel" else 1), kernel
    assert text.count("hipLaunchKernelGGL(kern, dim3(fs[0]->nupd, nv)") == 1      # (<true> and <false> meet in that one launch)
    # the route decision asks the one refusal helper before anything runs: on the multinomial branch and on the group branch,
    # and the executor decides the route before its first launch
    route = _body(text, r"static\s+int\s+lockstep_route\s*\([^)]*\)\s*(?=\{)")
    assert len(re.findall(r"group_refusal\(fs,\s*nv,\s*c\.held_ids,\s*c\.fn\)", route)) == 2
    soft, group = route.index("p->loss == FOS_LOSS_MULTINOMIAL"), route.index("any_grouped(fs, nv)")
    first = [route.index("group_refusal(", at) for at in (soft, group)]
    assert soft < first[0] < group < first[1] and "FOS_ERR_UNSUPPORTED" not in route[soft:first[0]] + route[group:first[1]]
    assert "hipLaunchKernelGGL" not in route and "run_multi_mfma" not in route and not re.search(r"[^r]->\w+\s*=[^=]", route)
    run = _body(text, r"static\s+int\s+run_lockstep\s*\([^)]*\)\s*(?=\{)")
    assert run.index("lockstep_route(c, &r)") < run.index("c.iters == 0") < run.index("stage_b16(") < run.index("run_multi_mfma(c, r)")
    refusal = _body(text, r"static\s+int\s+group_refusal\s*\([^)]*\)\s*(?=\{)")
    assert "FOS_ERR_ARG" not in refusal and "hipLaunchKernelGGL" not in refusal and not re.search(r"->\w+\s*=[^=]", refusal)
    for cond in (r"nv\s*%\s*G", r"p->classes", r"p->coord_lo\s*\|\|\s*p->coord_hi", r"plain_run\(f\)", r"f->precise", r"tau_from_state",
                 r"!unsharded_pair\(p\)", r"!fit_column_agrees\(fs,\s*v,\s*G,\s*held\)"):
        assert re.search(cond, refusal), cond
    # ... and the two shared helpers it calls hold the conditions it used to spell out
    pair = _body(text, r"static\s+bool\s+unsharded_pair\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"!p->comm\s*&&\s*!p->col_sharded\s*&&\s*pair_dd_multi_supported\(p\)", pair)
    agrees = _body(text, r"static\s+bool\s+fit_column_agrees\s*\([^)]*\)\s*(?=\{)")
    for cond in (r"a\.group\s*==\s*c\.group", r"a\.tau\s*==\s*c\.tau", r"a\.alpha1\s*==\s*c\.alpha1", r"a\.alpha2\s*==\s*c\.alpha2", r"a\.delta\s*==\s*c\.delta",
                 r"a\.mode\s*==\s*c\.mode", r"a\.prox_kind\s*==\s*c\.prox_kind", r"held\s*&&\s*held\[v\]\s*!=\s*held\[v0\]"):
        assert re.search(cond, agrees), cond


def test_the_group_kernel_has_no_atomics_flags_or_waits():
    with open(os.path.join(lgd.CSRC, "reduce_update.hpp")) as fh:
        code = re.sub(r"//[^\n]*", "", fh.read())
    m = re.search(r"void\s+fista_update_group_kernel\s*\(", code)
    body, depth, i = "", 0, code.index("{", m.end())
    start = i
    while True:
        depth += {"{": 1, "}": -1}.get(code[i], 0)
        i += 1
        if depth == 0:
            break
    body = code[start:i]
    for word in ("atomic", "__threadfence", "while", "volatile", "cooperative", "s_sleep"):
        assert word not in body, word
    assert "__shared__ double stash[BT_NV][4][RQ]" in body and "reduce_slab_block(" in body and "quad_lane(pf4" in body
