"""CPU: the entry point of include/fos_duality.h (fos_duality_gap) is exported, bound and declared with the signature the header
documents, in its own header and in no other, and refuses bad arguments before any HIP call; duality_gap and certified_path have
the documented signatures and refuse what they do not serve before any device work; the kernels of csrc/duality.hpp are free of
atomics, flags and waits and use no scratch."""
import ctypes
import inspect
import glob
import os
import re
import subprocess
import types

import numpy as np
import pytest

NEW = "fos_duality_gap"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
P, D = ctypes.c_void_p(0x1000), lambda k=0: ctypes.c_void_p(0x2000 + 0x100 * k)     # stand-ins: never dereferenced


@pytest.fixture(scope="module")
def lib():
    from fastoptsolver_amd import build, _lib
    build.build()
    return _lib.load()


def _header(name="fos_duality.h"):
    with open(os.path.join(ROOT, "include", name)) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def test_symbol_exported_bound_and_declared(lib):
    from fastoptsolver_amd import _lib, build
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = _header()
    assert re.findall(r"\b(fos_[a-z0-9_]+)\s*\(", header) == [NEW] == list(_lib.DUALITY_SIGNATURES)
    assert f" T {NEW}" in out
    assert getattr(lib, NEW).argtypes == _lib.DUALITY_SIGNATURES[NEW][1] and getattr(lib, NEW).restype is ctypes.c_int
    for table in (_lib.SIGNATURES, _lib.FEATURE_GROUP_SIGNATURES, _lib.WORKING_SET_SIGNATURES, _lib.LINK_LOSS_SIGNATURES):
        assert NEW not in table                                      # a table of its own, merged in load()
    assert lib.fos_abi_version() == 3                               # the ABI only grew
    sig = r"\s*,\s*".join
    assert re.search(r"int\s+fos_duality_gap\s*\(\s*" + sig([r"const\s+float\s*\*\s*X", r"int\s+nv", r"const\s+double\s*\*\s*alpha1",
                                                               r"const\s+double\s*\*\s*alpha2", r"fos_problem\s*\*\s*p",
                                                               r"float\s*\*\s*G", r"double\s*\*\s*out64"]) + r"\s*\)", header)
    assert os.path.join(ROOT, "include", "fos_duality.h") in build.HEADERS
    assert os.path.join(ROOT, "fastoptsolver_amd", "csrc", "duality.hpp") in build.HEADERS


def test_no_other_header_declares_it_and_the_closed_lists_did_not_grow():
    from tests import _logit_guard as gd
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.basename(path) != "fos_duality.h":
            assert not re.search(r"\b" + NEW + r"\s*\(", _header(os.path.basename(path))), path
    assert NEW not in gd.header_handle_functions()
    assert gd.header_handle_functions() == gd.SERVES | gd.LOSS_FREE | gd.REFUSES
    assert not re.match(r"fos_problem_set_|fos_\w+_bind$", NEW)      # it binds nothing to the handle
    from fastoptsolver_amd import _lib
    assert ctypes.sizeof(_lib.FistaParams) == 8 * 8 + 4 * 4         # fos_fista_params keeps its size


@pytest.mark.parametrize("case", ["null_X", "null_alpha1", "null_alpha2", "null_p", "null_G", "null_out64", "nv_0", "nv_17", "nv_-1",
                                  "alpha1_negative", "alpha1_nan", "alpha1_inf", "alpha2_negative", "alpha2_nan", "alpha2_inf"])
def test_argument_checks_come_before_any_hip_call(lib, case):
    a1 = (ctypes.c_double * 16)(*([0.5] * 16))
    a2 = (ctypes.c_double * 16)(*([0.0] * 16))
    args = dict(X=D(0), nv=3, alpha1=a1, alpha2=a2, p=P, G=D(1), out64=D(2))
    if case.startswith("null_"):
        args[case[5:]] = None
    elif case.startswith("nv_"):
        args["nv"] = int(case[3:])
    else:
        which, what = case.split("_")
        (a1 if which == "alpha1" else a2)[2] = {"negative": -1e-300, "nan": float("nan"), "inf": float("inf")}[what]
    assert lib.fos_duality_gap(*args.values()) == ARG
    assert NEW in lib.fos_last_error().decode()


def test_a_bad_weight_beyond_nv_is_not_read(lib):
    """Only the nv weights in use are checked: the refusal of a stand-in handle below would otherwise be FOS_ERR_ARG.  (No call
    is made here that would get past the argument checks: the stand-in handle must never be dereferenced.)"""
    a1 = (ctypes.c_double * 16)(*([0.5] * 16))
    a1[2] = float("nan")
    assert lib.fos_duality_gap(D(0), 3, a1, a1, P, D(1), D(2)) == ARG
    assert "weight 2" in lib.fos_last_error().decode()


A, B = np.ones((10, 4)), np.arange(10.0) / 10.0


def test_python_signatures_and_fields():
    import fastoptsolver_amd as fos
    from fastoptsolver_amd import _core, duality
    cp = inspect.signature(fos.certified_path).parameters
    assert list(cp) == ["A", "b", "alphas", "gap_tol", "max_iter", "max_rounds", "grow", "max_fraction", "L", "t_init_factor", "dtype",
                        "return_info"]
    assert [cp[k].default for k in ("gap_tol", "max_iter", "max_rounds", "grow", "max_fraction", "L", "t_init_factor", "dtype",
                                    "return_info")] == [1e-4, 500, 20, 2.0, 0.5, None, 1.0, None, False]
    assert all(cp[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(cp)[5:])
    assert all(cp[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in list(cp)[:5])
    assert list(inspect.signature(fos.duality_gap).parameters) == ["prob", "X", "alphas"]
    assert list(inspect.signature(_core.Problem.duality_gap_block).parameters) == ["self", "X", "alpha1", "alpha2"]
    assert fos.DualityGap._fields == ("primal", "dual", "gap", "scale")
    assert fos.GapInfo._fields == ("rounds", "sizes", "certificates", "primal", "dual", "gap", "scale", "certified", "fell_back")
    for name in ("duality_gap", "certified_path", "DualityGap", "GapInfo"):
        assert getattr(fos, name) is getattr(duality, name) and name not in fos.__all__
    # working_set_path keeps its signature
    ws = inspect.signature(fos.working_set_path).parameters
    assert list(ws) == ["A", "b", "alphas", "max_iter", "kkt_tol", "max_rounds", "grow", "max_fraction", "L", "t_init_factor", "dtype",
                        "initial", "return_info"]


def test_python_refusals_come_before_any_device_work():
    """No GPU here: a call that got past the host checks would raise FosError, not ValueError."""
    import fastoptsolver_amd as fos
    from fastoptsolver_amd import _core
    for kw in (dict(grow=1.0), dict(max_fraction=0.0), dict(max_fraction=1.5), dict(max_rounds=0), dict(gap_tol=-1.0),
               dict(gap_tol=float("nan"))):
        with pytest.raises(ValueError):
            fos.certified_path(A, B, [(0.1, 0.0)], **kw)
    with pytest.raises(ValueError):
        fos.certified_path(A, B, [])
    with pytest.raises(ValueError):
        fos.certified_path(A, None, [(0.1, 0.0)])

    def handle(**kw):                    # what _handle reads of a Problem, without a device
        h = _core.Problem.__new__(_core.Problem)
        h.loss, h.grouped, h._coord, h._fgroups, h.n, h.b = "squared", False, (None, None, None), None, 4, object()
        for k, v in kw.items():
            setattr(h, k, v)
        h.h = None
        return h
    lo = types.SimpleNamespace(__getitem__=None)
    for bad, word in ((handle(loss="multinomial"), "multinomial"), (handle(grouped=True), "group penalty"),
                      (handle(_coord=(None, np.zeros(4), None)), "bounds"), (handle(_coord=(None, None, np.zeros(4))), "bounds"),
                      (handle(_fgroups=(lo, lo, 0.0)), "feature groups"), (handle(comm=object()), "sharded"),
                      (handle(col_sharded=True), "sharded"), (handle(b=None), "without b")):
        for call, same in ((lambda: fos.certified_path(bad, None, [(0.1, 0.0)]), lambda: fos.working_set_path(bad, None, [(0.1, 0.0)])),
                           (lambda: fos.duality_gap(bad, np.zeros(4), [(0.1, 0.0)]), lambda: fos.kkt_excess(bad, np.zeros(4), [(0.1, 0.0)]))):
            with pytest.raises(ValueError, match=word) as mine:
                call()
            with pytest.raises(ValueError) as theirs:
                same()
            assert str(mine.value).split(": ", 1)[1] == str(theirs.value).split(": ", 1)[1]      # the same refusal, under its own name
    with pytest.raises(ValueError, match="alpha1 = 0"):
        fos.certified_path(handle(n_dev=4), None, [(0.1, 0.0), (0.0, 0.5)])


def _source():
    with open(os.path.join(ROOT, "fastoptsolver_amd", "csrc", "duality.hpp")) as fh:
        return fh.read()


def test_kernel_source_has_no_atomics_flags_or_waits():
    text = _source()
    for word in ("atomic", "volatile", "while", "__threadfence", "asm"):
        assert not re.search(word, text, flags=re.I), word
    code = re.sub(r"//[^\n]*", "", text)
    # the column pass serves every loss family: it takes the class count and the kind of penalty (1 and 0 from fos_duality_gap)
    assert re.search(r"dual_scale_kernel\(const float\* __restrict__ X, const float\* __restrict__ G,\s+int64_t n, int classes, int grouped, "
                     r"ClassWeights wts", code)
    assert re.search(r"template\s*<int LOSS, bool WEIGHT>\s*__global__\s+__launch_bounds__\(DL_THREADS\)\s+void\s+dual_link_kernel", code)
    assert re.search(r"__global__\s+__launch_bounds__\(DS_THREADS\)\s+void\s+dual_scale_kernel", code)
    assert re.search(r"__global__\s+__launch_bounds__\(DF_THREADS\)\s+void\s+dual_finish_kernel", code)
    # the row pass only reads the panel
    assert re.search(r"dual_link_kernel\(const float\* __restrict__ z16", code)


UNIT = """
#include "duality.hpp"
// every instantiation fos_duality_gap launches: four losses x WEIGHT, the column pass, the finish
void* fos_duality_kernels[] = {
    (void*)fos::dual_link_kernel<fos::DUAL_SQUARED, false>, (void*)fos::dual_link_kernel<fos::DUAL_SQUARED, true>,
    (void*)fos::dual_link_kernel<fos::DUAL_LOGISTIC, false>, (void*)fos::dual_link_kernel<fos::DUAL_LOGISTIC, true>,
    (void*)fos::dual_link_kernel<fos::DUAL_HUBER, false>, (void*)fos::dual_link_kernel<fos::DUAL_HUBER, true>,
    (void*)fos::dual_link_kernel<fos::DUAL_SQUARED_HINGE, false>, (void*)fos::dual_link_kernel<fos::DUAL_SQUARED_HINGE, true>,
    (void*)fos::dual_scale_kernel, (void*)fos::dual_finish_kernel};
"""


def test_kernels_use_no_scratch(tmp_path):
    from fastoptsolver_amd import build
    src = tmp_path / "du_unit.hip"
    src.write_text(UNIT)
    cmd = [build.hipcc_path(), *build.FLAGS, "-I", build.CSRC, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "du_unit.o"),
           str(src)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name:\s+(\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|VGPRs|LDS Size \[bytes/block\]):\s+(\d+)", line)
        if m and cur:
            kernels[cur][m.group(1)] = int(m.group(2))
    link = {k: v for k, v in kernels.items() if "dual_link_kernel" in k}
    scale = {k: v for k, v in kernels.items() if "dual_scale_kernel" in k}
    finish = {k: v for k, v in kernels.items() if "dual_finish_kernel" in k}
    assert len(link) == 8 and len(scale) == 1 and len(finish) == 1, sorted(kernels)
    for k, v in {**link, **scale, **finish}.items():
        assert not v.get("VGPRs Spill", 0) and not v.get("SGPRs Spill", 0) and not v.get("ScratchSize [bytes/lane]", 0), (k, v)
        assert v["VGPRs"] <= 128, (k, v)                                  # at least four waves per SIMD
    assert all(v["LDS Size [bytes/block]"] == 4096 for v in link.values())           # 16 rows x 32 doubles
    assert all(v["LDS Size [bytes/block]"] == 2048 for v in scale.values())          # one double per thread
    # the instantiations above are the ones the library launches
    with open(os.path.join(build.CSRC, "fos_fista.hip")) as fh:
        text = fh.read()
    assert set(re.findall(r"FOS_DUAL_FORM\((DUAL_\w+)\)", text)) == {"DUAL_SQUARED", "DUAL_LOGISTIC", "DUAL_HUBER", "DUAL_SQUARED_HINGE"}
    assert "fos::dual_scale_kernel" in text and "fos::dual_finish_kernel" in text
