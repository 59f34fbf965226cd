"""CPU: the three entry points of include/fos_multinomial_ws.h are exported, bound and declared with the signatures the header
documents, in their own header and in no other, and refuse bad arguments before any HIP call; the Python names have the documented
signatures and refuse what they do not serve before any device work; the kernels of csrc/multinomial_ws.hpp are free of atomics,
flags and waits and use no scratch.

The weights of fos_multinomial_kkt_scan and fos_multinomial_duality_gap are one per segment, and the number of segments is nv / C
with C read from the problem: those FOS_ERR_ARG rows need a real handle and are in tests/test_gpu_multinomial_ws.py."""
import ctypes
import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

NEW = ["fos_multinomial_gradient_batch", "fos_multinomial_kkt_scan", "fos_multinomial_duality_gap"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
P, D = ctypes.c_void_p(0x1000), lambda k=0: ctypes.c_void_p(0x2000 + 0x100 * k)     # stand-ins: never dereferenced


@pytest.fixture(scope="module")
def lib():
    from fastoptsolver_amd import build, _lib
    build.build()
    return _lib.load()


def _header(name="fos_multinomial_ws.h"):
    with open(os.path.join(ROOT, "include", name)) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def test_symbols_exported_bound_and_declared(lib):
    from fastoptsolver_amd import _lib, build
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = _header()
    assert re.findall(r"\b(fos_[a-z0-9_]+)\s*\(", header) == NEW == list(_lib.MULTINOMIAL_WS_SIGNATURES)
    for name in NEW:
        assert f" T {name}" in out
        assert getattr(lib, name).argtypes == _lib.MULTINOMIAL_WS_SIGNATURES[name][1] and getattr(lib, name).restype is ctypes.c_int
        for table in (_lib.SIGNATURES, _lib.FEATURE_GROUP_SIGNATURES, _lib.WORKING_SET_SIGNATURES, _lib.LINK_LOSS_SIGNATURES,
                      _lib.DUALITY_SIGNATURES):
            assert name not in table                                 # a table of its own, merged in load()
    assert lib.fos_abi_version() == 3                               # the ABI only grew
    sig = r"\s*,\s*".join
    fl, db, u8, i32 = r"const\s+float\s*\*\s*", r"const\s+double\s*\*\s*", r"const\s+uint8_t\s*\*\s*", r"int32_t\s*\*\s*"
    assert re.search(r"int\s+fos_multinomial_gradient_batch\s*\(\s*" + sig([fl + "X", r"int\s+nv", r"fos_problem\s*\*\s*p", r"float\s*\*\s*G",
                                                                             r"double\s*\*\s*loss16"]) + r"\s*\)", header)
    assert re.search(r"int\s+fos_multinomial_kkt_scan\s*\(\s*" + sig([fl + "G", r"int\s+nv", r"int\s+grouped", db + "alpha1", r"double\s+slack",
                                                                       u8 + "in_ws", r"fos_problem\s*\*\s*p", r"float\s*\*\s*excess",
                                                                       i32 + "viol_idx", i32 + "viol_count"]) + r"\s*\)", header)
    assert re.search(r"int\s+fos_multinomial_duality_gap\s*\(\s*" + sig([fl + "X", r"int\s+nv", r"int\s+grouped", db + "alpha1", db + "alpha2",
                                                                          r"fos_problem\s*\*\s*p", r"float\s*\*\s*G", r"double\s*\*\s*out64"])
                     + r"\s*\)", header)
    assert os.path.join(ROOT, "include", "fos_multinomial_ws.h") in build.HEADERS
    assert os.path.join(ROOT, "fastoptsolver_amd", "csrc", "multinomial_ws.hpp") in build.HEADERS


def test_no_other_header_declares_them_and_the_closed_lists_did_not_grow():
    from tests import _logit_guard as gd
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.basename(path) != "fos_multinomial_ws.h":
            for name in NEW:
                assert not re.search(r"\b" + name + r"\s*\(", _header(os.path.basename(path))), path
    assert not set(NEW) & gd.header_handle_functions()
    assert gd.header_handle_functions() == gd.SERVES | gd.LOSS_FREE | gd.REFUSES
    assert not any(re.match(r"fos_problem_set_|fos_\w+_bind$", name) for name in NEW)      # they bind nothing to the handle
    from fastoptsolver_amd import _lib
    assert ctypes.sizeof(_lib.FistaParams) == 8 * 8 + 4 * 4         # fos_fista_params keeps its size


@pytest.mark.parametrize("case", ["null_X", "null_p", "null_G", "nv_0", "nv_17", "nv_-1"])
def test_gradient_argument_checks_come_before_any_hip_call(lib, case):
    args = dict(X=D(0), nv=6, p=P, G=D(1), loss16=D(2))
    if case.startswith("null_"):
        args[case[5:]] = None
    else:
        args["nv"] = int(case[3:])
    assert lib.fos_multinomial_gradient_batch(*args.values()) == ARG
    assert NEW[0] in lib.fos_last_error().decode()


@pytest.mark.parametrize("case", ["null_G", "null_alpha1", "null_in_ws", "null_p", "null_excess", "null_viol_idx", "null_viol_count", "nv_0",
                                  "nv_17", "nv_-1", "grouped_2", "grouped_-1", "slack_negative", "slack_nan", "slack_inf"])
def test_scan_argument_checks_come_before_any_hip_call(lib, case):
    a1 = (ctypes.c_double * 8)(*([0.5] * 8))
    args = dict(G=D(0), nv=6, grouped=0, alpha1=a1, slack=0.0, in_ws=D(1), p=P, excess=D(2), viol_idx=D(3), viol_count=D(4))
    if case.startswith("null_"):
        args[case[5:]] = None
    elif case.startswith("slack_"):
        args["slack"] = {"negative": -1e-300, "nan": float("nan"), "inf": float("inf")}[case[6:]]
    else:
        which, value = case.split("_")
        args[which] = int(value)
    assert lib.fos_multinomial_kkt_scan(*args.values()) == ARG
    assert NEW[1] in lib.fos_last_error().decode()


@pytest.mark.parametrize("case", ["null_X", "null_alpha1", "null_alpha2", "null_p", "null_G", "null_out64", "nv_0", "nv_17", "nv_-1",
                                  "grouped_2", "grouped_-1"])
def test_certificate_argument_checks_come_before_any_hip_call(lib, case):
    a1 = (ctypes.c_double * 8)(*([0.5] * 8))
    a2 = (ctypes.c_double * 8)(*([0.0] * 8))
    args = dict(X=D(0), nv=6, grouped=1, alpha1=a1, alpha2=a2, p=P, G=D(1), out64=D(2))
    if case.startswith("null_"):
        args[case[5:]] = None
    else:
        which, value = case.split("_")
        args[which] = int(value)
    assert lib.fos_multinomial_duality_gap(*args.values()) == ARG
    assert NEW[2] in lib.fos_last_error().decode()


A, Y = np.ones((10, 4)), np.arange(10.0) % 3


def test_python_signatures_and_fields():
    import fastoptsolver_amd as fos
    from fastoptsolver_amd import _core, multinomial_ws
    ws = inspect.signature(fos.multinomial_working_set_path).parameters
    assert list(ws) == ["A", "y", "alphas", "classes", "max_iter", "kkt_tol", "max_rounds", "grow", "max_fraction", "L", "t_init_factor",
                        "dtype", "initial", "return_info"]
    assert [ws[k].default for k in list(ws)[3:]] == [None, 500, 1e-4, 20, 2.0, 0.5, None, 1.0, None, None, False]
    assert all(ws[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(ws)[5:])
    cp = inspect.signature(fos.multinomial_certified_path).parameters
    assert list(cp) == ["A", "y", "alphas", "classes", "gap_tol", "max_iter", "max_rounds", "grow", "max_fraction", "L", "t_init_factor",
                        "dtype", "return_info"]
    assert [cp[k].default for k in list(cp)[3:]] == [None, 1e-4, 500, 20, 2.0, 0.5, None, 1.0, None, False]
    assert all(cp[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(cp)[6:])
    assert list(inspect.signature(fos.multinomial_alpha_max).parameters) == ["prob"]
    assert list(inspect.signature(fos.multinomial_kkt_excess).parameters) == ["prob", "X", "alphas"]
    assert list(inspect.signature(fos.multinomial_duality_gap).parameters) == ["prob", "X", "alphas"]
    for name in ("multinomial_gradient_block", "multinomial_kkt_scan", "multinomial_duality_gap_block"):
        assert callable(getattr(_core.Problem, name))
    for name in ("multinomial_alpha_max", "multinomial_kkt_excess", "multinomial_duality_gap", "multinomial_working_set_path",
                 "multinomial_certified_path"):
        assert getattr(fos, name) is getattr(multinomial_ws, name) and name not in fos.__all__
    assert multinomial_ws.DualityGap is fos.DualityGap and multinomial_ws.GapInfo is fos.GapInfo
    assert multinomial_ws.WorkingSetInfo is fos.WorkingSetInfo
    # the names they stand beside keep their signatures
    assert list(inspect.signature(fos.working_set_path).parameters) == ["A", "b", "alphas", "max_iter", "kkt_tol", "max_rounds", "grow",
                                                                         "max_fraction", "L", "t_init_factor", "dtype", "initial", "return_info"]
    assert list(inspect.signature(fos.certified_path).parameters) == ["A", "b", "alphas", "gap_tol", "max_iter", "max_rounds", "grow",
                                                                       "max_fraction", "L", "t_init_factor", "dtype", "return_info"]
    for doc in (fos.working_set.__doc__, fos.duality.__doc__, fos.multinomial.__doc__):
        assert "multinomial_ws" in doc


def _handle(**kw):
    """What the host checks read of a Problem, without a device."""
    from fastoptsolver_amd import _core
    h = _core.Problem.__new__(_core.Problem)
    h.loss, h.grouped, h._coord, h._fgroups, h.n, h.n_dev, h.b, h.classes = "multinomial", False, (None, None, None), None, 4, 4, object(), 3
    for k, v in kw.items():
        setattr(h, k, v)
    h.h = None
    return h


def test_python_refusals_come_before_any_device_work():
    """No GPU here: a call that got past the host checks would raise FosError (or fail on the missing handle), not ValueError."""
    import fastoptsolver_amd as fos
    for kw in (dict(grow=1.0), dict(max_fraction=0.0), dict(max_fraction=1.5), dict(max_rounds=0)):
        with pytest.raises(ValueError):
            fos.multinomial_working_set_path(A, Y, [(0.1, 0.0)], **kw)
        with pytest.raises(ValueError):
            fos.multinomial_certified_path(A, Y, [(0.1, 0.0)], **kw)
    for kw in (dict(gap_tol=-1.0), dict(gap_tol=float("nan"))):
        with pytest.raises(ValueError):
            fos.multinomial_certified_path(A, Y, [(0.1, 0.0)], **kw)
    with pytest.raises(ValueError):
        fos.multinomial_working_set_path(A, Y, [(0.1, 0.0)], kkt_tol=-1.0)
    with pytest.raises(ValueError):
        fos.multinomial_certified_path(A, Y, [])
    with pytest.raises(ValueError, match="labels"):
        fos.multinomial_working_set_path(A, None, [(0.1, 0.0)])
    with pytest.raises(ValueError, match="classes"):
        fos.multinomial_working_set_path(A, Y, [(0.1, 0.0)], classes=17)
    for bad, word in ((_handle(loss="squared"), "working_set_path"), (_handle(loss="logistic"), "certified_path"),
                      (_handle(loss="huber"), "duality_gap"), (_handle(_coord=(None, np.zeros(4), None)), "bounds"),
                      (_handle(_coord=(None, None, np.zeros(4))), "bounds"), (_handle(comm=object()), "sharded"),
                      (_handle(col_sharded=True), "sharded"), (_handle(b=None), "without labels"), (_handle(classes=4), "classes")):
        kw = dict(classes=3) if word == "classes" else {}
        calls = [lambda: fos.multinomial_working_set_path(bad, None, [(0.1, 0.0)], **kw),
                 lambda: fos.multinomial_certified_path(bad, None, [(0.1, 0.0)], **kw)]
        if word != "classes":
            calls += [lambda: fos.multinomial_duality_gap(bad, np.zeros((4, 3)), [(0.1, 0.0)]),
                      lambda: fos.multinomial_kkt_excess(bad, np.zeros((4, 3)), [(0.1, 0.0)]), lambda: fos.multinomial_alpha_max(bad)]
        for call in calls:
            with pytest.raises(ValueError, match=word):
                call()
    with pytest.raises(ValueError, match="alpha1 = 0"):
        fos.multinomial_certified_path(_handle(), None, [(0.1, 0.0), (0.0, 0.5)])
    with pytest.raises(ValueError, match="alpha1 = 0"):
        fos.multinomial_working_set_path(_handle(), None, [(0.0, 0.5)])
    # the names they stand beside still refuse a multinomial handle, in their own words
    for call in (lambda: fos.working_set_path(_handle(), None, [(0.1, 0.0)]), lambda: fos.certified_path(_handle(), None, [(0.1, 0.0)]),
                 lambda: fos.duality_gap(_handle(), np.zeros(4), [(0.1, 0.0)]), lambda: fos.alpha_max(_handle())):
        with pytest.raises(ValueError, match="multinomial"):
            call()


def _source():
    with open(os.path.join(ROOT, "fastoptsolver_amd", "csrc", "multinomial_ws.hpp")) as fh:
        return fh.read()


def test_kernel_source_has_no_atomics_flags_or_waits():
    text = _source()
    for word in ("atomic", "volatile", "while", "__threadfence", "asm"):
        assert not re.search(word, text, flags=re.I), word
    code = re.sub(r"//[^\n]*", "", text)
    assert re.search(r"template\s*<bool WEIGHT>\s*__global__\s+__launch_bounds__\(SL_THREADS\)\s+void\s+dual_softmax_kernel", code)
    assert re.search(r"dual_softmax_kernel\(const float\* __restrict__ z16", code)          # the row pass only reads the panel
    assert re.search(r"__global__\s+__launch_bounds__\(KS_THREADS\)\s+void\s+class_kkt_scan_kernel", code)
    # the class scan is an instantiation of the one scan body of working_set.hpp and the column pass is dual_scale_kernel of
    # duality.hpp: the words above are refused there too, and the grouped decision of the scan is held to the comparison of
    # the squares in that body (tests/test_working_set_abi.py, tests/test_duality_abi.py)
    assert re.search(r"class_kkt_scan_kernel\([^)]*\)\s*\{\s*kkt_scan_body<false>\(G, n, nv, classes, grouped, w,", code)
    assert len(re.findall(r"__global__", code)) == 2


UNIT = """
#include "multinomial_ws.hpp"
// every instantiation the three entry points launch: the row pass x WEIGHT, the class scan, and the column pass of every loss
void* fos_multinomial_ws_kernels[] = {
    (void*)fos::dual_softmax_kernel<false>, (void*)fos::dual_softmax_kernel<true>, (void*)fos::class_kkt_scan_kernel,
    (void*)fos::dual_scale_kernel};
"""


def test_kernels_use_no_scratch_and_have_the_stated_resources(tmp_path):
    from fastoptsolver_amd import build
    src = tmp_path / "mw_unit.hip"
    src.write_text(UNIT)
    cmd = [build.hipcc_path(), *build.FLAGS, "-I", build.CSRC, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "mw_unit.o"),
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
    row = {k: v for k, v in kernels.items() if "dual_softmax_kernel" in k}
    scan = {k: v for k, v in kernels.items() if "class_kkt_scan_kernel" in k}
    col = {k: v for k, v in kernels.items() if "dual_scale_kernel" in k}
    assert len(row) == 2 and len(scan) == 1 and len(col) == 1, sorted(kernels)
    for k, v in {**row, **scan, **col}.items():
        assert not v.get("VGPRs Spill", 0) and not v.get("SGPRs Spill", 0) and not v.get("ScratchSize [bytes/lane]", 0), (k, v)
        assert v["VGPRs"] <= 128, (k, v)                                  # at least four waves per SIMD
    assert all(v["LDS Size [bytes/block]"] == 512 for v in row.values())             # 4 waves x 16 doubles
    assert all(v["LDS Size [bytes/block]"] == 64 for v in scan.values())
    assert all(v["LDS Size [bytes/block]"] == 2048 for v in col.values())            # one double per thread
    # the figures in the kernels' comments are the compiled ones: the class scan's and the row pass's here, the column pass's
    # in duality.hpp (the comment that ends on the LDS trees)
    def stated(header, before=r""):
        with open(os.path.join(build.CSRC, header)) as fh:
            return [int(x) for x in re.findall(before + r"Resources \(gfx950, -O3\): (\d+) VGPRs", fh.read())]
    assert stated("duality.hpp", r"Fixed-order trees through LDS\.  ") == [next(iter(col.values()))["VGPRs"]]
    assert stated("multinomial_ws.hpp") == [next(iter(scan.values()))["VGPRs"], max(v["VGPRs"] for v in row.values())]
    assert len({v["VGPRs"] for v in row.values()}) == 1
    # and they are the ones the library launches
    with open(os.path.join(build.CSRC, "fos_fista.hip")) as fh:
        lib_text = fh.read()
    for name in ("fos::dual_softmax_kernel<true>", "fos::dual_softmax_kernel<false>", "fos::class_kkt_scan_kernel", "fos::dual_scale_kernel",
                 "fos::dual_finish_kernel"):
        assert name in lib_text
