"""CPU: the three entry points of include/fos_resample.h are exported, bound and declared with the signatures the header documents,
in a header and a signature table of their own, and refuse bad arguments before any HIP call; pack_counts is the layout of the
header, the generators are seeded and do what they say, selection_frequencies counts; every launched instantiation of
csrc/resample_link.hpp compiles without spills or scratch; the fp64 reference of the stability test meets that test's own
conditions."""
import ctypes
import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import _resample as rsp

NEW = ("fos_fista_run_multi_resampled", "fos_gradient_batch_resampled", "fos_gram_apply_resampled")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
P, D = ctypes.c_void_p(0x1000), lambda k=0: ctypes.c_void_p(0x2000 + 0x100 * k)     # stand-ins: never dereferenced


@pytest.fixture(scope="module")
def lib():
    from fastoptsolver_amd import build, _lib
    build.build()
    return _lib.load()


def _header(name="fos_resample.h"):
    with open(os.path.join(ROOT, "include", name)) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def test_symbols_exported_bound_and_declared(lib):
    from fastoptsolver_amd import _lib, build
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = _header()
    assert tuple(re.findall(r"\b(fos_[a-z0-9_]+)\s*\(", header)) == NEW == tuple(_lib.RESAMPLE_SIGNATURES)
    for name in NEW:
        assert f" T {name}" in out
        assert getattr(lib, name).argtypes == _lib.RESAMPLE_SIGNATURES[name][1] and getattr(lib, name).restype is ctypes.c_int
        for table in (_lib.SIGNATURES, _lib.FEATURE_GROUP_SIGNATURES, _lib.WORKING_SET_SIGNATURES, _lib.LINK_LOSS_SIGNATURES,
                      _lib.DUALITY_SIGNATURES, _lib.MULTINOMIAL_WS_SIGNATURES):
            assert name not in table                                 # a table of its own, merged in load()
    assert lib.fos_abi_version() == 3                               # the ABI only grew
    assert ctypes.sizeof(_lib.FistaParams) == 8 * 8 + 4 * 4         # fos_fista_params keeps its size
    sig = r"\s*,\s*".join
    counts = r"const\s+uint64_t\s*\*\s*counts"
    assert re.search(r"int\s+fos_fista_run_multi_resampled\s*\(\s*" + sig([r"fos_fista\s*\*\s*const\s*\*\s*fs", r"int\s+nv", r"int\s+iters", counts]) +
                     r"\s*\)", header)
    assert re.search(r"int\s+fos_gradient_batch_resampled\s*\(\s*" + sig([r"const\s+float\s*\*\s*X", r"int\s+nv", counts, r"int\s+oob",
                                                                           r"fos_problem\s*\*\s*p", r"float\s*\*\s*G", r"double\s*\*\s*loss16"]) +
                     r"\s*\)", header)
    assert re.search(r"int\s+fos_gram_apply_resampled\s*\(\s*" + sig([r"const\s+float\s*\*\s*X", r"int\s+nv", counts, r"fos_problem\s*\*\s*p",
                                                                       r"float\s*\*\s*G"]) + r"\s*\)", header)
    assert os.path.join(ROOT, "include", "fos_resample.h") in build.HEADERS
    assert os.path.join(ROOT, "fastoptsolver_amd", "csrc", "resample_link.hpp") in build.HEADERS


def test_no_other_header_declares_them_and_the_closed_lists_did_not_grow():
    from tests import _logit_guard as gd
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.basename(path) != "fos_resample.h":
            for name in NEW:
                assert not re.search(r"\b" + name + r"\s*\(", _header(os.path.basename(path))), (path, name)
    assert not set(NEW) & gd.header_handle_functions()
    assert gd.header_handle_functions() == gd.SERVES | gd.LOSS_FREE | gd.REFUSES
    for name in NEW:
        assert not re.match(r"fos_problem_set_|fos_\w+_bind$", name)     # nothing is bound to the handle


RUN_CASES = ["null_fs", "null_counts", "nv_0", "nv_17", "nv_-1", "iters_-1", "counts_misaligned"]
GRAD_CASES = ["null_X", "null_counts", "null_p", "null_G", "null_loss16_oob", "nv_0", "nv_17", "counts_misaligned", "oob_2", "oob_-1"]
GRAM_CASES = ["null_X", "null_counts", "null_p", "null_G", "nv_0", "nv_17", "counts_misaligned"]


def _apply(args, case):
    if case == "null_loss16_oob":
        args["oob"], args["loss16"] = 1, None
    elif case.startswith("null_"):
        args[case[5:]] = None
    elif case == "counts_misaligned":
        args["counts"] = ctypes.c_void_p(0x3004)
    else:
        key, val = case.rsplit("_", 1)
        args[key] = int(val)
    return args


@pytest.mark.parametrize("case", RUN_CASES)
def test_run_argument_checks_come_before_any_hip_call(lib, case):
    fs = (ctypes.c_void_p * 2)(0x1000, 0x1000)
    args = _apply(dict(fs=fs, nv=2, iters=3, counts=ctypes.c_void_p(0x3000)), case)
    assert lib.fos_fista_run_multi_resampled(*args.values()) == ARG
    assert NEW[0] in lib.fos_last_error().decode()


@pytest.mark.parametrize("case", GRAD_CASES)
def test_gradient_argument_checks_come_before_any_hip_call(lib, case):
    args = _apply(dict(X=D(0), nv=3, counts=ctypes.c_void_p(0x3000), oob=0, p=P, G=D(1), loss16=D(2)), case)
    assert lib.fos_gradient_batch_resampled(*args.values()) == ARG
    assert NEW[1] in lib.fos_last_error().decode()


@pytest.mark.parametrize("case", GRAM_CASES)
def test_gram_argument_checks_come_before_any_hip_call(lib, case):
    args = _apply(dict(X=D(0), nv=3, counts=ctypes.c_void_p(0x3000), p=P, G=D(1)), case)
    assert lib.fos_gram_apply_resampled(*args.values()) == ARG
    assert NEW[2] in lib.fos_last_error().decode()


def test_a_null_handle_in_the_list_is_an_argument_error(lib):
    fs = (ctypes.c_void_p * 2)(0, 0)
    assert lib.fos_fista_run_multi_resampled(fs, 2, 1, ctypes.c_void_p(0x3000)) == ARG


# ---- the host layer -------------------------------------------------------------------------------------------------------------
def test_python_names_and_signatures():
    import fastoptsolver_amd as fos
    from fastoptsolver_amd import resample
    for name in ("pack_counts", "bootstrap_counts", "subsample_counts", "resampled_lipschitz", "resampled_path", "stability_selection",
                 "selection_frequencies", "ResampleResult", "StabilityResult"):
        assert getattr(fos, name) is getattr(resample, name) and name not in fos.__all__
    assert fos.ResampleResult._fields == ("alphas", "coefs", "oob_loss", "oob_size", "L", "info")
    assert fos.StabilityResult._fields == ("alphas", "frequency", "max_frequency", "selected")
    rp = inspect.signature(fos.resampled_path).parameters
    assert list(rp)[:4] == ["handle", "alphas", "counts", "max_iter"] and rp["max_iter"].default == 500
    named = ["L", "t_init_factor", "delta", "tol_ratio", "adaptive_restart", "restart_threshold", "oob"]
    assert list(rp)[4:11] == named and [rp[k].default for k in named] == [None, 1.0, None, 0.0, False, 1.0, False]
    assert all(rp[k].kind is inspect.Parameter.KEYWORD_ONLY for k in named)
    sp = inspect.signature(fos.subsample_counts).parameters
    assert list(sp) == ["m", "n_sub", "fraction", "seed", "complementary"] and [sp[k].default for k in list(sp)[2:]] == [0.5, 0, True]
    st = inspect.signature(fos.stability_selection).parameters
    assert list(st)[:6] == ["handle", "alphas", "n_pairs", "fraction", "threshold", "seed"]
    assert [st[k].default for k in list(st)[2:6]] == [50, 0.5, 0.6, 0] and st["path_args"].kind is inspect.Parameter.VAR_KEYWORD
    lp = inspect.signature(fos.resampled_lipschitz).parameters
    assert list(lp) == ["handle", "counts", "n_iter", "tol"] and (lp["n_iter"].default, lp["tol"].default) == (100, 1e-6)
    for bad in ("tol", "comm", "cols"):                                  # before any device work: no handle is looked at
        with pytest.raises(ValueError, match="gradient-norm"):
            fos.resampled_path(object(), [(0.1, 0.0)], np.ones((3, 1), dtype=np.int64), **{bad: 1})
    with pytest.raises(TypeError):
        fos.resampled_path(object(), [(0.1, 0.0)], np.ones((3, 1), dtype=np.int64), backtracking=True)
    with pytest.raises(ValueError, match="handle"):
        fos.resampled_path(np.ones((3, 2)), [(0.1, 0.0)], np.ones((3, 1), dtype=np.int64))


@pytest.mark.parametrize("nv", [1, 5, 16])
def test_pack_counts_is_the_layout_of_the_header(nv):
    from fastoptsolver_amd import resample
    rng = np.random.default_rng(nv)
    c = rng.integers(0, 16, size=(203, nv))
    c[0], c[1] = 15, 0
    want = rsp.pack_np(c)
    for given in (c, c.astype(np.uint8), torch.from_numpy(c), torch.from_numpy(c).to(torch.int32)):
        got = resample.pack_counts(given)
        assert got.dtype == torch.int64 and got.shape == (203,) and got.is_contiguous()
        assert np.array_equal(got.numpy().view(np.uint64), want)
    assert int(want[0]) == (1 << (4 * nv)) - 1 and int(want[1]) == 0
    # a lane reads its quad's four nibbles as the 16-bit element 4 i + q of the same buffer
    quads = want.view(np.uint16).reshape(203, 4)
    for q in range(4):
        for k in range(4):
            col = 4 * q + k
            assert np.array_equal((quads[:, q] >> (4 * k)) & 15, c[:, col] if col < nv else np.zeros(203, dtype=c.dtype))


def test_pack_counts_refuses_what_has_no_encoding():
    from fastoptsolver_amd import resample
    ok = np.ones((9, 3), dtype=np.int64)
    for bad in (16, -1):
        c = ok.copy()
        c[4, 1] = bad
        with pytest.raises(ValueError, match="0..15"):
            resample.pack_counts(c)
        with pytest.raises(ValueError, match="0..15"):
            resample.pack_counts(torch.from_numpy(c))
    with pytest.raises(ValueError, match="columns"):
        resample.pack_counts(np.ones((9, 17), dtype=np.int64))
    for shape in ((9,), (9, 3, 1)):
        with pytest.raises(ValueError, match="m x nv"):
            resample.pack_counts(np.ones(shape, dtype=np.int64))
    with pytest.raises(ValueError, match="integers"):
        resample.pack_counts(np.ones((9, 3)))


def test_the_generators_are_seeded_and_do_what_they_say():
    from fastoptsolver_amd import resample
    m = 1003
    boot = resample.bootstrap_counts(m, 7, 5)
    assert boot.shape == (m, 7) and boot.dtype == np.int64 and (boot.sum(axis=0) == m).all() and boot.min() == 0 and 2 <= boot.max() <= 15
    assert np.array_equal(boot, resample.bootstrap_counts(m, 7, 5)) and not np.array_equal(boot, resample.bootstrap_counts(m, 7, 6))
    assert len({boot[:, j].tobytes() for j in range(7)}) == 7
    for fraction in (0.5, 0.3):
        sub = resample.subsample_counts(m, 7, fraction, seed=2)
        k = int(np.floor(fraction * m))
        assert sub.shape == (m, 7) and set(np.unique(sub)) == {0, 1} and (sub.sum(axis=0) == k).all()
        assert np.array_equal(sub, resample.subsample_counts(m, 7, fraction, seed=2))
        assert not np.array_equal(sub, resample.subsample_counts(m, 7, fraction, seed=3))
        for p in range(3):                                                 # complementary pairs are disjoint; the seventh stands alone
            assert int((sub[:, 2 * p] * sub[:, 2 * p + 1]).sum()) == 0
    own = resample.subsample_counts(m, 6, 0.5, seed=2, complementary=False)
    assert (own.sum(axis=0) == m // 2).all() and any(int((own[:, 2 * p] * own[:, 2 * p + 1]).sum()) > 0 for p in range(3))
    assert (resample.subsample_counts(m, 2, 0.7, seed=0, complementary=False).sum(axis=0) == int(np.floor(0.7 * m))).all()
    with pytest.raises(ValueError, match="complementary"):
        resample.subsample_counts(m, 2, 0.7)


def test_selection_frequencies_on_a_hand_made_block():
    from fastoptsolver_amd import resample
    coefs = np.zeros((3, 4, 2))                                            # n = 3, B = 4, L = 2
    coefs[0, :, 0] = [1.0, -2.0, 0.0, 1e-30]                               # three of four (a tiny value is a selection)
    coefs[1, :, 1] = [0.5, 0.5, 0.5, 0.5]
    coefs[2, 1, 0] = -0.0                                                  # a signed zero is none
    want = np.array([[0.75, 0.0, 0.0], [0.0, 1.0, 0.0]])
    assert np.array_equal(resample.selection_frequencies(coefs), want)
    assert np.array_equal(resample.selection_frequencies(torch.from_numpy(coefs)), want)
    with pytest.raises(ValueError):
        resample.selection_frequencies(np.zeros((3, 4)))


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
LOSS_NAMES = ("RESAMPLE_SQUARED", "RESAMPLE_LOGISTIC", "RESAMPLE_HUBER", "RESAMPLE_SQUARED_HINGE")
FORMS = [("RESAMPLE_GRAM", "RESAMPLE_INBAG", w) for w in ("false", "true")] + \
        [(k, mode, w) for k in LOSS_NAMES for mode in ("RESAMPLE_INBAG", "RESAMPLE_OOB") for w in ("false", "true")]
UNIT = '#include "resample_link.hpp"\n// every instantiation launch_resample_link launches\nvoid* fos_resample_link_kernels[] = {\n' + \
    "".join(f"  (void*)fos::resample_link_kernel<fos::{k}, fos::{mode}, {w}>,\n" for k, mode, w in FORMS) + "};\n"


def _source():
    with open(os.path.join(ROOT, "fastoptsolver_amd", "csrc", "resample_link.hpp")) as fh:
        return fh.read()


def test_the_link_kernel_has_no_waits_flags_or_atomics_and_one_launcher():
    code = re.sub(r"//[^\n]*", "", _source())
    for word in ("atomic", "__threadfence", "while", "volatile", "cooperative", "s_sleep", "asm"):
        assert word not in code, word
    assert code.count("__syncthreads()") == 1
    assert re.search(r"template\s*<int LOSS,\s*int MODE,\s*bool WEIGHT>\s*__global__\s+__launch_bounds__\(RL_THREADS\)\s+void\s+resample_link_kernel", code)
    assert re.search(r"constexpr\s+int\s+RL_THREADS\s*=\s*256\s*;", code) and re.search(r"stride\s*=\s*\(int64_t\)gridDim\.x\s*\*\s*RL_THREADS", code)
    assert "pointwise_terms<LINK_HUBER>" in code and "pointwise_terms<LINK_SQUARED_HINGE>" in code and "logistic_terms(" in code
    from tests._menu_product1 import FISTA, PLAN, _body, _text
    text = _text(FISTA)
    launcher = _body(text, r"static\s+int\s+launch_resample_link\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"std::min<int64_t>\(\(4 \* rows \+ fos::RL_THREADS - 1\) / fos::RL_THREADS, 2 \* \(int64_t\)p->ncu\)", launcher)
    assert set(re.findall(r"FOS_RESAMPLE_FORM\((RESAMPLE_\w+)\)", launcher)) == set(LOSS_NAMES)
    assert text.count("resample_link_kernel") == 1 and "resample_link_kernel" not in _text(PLAN)
    # the lockstep puts it between the two products, and the entry point refuses before the route is asked
    mfma = _body(text, r"static\s+int\s+run_multi_mfma\s*\([^)]*\)\s*(?=\{)")
    assert mfma.index("launch_batch_product") < mfma.index("launch_resample_link") < mfma.index("launch_gram_panel")
    entry = _body(text, r"int\s+fos_fista_run_multi_resampled\s*\([^)]*\)\s*(?=\{)")
    assert entry.index("FOS_ERR_ARG") < entry.index("resample_refusal(") < entry.index("run_lockstep(")
    assert not re.search(r"hipLaunchKernelGGL|hipMalloc|hipMemcpy|hipMemset|reserve\(|->\w+\s*=[^=]|invalidate\(", entry)


def test_resample_link_kernels_do_not_spill(tmp_path):
    from fastoptsolver_amd import build
    src = tmp_path / "resample_unit.hip"
    src.write_text(UNIT)
    cmd = [build.hipcc_path(), *build.FLAGS, "-I", build.CSRC, "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
           str(tmp_path / "resample_unit.o"), str(src)]
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
    link = {k: v for k, v in kernels.items() if "resample_link_kernel" in k}
    assert len(link) == len(FORMS) == 18, sorted(kernels)
    for k, v in link.items():
        print(k, v)
        assert not v.get("VGPRs Spill", 0) and not v.get("SGPRs Spill", 0) and not v.get("ScratchSize [bytes/lane]", 0), (k, v)
        assert v["VGPRs"] <= 64, (k, v)                           # eight waves per SIMD, as the pointwise link: latency is hidden by occupancy
        assert v["LDS Size [bytes/block]"] in (0, 16 * 16 * 8), (k, v)     # one fp64 per (16-lane row, column); the Gram form has no sums
    assert sum(v["LDS Size [bytes/block]"] == 0 for v in link.values()) == 2


# ---- the stability test's condition, on the reference alone -------------------------------------------------------------------------
def test_the_reference_meets_the_conditions_of_the_stability_test():
    from fastoptsolver_amd import resample
    d = rsp.stability_case()
    nonzero, near = rsp.stability_reference()
    B, La, n = nonzero.shape
    assert (B, La, n) == (2 * rsp.ST_PAIRS, len(rsp.ST_FRACTIONS), rsp.ST_SHAPE[1]) and len(d["support"]) == rsp.ST_SUPPORT
    assert (d["counts"].sum(axis=0) == rsp.ST_SHAPE[0] // 2).all()
    print(f"near the threshold: {int(near.sum())} of {near.size} cells")
    assert near.mean() <= rsp.ST_LEFT_OUT
    freq = nonzero.mean(axis=0)
    assert np.array_equal(freq, resample.selection_frequencies(np.transpose(nonzero, (2, 0, 1)).astype(np.float64)))
    top = freq.max(axis=0)
    assert set(d["support"]) <= set(np.flatnonzero(top >= 0.6))
    off = np.setdiff1d(np.arange(n), d["support"])
    assert ((freq[-1, off] > 0) & (freq[-1, off] < 1)).any()
