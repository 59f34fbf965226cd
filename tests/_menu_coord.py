"""Coverage table of the coordinate update cells (a helper: no tests in here), beside tests/_menu_cv.py.

A problem with penalty factors or bounds (fos_coord_bind) takes the two-product lockstep; the one separable update launch of
run_multi_mfma (launch_separable_update, csrc/fos_fista.hip) then launches fista_update_multi_kernel<true>, the coordinate form
of csrc/reduce_update.hpp:

table  form                   chosen by
upd    one-launch-plain       host_beta = 1: same-family plain state machines
upd    one-launch-controlled  host_beta = 0: device-controlled state machines (restarts, ratio stop)
upd    mixed-families-plain   host_beta = 1 and the prox kind per column (MultiUpdate::prox_bits): plain state machines of
                              different families (a FISTA and two FISTA-delta handles in one fos_fista_run_multi call)

each for fp32 A (y_{k+1} in the YOUT_XP layout) and bf16 A (the three bf16 terms of YOUT_XQ), and for both prox kinds of the
update body (PROX_L1: ridge term in the gradient; PROX_ENET: inside the prox).  tests/test_kernel_menu_coord.py keeps the cells in
step with the source; tests/test_gpu_coord.py runs every case of every cell against the fp64 reference of tests/_coord.py."""
import re

from tests import _menu_cv
from tests._menu_product1 import CSRC, FISTA, _body, _text  # noqa: F401

import os

UPDATE = os.path.join(CSRC, "reduce_update.hpp")
YOUT = {"f32": "YOUT_XP", "bf16": "YOUT_XQ"}
FORMS = ("one-launch-plain", "one-launch-controlled", "mixed-families-plain")
PROX = ("PROX_L1", "PROX_ENET")


def shapes(dtype, cus):
    """(m, n) by name: the cases of tests/_menu_cv.shapes (one_tile: 68 fp32 / 72 bf16 columns, the last 64-column update
    workgroup owns a single quad (two for bf16); edges: 200 columns, a partial last workgroup; rb2 and panels: the 128-row tile
    and a second row panel in front of the update) and a width of whole update workgroups."""
    out = {k: dict(m=c["m"], n=c["n"]) for k, c in _menu_cv.shapes(dtype, cus).items()}
    out["whole_wgs"] = dict(m=515, n=256)
    return out


def cells():
    return {("upd", dtype, form, prox) for dtype in YOUT for form in FORMS for prox in PROX}


UPDATE_STAGE = (r"if\s*\(fgroup\)\s*rc\s*=\s*launch_fgroup_update\([^;]*\);\s*else\s+if\s*\(group_penalty\)\s*rc\s*=\s*launch_group_update\([^;]*\);\s*"
                r"else\s+rc\s*=\s*launch_separable_update\(fs,\s*nv,\s*g_splits,\s*y_mode,\s*controlled\)\s*;")


def source_cells(fista=FISTA, update=UPDATE):
    """The cells the two sources serve: the one separable launch site behind run_multi_mfma, the y layouts and the prox kinds of
    the COORD form."""
    text, upd = _text(fista), _text(update)
    body = _body(text, r"static\s+int\s+run_multi_mfma\s*\([^)]*\)\s*(?=\{)")
    assert re.search(UPDATE_STAGE, body), "the update stage of run_multi_mfma: feature groups, group penalty, else the separable launch"
    launcher = _body(text, r"static\s+int\s+launch_separable_update\s*\([^)]*\)\s*(?=\{)")
    builder = _body(text, r"static\s+fos::MultiUpdate\s+multi_update\s*\([^)]*\)\s*(?=\{)")
    kern = re.search(r"template\s*<bool COORD>\s*__global__[^{;]*void\s+fista_update_multi_kernel\s*\(([^)]*)\)\s*\{(.*?)\n\}", upd, flags=re.S)
    assert kern is not None and re.search(r"CoordData\s+cd\s*$", kern.group(1)) and "FistaParams" not in kern.group(1), "the one-launch kernel"
    assert re.search(r"fista_update_body<true,\s*true,\s*COORD>\([^;]*,\s*cd\)\s*;", kern.group(2), flags=re.S)
    for gone in ("fista_update_multi_coord_kernel", "fista_update_coord_kernel"):
        assert gone not in upd and gone not in text, gone
    forms = set()
    if re.search(r"has_coord\(p\)\s*\?\s*fos::fista_update_multi_kernel<true>\s*:\s*fos::fista_update_multi_kernel<false>\s*;", launcher) and \
            re.search(r"hipLaunchKernelGGL\(\s*kern\s*,\s*dim3\(fs\[0\]->nupd,\s*nv\)[^;]*?y_mode\s*,\s*controlled\s*\?\s*0\s*:\s*1\s*,\s*cd\s*\)\s*;",
                      launcher, flags=re.S):
        forms |= {"one-launch-plain", "one-launch-controlled"}
        # mixed families ride the same launch: the builder files every handle's prox kind, the kernel reads its column's, and no
        # family test stands between a call and the launch
        if re.search(r"mu\.prox_bits\s*\|=\s*\(f->prm\.prox_kind\s*==\s*fos::PROX_ENET\s*\?\s*1\s*:\s*0\)\s*<<\s*v\s*;", builder) and \
                re.search(r"prm\.prox_kind\s*=\s*\(mu\.prox_bits\s*>>\s*v\)\s*&\s*1\s*;", kern.group(2)) and "same_family" not in launcher:
            forms.add("mixed-families-plain")
    layouts = {d for d, y in YOUT.items() if re.search(r"is_bf16\s*\?\s*fos::YOUT_XQ\s*:\s*fos::YOUT_XP", body)}
    coord = re.search(r"if constexpr \(COORD\) \{\s*const double pe(.*?)\} else \{", upd, flags=re.S)
    assert coord is not None, "the COORD branch of fista_update_body"
    prox = {k for k in PROX if re.search(r"prm\.prox_kind\s*==\s*" + k, coord.group(1))}
    return {("upd", d, f, k) for d in layouts for f in forms for k in prox}


def check_coverage(fista=FISTA, update=UPDATE):
    have, want = source_cells(fista, update), cells()
    missing = sorted("/".join(c) for c in want - have)
    extra = sorted("/".join(c) for c in have - want)
    assert not missing and not extra, f"cells of tests/_menu_coord.py the source does not serve: {missing}; served and not filed: {extra}"
