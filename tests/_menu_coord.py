"""Coverage table of the coordinate update cells (a helper: no tests in here), beside tests/_menu_cv.py.

A problem with penalty factors or bounds (fos_coord_bind) takes the two-product lockstep; the two update launch sites of
run_multi_mfma (csrc/fos_fista.hip) then launch the coordinate kernels of csrc/reduce_update.hpp:

table  form                   kernel, chosen by
upd    one-launch-plain       fista_update_multi_coord_kernel with host_beta = 1: same-family plain state machines
upd    one-launch-controlled  the same kernel with host_beta = 0: device-controlled state machines (restarts, ratio stop)
upd    per-handle-plain       fista_update_coord_kernel: plain state machines of different families (a FISTA and a FISTA-delta
                              handle in one fos_fista_run_multi call)

each for fp32 A (y_{k+1} in the YOUT_XP layout) and bf16 A (the three bf16 terms of YOUT_XQ), and for both prox kinds of the
update body (PROX_L1: ridge term in the gradient; PROX_ENET: inside the prox).  tests/test_kernel_menu_coord.py keeps the cells in
step with the source; tests/test_gpu_coord.py runs every case of every cell against the fp64 reference of tests/_coord.py."""
import re

from tests import _menu_cv
from tests._menu_product1 import CSRC, FISTA, _body, _text  # noqa: F401

import os

UPDATE = os.path.join(CSRC, "reduce_update.hpp")
YOUT = {"f32": "YOUT_XP", "bf16": "YOUT_XQ"}
FORMS = ("one-launch-plain", "one-launch-controlled", "per-handle-plain")
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


def source_cells(fista=FISTA, update=UPDATE):
    """The cells the two sources serve: the launch sites of run_multi_mfma, the y layouts and the prox kinds of the COORD form."""
    body = _body(_text(fista), r"static\s+int\s+run_multi_mfma\s*\([^)]*\)\s*(?=\{)")
    forms = set()
    one = re.search(r"if\s*\(\s*controlled\s*\|\|\s*same_family\s*\)\s*\{(.*?)\}\s*else\s*\{(.*?)\n    \}", body, flags=re.S)
    assert one is not None, "the two update launch sites of run_multi_mfma"
    m = re.search(r"if\s*\(\s*coord\s*\)\s*hipLaunchKernelGGL\(\s*fos::fista_update_multi_coord_kernel\b[^;]*?y_mode\s*,\s*"
                  r"controlled\s*\?\s*0\s*:\s*1\s*,\s*cd\s*\)\s*;", one.group(1), flags=re.S)
    if m:
        forms |= {"one-launch-plain", "one-launch-controlled"}
    if re.search(r"if\s*\(\s*coord\s*\)\s*\{\s*hipLaunchKernelGGL\(\s*fos::fista_update_coord_kernel\b[^;]*?y_mode\s*,\s*v\s*,\s*cd\s*\)\s*;",
                 one.group(2), flags=re.S):
        forms.add("per-handle-plain")
    layouts = {d for d, y in YOUT.items() if re.search(r"is_bf16\s*\?\s*fos::YOUT_XQ\s*:\s*fos::YOUT_XP", body)}
    upd = _text(update)
    coord = re.search(r"if constexpr \(COORD\) \{\s*const double pe(.*?)\} else \{", upd, flags=re.S)
    assert coord is not None, "the COORD branch of fista_update_body"
    prox = {k for k in PROX if re.search(r"prm\.prox_kind\s*==\s*" + k, coord.group(1))}
    for kernel in ("fista_update_multi_coord_kernel", "fista_update_coord_kernel"):
        assert re.search(r"void\s+" + kernel + r"\s*\([^)]*CoordData\s+cd\s*\)\s*\{[^}]*fista_update_body<true,\s*true,\s*true>", upd, flags=re.S), kernel
    return {("upd", d, f, k) for d in layouts for f in forms for k in prox}


def check_coverage(fista=FISTA, update=UPDATE):
    have, want = source_cells(fista, update), cells()
    missing = sorted("/".join(c) for c in want - have)
    extra = sorted("/".join(c) for c in have - want)
    assert not missing and not extra, f"cells of tests/_menu_coord.py the source does not serve: {missing}; served and not filed: {extra}"
