"""Where every handle-taking entry point of include/fos.h stands on a multinomial problem (a helper: no tests in here).

SERVES: computes with the multinomial loss (class groups of the 16 columns, the link kernel between the two products).
LOSS_FREE: touches neither b nor a residual and works as before.  REFUSES: forms a residual, gradient or objective with b as a
squared-loss target and returns FOS_ERR_UNSUPPORTED through the one helper need_squared before any launch or change of handle
state.  The rows are those of tests/_logit_guard.py - a multinomial problem stands where a logistic one does - plus the entry
points that take their handle after their data, which that table does not file.  tests/test_multinomial_guard.py keeps the
table complete against the header and checks the bodies; tests/test_gpu_multinomial.py executes it."""
import os
import re

from tests import _logit_guard as lgd

ROOT, CSRC, GUARD, body_of = lgd.ROOT, lgd.CSRC, lgd.GUARD, lgd.body_of

SERVES = set(lgd.SERVES)
LOSS_FREE = set(lgd.LOSS_FREE) | {
    "fos_problem_set_multinomial", "fos_problem_get_classes",
    "fos_row_weights_bind", "fos_row_weights_get", "fos_coord_bind", "fos_coord_get",      # they compose with the loss
    "fos_gram_apply",                                                                     # A^T W A X: neither b nor the loss
}
REFUSES = set(lgd.REFUSES)


def header_handle_functions(path=None):
    """Every function of the header with a fos_problem* or fos_fista* parameter in any position."""
    with open(path or os.path.join(ROOT, "include", "fos.h")) as fh:
        txt = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    out = set()
    for name, args in re.findall(r"\b(fos_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        if re.search(r"\bfos_(problem|fista)\s*\*(?!\s*\*)", args):     # a handle, not the fos_problem** a constructor fills
            out.add(name)
    return out
