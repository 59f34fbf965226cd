"""CPU: the guard table of the logistic loss (tests/_logit_guard.py) files every handle-taking entry point of include/fos.h,
and every entry point it files under "refuses" calls the one guard helper in its body, before anything else of substance."""
import re

from tests import _logit_guard as gd


def test_table_is_complete_against_the_header():
    header = gd.header_handle_functions()
    filed = gd.SERVES | gd.LOSS_FREE | gd.REFUSES
    assert len(header) > 50, len(header)
    assert header - filed == set(), "entry points without a row in tests/_logit_guard.py"
    assert filed - header == set(), "rows without an entry point in include/fos.h"
    assert not (gd.SERVES & gd.LOSS_FREE or gd.SERVES & gd.REFUSES or gd.LOSS_FREE & gd.REFUSES)


def test_every_refusing_entry_point_calls_the_one_guard():
    for name in sorted(gd.REFUSES):
        body = gd.body_of(name)
        assert body is not None, name
        m = re.search(gd.GUARD + r"\s*\(", body)
        assert m, f"{name} does not call {gd.GUARD}"
        # nothing is launched, allocated or assigned through the handle in front of the guard
        before = body[:m.start()]
        assert not re.search(r"hipLaunchKernelGGL|hipMalloc|hipMemcpy|hipMemset|reserve\(|->\w+\s*=[^=]|invalidate\(", before), name
        assert "FOS_ERR_UNSUPPORTED" not in before, name


def test_serving_and_loss_free_entry_points_do_not_refuse_wholesale():
    """The guard sits only where the table says: fos_residual_batch carries it for use_b = 0 alone."""
    for name in sorted(gd.SERVES | gd.LOSS_FREE):
        body = gd.body_of(name)
        assert body is not None, name
        if name == "fos_residual_batch":
            assert re.search(r"if\s*\(\s*!use_b\s*\)[^;]*" + gd.GUARD, body, flags=re.S)
        else:
            assert gd.GUARD not in body, name


def test_there_is_one_helper():
    import os
    defs = []
    for unit in os.listdir(gd.CSRC):
        if unit.endswith((".hip", ".hpp")):
            with open(os.path.join(gd.CSRC, unit)) as fh:
                defs += re.findall(r"^int\s+" + gd.GUARD + r"\s*\([^;{]*\)\s*\{", fh.read(), flags=re.M)
    assert len(defs) == 1, defs
