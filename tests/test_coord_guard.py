"""CPU: a problem with coordinate data (fos_coord_bind) is refused by the ONE guard helper - need_squared reaches the coordinate
refusal after its two own branches - and the refusing entry points know nothing of the new fields, as they know nothing of the
row weights; the serving dispatchers send such a problem to the two-product lockstep."""
import os
import re

from tests import _logit_guard as gd
from tests._menu_product1 import FISTA, PLAN, _body, _text


def _definitions(name):
    defs = []
    for unit in os.listdir(gd.CSRC):
        if unit.endswith((".hip", ".hpp")):
            with open(os.path.join(gd.CSRC, unit)) as fh:
                defs += re.findall(r"^(?:inline\s+)?(?:int|bool)\s+" + name + r"\s*\([^;{]*\)\s*\{", fh.read(), flags=re.M)
    return defs


def test_there_is_still_one_guard_and_it_reaches_the_coordinate_refusal():
    assert len(_definitions(gd.GUARD)) == 1 and len(_definitions("coord_refusal")) == 1 and len(_definitions("has_coord")) == 1
    body = _body(_text(PLAN), r"int\s+" + gd.GUARD + r"\s*\([^)]*\)\s*(?=\{)")
    # after the two branches of its own, so that their messages keep precedence
    order = [body.index("p->row_weight"), body.index("p->loss"), body.index("coord_refusal(p, fn)")]
    assert order == sorted(order)
    assert re.search(r"return\s+coord_refusal\s*\(\s*p\s*,\s*fn\s*\)\s*;\s*$", body.strip())
    refusal = _body(_text(PLAN), r"int\s+coord_refusal\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"p\s*&&\s*has_coord\s*\(\s*p\s*\)", refusal) and len(re.findall(r"FOS_ERR_UNSUPPORTED", refusal)) == 1
    assert "fos_coord_bind" in refusal and "std::string(fn)" in refusal            # a message of its own, naming the caller
    assert "hipLaunchKernelGGL" not in refusal and not re.search(r"->\w+\s*=[^=]", refusal)      # nothing launched or assigned


def test_no_refusing_body_names_the_new_fields():
    for name in sorted(gd.REFUSES):
        body = gd.body_of(name)
        assert body is not None, name
        for word in ("coord_factor", "coord_lo", "coord_hi", "has_coord", "CoordData"):
            assert word not in body, (name, word)


def test_the_serving_dispatchers_send_coordinate_data_to_the_two_product_lockstep():
    text = _text(FISTA)
    # one branch of the one route decision serves both entry points: the matrix-core pair (the route's default engine), for
    # any nv - the single run, the VALU pass and the cluster form are decided behind it, for the plain squared loss alone
    route = _body(text, r"static\s+int\s+lockstep_route\s*\([^)]*\)\s*(?=\{)")
    m = re.search(r"if\s*\(\s*p->loss\s*==\s*FOS_LOSS_LOGISTIC\s*\|\|\s*p->row_weight\s*\|\|\s*has_coord\(p\)\s*\|\|\s*has_fgroups\(p\)\s*\)\s*\{", route)
    assert m and re.search(r"\*r\s*=\s*LockstepRoute\{ENGINE_MFMA,", route[:m.start()])
    branch = _body(route[m.start():], r"has_fgroups\(p\)\s*\)\s*(?=\{)")
    assert re.search(r"return\s+control_refusal\(\)\s*;\s*$", branch.strip()) and "engine" not in branch
    assert "ENGINE_SINGLE" not in route[:m.start()] and "ENGINE_VALU" not in route[:m.start()] and "launch_cluster_pass" not in route
    for name in ("fos_fista_run_multi", "fos_fista_run_multi_folds"):
        assert re.search(r"return\s+run_lockstep\(LockstepCall\{", gd.body_of(name)), name
    mfma = _body(text, r"static\s+int\s+run_multi_mfma\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"const\s+bool\s+two_products\s*=\s*b16\s*\|\|\s*fold_of_row\s*\|\|\s*logit\s*\|\|\s*weighted\s*\|\|\s*has_coord\(p\)\s*\|\|", mfma)
    # fos_residual_batch keeps its rule: use_b = 1 is served (the data term does not depend on the coordinate data)
    rb = gd.body_of("fos_residual_batch")
    assert re.search(r"if\s*\(\s*!use_b\s*\)[^;]*" + gd.GUARD, rb, flags=re.S) and "has_coord" not in rb
    # binding: argument checks first, then the refusals of fos_row_weights_bind, nothing invalidated
    bind = gd.body_of("fos_coord_bind")
    assert bind.index("FOS_ERR_ARG") < bind.index("FOS_ERR_UNSUPPORTED") and "invalidate(" not in bind and "hip" not in bind
    for cond in (r"!p->b", r"p->comm\s*\|\|\s*p->col_sharded", r"!pair_dd_multi_supported\(p\)"):
        assert re.search(cond, bind), cond
