"""CPU: the guard table of the multinomial loss (tests/_multinomial_guard.py) files every entry point of include/fos.h that takes
a handle in any position, the refusing ones call the one guard helper first, the guard names the loss it refuses, and the
dispatchers send a multinomial problem to the link-kernel route before any other."""
import re

from tests import _multinomial_guard as gd
from tests._menu_product1 import FISTA, PLAN, _body, _text


def test_table_is_complete_against_the_header():
    header = gd.header_handle_functions()
    filed = gd.SERVES | gd.LOSS_FREE | gd.REFUSES
    assert len(header) > 55, len(header)
    assert header - filed == set(), "entry points without a row in tests/_multinomial_guard.py"
    assert filed - header == set(), "rows without an entry point in include/fos.h"
    assert not (gd.SERVES & gd.LOSS_FREE or gd.SERVES & gd.REFUSES or gd.LOSS_FREE & gd.REFUSES)
    assert {"fos_problem_set_multinomial", "fos_problem_get_classes"} <= header


def test_every_refusing_entry_point_calls_the_one_guard_first():
    for name in sorted(gd.REFUSES):
        body = gd.body_of(name)
        m = re.search(gd.GUARD + r"\s*\(", body)
        assert m, name
        before = body[:m.start()]
        assert not re.search(r"hipLaunchKernelGGL|hipMalloc|hipMemcpy|hipMemset|reserve\(|->\w+\s*=[^=]|invalidate\(", before), name
        for word in ("MULTINOMIAL", "classes", "softmax"):          # the refusing bodies know nothing of the new loss
            assert word not in body, (name, word)


def test_the_guard_names_the_loss_it_refuses():
    body = _body(_text(PLAN), r"int\s+" + gd.GUARD + r"\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"p->loss\s*!=\s*FOS_LOSS_SQUARED", body)
    assert re.search(r"p->loss\s*==\s*FOS_LOSS_MULTINOMIAL\s*\?", body) and "multinomial problem" in body and "logistic problem" in body


def test_the_dispatchers_take_the_link_kernel_route_first():
    text = _text(FISTA)
    # both entry points go through the one route decision, whose multinomial branch comes before every other
    for name in ("fos_fista_run_multi", "fos_fista_run_multi_folds"):
        assert re.search(r"return\s+run_lockstep\(LockstepCall\{", gd.body_of(name)), name
    decide = _body(text, r"static\s+int\s+lockstep_route\s*\([^)]*\)\s*(?=\{)")
    soft = decide.index("if (p->loss == FOS_LOSS_MULTINOMIAL) {")
    assert soft < decide.index("any_grouped(fs, nv)") < decide.index("p->loss == FOS_LOSS_LOGISTIC") < decide.index("if (c.fold_of_row)")
    shared = _body(decide, r"control_refusal\s*=\s*\[&\]\(\)\s*(?=\{)")          # (defined ahead of the branches, called inside them)
    assert "FOS_ERR_UNSUPPORTED" not in decide[:soft].replace(shared, "")
    route = _body(decide, r"if\s*\(p->loss\s*==\s*FOS_LOSS_MULTINOMIAL\)\s*(?=\{)")
    # every refusal of the branch is FOS_ERR_UNSUPPORTED (four of its own, the shared control refusal, the group refusal) and
    # the branch ends by accepting; nothing in the whole decision launches or assigns to a handle or the problem
    assert "FOS_ERR_ARG" not in decide and len(re.findall(r"FOS_ERR_UNSUPPORTED", route)) == 4
    assert "control_refusal()" in route and "group_refusal(" in route and re.search(r"return\s+FOS_OK\s*;\s*$", route.strip())
    assert route.rindex("FOS_ERR_UNSUPPORTED") < route.rindex("return FOS_OK")
    assert "hipLaunchKernelGGL" not in decide and "run_multi_mfma" not in decide and not re.search(r"[^r]->\w+\s*=[^=]", decide)
    mfma = _body(text, r"static\s+int\s+run_multi_mfma\s*\([^)]*\)\s*(?=\{)")
    # product 1 gets neither b nor the mask nor the weights, and the link kernel sits before product 2 of the panel
    assert re.search(r"if\s*\(softmax\)\s*\{\s*L\.b\s*=\s*nullptr;\s*L\.use_b\s*=\s*0;\s*L\.fold_of_row\s*=\s*nullptr;\s*L\.held\s*=\s*nullptr;\s*"
                     r"L\.row_weight\s*=\s*nullptr;\s*\}", mfma)
    assert mfma.index("launch_batch_product") < mfma.index("launch_softmax_link") < mfma.index("launch_gram_panel")
    assert re.search(r"use_cluster\s*=\s*p->multi\.cp_cs\s*&&\s*!two_products\s*&&\s*!softmax", mfma)
    # fos_residual_batch hands the route no mask (FOLD_OFF), fos_residual_batch_folds its ids and held block (FOLD_HELD)
    assert re.search(r"residual_batch_softmax\(p,\s*\"fos_residual_batch\",\s*X,\s*nv,\s*out16,\s*nullptr,\s*nullptr\)", gd.body_of("fos_residual_batch"))
    assert re.search(r"residual_batch_softmax\(p,\s*\"fos_residual_batch_folds\",\s*X,\s*nv,\s*out16,\s*fold_of_row,\s*&hb\)",
                     gd.body_of("fos_residual_batch_folds"))
    rb = _body(_text(PLAN), r"static\s+int\s+residual_batch_softmax\s*\([^)]*\)\s*(?=\{)")
    assert rb.index("launch_batch_product") < rb.index("launch_softmax_link") and re.search(r"held\s*\?\s*fos::FOLD_HELD\s*:\s*fos::FOLD_OFF", rb)


def test_the_link_kernel_has_no_waits_flags_or_atomics():
    with open(gd.CSRC + "/softmax_link.hpp") as fh:
        code = re.sub(r"//[^\n]*", "", fh.read())
    for word in ("atomic", "__threadfence", "while", "volatile", "cooperative", "s_sleep"):
        assert word not in code, word
    assert code.count("__syncthreads()") == 1
    assert re.search(r"template\s*<int FOLD,\s*bool WEIGHT>\s*__global__\s+__launch_bounds__\(SL_THREADS\)\s+void\s+softmax_link_kernel", code)
    # six instantiations, all launched from the one launcher
    plan = _text(PLAN)
    launcher = _body(plan, r"int\s+launch_softmax_link\s*\([^)]*\)\s*(?=\{)")
    assert len(re.findall(r"FOS_LINK\((FOLD_OFF|FOLD_TRAIN|FOLD_HELD), (true|false)\)", launcher)) == 6
    assert plan.count("softmax_link_kernel") == 1 and "softmax_link_kernel" not in _text(FISTA)


def test_product_one_is_what_it_was():
    """The closed form list of product 1: 18 forms, two loss names, one launcher."""
    plan = _text(PLAN)
    forms = re.findall(r"^\s*X\((?:true|false), (?:true|false), FOLD_\w+, (LOSS_\w+), (?:true|false)\)", plan, flags=re.M)
    assert len(forms) == 18 and set(forms) == {"LOSS_SQUARED", "LOSS_LOGISTIC"}
    assert len(re.findall(r"^int\s+launch_batch_product\w*\s*\(", plan, flags=re.M)) == 1
