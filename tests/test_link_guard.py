"""CPU: the guard tables of the Huber and squared-hinge losses (tests/_link_guard.py) file every entry point of include/fos.h and of
the three side headers that takes a handle in any position and every public name; the refusing entry points call the one guard
helper first, the guard has a text of its own for these losses, and the dispatchers put the pointwise link kernel between the two
products."""
import re

from tests import _link_guard as gd
from tests._menu_product1 import FISTA, PLAN, _body, _text


def test_c_table_is_complete_and_disjoint():
    header = gd.header_handle_functions()
    filed = gd.SERVES | gd.LOSS_FREE | gd.REFUSES
    assert len(header) > 60, len(header)
    assert header - filed == set(), "entry points without a row in tests/_link_guard.py"
    assert filed - header == set(), "rows without an entry point in the headers"
    assert not (gd.SERVES & gd.LOSS_FREE or gd.SERVES & gd.REFUSES or gd.LOSS_FREE & gd.REFUSES)
    assert gd.NEW <= header and {"fos_gradient_batch", "fos_feature_groups_bind"} <= header


def test_python_table_is_complete():
    import fastoptsolver_amd as fos
    assert set(gd.PYTHON) == set(fos.__all__) | set(gd.NEW_PYTHON), set(gd.PYTHON) ^ (set(fos.__all__) | set(gd.NEW_PYTHON))
    assert set(gd.PYTHON.values()) == {"serves", "loss_free", "refuses", "no_handle"}
    assert all(hasattr(fos, name) for name in gd.PYTHON)


def test_every_refusing_entry_point_calls_the_one_guard_first():
    for name in sorted(gd.REFUSES):
        body = gd.body_of(name)
        m = re.search(gd.GUARD + r"\s*\(", body)
        assert m, name
        before = body[:m.start()]
        assert not re.search(r"hipLaunchKernelGGL|hipMalloc|hipMemcpy|hipMemset|reserve\(|->\w+\s*=[^=]|invalidate\(", before), name
        for word in ("HUBER", "HINGE", "link_loss", "link_param"):          # the refusing bodies know nothing of the new losses
            assert word not in body, (name, word)


def test_the_guard_has_a_text_of_its_own_and_keeps_the_others():
    body = _body(_text(PLAN), r"int\s+" + gd.GUARD + r"\s*\([^)]*\)\s*(?=\{)")
    own = body.index("link_refusal(p, fn)")                         # ahead of the text of the logistic / multinomial loss
    assert body.index("p->row_weight != nullptr") < own < body.index("p->loss != FOS_LOSS_SQUARED")
    assert "multinomial problem" in body and "logistic problem" in body
    refusal = _body(_text(PLAN), r"int\s+link_refusal\s*\([^)]*\)\s*(?=\{)")
    assert "link_loss(p)" in refusal and "fos_problem_set_link_loss" in refusal and "Huber" in refusal and "squared-hinge" in refusal
    assert len(re.findall(r"FOS_ERR_UNSUPPORTED", refusal)) == 1 and re.search(r"return\s+FOS_OK\s*;\s*$", refusal.strip().rstrip("}").strip())


def test_the_dispatchers_put_the_pointwise_link_between_the_products():
    text = _text(FISTA)
    decide = _body(text, r"static\s+int\s+lockstep_route\s*\([^)]*\)\s*(?=\{)")
    # behind the group branch (group_refusal refuses the group penalty on these losses), ahead of the logistic one
    assert decide.index("any_grouped(fs, nv)") < decide.index("if (link_loss(p)) {") < decide.index("p->loss == FOS_LOSS_LOGISTIC")
    route = _body(decide, r"if\s*\(link_loss\(p\)\)\s*(?=\{)")
    assert len(re.findall(r"FOS_ERR_UNSUPPORTED", route)) == 1 and re.search(r"return\s+control_refusal\(\)\s*;\s*$", route.strip())
    assert "all_plain" not in route                                 # controlled runs are served: the columns are independent
    assert "link_loss(p)" in _body(text, r"static\s+int\s+group_refusal\s*\([^)]*\)\s*(?=\{)")
    mfma = _body(text, r"static\s+int\s+run_multi_mfma\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"if\s*\(link\)\s*\{\s*L\.b\s*=\s*nullptr;\s*L\.use_b\s*=\s*0;\s*L\.fold_of_row\s*=\s*nullptr;\s*L\.held\s*=\s*nullptr;\s*"
                     r"L\.row_weight\s*=\s*nullptr;\s*\}", mfma)
    assert mfma.index("launch_batch_product") < mfma.index("launch_pointwise_link") < mfma.index("launch_gram_panel")
    assert re.search(r"use_cluster\s*=\s*p->multi\.cp_cs\s*&&\s*!two_products\s*&&\s*!softmax\s*&&\s*!link", mfma)
    # fos_gradient_batch hands its panel loop to the walk it shares with the multinomial gradient: plain product 1 and the pointwise
    # stage exactly on a link loss, and in the walk the stage stands between the products
    assert re.search(r"const bool link = link_loss\(p\);\s*return gradient_walk\(\{\"fos_gradient_batch\",[^;]*, link, "
                     r"link \? WalkLink::pointwise : WalkLink::none, true\},", gd.body_of("fos_gradient_batch"))
    grad = _body(text, r"static\s+int\s+gradient_walk\s*\([^)]*\)\s*(?=\{)")
    assert grad.index("launch_batch_product") < grad.index("launch_pointwise_link") < grad.index("launch_gram_panel")
    assert re.search(r"if \(w\.link == WalkLink::pointwise && \(rc = launch_pointwise_link\(", grad) and grad.count("launch_gram_panel") == 1
    assert re.search(r"residual_batch_link\(p,\s*\"fos_residual_batch\",\s*X,\s*nv,\s*out16,\s*nullptr,\s*nullptr\)", gd.body_of("fos_residual_batch"))
    assert re.search(r"residual_batch_link\(p,\s*\"fos_residual_batch_folds\",\s*X,\s*nv,\s*out16,\s*fold_of_row,\s*&hb\)",
                     gd.body_of("fos_residual_batch_folds"))
    rb = _body(_text(PLAN), r"static\s+int\s+residual_batch_link\s*\([^)]*\)\s*(?=\{)")
    assert rb.index("launch_batch_product") < rb.index("launch_pointwise_link") and re.search(r"held\s*\?\s*fos::FOLD_HELD\s*:\s*fos::FOLD_OFF", rb)


def test_the_link_kernel_has_no_waits_flags_or_atomics():
    with open(gd.mgd.CSRC + "/pointwise_link.hpp") as fh:
        code = re.sub(r"//[^\n]*", "", fh.read())
    for word in ("atomic", "__threadfence", "while", "volatile", "cooperative", "s_sleep"):
        assert word not in code, word
    assert code.count("__syncthreads()") == 1
    assert re.search(r"template\s*<int LINK,\s*int FOLD,\s*bool WEIGHT>\s*__global__\s+__launch_bounds__\(PL_THREADS\)\s+void\s+pointwise_link_kernel", code)
    # the grid stride is a multiple of 4 (a lane's quad is fixed) and the grid stays within the rows of cand.q_part
    assert re.search(r"constexpr\s+int\s+PL_THREADS\s*=\s*256\s*;", code) and re.search(r"stride\s*=\s*\(int64_t\)gridDim\.x\s*\*\s*PL_THREADS", code)
    plan = _text(PLAN)
    launcher = _body(plan, r"int\s+launch_pointwise_link\s*\([^)]*\)\s*(?=\{)")
    assert re.search(r"std::min<int64_t>\(\(4 \* rows \+ fos::PL_THREADS - 1\) / fos::PL_THREADS, 2 \* \(int64_t\)p->ncu\)", launcher)
    # twelve instantiations, all launched from the one launcher
    assert len(re.findall(r"FOS_LINK\(K, (FOLD_OFF|FOLD_TRAIN|FOLD_HELD), (true|false)\)", plan)) == 6
    assert len(re.findall(r"FOS_LINK_FORM\((LINK_HUBER|LINK_SQUARED_HINGE)\)", launcher)) == 2
    assert plan.count("pointwise_link_kernel") == 1 and "pointwise_link_kernel" not in _text(FISTA)
