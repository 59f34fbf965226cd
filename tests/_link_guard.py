"""Where every handle-taking entry point stands on a Huber or squared-hinge problem (fos_problem_set_link_loss) - a helper: no
tests in here.

The C table files every function of include/fos.h and of the three side headers (fos_feature_groups.h, fos_working_set.h,
fos_link_loss.h) that takes a fos_problem* or a fos_fista* in any position: the rows of tests/_multinomial_guard.py - such a
problem stands where a logistic one does - plus the side headers' entry points.  SERVES: computes with the problem's loss
(product 1 plain, the pointwise link kernel, product 2).  LOSS_FREE: touches neither b nor a residual and works as before (row
weights, coordinate data and feature groups compose; the setters of the other losses leave the link loss).  REFUSES: returns
FOS_ERR_UNSUPPORTED through the one helper need_squared, whose refusal names fos_problem_set_link_loss, before any launch or change
of handle state.

The Python table files every name of fastoptsolver_amd.__all__ plus the names this loss adds: "serves", "loss_free", "refuses"
(raises FosError or ValueError on such a handle) and "no_handle".  tests/test_link_guard.py keeps both tables complete;
tests/test_gpu_link_guard.py executes them."""
import os

from tests import _multinomial_guard as mgd

ROOT, GUARD, body_of = mgd.ROOT, mgd.GUARD, mgd.body_of
SIDE_HEADERS = tuple(os.path.join(ROOT, "include", h) for h in ("fos_feature_groups.h", "fos_working_set.h", "fos_link_loss.h"))
NEW = {"fos_problem_set_link_loss", "fos_problem_get_link_loss"}


def header_handle_functions():
    """Every function of the four headers with a fos_problem* or fos_fista* parameter in any position."""
    out = mgd.header_handle_functions()
    for h in SIDE_HEADERS:
        out |= mgd.header_handle_functions(h)
    return out


SERVES = set(mgd.SERVES) | {"fos_gradient_batch"}
LOSS_FREE = set(mgd.LOSS_FREE) | NEW | {"fos_feature_groups_bind", "fos_feature_groups_get", "fos_gather_columns", "fos_kkt_scan"}
REFUSES = set(mgd.REFUSES)

NEW_PYTHON = ("huber_path", "huber_cv", "huber_objective", "hinge_path", "hinge_cv", "hinge_objective", "HuberCVResult", "HingeCVResult",
              "prepare_huber", "prepare_hinge", "working_set_path", "kkt_excess", "alpha_max", "WorkingSetInfo")

PYTHON = {
    # each of the six serves the handle of its own loss and refuses the other's
    "huber_path": "serves", "huber_cv": "serves", "huber_objective": "serves",
    "hinge_path": "serves", "hinge_cv": "serves", "hinge_objective": "serves",
    "working_set_path": "serves", "kkt_excess": "serves", "alpha_max": "serves",
    "estimate_lipschitz": "loss_free", "Problem": "loss_free", "prepare": "loss_free",
    "fista": "refuses", "fista_delta": "refuses", "ista": "refuses", "LBFGSSolver": "refuses", "compute_objective": "refuses",
    "LeastSquares": "refuses", "group_lasso_objective": "refuses",
    "fista_path": "refuses", "fista_cv": "refuses", "logistic_path": "refuses", "logistic_cv": "refuses", "logistic_objective": "refuses",
    "multinomial_path": "refuses", "multinomial_cv": "refuses", "multinomial_objective": "refuses",
    "multitask_path": "refuses", "multitask_objective": "refuses",
    "prepare_weighted": "refuses", "prepare_penalized": "refuses", "prepare_grouped": "refuses", "prepare_multinomial": "refuses",
    "prepare_huber": "refuses", "prepare_hinge": "refuses",
    "CVResult": "no_handle", "LogisticCVResult": "no_handle", "MultinomialCVResult": "no_handle", "HuberCVResult": "no_handle",
    "HingeCVResult": "no_handle", "WorkingSetInfo": "no_handle", "FosError": "no_handle",
    "reset_metrics": "no_handle", "get_metrics": "no_handle", "prox_l1": "no_handle", "prox_elastic_net": "no_handle",
    "L1Prox": "no_handle", "ElasticNetProx": "no_handle",
}
