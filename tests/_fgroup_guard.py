"""Where every handle-taking entry point stands on a problem with feature groups (fos_feature_groups_bind) - a helper: no tests
in here.

The C table files every function of include/fos.h and of include/fos_feature_groups.h that takes a fos_problem* or a fos_fista*
in any position: the rows of tests/_multinomial_guard.py re-filed for this binding, and the two entry points of the feature
groups' own header (fos.h's handle-taking entry points are a closed list, so the two are declared beside it).  SERVES: computes with the group penalty, or with the data term alone,
which does not depend on it.  LOSS_FREE: touches neither b nor a residual and works as before (fos_row_weights_bind and
fos_problem_set_loss compose; the bind and the get of the feature groups themselves are here).  REFUSES: returns
FOS_ERR_UNSUPPORTED before any launch or change of handle state - through the one helper need_squared, whose refusal names
fos_feature_groups_bind, or (OWN_CHECK) through a check of its own: fos_coord_bind and fos_problem_set_multinomial, which do not
compose with the group norm.

The Python table files every name of fastoptsolver_amd.__all__: "serves" (answers for the objective with the group penalty),
"loss_free" (works as before), "refuses" (raises FosError or ValueError on such a handle) and "no_handle" (takes no problem
handle).  tests/test_fgroup_abi.py keeps both tables complete; tests/test_gpu_fgroup_guard.py executes them."""
from tests import _multinomial_guard as mgd

import os

GUARD, body_of = mgd.GUARD, mgd.body_of
OWN_HEADER = os.path.join(mgd.ROOT, "include", "fos_feature_groups.h")
NEW = {"fos_feature_groups_bind", "fos_feature_groups_get"}


def header_handle_functions():
    """Every function of the two headers with a fos_problem* or fos_fista* parameter in any position."""
    return mgd.header_handle_functions() | mgd.header_handle_functions(OWN_HEADER)


OWN_CHECK = {"fos_coord_bind", "fos_problem_set_multinomial"}
SERVES = set(mgd.SERVES)
LOSS_FREE = (set(mgd.LOSS_FREE) - OWN_CHECK) | NEW
REFUSES = set(mgd.REFUSES) | OWN_CHECK

PYTHON = {
    "fista_path": "serves", "fista_cv": "serves", "logistic_path": "serves", "logistic_cv": "serves",
    "group_lasso_objective": "serves",
    "estimate_lipschitz": "loss_free", "Problem": "loss_free", "prepare": "loss_free",
    "fista": "refuses", "fista_delta": "refuses", "ista": "refuses", "LBFGSSolver": "refuses", "compute_objective": "refuses",
    "logistic_objective": "refuses",
    "multinomial_path": "refuses", "multinomial_cv": "refuses", "multinomial_objective": "refuses",
    "multitask_path": "refuses", "multitask_objective": "refuses",
    "prepare_weighted": "refuses", "prepare_penalized": "refuses", "prepare_grouped": "refuses", "prepare_multinomial": "refuses",
    "CVResult": "no_handle", "LogisticCVResult": "no_handle", "MultinomialCVResult": "no_handle", "FosError": "no_handle",
    "reset_metrics": "no_handle", "get_metrics": "no_handle", "prox_l1": "no_handle", "prox_elastic_net": "no_handle",
    "LeastSquares": "no_handle", "L1Prox": "no_handle", "ElasticNetProx": "no_handle",
}
