"""Where every handle-taking entry point of include/fos.h stands on a logistic problem (a helper: no tests in here).

SERVES: computes with the logistic loss.  LOSS_FREE: touches neither b nor a residual and works as before.  REFUSES: forms a
residual, gradient or objective with b as a squared-loss target (or attaches what the logistic lockstep does not serve) and
returns FOS_ERR_UNSUPPORTED through the one helper need_squared before any launch or change of handle state.
tests/test_logit_guard.py keeps the table complete against the header and checks the helper call in every REFUSES body;
tests/test_gpu_logit_guard.py calls every REFUSES entry point on a logistic problem."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastoptsolver_amd", "csrc")

SERVES = {
    "fos_fista_run_multi", "fos_fista_run_multi_folds",
    "fos_residual_batch",            # use_b = 1; use_b = 0 goes through the guard
    "fos_residual_batch_folds",
}
LOSS_FREE = {
    "fos_problem_destroy", "fos_problem_set_stream", "fos_problem_plan", "fos_problem_replan", "fos_problem_tune",
    "fos_problem_tune_dd", "fos_problem_set_gbuf", "fos_problem_set_loss", "fos_problem_get_loss", "fos_problem_profile",
    "fos_problem_profile_read", "fos_problem_set_fused_stamps", "fos_power_iter",
    "fos_fista_create", "fos_fista_destroy", "fos_fista_reset", "fos_fista_set_tau", "fos_fista_status_get", "fos_fista_get_x",
    "fos_fista_x", "fos_fista_gbuf",
    # settings and sizes: a handle with the fp64 split gradient is refused by the lockstep itself when it runs
    "fos_fista_set_precise", "fos_fista_set_gbuf64", "fos_fista_history_workspace",
}
REFUSES = {
    "fos_problem_set_comm", "fos_problem_set_comm_cols",
    "fos_gemv_pair", "fos_gemv_pair_f64", "fos_gemv_pair_dd", "fos_gemv_pair_dd_multi", "fos_residual_objective",
    "fos_residual_batch_rhs", "fos_fista_run_multi_rhs",
    "fos_fista_run", "fos_fista_run_history", "fos_fista_run_resident", "fos_fista_run_fused", "fos_fista_run_chip",
    "fos_fista_grad", "fos_fista_grad_dual", "fos_fista_update", "fos_fista_trial", "fos_fista_trial_batch",
    "fos_fista_run_backtracking", "fos_fista_run_recorded", "fos_fista_resume_after_stall",
    "fos_lbfgs_direction_cols", "fos_lbfgs_minimize", "fos_lbfgs_minimize_multi",
}
GUARD = "need_squared"


def header_handle_functions(path=None):
    """Every function of the header whose first parameter is a fos_problem*, a fos_fista* or a fos_fista* const*."""
    with open(path or os.path.join(ROOT, "include", "fos.h")) as fh:
        txt = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    return set(re.findall(r"\b(fos_[a-z0-9_]+)\s*\(\s*(?:const\s+)?(?:fos_problem\s*\*|fos_fista\s*\*(?:\s*const\s*\*)?)\s*\w+", txt))


def body_of(name):
    """The body of the definition of an exported function, from the translation units of the library."""
    for unit in ("fos_plan.hip", "fos_fista.hip", "fos_lbfgs.hip", "fos_comm.hip"):
        with open(os.path.join(CSRC, unit)) as fh:
            txt = fh.read()
        m = re.search(r"^[\w\*]+\s+" + name + r"\s*\((?:[^{;])*?\)\s*\{", txt, flags=re.M)
        if not m:
            continue
        depth, i = 1, m.end()
        while depth and i < len(txt):
            depth += {"{": 1, "}": -1}.get(txt[i], 0)
            i += 1
        return txt[m.end():i]
    return None
