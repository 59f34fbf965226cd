"""fastoptsolver_amd — MI355X-native inner loops (FISTA / ISTA / FISTA-Δ / L-BFGS) behind the call signatures
of ElBaldo1/FastOptSolver.  Hand-written HIP for gfx950 through a C ABI (include/fos.h); no CPU fallback."""
from ._core import Problem, prepare, prepare_grouped, prepare_weighted, prepare_penalized                               # noqa: F401
from ._lib import FosError                                            # noqa: F401
from .iterative_solvers import (CVResult, estimate_lipschitz, fista, fista_cv, fista_delta, fista_path,  # noqa: F401
                                get_metrics, ista, reset_metrics)
from .lbfgs import LBFGSSolver                                        # noqa: F401
from .logistic import LogisticCVResult, logistic_cv, logistic_objective, logistic_path   # noqa: F401
from .multinomial import (MultinomialCVResult, multinomial_cv, multinomial_objective, multinomial_path,   # noqa: F401
                          prepare_multinomial)
from .multitask import multitask_objective, multitask_path         # noqa: F401
from .objective_functions import compute_objective, group_lasso_objective                    # noqa: F401
from .operators import ElasticNetProx, L1Prox, LeastSquares           # noqa: F401
from .prox_operators import prox_elastic_net, prox_l1                 # noqa: F401
# the working-set solve: importable from the package; __all__ stays the list the guard tables of the handle kinds file name by name
from .working_set import WorkingSetInfo, alpha_max, kkt_excess, working_set_path   # noqa: F401

# the Huber and squared-hinge losses: importable from the package likewise
from ._core import prepare_hinge, prepare_huber                                                      # noqa: F401
from .robust import (HingeCVResult, HuberCVResult, hinge_cv, hinge_objective, hinge_path,            # noqa: F401
                     huber_cv, huber_objective, huber_path)

# the duality-gap certificate and the gap-stopped path: importable from the package likewise
from .duality import DualityGap, GapInfo, certified_path, duality_gap                                # noqa: F401

# the working set and the duality gap of the multinomial lockstep: importable from the package likewise
from .multinomial_ws import (multinomial_alpha_max, multinomial_certified_path, multinomial_duality_gap,   # noqa: F401
                             multinomial_kkt_excess, multinomial_working_set_path)

# resampled fits in the lockstep (bootstrap paths, stability selection): importable from the package likewise
from .resample import (ResampleResult, StabilityResult, bootstrap_counts, pack_counts, resampled_lipschitz,   # noqa: F401
                       resampled_path, selection_frequencies, stability_selection, subsample_counts)

__all__ = ["fista", "fista_delta", "fista_path", "fista_cv", "CVResult", "ista", "estimate_lipschitz", "reset_metrics", "get_metrics", "LBFGSSolver",
           "compute_objective", "prox_l1", "prox_elastic_net", "LeastSquares", "L1Prox", "ElasticNetProx",
           "prepare", "prepare_weighted", "prepare_penalized", "Problem", "FosError", "logistic_path", "logistic_cv", "logistic_objective", "LogisticCVResult",
           "multinomial_path", "multinomial_cv", "multinomial_objective", "MultinomialCVResult", "prepare_multinomial",
           "multitask_path", "multitask_objective", "prepare_grouped", "group_lasso_objective"]
