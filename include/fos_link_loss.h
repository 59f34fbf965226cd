/* fos_link_loss.h - the Huber and the squared-hinge loss of the matrix-core lockstep: two entry points of libfos_hip.so beside
 * fos.h.
 *
 * They live in a header of their own: the entry points of fos.h that take a handle and its FOS_LOSS_* enum are closed lists, and
 * these losses need a parameter that fos_problem_set_loss does not take.  Conventions, error codes and handle types are those of
 * fos.h.
 */
#ifndef FOS_LINK_LOSS_H_
#define FOS_LINK_LOSS_H_

#include "fos.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The losses that a pointwise link kernel between the two products of the lockstep serves; they continue FOS_LOSS_* of fos.h and
 * are what fos_problem_get_loss reports. */
enum { FOS_LOSS_HUBER = 3, FOS_LOSS_SQUARED_HINGE = 4 };

/* With W the bound row weights (fos_row_weights_bind) or the identity, z_i = a_i . x:
 *   FOS_LOSS_HUBER, param = the threshold c > 0, r_i = z_i - b_i:
 *     data term sum_i w_i rho_c(r_i), rho_c(r) = r^2 / 2 for |r| <= c and c |r| - c^2 / 2 otherwise; gradient A^T (w * clip(r, -c, c))
 *   FOS_LOSS_SQUARED_HINGE, param = 0, b_i the label -1 or +1 (the caller's duty), u_i = max(0, 1 - b_i z_i):
 *     data term sum_i w_i u_i^2 / 2; gradient A^T (w * (-b u))
 * The derivative of either is 1-Lipschitz in z, so the Lipschitz constant of the gradient is lambda_max(A^T W A), the squared
 * loss's (fos_power_iter), and the lockstep keeps its fixed step.  On such a problem
 *   - fos_fista_run_multi (any nv in 1..16) and fos_fista_run_multi_folds run per row panel product 1 in its plain storing form,
 *     the pointwise link kernel on the panel, and product 2; plain or controlled (adaptive restart, step and ratio tolerance per
 *     column).  Row weights, fold masks, penalty factors, box bounds and feature groups compose.  The gradient-norm rule, the fp64
 *     split gradient, a device-held step, the group penalty across columns (fos_fista_params.group >= 2) and
 *     fos_fista_run_multi_rhs are refused;
 *   - fos_residual_batch (use_b = 1) and fos_residual_batch_folds answer with the data term above, its 1/2 included (the squared
 *     problem's own answer stays sum r^2), fos_gradient_batch with its gradient and, in loss16, the data term;
 *   - every entry point that refuses a logistic problem refuses this one (FOS_ERR_UNSUPPORTED before any launch or change of
 *     handle state, with a message of its own); the ones that touch neither b nor a residual serve.
 * FOS_ERR_ARG, before any HIP call: null p, a loss other than the two, FOS_LOSS_HUBER with a param that is not finite and > 0,
 * FOS_LOSS_SQUARED_HINGE with param != 0.  FOS_ERR_UNSUPPORTED under the conditions of fos_problem_set_multinomial except for
 * feature groups, which compose: no b, a sharded problem, a shape without the matrix-core pair.  No buffer depends on the loss and
 * nothing is replanned.  fos_problem_set_loss (squared, logistic) and fos_problem_set_multinomial leave the loss again;
 * fos_problem_set_loss(p, 3 or 4) stays FOS_ERR_ARG.  The data comes first, the handle last.
 * fos_problem_get_link_loss: *loss = 0 and *param = 0 on a problem that has neither loss. */
int fos_problem_set_link_loss(int loss, double param, fos_problem* p);
int fos_problem_get_link_loss(int* loss, double* param, const fos_problem* p);

#ifdef __cplusplus
}
#endif
#endif /* FOS_LINK_LOSS_H_ */
