/* fos_multinomial_ws.h - the working set and the duality gap of the multinomial lockstep: three entry points of libfos_hip.so
 * beside fos.h.
 *
 * fos_working_set.h and fos_duality.h serve the losses whose 16 lockstep columns are 16 independent fits and refuse a
 * multinomial problem, whose columns are the C class vectors of floor(16 / C) joint fits.  That family needs both most: only
 * floor(16 / C) weights advance per pass over A, the multinomial lockstep has no stopping rule at all, and a grouped fit is sparse
 * in whole rows of X.  The functions of those headers, their refusals and their texts stay as they are; what is declared here are
 * the same three steps with the C columns of a fit seen together.
 *
 * Throughout: the problem is a multinomial one (fos_problem_set_multinomial) with C classes; nv is a multiple of C, nv / C >= 1
 * "segments"; segment s is columns s*C .. s*C + C-1 of the 16-column block (csrc/softmax_link.hpp); `grouped` (0 / 1) says whether
 * the penalty is the l1 penalty over the entries or the group penalty over the classes (the rows of X) - an argument, because the
 * group belongs to fos_fista_params, which a fos_problem does not see; a quantity of a segment is reported at entry s*C of a
 * 16-entry block and the other entries are 0, the way fos_residual_batch reports a multinomial loss.
 *
 * For segment s with the weights alpha1, alpha2: Z = A X_seg (m x C), sigma_i = softmax(z_i), w_i the bound row weight (or 1), p_k
 * the bound penalty factor (or 1), tau_k = alpha1 p_k, rho_k = alpha2 p_k, g_kc the gradient entry of row k of X, class c.
 *
 *   primal  P = sum_i w_i [logsumexp(z_i) - z_{i,y_i}] + Omega(X)
 *   l1      Omega = sum_k sum_c (tau_k |x_kc| + rho_k x_kc^2 / 2); the minimum and the conjugate below run over every entry
 *           (k, c) with v = |g_kc|
 *   group   Omega = sum_k (tau_k ||x_k:||_2 + rho_k ||x_k:||_2^2 / 2); they run over the rows k with v = ||g_k:||_2
 *   scale   s = min(1, min over {rho = 0 and v != 0} of tau / v), in fp64; the minimum of an empty set is 1
 *   dual    D = sum_i w_i d_i - sum over {rho > 0} of max(s v - tau, 0)^2 / (2 rho)
 *           d_i = -sum_c q_ic log q_ic,  q_ic = [y_i = c] + s (sigma_ic - [y_i = c]),  0 log 0 = 0
 *   gap     = P - D >= P - P*
 *
 * The conjugate of the softmax cross-entropy is the negative entropy on the simplex; the dual point is Theta = -s W (sigma -
 * onehot), and row i of q is a convex combination of two points of the simplex for s in [0, 1], so the conjugate is finite.  q is
 * the logistic formula of fos_duality.h with C entries instead of two.  An unpenalised coordinate (p_k = 0) with a non-zero
 * gradient gives s = 0: the bound is valid and loose, as in fos_duality.h.
 *
 * Conventions, error codes and handle types are those of fos.h: enqueue-only on the problem's stream, FOS_ERR_ARG before any HIP
 * call, FOS_ERR_UNSUPPORTED before any launch or change of handle state, text through fos_last_error.  A header of its own for the
 * reason fos_feature_groups.h gives: the handle-taking entry points of fos.h are a closed list filed by the guard tables.
 */
#ifndef FOS_MULTINOMIAL_WS_H_
#define FOS_MULTINOMIAL_WS_H_

#include "fos.h"

#ifdef __cplusplus
extern "C" {
#endif

/* G + j*n (n floats, device) = the class gradient of column j = s*C + c, A^T (w (softmax(A X_seg)_c - [y = c])), for the nv columns
 * of X (n x 16 floats, row-major, columns 0..nv-1 used; columns >= nv are not read).  loss16 (device, 16 doubles; may be NULL):
 * loss16[s*C] = the (weighted) cross-entropy sum of segment s - the value fos_residual_batch(use_b = 1) gives -, 0 elsewhere.
 * Existing launches only: per row panel product 1 in its plain storing form, the softmax link kernel (no fold mask, with the
 * weights), product 2; then the slab sum and the partial fold of fos_gradient_batch.  Two reads of A.
 * FOS_ERR_ARG: null X / p / G, nv outside 1..16.  FOS_ERR_UNSUPPORTED: a problem that is not multinomial, a problem without
 * labels, a sharded problem, a shape without the matrix-core pair, nv not a multiple of C. */
int fos_multinomial_gradient_batch(const float* X, int nv, fos_problem* p, float* G, double* loss16);

/* The optimality check of the coordinates (rows of X) outside a working set, on the block G of fos_multinomial_gradient_batch.
 * alpha1: HOST memory, nv / C weights, one per segment; in_ws: device, n bytes; p_i: the bound penalty factor or 1.  For every
 * coordinate i with in_ws[i] == 0, everything formed in fp64 from the float G:
 *   l1      v_is = max_c |G[s*C + c][i]|
 *   group   q_is = sum_c G[s*C + c][i]^2 with c ascending, v_is = sqrt(q_is)
 *   excess[i] (device, n floats) = (float) max_s v_is / (alpha1[s] p_i); a zero denominator gives +inf where v > 0 and 0 where
 *           v = 0; a coordinate inside the set gets 0
 *   i is a violator when some s has   l1: v_is > alpha1[s] p_i (1 + slack)     group: q_is > (alpha1[s] p_i (1 + slack))^2
 *           - the grouped decision takes no square root.
 * viol_idx (device, n int32) receives the violators in increasing order, *viol_count (device) their number.  ONE workgroup:
 * per-wave ballots and a block prefix sum, no atomics - two runs give the same bytes.
 * FOS_ERR_ARG: a null pointer, nv outside 1..16, grouped outside 0..1, slack not finite and >= 0; and, once the class count is
 * read from the problem (still before any HIP call), a weight that is not finite and >= 0.  FOS_ERR_UNSUPPORTED: a problem that is
 * not multinomial, nv not a multiple of C, box bounds (fos_coord_bind) are bound. */
int fos_multinomial_kkt_scan(const float* G, int nv, int grouped, const double* alpha1, double slack, const uint8_t* in_ws,
                             fos_problem* p, float* excess, int32_t* viol_idx, int32_t* viol_count);

/* The certificate of the nv / C segments of X under the weights alpha1[s], alpha2[s] (HOST memory, nv / C each).
 *   G      device, nv x n floats, an OUTPUT: bit for bit the block of fos_multinomial_gradient_batch at X;
 *   out64  device, 64 doubles: primal[16], dual[16], gap[16] = primal - dual, scale[16], at the entries s*C; 0 elsewhere.
 * Enqueues only: the launches of fos_multinomial_gradient_batch; the column pass (one workgroup per segment: the scale, then the
 * penalty and its conjugate, fp64); per row panel product 1 in its plain storing form once more and the row pass, which forms
 * w f and w d of every row in fp64 from the same fp32 logits; dual_finish_kernel of fos_duality_gap.  Every sum has a fixed order:
 * two calls give the same 64 doubles.  Three reads of A.  The handle's configuration is not changed; the buffers belong to the
 * handle's workspace.
 * FOS_ERR_ARG: a null pointer, nv outside 1..16, grouped outside 0..1; once the class count is read, a weight that is not finite
 * and >= 0.  FOS_ERR_UNSUPPORTED: a problem that is not multinomial, a problem without labels, a sharded problem, a shape without
 * the matrix-core pair, nv not a multiple of C, box bounds, feature groups. */
int fos_multinomial_duality_gap(const float* X, int nv, int grouped, const double* alpha1, const double* alpha2, fos_problem* p,
                                float* G, double* out64);

#ifdef __cplusplus
}
#endif
#endif /* FOS_MULTINOMIAL_WS_H_ */
