/* fos_duality.h - the duality-gap certificate of lockstep solutions: one entry point of libfos_hip.so beside fos.h.
 *
 * The lockstep stops on an iteration budget or on the reference's step and ratio rules; none of them says how far a returned x is
 * from the minimum.  The duality gap does, for every loss the lockstep serves: gap = P(x) - D(theta) >= P(x) - P*.
 *
 * For one column - a point x with its weights alpha1, alpha2 - let z_i = a_i . x, w_i the bound row weight (or 1), p_k the bound
 * penalty factor (or 1), tau_k = alpha1 p_k, rho_k = alpha2 p_k, psi_i = df/dz the unweighted derivative of the loss, and
 * G = A^T (w psi) the gradient of the data term (fos_gradient_batch).  Then
 *
 *   primal  P = sum_i w_i f(z_i, b_i) + sum_k (tau_k |x_k| + rho_k x_k^2 / 2)
 *   scale   s = min(1, min over {k : rho_k = 0 and G_k != 0} of tau_k / |G_k|), formed in fp64 from the float G_k and the double
 *               alpha1 * (double)p_k in exactly this arithmetic; the minimum of an empty set is 1
 *   dual    D = sum_i w_i d(z_i, b_i; s) - sum over {k : rho_k > 0} of max(s |G_k| - tau_k, 0)^2 / (2 rho_k)
 *             at the dual point theta = -s (w psi), with
 *               squared, Huber (psi = z - b, or clip(z - b, -c, c))   d = -s psi b - s^2 psi^2 / 2
 *               squared hinge  (h = max(0, 1 - b z))                  d = s h - s^2 h^2 / 2
 *               logistic       (q = b + s (sigma(z) - b))             d = -(q log q + (1 - q) log(1 - q)),  0 log 0 = 0
 *   gap     = P - D >= 0
 *
 * The data term of the squared loss is sum w (z - b)^2 / 2: half of what fos_residual_batch reports on a squared problem.
 * An unpenalised coordinate (p_k = 0) with a non-zero gradient gives s = 0; the bound D = -F*(0) is then valid but loose - the
 * dual point is not projected off the free columns.
 *
 * It lives in a header of its own for the reason fos_feature_groups.h gives: the handle-taking entry points of fos.h are a
 * closed list filed by the guard tables.  Conventions, error codes and handle types are those of fos.h: data pointers first, the
 * handle before the outputs, enqueue-only, FOS_ERR_ARG checked before any HIP call, text through fos_last_error.
 */
#ifndef FOS_DUALITY_H_
#define FOS_DUALITY_H_

#include "fos.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The certificate of the nv <= 16 columns of X (the layout of fos_gradient_batch: n x 16 floats, row-major, columns 0..nv-1 used)
 * under the weights alpha1[j], alpha2[j] (HOST memory, nv each).
 *   G      device, nv x n floats, an OUTPUT: the gradient block of fos_gradient_batch at X, bit for bit, the block fos_kkt_scan
 *          reads - a caller gets the KKT scan from the same gradient;
 *   out64  device, 64 doubles: primal[16], dual[16], gap[16] = primal - dual, scale[16]; the entries of columns >= nv are 0.
 * Enqueues only, on the handle's stream: the launches of fos_gradient_batch; the column pass (one workgroup per column: the
 * scale, then the penalty and its conjugate, fp64); a second loop over the row panels - product 1 in its plain storing form,
 * then the row pass, which forms w f and w d of every element in fp64 from the same fp32 z; a one-workgroup finish.  Every sum
 * has a fixed order: two calls give the same 64 doubles.  Three reads of A per certificate, two of them from the Infinity Cache
 * where a row panel fits.  The handle's configuration is not changed; its device buffers belong to the handle's workspace.
 * FOS_ERR_ARG (before any HIP call): a null pointer, nv outside 1..16, a weight that is not finite and >= 0.
 * FOS_ERR_UNSUPPORTED (before any launch or change of handle state): what fos_gradient_batch and fos_kkt_scan refuse - a
 * multinomial problem, a problem without b, a sharded problem, a shape without the matrix-core pair, box bounds, feature groups. */
int fos_duality_gap(const float* X, int nv, const double* alpha1, const double* alpha2, fos_problem* p, float* G, double* out64);

#ifdef __cplusplus
}
#endif
#endif /* FOS_DUALITY_H_ */
