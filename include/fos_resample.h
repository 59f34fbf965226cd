/* fos_resample.h - resampled fits in the matrix-core lockstep: three entry points of libfos_hip.so beside fos.h.
 *
 * The lockstep solves up to 16 fits with one read of A per iteration.  Here every column fits a resample of the rows of its own:
 * a bootstrap sample (a row drawn 0, 1, 2, ... times), a random subsample (0 / 1), a bag.  Stability selection, the bootstrap
 * lasso, bagged paths and out-of-bag error are "many fits, one A" and run as columns of one pass instead of one weighted handle
 * per resample.
 *
 * The multiplicities: counts[i], one 8-byte word per row on the device, 8-byte aligned, little-endian; bits 4 j .. 4 j + 3 hold
 * c_ij in 0 .. 15, the multiplicity of row i in the resample that lockstep column j fits.  0 / 1 words are subsamples.  A count
 * above 15 has no encoding; the caller refuses it (fastoptsolver_amd.resample.pack_counts raises).
 *
 * Column j then carries the data term  sum_i c_ij w_i f(a_i . x_j, b_i)  with f the loss of the problem (squared with its 1/2,
 * logistic, Huber, squared hinge) and w the bound row weights or 1: the problem with the weights w * c_j.  Per row panel the
 * launches are product 1 in its plain storing form (Z = A_panel Y: neither b nor the weights enter it), the resample link kernel
 * (csrc/resample_link.hpp), which rewrites the panel in place as R_ij = (psi(z_ij, b_i) w_i) c_ij, and product 2.  Nothing after
 * product 1's panel depends on the counts, so the updates, restarts and stops are the lockstep's own.
 *
 * They live in a header of their own for the reason fos_feature_groups.h gives: the handle-taking entry points of fos.h are a
 * closed list filed by the guard tables.  Conventions, error codes and handle types are those of fos.h: data pointers first, the
 * handle before the outputs, enqueue-only, FOS_ERR_ARG checked before any HIP call, text through fos_last_error.
 */
#ifndef FOS_RESAMPLE_H_
#define FOS_RESAMPLE_H_

#include "fos.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fos_fista_run_multi with state machine v fitting the resample in nibble v of counts (m words).  Any nv in 1..16, on a problem
 * with the squared, logistic, Huber or squared-hinge loss; plain or controlled runs (adaptive restart, step and ratio tolerance
 * per column).  Row weights, penalty factors, box bounds and feature groups compose.  The step is the caller's: a bootstrap
 * column's Lipschitz constant lambda_max(A^T diag(w * c_j) A) can exceed that of the whole A (fos_gram_apply_resampled is the
 * operator of its power iteration); for 0 / 1 counts the constant of the whole A is valid.  A handle that ran resampled serves
 * every other run form afterwards as a fresh one does: nothing is bound to the problem.
 * FOS_ERR_ARG (before any HIP call): a null pointer, nv outside 1..16, iters < 0, counts not 8-byte aligned, handles of
 * different problems.
 * FOS_ERR_UNSUPPORTED (before any launch or change of handle state): a multinomial problem; handles under the group penalty
 * across columns (fos_fista_params.group >= 2); a sharded or column-sharded problem; a problem without b; a shape without the
 * matrix-core pair; the gradient-norm rule, the fp64 split gradient or a device-held step. */
int fos_fista_run_multi_resampled(fos_fista* const* fs, int nv, int iters, const uint64_t* counts);

/* The gradient of the resampled data term at the nv <= 16 columns of X (the layout of fos_gradient_batch: n x 16 floats,
 * row-major, columns 0..nv-1 used): G (device, nv x n floats) row j = A^T ((w * c_j) psi(A x_j, b)), loss16 (device, 16 doubles,
 * nullable) entry j = sum_i c_ij w_i f(a_i . x_j, b_i), the squared loss with its 1/2; entries >= nv are 0.
 * oob = 1: only the out-of-bag sums, loss16[j] = sum over {i : c_ij = 0} of w_i f(a_i . x_j, b_i) - every such row once -; A is
 * read once, product 2 does not run and G may be null (loss16 may not).
 * FOS_ERR_ARG: a null X, counts, p (G with oob = 0, loss16 with oob = 1), nv outside 1..16, counts not 8-byte aligned, oob
 * outside 0..1.  FOS_ERR_UNSUPPORTED: a multinomial, sharded or column-sharded problem, one without b, a shape without the
 * matrix-core pair. */
int fos_gradient_batch_resampled(const float* X, int nv, const uint64_t* counts, int oob, fos_problem* p, float* G, double* loss16);

/* G (device, nv x n floats) row j = A^T ((w * c_j) * (A x_j)): fos_gram_apply under the resamples, the operator of the power
 * iteration per resample.  Loss-free: it serves a squared, logistic, Huber or squared-hinge problem alike, with or without b.
 * FOS_ERR_ARG: a null pointer, nv outside 1..16, counts not 8-byte aligned.  FOS_ERR_UNSUPPORTED: a multinomial, sharded or
 * column-sharded problem, a shape without the matrix-core pair. */
int fos_gram_apply_resampled(const float* X, int nv, const uint64_t* counts, fos_problem* p, float* G);

#ifdef __cplusplus
}
#endif
#endif /* FOS_RESAMPLE_H_ */
