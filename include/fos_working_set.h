/* fos_working_set.h - the pieces of a working-set solve of a sparse path: three entry points of libfos_hip.so beside fos.h.
 *
 * A lasso, elastic-net or sparse logistic path at useful weights keeps a few percent of the coordinates non-zero, yet every
 * lockstep iteration streams all n columns of A twice.  A working-set solve (glmnet, celer, skglm) runs the lockstep on the
 * columns that can be non-zero, checks the optimality conditions of the FULL problem with one gradient over all columns, adds the
 * violators and repeats; the result is the minimiser of the full problem, certified by its KKT conditions.  The lockstep itself is
 * untouched: the sub-problem is an ordinary fos_problem on a gathered matrix.  What was missing is declared here - the gradient of
 * the data term at a given X, the column gather and the KKT scan; the outer loop lives in fastoptsolver_amd/working_set.py.
 *
 * They live in a header of their own for the reason fos_feature_groups.h gives: the handle-taking entry points of fos.h are a
 * closed list filed by the guard tables.  Conventions, error codes and handle types are those of fos.h: data pointers first, the
 * handle last, enqueue-only unless stated, FOS_ERR_ARG checked before any HIP call, text through fos_last_error.
 */
#ifndef FOS_WORKING_SET_H_
#define FOS_WORKING_SET_H_

#include "fos.h"

#ifdef __cplusplus
extern "C" {
#endif

/* G + j*n (n floats, device) = A^T l'(A X_j; b, w) for the nv <= 16 columns of X (the layout of fos_gram_apply: X is n x 16
 * floats, row-major, columns 0..nv-1 used): the gradient of the data term - A^T W (A X_j - b) on a squared problem, A^T W
 * (sigma(A X_j) - b) on a logistic one, W the bound row weights or the identity.  Penalty factors, bounds and feature groups do not
 * enter the data term and are ignored.  loss16 (device, 16 doubles; may be NULL): loss16[j] = the data-term sum that
 * fos_residual_batch(use_b = 1) gives for column j, from the same pass.  Existing launches only: per row panel product 1 in its
 * storing form with b, the problem's loss epilogue and the weights, then product 2; the slab sum of fos_gram_apply at the end.
 * Two reads of A (the second from the Infinity Cache where the panel fits).  Enqueues only.
 * FOS_ERR_ARG: null X / p / G, nv outside 1..16.  FOS_ERR_UNSUPPORTED (before any launch or change of handle state): a
 * multinomial problem, a problem without b, a sharded problem, a shape without the matrix-core pair. */
int fos_gradient_batch(const float* X, int nv, fos_problem* p, float* G, double* loss16);

/* A_ws[i][c] = A[i][idx[c]] for c < n_ws and exactly 0 for n_ws <= c < n_ws_pad, for every row i of the problem's A.  A_ws
 * (device, m rows of lda_ws elements) has the element type of A (fp32 or bf16); elements beyond column n_ws_pad of a row are not
 * written.  idx: DEVICE memory, n_ws entries, strictly increasing, each in 0..n-1 - the values are the caller's to check (the
 * Python layer does); this call checks pointers, alignment and the ranges of the scalars.  One kernel, one lane per working-set
 * column, non-temporal loads of A, contiguous stores (csrc/working_set.hpp); it fetches the cache lines of A that hold a gathered
 * column, never more than one read of A, and writes A_ws once.  Enqueues only on the problem's stream.
 * FOS_ERR_ARG: a null pointer, n_ws outside 1..n, n_ws_pad < n_ws or not a multiple of 8, lda_ws < n_ws_pad or not a multiple of
 * 8, an A_ws that is not 16-byte aligned. */
int fos_gather_columns(const int32_t* idx, int32_t n_ws, void* A_ws, int64_t lda_ws, int32_t n_ws_pad, const fos_problem* p);

/* The optimality check of the coordinates outside a working set, on the gradient block G of fos_gradient_batch (nv columns of n
 * floats).  alpha1: HOST memory, nv weights; in_ws: device, n bytes; p_i: the bound penalty factor of coordinate i, or 1.  For
 * every coordinate i with in_ws[i] == 0 - by construction the iterate is zero there, so the ridge term vanishes for both prox
 * kinds -
 *   excess[i] (device, n floats) = max over j of |G_ij| / (alpha1[j] * p_i), formed in fp64 and rounded to float; a zero
 *                denominator gives +inf where |G_ij| > 0 and 0 where G_ij = 0; a coordinate inside the set gets 0;
 *   i is a violator when, for some j, (double)|G_ij| > alpha1[j] * (double)p_i * (1 + slack) in exactly this fp64 arithmetic.
 * viol_idx (device, n int32) receives the violators in increasing order, *viol_count (device) their number.  ONE workgroup:
 * per-wave ballots and a block prefix sum, no atomics - two runs give the same bytes.  Enqueues only.
 * FOS_ERR_ARG: a null pointer, nv outside 1..16, a weight that is not finite and >= 0, slack not finite and >= 0.
 * FOS_ERR_UNSUPPORTED: box bounds are bound (a coordinate at a bound has another optimality condition), feature groups are
 * bound, a multinomial problem.  The group penalty (fos_fista_params.group >= 2) belongs to fos_fista handles, which this call
 * does not see: its callers refuse it (working_set.py does). */
int fos_kkt_scan(const float* G, int nv, const double* alpha1, double slack, const uint8_t* in_ws, fos_problem* p, float* excess,
                 int32_t* viol_idx, int32_t* viol_count);

#ifdef __cplusplus
}
#endif
#endif /* FOS_WORKING_SET_H_ */
