/* fos_feature_groups.h - the group lasso over feature groups of one fit: two entry points of libfos_hip.so beside fos.h.
 *
 * They live in a header of their own: the entry points of fos.h that take a handle are a closed list (every one of them is filed
 * by what it does on a logistic and on a multinomial problem), and these two stand outside that list - the bind refuses a
 * multinomial problem by a check of its own.  Conventions, error codes and handle types are those of fos.h.
 */
#ifndef FOS_FEATURE_GROUPS_H_
#define FOS_FEATURE_GROUPS_H_

#include "fos.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Group lasso over feature groups of one fit (sparse-group lasso with l1_mix > 0).  The coordinates 0..n-1 are partitioned into
 * ngroups contiguous groups g = [group_start[g], group_start[g+1]) and the objective of every lockstep column x is
 *   data term (squared or logistic, weighted or not, fold-masked or not)
 *     + alpha1 [ (1 - l1_mix) sum_g w_g ||x_g||_2 + l1_mix ||x||_1 ] + 0.5 alpha2 ||x||_2^2 .
 * A group is in the model whole or not at all (l1_mix = 0); w_g = 0 leaves a group out of the group term (an intercept column);
 * l1_mix = 1 is the plain lasso, bit for bit.  group_start: HOST memory, ngroups + 1 entries; group_weight: HOST memory, ngroups
 * floats, NULL stands for sqrt(group size).  Both are checked here, on the host, before any HIP call, and copied into device
 * buffers the problem owns (with a coordinate-to-group map and the workspace of the update, reserved once); a second bind
 * replaces them, ngroups = 0 with a NULL table detaches, fos_problem_destroy frees them.  The data comes first, the handle last.
 * The call waits for the work enqueued on the problem's stream.  With groups bound
 *   - fos_fista_run_multi (any nv in 1..16) and fos_fista_run_multi_folds minimise the objective above, plain or controlled:
 *     always the two matrix-core products per iteration, unchanged, and the update in three launches - u = soft_threshold(y - tau
 *     g_full, tau alpha1 l1_mix) per coordinate, ||u_g||^2 per (group, column) summed in a fixed order, then
 *     x_g = (||u_g|| <= thr_g ? 0 : 1 - thr_g / ||u_g||) u_g with thr_g = tau alpha1 (1 - l1_mix) w_g, divided by 1 + tau alpha2
 *     for PROX_ENET - in fp64, without atomics: two runs are bitwise equal.  A group at or below its threshold is exactly 0.0.
 *     The step is that of the separable penalty (the penalty does not enter L);
 *   - a handle with fos_fista_params.group >= 2 is refused on such a problem, and so is fos_fista_run_multi_rhs;
 *   - fos_residual_batch (use_b = 1) and fos_residual_batch_folds answer as before, as do the entry points that touch neither b
 *     nor a residual;
 *   - every entry point that refuses a problem with coordinate data refuses this one too (FOS_ERR_UNSUPPORTED before any launch
 *     or change of handle state, with a message of its own).
 * FOS_ERR_ARG: null p, a NULL table with ngroups != 0, ngroups outside 1..n, group_start[0] != 0, group_start not strictly
 * increasing, group_start[ngroups] != n, a weight that is not finite and >= 0, l1_mix outside [0, 1].  FOS_ERR_UNSUPPORTED under
 * the conditions of fos_coord_bind (no b, a sharded problem, a shape without the matrix-core pair), with coordinate data bound
 * (and fos_coord_bind on a problem with feature groups) and on a multinomial problem (and fos_problem_set_multinomial on a problem
 * with feature groups).  Nothing is replanned.  fos_feature_groups_get: *ngroups = 0 when none are bound. */
int fos_feature_groups_bind(const int32_t* group_start, const float* group_weight, int32_t ngroups, double l1_mix, fos_problem* p);
int fos_feature_groups_get(int32_t* ngroups, double* l1_mix, const fos_problem* p);

#ifdef __cplusplus
}
#endif
#endif /* FOS_FEATURE_GROUPS_H_ */
