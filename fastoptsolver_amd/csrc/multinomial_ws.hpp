// Working set and duality gap of the multinomial lockstep (include/fos_multinomial_ws.h): the class scan - the instantiation of
// the one scan body of working_set.hpp that takes C and the kind of penalty at run time - and the fp64 row pass on the logit
// panel.  The column pass and the finish (dual_scale_kernel and dual_finish_kernel of duality.hpp) are those of every loss,
// launched with C columns per fit.
//
// The 16 columns of a block are the C class vectors of nv / C fits ("segments": segment s is columns s*C .. s*C + C-1, as in
// softmax_link.hpp).  For one segment with the weights alpha1, alpha2, Z = A X_seg (m x C), sigma_i = softmax(z_i), w_i the bound
// row weight (or 1), p_k the bound penalty factor (or 1), tau_k = alpha1 p_k, rho_k = alpha2 p_k and g_kc the gradient entry of
// row k of X, class c (the block of fos_multinomial_gradient_batch):
//
//     primal  P = sum_i w_i [logsumexp(z_i) - z_{i,y_i}] + Omega(X)
//     l1      Omega = sum_k sum_c (tau_k |x_kc| + rho_k x_kc^2 / 2)           v runs over the entries (k, c):  v = |g_kc|
//     group   Omega = sum_k (tau_k ||x_k:|| + rho_k ||x_k:||^2 / 2)           v runs over the rows k:           v = ||g_k:||_2
//     scale   s = min(1, min over {rho = 0 and v != 0} of tau / v)
//     dual    D = sum_i w_i d_i - sum over {rho > 0} of max(s v - tau, 0)^2 / (2 rho)
//             d_i = -sum_c q_ic log q_ic,   q_ic = [y_i = c] + s (sigma_ic - [y_i = c]),   0 log 0 = 0
//
// The dual point is Theta = -s W (sigma - onehot).  Row i of q is a convex combination of two points of the simplex for s in
// [0, 1], so the conjugate of the softmax cross-entropy - the negative entropy, +inf off the simplex - is finite at it.
//
// As in duality.hpp: every sum has a fixed order (DPP within a wave, LDS across the waves, one workgroup over the partials), no
// read-modify-write of global memory, no flags and no waits - two runs give the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "batch_trial.hpp"
#include "duality.hpp"
#include "softmax_link.hpp"

namespace fos {

// ---- class scan ---------------------------------------------------------------------------------------------------------------
// kkt_scan_body of working_set.hpp with the C columns of a fit seen together; classes and grouped are the same for every lane.
// Resources (gfx950, -O3): 47 VGPRs, 64 bytes of LDS, no scratch.
static __global__ __launch_bounds__(KS_THREADS) void class_kkt_scan_kernel(const float* __restrict__ G, int64_t n, int nv, int classes,
                                                                           int grouped, ScanWeights w, double one_plus_slack,
                                                                           const uint8_t* __restrict__ in_ws,
                                                                           const float* __restrict__ factor, float* __restrict__ excess,
                                                                           int32_t* __restrict__ viol_idx,
                                                                           int32_t* __restrict__ viol_count) {
  kkt_scan_body<false>(G, n, nv, classes, grouped, w, one_plus_slack, in_ws, factor, excess, viol_idx, viol_count);
}

// ---- row pass -----------------------------------------------------------------------------------------------------------------
// z16: the panel Z = A_panel X (rows x 16 fp32, row-major) that product 1 left in its plain storing form; it is only read.
// labels[i], row_weight[i] (WEIGHT): offset to the panel by the caller.  col: DEVICE, the output of dual_scale_kernel - the
// scale of segment s is col[s*C] (known on the device alone: the certificate enqueues and never waits).
// One thread per row, as in softmax_link_kernel: four 16-byte loads; the row stays in registers (constant indices only) and
// every branch is on a value all lanes share.  The segment's logits are shifted to the front of the row (four shifts by the bits
// of s*C); the walks over its classes are rolled loops that move the row down one entry per class, so a segment costs its own C
// classes and no more, and exp and log are compiled a few times instead of 16 times each.  (The unrolled form - 16 predicated
// columns per walk - kept 15 lane masks and the 35 scalar halves of the fp64 constants of exp and log alive together and spilled
// up to 45 scalar registers.)  In fp64, from the same fp32 z: the maximum, the exponentials, f = logsumexp - z_y, q and
// d = -sum q log q; the exponentials are formed twice rather than kept.
// A segment at a time, the rows inside: with all nv / C segments of a row in flight the 16 accumulators and the unrolled
// predicates of 8 segments cost 191 VGPRs and spilled scalar registers; one segment in flight needs two accumulators.  The price
// is that the panel - 64 bytes a row, written by product 1 just before and resident in L2 - is read nv / C times, next to the
// 4 n bytes of A per row that product 1 read to make it.
// part[wg][s*C] = this workgroup's sum of w f of segment s, part[wg][16 + s*C] = of w d, the other entries 0: the layout of
// dual_link_kernel.  Rows >= rows are not read; the grid may be any size (grid-stride over rows).
// Resources (gfx950, -O3): 90 VGPRs plain and weighted, 512 bytes of LDS, no scratch, no spilled register.
template <bool WEIGHT>
__global__ __launch_bounds__(SL_THREADS) void dual_softmax_kernel(const float* __restrict__ z16, int64_t rows,
                                                                  const float* __restrict__ labels, int classes, int nv,
                                                                  const float* __restrict__ row_weight,
                                                                  const double* __restrict__ col, double* __restrict__ part) {
  __shared__ double wsum[SL_THREADS / 64][2 * SL_MAX_SEG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nseg = nv / classes;
#pragma unroll 1
  for (int s = 0; s < nseg; ++s) {
    const int lo = s * classes;
    const double sc = col[lo];
    double psum = 0.0, dsum = 0.0;
    for (int64_t row = (int64_t)blockIdx.x * SL_THREADS + tid; row < rows; row += (int64_t)gridDim.x * SL_THREADS) {
      const f32x4* rp = reinterpret_cast<const f32x4*>(z16 + row * BT_NV);
      float z[BT_NV];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 v = rp[q];
        z[4 * q] = v.x; z[4 * q + 1] = v.y; z[4 * q + 2] = v.z; z[4 * q + 3] = v.w;
      }
      const int lab = (int)labels[row];
      // the segment's C logits to the front of the row: four shifts by the bits of lo, each under a branch every lane shares
      // (entries that come in from beyond the segment are never used: lo + C <= 16)
      if (lo & 1) {
#pragma unroll
        for (int j = 0; j < BT_NV - 1; ++j) z[j] = z[j + 1];
      }
      if (lo & 2) {
#pragma unroll
        for (int j = 0; j < BT_NV - 2; ++j) z[j] = z[j + 2];
      }
      if (lo & 4) {
#pragma unroll
        for (int j = 0; j < BT_NV - 4; ++j) z[j] = z[j + 4];
      }
      if (lo & 8) {
#pragma unroll
        for (int j = 0; j < BT_NV - 8; ++j) z[j] = z[j + 8];
      }
      float zlab = z[0];                           // the label's logit (label < C): a lane's own choice, no count needed
#pragma unroll
      for (int c = 1; c < BT_NV; ++c) zlab = (c == lab) ? z[c] : zlab;
      // three walks over the C classes, each a rolled loop on a copy of the row that moves down one entry per class: entry 0
      // is the class at hand, every index is a constant, and exp and log are compiled once per walk
      float zt[BT_NV], zmax = -INFINITY;
#pragma unroll
      for (int j = 0; j < BT_NV; ++j) zt[j] = z[j];
#pragma unroll 1
      for (int c = 0; c < classes; ++c) {
        zmax = fmaxf(zmax, zt[0]);
#pragma unroll
        for (int j = 0; j < BT_NV - 1; ++j) zt[j] = zt[j + 1];
      }
      double sum = 0.0;
#pragma unroll
      for (int j = 0; j < BT_NV; ++j) zt[j] = z[j];
#pragma unroll 1
      for (int c = 0; c < classes; ++c) {
        sum += exp((double)zt[0] - (double)zmax);
#pragma unroll
        for (int j = 0; j < BT_NV - 1; ++j) zt[j] = zt[j + 1];
      }
      const double inv = 1.0 / sum;
      const double f = (log(sum) + (double)zmax) - (double)zlab;
      // d = -sum_c q_c log q_c with q_c = s sigma_c off the label and 1 + s (sigma_y - 1) on it: every class as if off the
      // label, then the label's term exchanged.  The exponentials are formed again (the same values: the same arguments)
      // instead of 16 doubles kept per lane.
      const double slab = exp((double)zlab - (double)zmax) * inv;
      double d = dual_xlogx(sc * slab) - dual_xlogx(1.0 + sc * (slab - 1.0));
#pragma unroll 1
      for (int c = 0; c < classes; ++c) {
        d -= dual_xlogx(sc * (exp((double)z[0] - (double)zmax) * inv));
#pragma unroll
        for (int j = 0; j < BT_NV - 1; ++j) z[j] = z[j + 1];
      }
      if constexpr (WEIGHT) {
        const double w = (double)row_weight[row];
        psum += w * f;
        dsum += w * d;
      } else {
        psum += f;
        dsum += d;
      }
    }
    // per thread fp64 -> wave (DPP) -> LDS; the workgroup's row of part is written once, below
    const double pv = wave_sum(psum), dv = wave_sum(dsum);
    if (lane == 0) { wsum[wave][s] = pv; wsum[wave][SL_MAX_SEG + s] = dv; }
  }
  __syncthreads();
  if (tid < DL_WIDTH) {
    const int j = tid & (BT_NV - 1), s = j / classes, k = (tid >> 4) * SL_MAX_SEG + s;
    double v = 0.0;
    if (j < nv && j == s * classes) v = (wsum[0][k] + wsum[1][k]) + (wsum[2][k] + wsum[3][k]);
    part[(int64_t)blockIdx.x * DL_WIDTH + tid] = v;
  }
}

}  // namespace fos
