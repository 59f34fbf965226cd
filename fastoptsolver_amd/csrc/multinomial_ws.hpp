// Working set and duality gap of the multinomial lockstep (include/fos_multinomial_ws.h): the class scan, the class column pass
// and the fp64 row pass on the logit panel.  The finish is dual_finish_kernel of duality.hpp, unchanged.
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
#include "working_set.hpp"

namespace fos {

struct ClassWeights { double a1[SL_MAX_SEG], a2[SL_MAX_SEG]; };      // per segment

// ---- class scan ---------------------------------------------------------------------------------------------------------------
// kkt_scan_kernel with the C columns of a fit seen together: ONE workgroup of 16 waves walks the n coordinates in order, 1024 at
// a time.  For coordinate i outside the set, per segment s, all in fp64 from the float G:
//     l1      v = max_c |G[s*C + c][i]|                                       violator: v > alpha1[s] p_i (1 + slack)
//     group   q = sum_c G[s*C + c][i]^2 (c ascending),  v = sqrt(q)           violator: q > (alpha1[s] p_i (1 + slack))^2
// (the grouped decision takes no square root: it is the comparison of the squares, exact in the products of the floats), and
// excess[i] = (float) max_s v / (alpha1[s] p_i); a zero denominator gives +inf where v > 0 and 0 where v = 0.  The violators
// leave in increasing order through per-wave ballots and a block prefix sum.  classes and grouped are the same for every lane.
// Resources (gfx950, -O3): 45 VGPRs, 64 bytes of LDS, no scratch.
static __global__ __launch_bounds__(KS_THREADS) void class_kkt_scan_kernel(const float* __restrict__ G, int64_t n, int nv, int classes,
                                                                           int grouped, ClassWeights w, double one_plus_slack,
                                                                           const uint8_t* __restrict__ in_ws,
                                                                           const float* __restrict__ factor, float* __restrict__ excess,
                                                                           int32_t* __restrict__ viol_idx,
                                                                           int32_t* __restrict__ viol_count) {
  __shared__ int wcount[KS_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nseg = nv / classes;
  int running = 0;
  for (int64_t base = 0; base < n; base += KS_THREADS) {
    const int64_t i = base + tid;
    bool viol = false;
    double ex = 0.0;
    if (i < n && in_ws[i] == 0) {
      const double pf = factor ? (double)factor[i] : 1.0;
      for (int s = 0; s < nseg; ++s) {
        const float* __restrict__ g = G + (int64_t)s * classes * n + i;
        const double d = w.a1[s] * pf;
        const double thr = d * one_plus_slack;
        double v = 0.0;
        if (grouped) {
          double q = 0.0;
          for (int c = 0; c < classes; ++c) {
            const double a = (double)g[(int64_t)c * n];
            q += a * a;
          }
          v = sqrt(q);
          viol = viol || q > thr * thr;
        } else {
          for (int c = 0; c < classes; ++c) {
            const double a = (double)fabsf(g[(int64_t)c * n]);
            v = a > v ? a : v;
          }
          viol = viol || v > thr;
        }
        const double e = d > 0.0 ? v / d : (v > 0.0 ? (double)INFINITY : 0.0);
        ex = e > ex ? e : ex;
      }
    }
    if (i < n) excess[i] = (float)ex;
    const unsigned long long bal = __ballot(viol);
    if (lane == 0) wcount[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < KS_THREADS / 64; ++v) {
      const int c = wcount[v];
      before += v < wave ? c : 0;
      total += c;
    }
    if (viol) viol_idx[running + before + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)i;
    running += total;
    __syncthreads();                 // wcount is rewritten by the next trip
  }
  if (tid == 0) *viol_count = running;
}

// ---- class column pass --------------------------------------------------------------------------------------------------------
// Workgroup s < nv / C walks the n x C entries of segment s twice, all in fp64: first the scale (the minimum of an empty set is
// 1), then, with it, the penalty and the conjugate of the ridge-carrying rows.  X: n x 16 floats, row-major - the C entries of a
// row are adjacent; G: nv x n floats; factor: the bound penalty factors or null (1).  col[s*C] = the scale, col[16 + s*C] = the
// penalty, col[32 + s*C] = the conjugate, and 0 in the other C - 1 entries of the segment in all three, so that
// dual_finish_kernel (which adds entry j of the column pass to entry j of the row pass) serves unchanged.
// Resources (gfx950, -O3): 38 VGPRs, 2 KiB of LDS, no scratch.
static __global__ __launch_bounds__(DS_THREADS) void class_dual_scale_kernel(const float* __restrict__ X, const float* __restrict__ G,
                                                                             int64_t n, int classes, int grouped, ClassWeights wts,
                                                                             const float* __restrict__ factor,
                                                                             double* __restrict__ col) {
  __shared__ double red[DS_THREADS];
  const int tid = threadIdx.x, seg = blockIdx.x, lo = seg * classes;
  const double a1 = wts.a1[seg], a2 = wts.a2[seg];
  const float* __restrict__ g = G + (int64_t)lo * n;
  double smin = 1.0;
  for (int64_t k = tid; k < n; k += DS_THREADS) {
    const double pf = factor ? (double)factor[k] : 1.0;
    const double tau = a1 * pf, rho = a2 * pf;
    if (rho != 0.0) continue;
    if (grouped) {
      double q = 0.0;
      for (int c = 0; c < classes; ++c) {
        const double a = (double)g[(int64_t)c * n + k];
        q += a * a;
      }
      const double v = sqrt(q);
      if (v != 0.0) smin = fmin(smin, tau / v);
    } else {
      for (int c = 0; c < classes; ++c) {
        const double a = (double)fabsf(g[(int64_t)c * n + k]);
        if (a != 0.0) smin = fmin(smin, tau / a);
      }
    }
  }
  const double s = dual_block_min(smin, red);
  double pen = 0.0, conj = 0.0;
  for (int64_t k = tid; k < n; k += DS_THREADS) {
    const double pf = factor ? (double)factor[k] : 1.0;
    const double tau = a1 * pf, rho = a2 * pf;
    const float* __restrict__ x = X + k * BT_NV + lo;
    if (grouped) {
      double x2 = 0.0, q = 0.0;
      for (int c = 0; c < classes; ++c) {
        const double xv = (double)x[c], a = (double)g[(int64_t)c * n + k];
        x2 += xv * xv;
        q += a * a;
      }
      pen += tau * sqrt(x2) + 0.5 * rho * x2;
      if (rho > 0.0) {
        const double e = fmax(s * sqrt(q) - tau, 0.0);
        conj += e * e / (2.0 * rho);
      }
    } else {
      for (int c = 0; c < classes; ++c) {
        const double xv = (double)x[c];
        pen += tau * fabs(xv) + 0.5 * rho * xv * xv;
        if (rho > 0.0) {
          const double e = fmax(s * (double)fabsf(g[(int64_t)c * n + k]) - tau, 0.0);
          conj += e * e / (2.0 * rho);
        }
      }
    }
  }
  pen = dual_block_sum(pen, red);
  conj = dual_block_sum(conj, red);
  if (tid < classes) {
    const bool first = tid == 0;
    col[lo + tid] = first ? s : 0.0;
    col[BT_NV + lo + tid] = first ? pen : 0.0;
    col[2 * BT_NV + lo + tid] = first ? conj : 0.0;
  }
}

// ---- row pass -----------------------------------------------------------------------------------------------------------------
// z16: the panel Z = A_panel X (rows x 16 fp32, row-major) that product 1 left in its plain storing form; it is only read.
// labels[i], row_weight[i] (WEIGHT): offset to the panel by the caller.  col: DEVICE, the output of class_dual_scale_kernel - the
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
