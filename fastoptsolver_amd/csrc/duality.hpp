// The duality-gap certificate of lockstep solutions (include/fos_duality.h): the column pass, the row pass and the finish.
//
// For one column - a point x with the weights alpha1, alpha2 - with z_i = a_i . x, w_i the bound row weight (or 1), p_k the bound
// penalty factor (or 1), tau_k = alpha1 p_k, rho_k = alpha2 p_k, psi_i = df/dz the unweighted derivative of the loss and
// G = A^T (w psi) the gradient block of fos_gradient_batch:
//
//     primal  P = sum_i w_i f(z_i, b_i) + sum_k (tau_k |x_k| + rho_k x_k^2 / 2)
//     scale   s = min(1, min over {k : rho_k = 0 and G_k != 0} of tau_k / |G_k|)
//     dual    D = sum_i w_i d(z_i, b_i; s) - sum over {k : rho_k > 0} of max(s |G_k| - tau_k, 0)^2 / (2 rho_k)
//
// The dual point is theta = -s (w psi): the scale pulls A^T theta into the box of the coordinates that carry no ridge term, the
// others pay the conjugate of the elastic-net penalty.  d is minus the conjugate of the loss at s psi:
//
//     squared, Huber (psi = z - b, or clip(z - b, -c, c))   d = -s psi b - s^2 psi^2 / 2
//     squared hinge  (h = max(0, 1 - b z))                  d = s h - s^2 h^2 / 2
//     logistic       (q = b + s (sigma(z) - b))             d = -(q log q + (1 - q) log(1 - q)),   0 log 0 = 0
//
// gap = P - D >= 0 bounds P(x) - P*.  An unpenalised coordinate (p_k = 0) with a non-zero gradient gives s = 0: the bound
// D = -F*(0) is valid and loose.
//
// The row pass forms w f and w d of an element in fp64 from the same fp32 z, so the gap cannot hide behind two roundings of A x.
// Every sum has a fixed order (DPP within 16-lane rows, LDS across them, one workgroup over the partials); the three kernels use
// no read-modify-write of global memory, no flags and no waits: two runs give the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "batch_trial.hpp"
#include "working_set.hpp"

namespace fos {

constexpr int DL_THREADS = 256;          // row pass: one 16-byte quad of a panel row per lane, as pointwise_link_kernel
constexpr int DL_WIDTH = 2 * BT_NV;      // a row of the partial buffer: 16 primal data terms, then 16 dual data terms
constexpr int DS_THREADS = 256;          // column pass: one workgroup per column
// LOSS of dual_link_kernel: the loss ids of fos.h.  A multinomial problem (2) is refused before any launch.
constexpr int DUAL_SQUARED = 0, DUAL_LOGISTIC = 1, DUAL_HUBER = 3, DUAL_SQUARED_HINGE = 4;

__device__ __forceinline__ double dual_xlogx(double q) { return q > 0.0 ? q * log(q) : 0.0; }

// (f, d) of one element in fp64: the loss and minus its conjugate at the scaled derivative s psi.
template <int LOSS>
__device__ __forceinline__ void dual_terms(double z, double b, double c, double s, double* f, double* d) {
  if constexpr (LOSS == DUAL_SQUARED) {
    const double r = z - b;
    *f = 0.5 * r * r;
    *d = -s * r * b - 0.5 * (s * r) * (s * r);
  } else if constexpr (LOSS == DUAL_HUBER) {
    const double r = z - b, a = fabs(r);
    const double psi = fmin(fmax(r, -c), c);
    *f = a <= c ? 0.5 * r * r : c * a - 0.5 * c * c;
    *d = -s * psi * b - 0.5 * (s * psi) * (s * psi);
  } else if constexpr (LOSS == DUAL_SQUARED_HINGE) {
    const double h = fmax(0.0, 1.0 - b * z);
    *f = 0.5 * h * h;
    *d = s * h - 0.5 * (s * h) * (s * h);
  } else {
    static_assert(LOSS == DUAL_LOGISTIC, "dual_link_kernel: squared, logistic, Huber and squared hinge");
    const double e = exp(-fabs(z));                       // in (0, 1]: no overflow at either end
    const double sig = z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
    const double q = b + s * (sig - b);
    *f = fmax(z, 0.0) - b * z + log1p(e);
    *d = -(dual_xlogx(q) + dual_xlogx(1.0 - q));          // exactly 0 where q or 1 - q is 0
  }
}

// ---- row pass -----------------------------------------------------------------------------------------------------------------
// z16: the panel Z = A_panel X (rows x 16 fp32, row-major) that product 1 left in its plain storing form; it is only read.
// b[i], row_weight[i] (WEIGHT): offset to the panel by the caller.  param: the Huber threshold c.  scale: DEVICE, the 16 scales of
// dual_scale_kernel (they are known on the device alone: the certificate enqueues and never waits).  Columns >= nv contribute 0.
// part[wg][0..15] = this workgroup's sum of w f per column, part[wg][16..31] = of w d.  Rows >= rows are not read; the grid
// may be any size (grid-stride over the quads, a multiple of 4: a lane's four columns are fixed for the launch).
// Resources (gfx950, -O3): 46 .. 58 VGPRs (128 for the logistic forms, whose four elements carry exp, log1p and two logs in
// fp64), no scratch, 4 KiB of LDS.
template <int LOSS, bool WEIGHT>
__global__ __launch_bounds__(DL_THREADS) void dual_link_kernel(const float* __restrict__ z16, int64_t rows,
                                                               const float* __restrict__ b, float param, int nv,
                                                               const float* __restrict__ row_weight,
                                                               const double* __restrict__ scale, double* __restrict__ part) {
  __shared__ double red[DL_THREADS / 16][DL_WIDTH];     // [16-lane row of the workgroup][primal 0..15, dual 16..31]
  const int tid = threadIdx.x, quad = tid & 3;
  const double c = (double)param;
  bool live[4];
  double s[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    live[k] = 4 * quad + k < nv;
    s[k] = live[k] ? scale[4 * quad + k] : 0.0;
  }
  double psum[4] = {0.0, 0.0, 0.0, 0.0}, dsum[4] = {0.0, 0.0, 0.0, 0.0};

  const int64_t total = rows * 4, stride = (int64_t)gridDim.x * DL_THREADS;
  for (int64_t idx = (int64_t)blockIdx.x * DL_THREADS + tid; idx < total; idx += stride) {
    const int64_t row = idx >> 2;
    const f32x4 z4 = *(reinterpret_cast<const f32x4*>(z16) + idx);
    const double bi = (double)b[row];
    double w = 1.0;
    if constexpr (WEIGHT) w = (double)row_weight[row];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double f, d;
      dual_terms<LOSS>((double)z4[k], bi, c, s[k], &f, &d);
      if constexpr (WEIGHT) { f *= w; d *= w; }
      psum[k] += live[k] ? f : 0.0;
      dsum[k] += live[k] ? d : 0.0;
    }
  }

  // lanes of equal quad within a 16-lane row (DPP row_shr 4, 8: lanes 12 .. 15 hold the totals) -> LDS -> the workgroup's row
#pragma unroll
  for (int k = 0; k < 4; ++k) { psum[k] += dpp_fetch<0x114, 0xF>(psum[k]); dsum[k] += dpp_fetch<0x114, 0xF>(dsum[k]); }   // row_shr:4
#pragma unroll
  for (int k = 0; k < 4; ++k) { psum[k] += dpp_fetch<0x118, 0xF>(psum[k]); dsum[k] += dpp_fetch<0x118, 0xF>(dsum[k]); }   // row_shr:8
  if ((tid & 15) >= 12) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      red[tid >> 4][4 * quad + k] = psum[k];
      red[tid >> 4][BT_NV + 4 * quad + k] = dsum[k];
    }
  }
  __syncthreads();
  if (tid < DL_WIDTH) {
    double v = 0.0;
#pragma unroll
    for (int g = 0; g < DL_THREADS / 16; ++g) v += red[g][tid];
    part[(int64_t)blockIdx.x * DL_WIDTH + tid] = v;
  }
}

// ---- column pass --------------------------------------------------------------------------------------------------------------
// The columns of a block are fits of C columns each (the segments of kkt_scan_kernel; C = 1 for every loss but the multinomial
// one).  Workgroup s < nv / C walks the n x C entries of segment s twice, all in fp64, with tau_k = a1[s] * (double)p_k and
// rho_k = a2[s] * (double)p_k.  v runs over the entries (k, c), v = |G_kc| - or, grouped, over the rows k, v = ||G_k:||_2 (the
// squares summed with c ascending).  First the scale
//     s = min(1, min over {rho = 0 and v != 0} of tau / v)                    (the minimum of an empty set is 1),
// then, with it, pen = sum tau |x| + rho x^2 / 2 (grouped: of the row norms) and conj = sum over {rho > 0} of
// max(s v - tau, 0)^2 / (2 rho).  X: n x 16 floats, row-major (the layout of fos_gradient_batch; the C entries of a row are
// adjacent); G: nv x n floats; factor: the bound penalty factors or null (1).  col[s*C] = the scale, col[16 + s*C] = pen,
// col[32 + s*C] = conj, and 0 in the other C - 1 entries of the segment in all three, so that dual_finish_kernel adds entry j of
// the column pass to entry j of the row pass for every family.
// Fixed-order trees through LDS.  Resources (gfx950, -O3): 38 VGPRs, no scratch, 2 KiB of LDS.
__device__ __forceinline__ double dual_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();                   // the readers of the previous tree are done
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int h = DS_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ double dual_block_min(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int h = DS_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] = fmin(red[tid], red[tid + h]);
    __syncthreads();
  }
  return red[0];
}

static __global__ __launch_bounds__(DS_THREADS) void dual_scale_kernel(const float* __restrict__ X, const float* __restrict__ G,
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

// ---- finish -------------------------------------------------------------------------------------------------------------------
// ONE workgroup of 16 waves folds the nparts rows of the row pass as fold_partials_kernel does (wave v: columns v and 16 + v, the
// lanes stride over the rows, a DPP sum at the end) and writes out64: primal[16], dual[16], gap[16] = primal - dual, scale[16].
// Columns >= nv get 0 in all four.
constexpr int DF_THREADS = 1024;
static __global__ __launch_bounds__(DF_THREADS) void dual_finish_kernel(const double* __restrict__ part, int nparts,
                                                                        const double* __restrict__ col, int nv,
                                                                        double* __restrict__ out64) {
  __shared__ double tot[DL_WIDTH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int w = wave; w < DL_WIDTH; w += DF_THREADS / 64) {
    double s = 0.0;
    for (int i = lane; i < nparts; i += 64) s += part[(int64_t)i * DL_WIDTH + w];
    s = wave_sum(s);
    if (lane == 0) tot[w] = s;
  }
  __syncthreads();
  if (threadIdx.x < BT_NV) {
    const int j = threadIdx.x;
    const bool on = j < nv;
    const double primal = on ? tot[j] + col[BT_NV + j] : 0.0;
    const double dual = on ? tot[BT_NV + j] - col[2 * BT_NV + j] : 0.0;
    out64[j] = primal;
    out64[BT_NV + j] = dual;
    out64[2 * BT_NV + j] = primal - dual;
    out64[3 * BT_NV + j] = on ? col[j] : 0.0;
  }
}

}  // namespace fos
