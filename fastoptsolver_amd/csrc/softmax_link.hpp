// The link between the two products of the multinomial (softmax) lockstep.
//
// Model: C classes, one coefficient vector per class.  The 16 candidate columns of the lockstep hold the C class vectors of
// floor(16 / C) fits ("segments": segment s is columns s*C .. s*C + C-1), so product 1 in its plain storing form leaves all
// class logits Z = A_panel Y of a row panel in rbuf16 (rows x 16 fp32, row-major) with one read of A, and product 2 turns a
// residual block R into all class gradients A^T R with the other.  What couples the C columns of a fit sits between them:
//
//     R[i][s*C + c] = softmax(z_i[s*C ..])[c] - [label_i == c]            l_i = logsumexp(z_i[s*C ..]) - z_i[s*C + label_i]
//
// No epilogue of product 1 can do that - its 16 candidate lanes never meet - so it is a kernel of its own on the panel the two
// products hand over anyway: one read and one write of 64 bytes per row, next to the 2 * 4 n bytes of A per row.
//
// One thread per row: four aligned 16-byte loads, every segment's softmax in registers, four 16-byte stores - a wave moves 4 KiB
// of contiguous memory and no lane needs another's data for any C.  C is a run-time value that is the same for every lane, so
// the segment a column belongs to is decided by wave-uniform predicates over fully unrolled column loops: the row stays in
// registers (constant indices only) and there is no divergence.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "batch_trial.hpp"

namespace fos {

constexpr int SL_THREADS = 256;
constexpr int SL_MAX_SEG = BT_NV / 2;   // the most segments a block holds (C = 2)

// r16: the panel (rows x 16 fp32), logits in, residuals out.  labels[i]: the class of row i, 0 .. classes-1, stored as a float.
// classes: C, 2 .. 16.  nv: the active columns, a multiple of C; columns >= nv are written as 0.
// WEIGHT: R and l are multiplied by row_weight[i].  FOLD: the mask of K-fold cross-validation with the semantics of fold_mask
// (batch_trial.hpp) - the held id of a segment is the one of its first column; FOLD_TRAIN zeroes R and l on the rows a segment
// holds out, FOLD_HELD everywhere else.  In the FOLD_HELD form only the sums are wanted and R is not written.
// q_part[wg][s*C] = the sum of l over this workgroup's rows for segment s (fp64), the other columns of q_part[wg] are 0.
// stopped: the parking convention of product 1 (a set flag makes the launch a no-op).
// Rows >= rows are neither read nor written; the grid may be any size (grid-stride over rows).
template <int FOLD, bool WEIGHT>
__global__ __launch_bounds__(SL_THREADS) void softmax_link_kernel(float* __restrict__ r16, int64_t rows,
                                                                  const float* __restrict__ labels, int classes, int nv,
                                                                  const float* __restrict__ row_weight,
                                                                  const uint8_t* __restrict__ fold_of_row, FoldHeld held,
                                                                  double* __restrict__ q_part,
                                                                  const int* __restrict__ stopped) {
  if (stopped != nullptr && *stopped != 0) return;
  __shared__ double wsum[SL_THREADS / 64][SL_MAX_SEG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double qsum[SL_MAX_SEG];
#pragma unroll
  for (int s = 0; s < SL_MAX_SEG; ++s) qsum[s] = 0.0;

  for (int64_t row = (int64_t)blockIdx.x * SL_THREADS + tid; row < rows; row += (int64_t)gridDim.x * SL_THREADS) {
    f32x4* rp = reinterpret_cast<f32x4*>(r16 + row * BT_NV);
    float z[BT_NV];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 v = rp[q];
      z[4 * q] = v.x; z[4 * q + 1] = v.y; z[4 * q + 2] = v.z; z[4 * q + 3] = v.w;
    }
    const int lab = (int)labels[row];
    float w = 1.f;
    if constexpr (WEIGHT) w = row_weight[row];
    unsigned fold_id = 0u;
    if constexpr (FOLD != FOLD_OFF) fold_id = fold_of_row[row];

    // the maximum of every column's segment (a column beyond nv keeps its own value: its exponential is 1 and unused)
    float mx[BT_NV];
#pragma unroll
    for (int j = 0; j < BT_NV; ++j) mx[j] = z[j];
#pragma unroll
    for (int s = 0; s < SL_MAX_SEG; ++s) {
      const int lo = s * classes, hi = lo + classes;
      if (lo < nv) {                               // wave-uniform
        float smax = -INFINITY;
#pragma unroll
        for (int j = 0; j < BT_NV; ++j) smax = (j >= lo && j < hi) ? fmaxf(smax, z[j]) : smax;
#pragma unroll
        for (int j = 0; j < BT_NV; ++j) mx[j] = (j >= lo && j < hi) ? smax : mx[j];
      }
    }
    float e[BT_NV];
#pragma unroll
    for (int j = 0; j < BT_NV; ++j) e[j] = expf(z[j] - mx[j]);      // the accurate forms, as logistic_terms uses
    float r[BT_NV];
#pragma unroll
    for (int j = 0; j < BT_NV; ++j) r[j] = 0.f;
#pragma unroll
    for (int s = 0; s < SL_MAX_SEG; ++s) {
      const int lo = s * classes, hi = lo + classes;
      if (lo < nv) {                               // wave-uniform
        float sum = 0.f, smax = 0.f, zlab = 0.f;
#pragma unroll
        for (int j = 0; j < BT_NV; ++j) {
          const bool in = j >= lo && j < hi;
          sum += in ? e[j] : 0.f;
          smax = in ? mx[j] : smax;
          zlab = (in && j - lo == lab) ? z[j] : zlab;
        }
        float scale = w;                           // weight, then the fold mask: both multiply R and l alike
        if constexpr (FOLD != FOLD_OFF) {
          const bool is_held = fold_id == fold_held_of(held, lo);
          if (FOLD == FOLD_TRAIN ? is_held : !is_held) scale = 0.f;
        }
        const float inv = 1.f / sum;
        const float l = (logf(sum) + smax) - zlab;
        qsum[s] += (double)(scale * l);
#pragma unroll
        for (int j = 0; j < BT_NV; ++j)
          if (j >= lo && j < hi) r[j] = scale * (e[j] * inv - ((j - lo == lab) ? 1.f : 0.f));
      }
    }
    if constexpr (FOLD != FOLD_HELD) {
#pragma unroll
      for (int q = 0; q < 4; ++q) rp[q] = f32x4{r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]};
    }
  }

  // per thread fp64 -> wave (DPP) -> LDS -> the workgroup's row of q_part; no atomics
#pragma unroll
  for (int s = 0; s < SL_MAX_SEG; ++s) {
    const double v = wave_sum(qsum[s]);
    if (lane == 0) wsum[wave][s] = v;
  }
  __syncthreads();
  if (tid < BT_NV) {
    const int s = tid / classes;
    double v = 0.0;
    if (tid < nv && tid == s * classes) v = (wsum[0][s] + wsum[1][s]) + (wsum[2][s] + wsum[3][s]);
    q_part[(int64_t)blockIdx.x * BT_NV + tid] = v;
  }
}

}  // namespace fos
